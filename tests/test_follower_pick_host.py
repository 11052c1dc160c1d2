"""CPU-side proof of the follower-card forms of k_play_wide's trick-aligned card loop (tarok_device.h: legal_mask_follow,
kth_bit_word, the C plane that carries TK_C_PAD): once somebody has led, every legal card of the seat to play lies in one
32-bit word, so the pick needs no first level.  The device header is compiled by g++ with the gfx950 builtins emulated
(tests/host_emu/follower_pick_host.cpp).  No GPU involved."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "host_emu")
SRC = os.path.join(EMU, "follower_pick_host.cpp")
REC = np.dtype([("masks", np.uint64, 48), ("fmasks", np.uint64, 48), ("hisel", np.uint8, 48), ("actions", np.uint8, 48), ("nsteps", np.int16)])


@pytest.fixture(scope="module")
def host_binary(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu") / "follower_pick_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-w", "-I", EMU, "-o", out, SRC])
    return out


def test_kth_bit_word_equals_kth_bit(host_binary):
    """Every 8-bit pattern in each suit byte, 200,000 sampled tarok subsets of up to 12 bits (and 40,000 low-word hands),
    every k below the popcount: the one-word pick returns kth_bit's card."""
    out = subprocess.check_output([host_binary, "pick"], text=True).split()
    assert int(out[0]) >= 4 * 255 + 200000 and int(out[2]) > int(out[0])


@pytest.mark.parametrize("mix,seed", [(0, 5), (1, 7), (2, 9), (16, 1), (23, 1), (24, 3), (25, 2)])
def test_follower_mask_lies_in_one_word(host_binary, tmp_path, mix, seed):
    from oracle import oracle as O
    n = 2000
    path = str(tmp_path / "out.bin")
    subprocess.check_call([host_binary, str(seed), "0", str(n), "0", str(mix), path])
    got = np.fromfile(path, dtype=REC)
    assert got.shape == (n,)
    ref = O.rollout(seed, 0, n, 0, mix)
    assert (got["nsteps"] == ref["nsteps"]).all()
    t = np.arange(48)[None, :]
    live = t < ref["nsteps"][:, None]
    follow = live & (t % 4 != 0)                       # games are whole tricks long: card t is card t % 4 of its trick
    assert follow.sum() >= 3 * n                       # (a Berac can be over after one trick)
    m = ref["masks"].astype(np.uint64)
    lo, hi = m & np.uint64(0xFFFFFFFF), m >> np.uint64(32)
    # the oracle's own mask: exactly one word holds cards once somebody has led
    assert ((lo[follow] != 0) ^ (hi[follow] != 0)).all()
    assert ((lo[live & ~follow] != 0) & (hi[live & ~follow] != 0)).any()        # (the lead itself is NOT of that kind)
    assert (got["masks"][live] == m[live]).all()
    assert (got["fmasks"][follow] == m[follow]).all()
    assert (got["hisel"][follow] == (hi[follow] != 0).astype(np.uint8)).all()
    assert (got["hisel"][~follow] == 255).all() and (got["fmasks"][~follow] == 0).all()
    # the card drawn through the one-word pick is the oracle's card
    assert (got["actions"][live] == ref["actions"][live]).all()
    if mix in (0, 23, 25):                             # the pagat rule (Klop, Berac, Odprti berac) met in the high word
        assert (follow & (hi != 0)).any()


def test_follower_forms_under_address_and_ub_sanitizers(tmp_path):
    """The same stand-alone program with -fsanitize=address,undefined: the exhaustive pick check and 1,500 games."""
    exe = str(tmp_path / "follower_pick_host_san")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", EMU, "-o", exe, SRC])
    subprocess.check_call([exe, "pick"], stdout=subprocess.DEVNULL)
    for mix, seed, n in ((0, 5, 500), (2, 9, 500), (25, 1, 500)):
        subprocess.check_call([exe, str(seed), "0", str(n), "0", str(mix), str(tmp_path / "o.bin")])
