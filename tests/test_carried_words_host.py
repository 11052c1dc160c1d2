"""CPU-side proof of the carried words of k_play_wide's trick-aligned card loop (tarok_device.h: FamilyWord, LeadWord, the
error bit and the seat's smears inside the observation carry, apply_step<.., .., CARRIED>): what only changes with the game or
with the trick is kept from card to card, and every overload that takes such a word returns what the helper it replaces
returns.  The device header is compiled by g++ with the gfx950 builtins emulated (tests/host_emu/carried_words_host.cpp).
No GPU involved."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "host_emu")
SRC = os.path.join(EMU, "carried_words_host.cpp")
REC = np.dtype([("masks", np.uint64, 48), ("obs", np.uint64, 48), ("actions", np.uint8, 48), ("scores", np.int16, 4), ("nsteps", np.int16)])
GAMES = 3


@pytest.fixture(scope="module")
def host_binary(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu") / "carried_words_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-w", "-I", EMU, "-o", out, SRC])
    return out


def test_overloads_equal_the_helpers_they_replace(host_binary):
    """All ten contracts x every card led 0..53 x 48 random tricks (all four leaders, both error values, a twelfth trick in
    every sixth, Klop with 0..6 talon cards left), each walked on a clean and on a padded C plane: hands, legal masks, hi_sel,
    the observation word, and apply_step's result, planes, trick_info and over01, bit for bit."""
    out = subprocess.check_output([host_binary, "helpers"], text=True).split()
    tricks, cards, ended, gifts = int(out[0]), int(out[2]), int(out[4]), int(out[7])
    assert tricks == 10 * 54 * 48 and cards == 8 * tricks
    assert 0 < ended < tricks and gifts > 0


# the mixes of test_device_rules_host.py
@pytest.mark.parametrize("mix,seed,offset,episode", [(0, 5, 0, 0), (0, 123456789, 987654321, 3), (1, 7, 11, 1), (2, 9, 0, 0),
                                                      (16, 1, 0, 0), (23, 1, 0, 2), (25, 2, 5, 0), (24, 3, 0, 0)])
def test_games_in_a_row_equal_the_oracle(host_binary, tmp_path, mix, seed, offset, episode):
    """Three games in a row per slot by the host copy of the aligned trick sequence: carried words set in front of the loop,
    the per-game words set again where a finished game is replaced by a freshly set-up one (another contract, another error
    bit).  The program itself compares every card with the per-card helpers; here the games are compared with the oracle."""
    from oracle import oracle as O
    n = 1500
    path = str(tmp_path / "out.bin")
    subprocess.check_call([host_binary, str(seed), str(offset), str(n), str(episode), str(mix), str(GAMES), path])
    got = np.fromfile(path, dtype=REC).reshape(n, GAMES)
    t = np.arange(48)[None, :]
    err = (np.arange(n)[:, None] + np.arange(GAMES + 1)[None, :]) % 3 == 0        # the error bit game k of slot i starts with
    refs = [O.rollout(seed, offset, n, episode + k, mix) for k in range(GAMES)]
    contracts_change = False
    for k, ref in enumerate(refs):
        g = got[:, k]
        assert (g["nsteps"] == ref["nsteps"]).all()
        assert (g["scores"] == ref["scores"]).all()
        live = t < ref["nsteps"][:, None]
        m = ref["masks"].astype(np.uint64)
        assert (g["masks"][live] == m[live]).all()
        assert (g["actions"][live] == ref["actions"][live]).all()
        # the observation after card t: the mask and the seat of card t + 1, the position, no done bit, the game's error bit
        nxt = live[:, 1:]
        obs = g["obs"][:, :-1]
        assert ((obs & np.uint64((1 << 54) - 1))[nxt] == m[:, 1:][nxt]).all()
        assert (((obs >> np.uint64(54)) & np.uint64(3)).astype(np.int64)[nxt] == ref["seats"][:, 1:][nxt]).all()
        assert (((obs >> np.uint64(56)) & np.uint64(63)).astype(np.int64)[nxt] == np.broadcast_to(t[:, 1:], nxt.shape)[nxt]).all()
        assert ((obs >> np.uint64(62))[nxt] == np.broadcast_to(2 * err[:, k:k + 1].astype(np.uint64), nxt.shape)[nxt]).all()
        # the observation after the game's last card: done, and the NEXT game's first mask, leader and error bit
        last = g["obs"][np.arange(n), ref["nsteps"] - 1]
        assert ((last >> np.uint64(62)) == (1 + 2 * err[:, k + 1]).astype(np.uint64)).all()
        assert (((last >> np.uint64(56)) & np.uint64(63)) == 0).all()
        if k + 1 < GAMES:
            assert ((last & np.uint64((1 << 54) - 1)) == refs[k + 1]["masks"][:, 0].astype(np.uint64)).all()
            assert (((last >> np.uint64(54)) & np.uint64(3)).astype(np.int64) == refs[k + 1]["seats"][:, 0]).all()
            contracts_change = contracts_change or bool((refs[k + 1]["masks"][:, 0] != ref["masks"][:, 0]).any())
    assert contracts_change
    assert err[:, :GAMES].any() and (err[:, 1:] != err[:, :-1]).any()


def test_carried_words_under_address_and_ub_sanitizers(tmp_path):
    """The same stand-alone program with -fsanitize=address,undefined: the helper walk and 400 slots of three games."""
    exe = str(tmp_path / "carried_words_host_san")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", EMU, "-o", exe, SRC])
    subprocess.check_call([exe, "helpers"], stdout=subprocess.DEVNULL)
    for mix, seed in ((0, 5), (2, 9), (25, 1)):
        subprocess.check_call([exe, str(seed), "0", "400", "0", str(mix), str(GAMES), str(tmp_path / "o.bin")])
