"""CPU-side proof of the two words k_play_wide's trick-aligned card loop carries from card to card instead of rebuilding
them (tarok_device.h): the premultiplied RNG counter (RngCtr: rng32 / policy_action / policy_action_follow on it) and
the seat and position bits of the observation word (obs_carry, obs_word_with on the carried word).  The device header is
compiled by g++ with the gfx950 builtins emulated (tests/host_emu/renewal_fetch_host.cpp).  No GPU involved."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "host_emu")
SRC = os.path.join(EMU, "renewal_fetch_host.cpp")
REC = np.dtype([("actions", np.uint8, 48), ("half", np.uint8, 48), ("nsteps", np.int16)])
EPISODES = 3


@pytest.fixture(scope="module")
def host_binary(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu") / "renewal_fetch_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-w", "-I", EMU, "-o", out, SRC])
    return out


def test_premultiplied_counter_draws_the_same_numbers(host_binary):
    """4,000 keys (the all-zero and all-one words among them), every position 0..47: rng32 on rng_ctr(128 + pos), and on
    a counter advanced by TK_RNG_STEP per card, equals rng32(key, 128 + pos)."""
    out = subprocess.check_output([host_binary, "rng"], text=True).split()
    assert int(out[0]) == 4000 * 48


@pytest.mark.parametrize("mix,seed", [(0, 5), (1, 7), (2, 9), (16, 1), (23, 1), (24, 3), (25, 2)])
def test_carried_words_along_oracle_games(host_binary, tmp_path, mix, seed):
    """1,000 slots, three consecutive games each (the words are carried across the renewal): the program itself compares
    the carried counter with the rebuilt one and the observation word from the carried half with obs_word_with's at every
    card; here the cards it drew and the seat / position bits it wrote are compared with the oracle's games."""
    from oracle import oracle as O
    n = 1000
    path = str(tmp_path / "out.bin")
    subprocess.check_call([host_binary, str(seed), "0", str(n), str(EPISODES), str(mix), path])
    got = np.fromfile(path, dtype=REC).reshape(n, EPISODES)
    t = np.arange(48)[None, :]
    cards = 0
    for e in range(EPISODES):
        ref = O.rollout(seed, 0, n, e, mix)
        g = got[:, e]
        assert (g["nsteps"] == ref["nsteps"]).all()
        live = t < ref["nsteps"][:, None]
        assert (g["actions"][live] == ref["actions"][live]).all()
        # after card t the word names the seat to play card t + 1 and the position t + 1 (bits 54..55 and 56..61)
        nxt = (t + 1) < ref["nsteps"][:, None]
        want = (ref["seats"][:, 1:].astype(np.int64) & 3) | (np.arange(1, 48)[None, :] << 2)
        assert (g["half"][:, :47][nxt[:, :47]] == want[nxt[:, :47]]).all()
        assert (g["half"][~nxt] == 255).all()
        cards += int(live.sum())
    assert cards >= 3 * 4 * n


def test_carried_words_under_address_and_ub_sanitizers(tmp_path):
    """The same stand-alone program with -fsanitize=address,undefined: the counter check and 300 slots of three mixes."""
    exe = str(tmp_path / "renewal_fetch_host_san")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", EMU, "-o", exe, SRC])
    subprocess.check_call([exe, "rng"], stdout=subprocess.DEVNULL)
    for mix, seed, n in ((0, 5, 300), (2, 9, 300), (25, 1, 300)):
        subprocess.check_call([exe, str(seed), "0", str(n), str(EPISODES), str(mix), str(tmp_path / "o.bin")])
