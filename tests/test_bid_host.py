"""CPU-side proof of the device code of tarok_playout_bids and tarok_bid_round (tarok_amd/csrc/tarok_device.h): the
header is compiled by g++ with the gfx950 builtins emulated (tests/host_emu/bid_host.cpp) and what it makes of 2,000
deals x 4 viewers x 2 worlds — bid_world's hands and talon slots, the viewer's score of one row per world played out as
the kernel's item does, and bid_round's contract, declarer and king on synthetic sums for the seat sets 0, 15 and one
seat — is compared with the model on the oracle (tests/playout_bids_model.py).  The program itself checks that a world
keeps the viewer's hand, the sizes and the deck.  No GPU involved."""
import os
import subprocess

import numpy as np
import pytest

import playout_bids_model as BM
from oracle import tarok_spec as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "host_emu")
SRC = os.path.join(EMU, "bid_host.cpp")
WORLDS = 2
REC = np.dtype([("hands", np.uint64, (4, WORLDS, 4)), ("talon", np.uint64, (4, WORLDS)), ("score", np.int16, (4, WORLDS)),
                ("bid", np.int8, (3, 3)), ("pad", np.uint8, 7)])
SALT = 5
EPISODE = 3


@pytest.fixture(scope="module")
def host_binary(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu") / "bid_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-w", "-I", EMU, "-o", out, SRC])
    return out


def synthetic_sums(key):
    return [[S.rng32(key, 200 + 20 * v + r) % 41 - 20 if r < BM.OPTIONS else 0 for r in range(BM.ROWS)] for v in range(4)]


def mask(cards):
    m = 0
    for c in cards:
        m |= 1 << c
    return m


@pytest.mark.parametrize("seed,contracts,threshold", [(4, BM.ALL_CONTRACTS, 0), (6, BM.DEFAULT_CONTRACTS, -5)])
def test_the_device_code_equals_the_model(host_binary, tmp_path, seed, contracts, threshold):
    n = 2000
    path = str(tmp_path / "out.bin")
    subprocess.check_call([host_binary, str(seed), "0", str(n), str(EPISODE), str(SALT), str(contracts), str(threshold), path])
    got = np.fromfile(path, dtype=REC)
    assert got.shape == (n,)
    seen_contracts, seen_declarers = set(), set()
    for i in range(n):
        key = S.game_key(seed, i, EPISODE)
        perm = S.deal(key)
        for v in range(4):
            for w in range(WORLDS):
                world = BM.world_of(perm, v, BM.world_key(seed, SALT, i, EPISODE, v, w))
                assert [int(x) for x in got["hands"][i, v, w]] == [mask(world[12 * s:12 * s + 12]) for s in range(4)], (i, v, w)
                assert [(int(got["talon"][i, v, w]) >> (6 * j)) & 63 for j in range(6)] == world[48:], (i, v, w)
                r = (i + 5 * v + 11 * w) % 19
                assert int(got["score"][i, v, w]) == BM.one_playout(world, v, r, BM.playout_key(seed, SALT, i, EPISODE, v, r, w, 0)), (i, v, w, r)
        sums = synthetic_sums(key)
        for s, seats in enumerate((0, 15, 1 << (i & 3))):
            exp = BM.bid_round(key, sums, 1, threshold, contracts, seats)
            assert tuple(int(x) for x in got["bid"][i, s]) == exp, (i, seats)
            if s == 2:                                                   # (four playout bidders on random sums always end at the top)
                seen_contracts.add(exp[0])
                seen_declarers.add(exp[1])
        c, d, k = S.sample_setup(key, S.MIX_BOT)
        assert tuple(int(x) for x in got["bid"][i, 0]) == (c, d, max(k, 0)), i
    assert len(seen_contracts) >= 3 and seen_declarers == {0, 1, 2, 3}


def test_under_address_and_ub_sanitizers(tmp_path):
    """The same stand-alone program (its own main, nothing preloaded) with -fsanitize=address,undefined on 300 deals."""
    exe = str(tmp_path / "bid_host_san")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", EMU, "-o", exe, SRC])
    subprocess.check_call([exe, "4", "0", "300", "1", "3", str(BM.ALL_CONTRACTS), "0", str(tmp_path / "o.bin")])
    subprocess.check_call([exe, "9", "7", "300", "2", "0", str(BM.DEFAULT_CONTRACTS), "2", str(tmp_path / "o.bin")])
