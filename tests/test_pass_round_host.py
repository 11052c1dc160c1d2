"""CPU-side proof of the device code of tarok_playout_bids_pass and tarok_bid_round_pass (tarok_amd/csrc/tarok_device.h):
the header is compiled by g++ with the gfx950 builtins emulated (tests/host_emu/pass_round_host.cpp) and what it makes of
1,000 deals x 4 viewers x 2 worlds — pass_round's contract, declarer and king under the key of row 19, the viewer's score
of the pass playout played as the kernel's item plays it, and the pass-aware bid_round's three outputs on synthetic sums
with a live row 19 for the seat sets 0, 15 and one seat — is compared with the model on the oracle
(tests/playout_pass_model.py).  The program itself checks that with row 19 zeroed the pass-aware round is bid_round at
threshold = margin.  No GPU involved; the sanitizer run is the same stand-alone program, nothing is loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

import playout_bids_model as BM
import playout_pass_model as PS
from oracle import tarok_spec as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "host_emu")
SRC = os.path.join(EMU, "pass_round_host.cpp")
WORLDS = 2
REC = np.dtype([("round", np.int8, (4, WORLDS, 3)), ("score", np.int16, (4, WORLDS)), ("bid", np.int8, (3, 3)), ("pad", np.uint8, 7)])
SALT = 5
EPISODE = 3


@pytest.fixture(scope="module")
def host_binary(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu") / "pass_round_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-w", "-I", EMU, "-o", out, SRC])
    return out


def synthetic_sums(key):
    return [[S.rng32(key, 200 + 20 * v + r) % 41 - 20 for r in range(BM.ROWS)] for v in range(4)]


@pytest.mark.parametrize("seed,contracts,margin,playouts", [(4, BM.ALL_CONTRACTS, 0, 1), (6, BM.DEFAULT_CONTRACTS, -3, 2), (7, 0x2AB, 4, 1)])
def test_the_device_code_equals_the_model(host_binary, tmp_path, seed, contracts, margin, playouts):
    n = 1000
    path = str(tmp_path / "out.bin")
    subprocess.check_call([host_binary, str(seed), "0", str(n), str(EPISODE), str(SALT), str(contracts), str(margin), str(playouts), path])
    got = np.fromfile(path, dtype=REC)
    assert got.shape == (n,)
    rounds, bids, scored = set(), set(), 0
    for i in range(n):
        key = S.game_key(seed, i, EPISODE)
        perm = S.deal(key)
        for v in range(4):
            for w in range(WORLDS):
                pkey = PS.pass_key(seed, SALT, i, EPISODE, v, w, i % 3)
                want = PS.pass_round(pkey, v)
                assert tuple(int(x) for x in got["round"][i, v, w]) == want, (i, v, w)
                rounds.add((v,) + want[:2])
                world = BM.world_of(perm, v, BM.world_key(seed, SALT, i, EPISODE, v, w))
                score = PS.one_pass_playout(world, v, pkey)
                assert int(got["score"][i, v, w]) == score, (i, v, w)
                scored += score != 0
        sums = synthetic_sums(key)
        for s, seats in enumerate((0, 15, 1 << (i & 3))):
            exp = PS.bid_round(key, sums, playouts, margin, contracts, seats)
            assert tuple(int(x) for x in got["bid"][i, s]) == exp, (i, seats)
            bids.add(exp[:2])
        c, d, k = S.sample_setup(key, S.MIX_BOT)
        assert tuple(int(x) for x in got["bid"][i, 0]) == (c, d, max(k, 0)), i
    # every seat is seen muted with every other seat declaring, seat 0 with its forced Klop, and the playouts score
    assert {(v, d) for v, _, d in rounds} >= {(v, d) for v in range(4) for d in range(4) if d != v} | {(0, 0)}
    assert len({c for _, c, _ in rounds}) == 4 and scored > n // 4 and len({c for c, _ in bids}) >= 3


def test_under_address_and_ub_sanitizers(tmp_path):
    """The same stand-alone program (its own main, nothing preloaded) with -fsanitize=address,undefined on 300 deals."""
    exe = str(tmp_path / "pass_round_host_san")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", EMU, "-o", exe, SRC])
    subprocess.check_call([exe, "4", "0", "300", "1", "3", str(BM.ALL_CONTRACTS), "0", "1", str(tmp_path / "o.bin")])
    subprocess.check_call([exe, "9", "7", "300", "2", "0", str(BM.DEFAULT_CONTRACTS), "-30", "16", str(tmp_path / "o.bin")])
