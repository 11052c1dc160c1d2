"""CPU-side proof of exchange_feature_words, exchange_choice and exchange_select (tarok_amd/csrc/tarok_device.h), the input
rows and the decision of tarok_exchange_values: the header is compiled by g++ with the gfx950 builtins emulated
(tests/host_emu/exchange_features_host.cpp) and, on 2,000 of the device's own deals under each of the six exchange
contracts, the four feature words of all eight rows, the chosen group and the discards are compared with the model
(tests/exchange_head_model.py on the oracle's game); once more as a stand-alone program under the address and
undefined-behaviour sanitizers.  No GPU involved."""
import os
import subprocess

import numpy as np
import pytest

import exchange_head_model as EM
from oracle import oracle as O
from oracle import tarok_spec as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "host_emu")
SRC = os.path.join(EMU, "exchange_features_host.cpp")
EPISODE = 3
REC = np.dtype([("words", "<u8", (8, 4)), ("y", "<f4", (8, 64)), ("choice", "<u4"), ("dpk", "<u4"), ("cand", "<u4", (2,))])


@pytest.fixture(scope="module")
def host_binary(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu") / "exchange_features_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-w", "-I", EMU, "-o", out, SRC])
    return out


@pytest.mark.parametrize("seed,offset", [(4, 0), (6, 12345)])
def test_the_device_code_equals_the_model(host_binary, tmp_path, seed, offset):
    n = 2000
    path = str(tmp_path / "out.bin")
    subprocess.check_call([host_binary, str(seed), str(offset), str(n), str(EPISODE), path])
    got = np.fromfile(path, dtype=REC).reshape(n, 6)
    king_where, fallback, odd_choice = set(), 0, 0
    for i in range(n):
        perm = S.deal(S.game_key(seed, offset + i, EPISODE))
        for c in range(1, 7):
            r = got[i, c - 1]
            game = O.Game(perm, c, (i + c) % 4, (i // 4 + c) % 4 if c <= 3 else -1)
            want = EM.game_words(game)
            assert [[int(x) for x in row] for row in r["words"]] == want, (i, c)
            gs, ngroups = S.GROUP_SIZE[c], 6 // S.GROUP_SIZE[c]
            choice = EM.choice_of(r["y"], ngroups)
            assert int(r["choice"]) == choice, (i, c)
            pickup = want[choice][0] & S.DECK
            cand = pickup if i % 8 == 7 else EM.candidate_mask(pickup, gs)
            assert int(r["cand"][0]) | (int(r["cand"][1]) << 32) == cand, (i, c)
            assert [(int(r["dpk"]) >> (8 * j)) & 255 for j in range(3)] == EM.XM.padded(EM.select(r["y"][choice], cand, gs)), (i, c)
            king_where.add((want[0][2] >> 54) & 7)
            fallback += cand != pickup & S.DISCARDABLE
            odd_choice += bool(np.isnan(r["y"][:ngroups, 54]).any())
    # coverage: the called king seen in the group, in the hand and in the rest of the talon (and nowhere: another hand);
    # whole-hand candidate masks; value columns with a NaN among them
    assert king_where == {0, 1, 2, 4} and fallback >= n // 8 and odd_choice > 100


def test_under_address_and_ub_sanitizers(tmp_path):
    """The same stand-alone program (its own main, nothing preloaded) with -fsanitize=address,undefined on 300 deals."""
    exe = str(tmp_path / "exchange_features_host_san")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", EMU, "-o", exe, SRC])
    subprocess.check_call([exe, "4", "0", "300", "1", str(tmp_path / "o.bin")])
    subprocess.check_call([exe, "9", "7", "300", "2", str(tmp_path / "o.bin")])
