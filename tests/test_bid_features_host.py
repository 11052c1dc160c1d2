"""CPU-side proof of bid_feature_words (tarok_amd/csrc/tarok_device.h), the input row of tarok_bid_values: the header is
compiled by g++ with the gfx950 builtins emulated (tests/host_emu/bid_features_host.cpp) and the four feature words of
every seat of 2,000 of the device's own deals are compared with the model (tests/bid_head_model.py on the oracle's
deal); once more as a stand-alone program under the address and undefined-behaviour sanitizers.  No GPU involved."""
import os
import subprocess

import numpy as np
import pytest

import bid_head_model as HM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "host_emu")
SRC = os.path.join(EMU, "bid_features_host.cpp")
EPISODE = 3


@pytest.fixture(scope="module")
def host_binary(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu") / "bid_features_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-w", "-I", EMU, "-o", out, SRC])
    return out


@pytest.mark.parametrize("seed,offset", [(4, 0), (6, 12345)])
def test_the_device_code_equals_the_model(host_binary, tmp_path, seed, offset):
    n = 2000
    path = str(tmp_path / "out.bin")
    subprocess.check_call([host_binary, str(seed), str(offset), str(n), str(EPISODE), path])
    got = np.fromfile(path, dtype=np.uint64).reshape(n, 4, 4)
    taroks, kings = set(), 0
    for i in range(n):
        perm = HM.own_deal(seed, offset + i, EPISODE)
        want = HM.game_words(perm)
        assert [[int(x) for x in row] for row in got[i]] == want, i
        for v in range(4):
            taroks.add(bin(want[v][1] & 0xFFF).count("1"))
            kings += bin((want[v][1] >> 48) & 15).count("1")
    # coverage of the inputs (a king may lie in the talon): short and long tarok holdings, most kings in hands
    assert 3 * n < kings <= 4 * n and min(taroks) <= 1 and max(taroks) >= 9


def test_under_address_and_ub_sanitizers(tmp_path):
    """The same stand-alone program (its own main, nothing preloaded) with -fsanitize=address,undefined on 300 deals."""
    exe = str(tmp_path / "bid_features_host_san")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", EMU, "-o", exe, SRC])
    subprocess.check_call([exe, "4", "0", "300", "1", str(tmp_path / "o.bin")])
    subprocess.check_call([exe, "9", "7", "300", "2", str(tmp_path / "o.bin")])
