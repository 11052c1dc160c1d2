"""CPU-side proof of halve_alive and best_alive (tarok_amd/csrc/tarok_device.h), the two new rules of
tarok_playout_cards_halving: the device header is compiled by g++ with the gfx950 builtins emulated
(tests/host_emu/halving_host.cpp) and its results on 6,000 random rows with planted ties, k = 1..12 alive ranks, are
compared with the sort of tests/playout_halving_model.py.  A stand-alone program; no GPU involved."""
import os
import subprocess

import numpy as np

import playout_halving_model as HM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "host_emu")
SRC = os.path.join(EMU, "halving_host.cpp")
REC = np.dtype([("row", np.int32, (12, 4)), ("alive", np.uint32), ("seat", np.uint32), ("out", np.uint32), ("best", np.uint32)])


def bits(m):
    return [j for j in range(12) if (int(m) >> j) & 1]


def check(exe, tmp_path, seed, n):
    path = str(tmp_path / "out.bin")
    subprocess.check_call([exe, str(seed), str(n), path])
    got = np.fromfile(path, dtype=REC)
    assert got.shape == (n,)
    ties = 0
    for r in got:
        alive, v = bits(r["alive"]), r["row"][:, int(r["seat"])]
        assert bits(r["out"]) == HM.survivors(v, alive), (r["row"].tolist(), alive)
        assert int(r["best"]) == min(alive, key=lambda j: (-int(v[j]), j))
        ties += len({int(v[j]) for j in alive}) < len(alive)
    return got, ties


def test_the_device_rule_equals_the_sort(tmp_path):
    exe = str(tmp_path / "halving_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-w", "-I", EMU, "-o", exe, SRC])
    got, ties = check(exe, tmp_path, 7, 6000)
    assert ties > 2000                                                   # the planted ties are there
    assert {len(bits(m)) for m in got["alive"]} == set(range(1, 13))
    assert {len(bits(m)) for m in got["out"]} == {1, 2, 3, 4, 5, 6}


def test_the_device_rule_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "halving_host_san")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", EMU, "-o", exe, SRC])
    check(exe, tmp_path, 3, 500)
