"""CPU-side proof of the item numbering of tarok_playout_cards_net_sampled (net_sampled_slot and its siblings,
tarok_amd/csrc/tarok_device.h): the device header is compiled by g++ (tests/host_emu/net_sampled_host.cpp), and the program —
which walks every (rank, world, sample) of every small shape and of the corner shapes, splitting each slot and putting it
together again — prints per shape a checksum that is compared with the header's formula, item = ((g * 12 + j) * worlds + w)
* samples + k, computed here.  A stand-alone program, also under the address and undefined-behaviour sanitizers; no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "host_emu")
SRC = os.path.join(EMU, "net_sampled_host.cpp")
SHAPES = [(w, s) for w in range(1, 9) for s in range(1, 9)] + [(64, 1024), (1, 1024), (64, 1)]


def checksum(worlds, samples):
    return sum((j + 13 * w + 1031 * k) * (((j * worlds + w) * samples + k) + 1) for j in range(12) for w in range(worlds) for k in range(samples))


def run(exe):
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0, (out.stdout, out.stderr)
    lines = out.stdout.strip().split("\n")
    assert len(lines) == len(SHAPES) + 2 and lines[-1] == "ok %d" % len(SHAPES), lines[-2:]
    for (worlds, samples), line in zip(SHAPES, lines):
        assert [int(x) for x in line.split()] == [worlds, samples, 12 * worlds * samples, checksum(worlds, samples)], (worlds, samples, line)
    n = 1 << 20
    assert [int(x) for x in lines[-2].split()] == [n * 12 * 160, -1, -1, 2730 * 12 * 65536]
    assert n * 12 * 160 < 2 ** 31 <= n * 12 * 176 and 2730 * 12 * 65536 < 2 ** 31 <= 2731 * 12 * 65536


def test_the_numbering_is_the_headers(tmp_path):
    exe = str(tmp_path / "net_sampled_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-w", "-I", EMU, "-o", exe, SRC])
    run(exe)


def test_the_numbering_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "net_sampled_host_san")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", EMU, "-o", exe, SRC])
    run(exe)
