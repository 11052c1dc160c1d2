"""CPU-side proof of the survivor rule, the bounds and the slot map of tarok_playout_exchange_net_halving /
tarok_playout_bids_net_halving (front_halving_stays, front_halving_alive, the two round bounds and front_halving_value,
tarok_amd/csrc/tarok_device.h): the device header is compiled by g++ (tests/host_emu/front_halving_host.cpp) and the program
checks the shared survivor function against a sort-based restatement for every alive count 1..48 with ties and random alive
masks, the keep count and stability on ties, a_r for a_0 in 1..48, that per round (unit, alive bit, world) -> slot is an
ascending bijection onto [0, total) within B_r, and the rounding of value_out.  A stand-alone program; no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "host_emu")
SRC = os.path.join(EMU, "front_halving_host.cpp")
CASES = 48 * 40 + 1 + 48 + 8 * 4 + 147 * 2 * 4 + 1


def run(exe):
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0, (out.stdout, out.stderr)
    assert out.stdout.strip() == "ok %d" % CASES, out.stdout


def test_the_survivor_rule_the_bounds_and_the_slot_map(tmp_path):
    exe = str(tmp_path / "front_halving_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-w", "-I", EMU, "-o", exe, SRC])
    run(exe)


def test_the_same_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "front_halving_host_san")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", EMU, "-o", exe, SRC])
    run(exe)
