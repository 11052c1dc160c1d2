"""CPU-side proof of the `on` words and bounds of tarok_playout_exchange_net_list / tarok_playout_bids_net_list
(exchange_list_on, bid_list_on and their bounds, tarok_amd/csrc/tarok_device.h): the device header is compiled by g++
(tests/host_emu/front_list_host.cpp) and the program checks, for every contract family, sets 1..8, every `contracts` value,
every seat set and both pass_value, that (unit, row, world) -> slot is a bijection onto [0, total) that ascends in (game,
group or viewer, row, world), and that the total stays within the host's bound.  A stand-alone program; no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "host_emu")
SRC = os.path.join(EMU, "front_list_host.cpp")
CASES = 8 * 3 + 0x3FF * 2 * 2 * 17


def run(exe):
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0, (out.stdout, out.stderr)
    assert out.stdout.strip() == "ok %d" % CASES, out.stdout


def test_the_lists_are_bijections_in_unit_row_world_order(tmp_path):
    exe = str(tmp_path / "front_list_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-w", "-I", EMU, "-o", exe, SRC])
    run(exe)


def test_the_lists_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "front_list_host_san")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", EMU, "-o", exe, SRC])
    run(exe)
