"""CPU-side proof of the slot arithmetic of tarok_playout_cards_net_halving's compacted item list (net_list_slot and its
siblings, tarok_amd/csrc/tarok_device.h): the device header is compiled by g++ (tests/host_emu/net_halving_host.cpp) and
the program checks, for every `on` word of 12 bits and W_r in {1, 2, 7, 16, 64}, that a game's slots are a bijection onto
[0, popc(on) * W_r) in (rank, world) order, and that the alive bounds are 12, 6, 3, 2.  A stand-alone program; no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "host_emu")
SRC = os.path.join(EMU, "net_halving_host.cpp")


def run(exe):
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0, (out.stdout, out.stderr)
    assert out.stdout.strip() == "ok %d" % (5 * 4096), out.stdout


def test_the_slots_are_a_bijection_in_rank_world_order(tmp_path):
    exe = str(tmp_path / "net_halving_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-w", "-I", EMU, "-o", exe, SRC])
    run(exe)


def test_the_slots_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "net_halving_host_san")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", EMU, "-o", exe, SRC])
    run(exe)
