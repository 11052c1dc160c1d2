"""CPU-side proof of the role function of tarok_playout_cards_net_versus (net_versus_role and its siblings,
tarok_amd/csrc/tarok_device.h): the device header is compiled by g++ (tests/host_emu/net_versus_host.cpp) and the program's
table — the role for all 4 x 4 x 16 x 16 (viewer, mover, own_rel, opp_rel) — is compared with tests/playout_net_versus_model.py,
the refused pairs with the overlap of the two sets, the viewer networks with the model's.  A stand-alone program; no GPU."""
import os
import subprocess

import playout_net_versus_model as XM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "host_emu")
SRC = os.path.join(EMU, "net_versus_host.cpp")


def run(exe):
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0, (out.stdout, out.stderr)
    lines = out.stdout.split()
    assert len(lines) == 16 + 1 + 2 and lines[-2:] == ["ok", str(4 * 4 * 16 * 16)], lines[-3:]
    roles = 0
    for viewer in range(4):
        for mover in range(4):
            row = lines[viewer * 4 + mover]
            assert len(row) == 256
            for own in range(16):
                for opp in range(16):
                    got = int(row[own * 16 + opp])
                    if own & opp:
                        assert got == 9, (viewer, mover, own, opp)
                    else:
                        assert got == XM.role(viewer, mover, own, opp), (viewer, mover, own, opp)
                        roles += 1
    assert roles == 16 * 81                           # 3^4 disjoint pairs of sets
    assert [int(c) for c in lines[16]] == [XM.viewer_net(opp) for opp in range(16)]


def test_the_roles_are_the_models(tmp_path):
    exe = str(tmp_path / "net_versus_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-w", "-I", EMU, "-o", exe, SRC])
    run(exe)


def test_the_roles_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "net_versus_host_san")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", EMU, "-o", exe, SRC])
    run(exe)
