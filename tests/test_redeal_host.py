"""CPU-side proof of redeal_unseen (tarok_amd/csrc/tarok_device.h), the one new step of the determinized playouts
(tarok_playout_cards_det): the device header is compiled by g++ with the gfx950 builtins emulated
(tests/host_emu/redeal_host.cpp) and what it makes of 2,000 synthetic games per mix and 4 worlds — the four hands, the
team, the seat the un-owned talon is parked on, and the scores of the world played out by the Bot — is compared with the
model on the oracle (tests/playout_det_model.py).  No GPU involved."""
import os
import subprocess

import numpy as np
import pytest

import playout_det_model as DM
import playout_model as PM
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "host_emu")
SRC = os.path.join(EMU, "redeal_host.cpp")
WORLDS = 4
REC = np.dtype([("in_play", np.uint8), ("mover", np.uint8), ("played", np.uint8), ("pad", np.uint8, 5),
                ("hands", np.uint64, (WORLDS, 4)), ("team", np.uint8, WORLDS), ("park", np.uint8, WORLDS),
                ("scores", np.int16, (WORLDS, 4))])
SALT = 9
EPISODE = 2


@pytest.fixture(scope="module")
def host_binary(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu") / "redeal_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-w", "-I", EMU, "-o", out, SRC])
    return out


def played_on(seed, gidx, episode, mix, cards):
    g = O.Game.synth(seed, gidx, episode, mix)
    key = O.game_key(seed, gidx, episode)
    for q in range(cards):
        if g.done:
            break
        g.step(O.policy_action(key, q, g.legal()))
    return g


@pytest.mark.parametrize("mix,seed,cards", [(0, 5, 5), (1, 7, 0), (2, 9, 22), (16, 1, 2), (23, 1, 3), (24, 3, 1), (25, 2, 46)])
def test_redeal_unseen_equals_the_model(host_binary, tmp_path, mix, seed, cards):
    n = 2000
    path = str(tmp_path / "out.bin")
    subprocess.check_call([host_binary, str(seed), "0", str(n), str(EPISODE), str(mix), str(cards), str(SALT), path])
    got = np.fromfile(path, dtype=REC)
    assert got.shape == (n,)
    seen = hidden = moved = 0
    for i in range(n):
        g = played_on(seed, i, EPISODE, mix, cards)
        in_play, seat, _, played = PM.position(g)
        assert bool(got["in_play"][i]) == in_play
        if not in_play:
            assert not got["hands"][i].any() and not got["team"][i].any()
            continue
        assert (got["mover"][i], got["played"][i]) == (seat, played)
        seen += 1
        for w in range(WORLDS):
            wkey = DM.world_key(seed, SALT, i, EPISODE, played, w)
            world = DM.world_of(g, wkey)
            assert [int(x) for x in got["hands"][i, w]] == [int(world.g.hand[s]) for s in range(4)], (i, w)
            team = int(world.g.team)
            assert int(got["team"][i, w]) == team, (i, w)
            hidden += team != int(g.g.team)
            moved += any(int(world.g.hand[s]) != int(g.g.hand[s]) for s in range(4))
            park = int(got["park"][i, w])
            assert park != 254, "the un-owned talon cards sit on different seats"
            if park != 255 and team not in (0, 15):
                assert not (team >> park) & 1, (i, w, team, park)
            # the world played out by the Bot under the world key: the scores go through score_game and the parking
            q = played
            while not world.done:
                assert world.step(O.policy_action(wkey, q, world.legal())) >= 0
                q += 1
            assert [int(x) for x in got["scores"][i, w]] == world.scores, (i, w)
    assert seen >= (100 if mix in (0, 23, 25) else n)                   # (a Berac can be over early)
    if cards < 46:
        assert moved > seen                                   # the worlds do differ from the true deal
    if mix in (1, 2):                                         # Tri, Dve: called king, so some worlds change the team
        assert hidden > 50


def test_redeal_unseen_under_address_and_ub_sanitizers(tmp_path):
    """The same stand-alone program with -fsanitize=address,undefined on 500 games of four mixes."""
    exe = str(tmp_path / "redeal_host_san")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", EMU, "-o", exe, SRC])
    for mix, seed, cards in ((0, 5, 5), (2, 9, 22), (16, 1, 47), (25, 1, 3)):
        subprocess.check_call([exe, str(seed), "0", "500", "1", str(mix), str(cards), "3", str(tmp_path / "o.bin")])
