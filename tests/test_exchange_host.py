"""CPU-side proof of the device code of tarok_playout_exchange (tarok_amd/csrc/tarok_device.h): the header is compiled
by g++ with the gfx950 builtins emulated (tests/host_emu/exchange_host.cpp) and what it makes of 2,000 synthetic games
per exchange contract and 2 worlds — exchange_discards' cards, and the hands, piles, team, parking seat and played-out
scores of the world after redeal_unseen (the DECLARER as the viewer, on a game that still waits: plane C holds the whole
talon) and the candidate's apply_exchange — is compared with the model on the oracle
(tests/playout_exchange_model.py).  The program itself checks that the re-deal touches only the pool's planes, the
parked talon and the team, and that exchange and re-deal commute.  No GPU involved."""
import os
import subprocess

import numpy as np
import pytest

import playout_exchange_model as XM
from oracle import oracle as O
from oracle import tarok_spec as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "host_emu")
SRC = os.path.join(EMU, "exchange_host.cpp")
WORLDS = 2
REC = np.dtype([("waiting", np.uint8), ("declarer", np.uint8), ("gs", np.uint8), ("bot_same", np.uint8),
                ("bot_disc", np.uint8, 3), ("pad", np.uint8), ("cand_i", np.uint8, WORLDS), ("cand_disc", np.uint8, (WORLDS, 3)),
                ("hands", np.uint64, (WORLDS, 4)), ("piles", np.uint64, (WORLDS, 4)), ("team", np.uint8, WORLDS),
                ("park", np.uint8, WORLDS), ("scores", np.int16, (WORLDS, 4))])
SALT = 9
EPISODE = 2


@pytest.fixture(scope="module")
def host_binary(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu") / "exchange_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-w", "-I", EMU, "-o", out, SRC])
    return out


@pytest.mark.parametrize("code,seed", [(S.TRI, 5), (S.DVE, 7), (S.ENA, 9), (S.SOLO_TRI, 1), (S.SOLO_DVE, 3), (S.SOLO_ENA, 2)])
def test_the_device_code_equals_the_model(host_binary, tmp_path, code, seed):
    n, mix = 2000, S.MIX_FIXED + code
    path = str(tmp_path / "out.bin")
    subprocess.check_call([host_binary, str(seed), "0", str(n), str(EPISODE), str(mix), str(SALT), path])
    got = np.fromfile(path, dtype=REC)
    assert got.shape == (n,)
    new_team = 0
    gs, ngroups = S.GROUP_SIZE[code], 6 // S.GROUP_SIZE[code]
    for i in range(n):
        g = XM.deferred_game(seed, i, EPISODE, mix)
        assert XM.waiting(g) and got["waiting"][i] == 1
        declarer = int(g.g.declarer)
        assert (got["declarer"][i], got["gs"][i]) == (declarer, gs)
        bot = XM.padded(XM.discards_under(g, 0, S.game_key(seed, i, EPISODE)))
        assert got["bot_disc"][i].tolist() == bot and got["bot_same"][i] == 1, i
        for w in range(WORLDS):
            ci, cd = w % ngroups, w
            disc = XM.discards_under(g, ci, XM.candidate_key(seed, SALT, i, EPISODE, ci, cd))
            assert got["cand_i"][i, w] == ci and got["cand_disc"][i, w].tolist() == XM.padded(disc), (i, w)
            wkey = XM.world_key(seed, SALT, i, EPISODE, w)
            world = XM.world_for(g, declarer, wkey)
            assert world.exchange(ci, disc) == 0
            assert [int(x) for x in got["hands"][i, w]] == [int(world.g.hand[s]) for s in range(4)], (i, w)
            assert [int(x) for x in got["piles"][i, w]] == [int(world.g.pile[s]) for s in range(4)], (i, w)
            team = int(world.g.team)
            assert int(got["team"][i, w]) == team, (i, w)
            new_team += team != int(g.g.team)
            park = int(got["park"][i, w])
            assert park not in (254, 255), "the un-owned talon cards sit together on one seat"
            assert not (team >> park) & 1 and all((team >> s) & 1 for s in range(park)), (i, w, team, park)
            q = 0
            while not world.done:
                assert world.step(O.policy_action(wkey, q, world.legal())) >= 0
                q += 1
            assert [int(x) for x in got["scores"][i, w]] == world.scores, (i, w)
    if code in (S.TRI, S.DVE, S.ENA):
        assert new_team > 500                                            # called king: many worlds move the partner
    else:
        assert new_team == 0


def test_under_address_and_ub_sanitizers(tmp_path):
    """The same stand-alone program (its own main, nothing preloaded) with -fsanitize=address,undefined, 300 games of
    each exchange contract."""
    exe = str(tmp_path / "exchange_host_san")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", EMU, "-o", exe, SRC])
    for code in (S.TRI, S.DVE, S.ENA, S.SOLO_TRI, S.SOLO_DVE, S.SOLO_ENA):
        subprocess.check_call([exe, "4", "0", "300", "1", str(S.MIX_FIXED + code), "3", str(tmp_path / "o.bin")])
