"""CPU-side proof of redeal_hidden (tarok_amd/csrc/tarok_device.h), the one new step of tarok_playout_cards_hidden: the
device header is compiled by g++ with the gfx950 builtins emulated (tests/host_emu/redeal_hidden_host.cpp) and what it
makes of synthetic games — the four hands, the four won piles, the talon ids, the team, the seat the un-owned talon is
parked on, and the scores of the world played out by the Bot (through score_game and Klop's gifts) — is compared with
the model on the oracle (tests/playout_hidden_model.py): 2,000 games of each of Klop and the six exchange contracts x 2
worlds at 0, 5 and 23 cards, 500 games of Berac and Solo_brez.  No GPU involved."""
import os
import subprocess

import numpy as np
import pytest

import playout_det_model as DM
import playout_hidden_model as HM
import playout_model as PM
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "host_emu")
SRC = os.path.join(EMU, "redeal_hidden_host.cpp")
WORLDS = 2
REC = np.dtype([("in_play", np.uint8), ("mover", np.uint8), ("played", np.uint8), ("pad", np.uint8, 5), ("word", np.uint64),
                ("hands", np.uint64, (WORLDS, 4)), ("piles", np.uint64, (WORLDS, 4)), ("talon", np.uint64, WORLDS),
                ("team", np.uint8, WORLDS), ("park", np.uint8, WORLDS), ("pad2", np.uint8, 4), ("scores", np.int16, (WORLDS, 4))])
SALT = 9
EPISODE = 2
FIXED = 16                                                   # MIX_FIXED + contract code
KLOP, BERAC, SOLO_BREZ = 0, 7, 8


@pytest.fixture(scope="module")
def host_binary(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu") / "redeal_hidden_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-w", "-I", EMU, "-o", out, SRC])
    return out


def compare(host_binary, tmp_path, contract, seed, cards, n):
    mix = FIXED + contract
    path = str(tmp_path / "out.bin")
    subprocess.check_call([host_binary, str(seed), "0", str(n), str(EPISODE), str(mix), str(cards), str(SALT), path])
    got = np.fromfile(path, dtype=REC)
    assert got.shape == (n,)
    seen = wider = 0
    for i in range(n):
        g, word = HM.bot_game(seed, i, EPISODE, mix, cards)
        in_play, seat, _, played = PM.position(g)
        assert bool(got["in_play"][i]) == in_play
        if not in_play:
            assert not got["hands"][i].any() and not got["team"][i].any()
            continue
        assert (got["mover"][i], got["played"][i], int(got["word"][i])) == (seat, played, word)
        seen += 1
        for w in range(WORLDS):
            wkey = DM.world_key(seed, SALT, i, EPISODE, played, w)
            world = HM.world_for(g, wkey, word)
            assert [int(x) for x in got["hands"][i, w]] == [int(world.g.hand[s]) for s in range(4)], (i, w)
            assert [int(x) for x in got["piles"][i, w]] == [int(world.g.pile[s]) for s in range(4)], (i, w)
            assert int(got["talon"][i, w]) == sum(int(world.g.talon[j]) << (6 * j) for j in range(6)), (i, w)
            team = int(world.g.team)
            assert int(got["team"][i, w]) == team, (i, w)
            wider += (any(int(world.g.pile[s]) != int(g.g.pile[s]) for s in range(4))
                      or any(int(world.g.talon[j]) != int(g.g.talon[j]) for j in range(6)))
            park = int(got["park"][i, w])
            assert park != 254, "the un-owned talon cards sit on different seats"
            if park != 255 and team not in (0, 15):
                assert not (team >> park) & 1, (i, w, team, park)
            q = played
            while not world.done:
                assert world.step(O.policy_action(wkey, q, world.legal())) >= 0
                q += 1
            assert [int(x) for x in got["scores"][i, w]] == world.scores, (i, w)
    return seen, wider


@pytest.mark.parametrize("cards", [0, 5, 23])
@pytest.mark.parametrize("contract", [0, 1, 2, 3, 4, 5, 6])
def test_redeal_hidden_equals_the_model(host_binary, tmp_path, contract, cards):
    n = 2000
    seen, wider = compare(host_binary, tmp_path, contract, 3 + contract, cards, n)
    assert seen == n
    assert wider > n // 2                                     # the worlds do move the talon / the discards


@pytest.mark.parametrize("contract,cards", [(BERAC, 5), (SOLO_BREZ, 5)])
def test_nothing_more_is_hidden_in_berac_and_solo_brez(host_binary, tmp_path, contract, cards):
    seen, wider = compare(host_binary, tmp_path, contract, 11, cards, 500)
    assert seen >= 100 and wider == 0


def test_redeal_hidden_under_address_and_ub_sanitizers(tmp_path):
    """The same stand-alone program with -fsanitize=address,undefined, run directly, on 500 games of five contracts."""
    exe = str(tmp_path / "redeal_hidden_host_san")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", EMU, "-o", exe, SRC])
    for contract, seed, cards in ((0, 5, 0), (0, 5, 23), (1, 9, 5), (3, 1, 47), (5, 2, 22), (7, 1, 3)):
        subprocess.check_call([exe, str(seed), "0", "500", "1", str(FIXED + contract), str(cards), "3", str(tmp_path / "o.bin")])
