"""CPU-side proof of redeal_voids (tarok_amd/csrc/tarok_device.h), the new step of the void-aware determinized playouts
(tarok_playout_cards_voids): the device header is compiled by g++ with the gfx950 builtins emulated
(tests/host_emu/redeal_voids_host.cpp) and what it makes of 2,000 synthetic games per mix and 4 worlds — the four hands,
the team, the seat the un-owned talon is parked on, and the scores of the world played out by the Bot — is compared with
the model on the oracle (tests/playout_voids_model.py), under three void words per game: the game's own (from the cards
played), the largest sound one (every class a seat truly lacks: forced cards and every group), and a random one (mostly
inconsistent: the fallbacks).  No GPU involved."""
import os
import subprocess

import numpy as np
import pytest

import playout_det_model as DM
import playout_model as PM
import playout_voids_model as VM
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "host_emu")
SRC = os.path.join(EMU, "redeal_voids_host.cpp")
WORLDS, VARIANTS = 4, 3
REC = np.dtype([("in_play", np.uint8), ("mover", np.uint8), ("played", np.uint8), ("pad", np.uint8, 5),
                ("hands", np.uint64, (VARIANTS, WORLDS, 4)), ("team", np.uint8, (VARIANTS, WORLDS)),
                ("park", np.uint8, (VARIANTS, WORLDS)), ("scores", np.int16, (VARIANTS, WORLDS, 4))])
SALT = 9
EPISODE = 2


@pytest.fixture(scope="module")
def host_binary(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu") / "redeal_voids_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-w", "-I", EMU, "-o", out, SRC])
    return out


def void_words(seed, n, mix, cards):
    """[n, 3] u32: own, largest sound, random (bits 20..31 set in some: they are ignored), and the games."""
    rnd = np.random.RandomState(1000 * mix + cards)
    words = np.zeros((n, VARIANTS), np.uint32)
    games = []
    for i in range(n):
        g, played, lead = VM.bot_game(seed, i, EPISODE, mix, cards)
        games.append(g)
        words[i] = (VM.shown_voids(played, lead), VM.true_voids(g), int(rnd.randint(0, 1 << 20)) & int(rnd.randint(0, 1 << 20)) | (i % 3 == 0) << 25)
    return words, games


@pytest.mark.parametrize("mix,seed,cards", [(0, 5, 13), (1, 7, 22), (2, 9, 34), (16, 1, 22), (23, 1, 5), (19, 3, 30), (2, 2, 46)])
def test_redeal_voids_equals_the_model(host_binary, tmp_path, mix, seed, cards):
    n = 2000
    words, games = void_words(seed, n, mix, cards)
    vpath, path = str(tmp_path / "voids.bin"), str(tmp_path / "out.bin")
    words.tofile(vpath)
    subprocess.check_call([host_binary, str(seed), "0", str(n), str(EPISODE), str(mix), str(cards), str(SALT), vpath, path])
    got = np.fromfile(path, dtype=REC)
    assert got.shape == (n,)
    seen = 0
    constrained = [0] * VARIANTS              # worlds that differ from the plain re-deal's
    for i in range(n):
        g = games[i]
        in_play, seat, _, played = PM.position(g)
        assert bool(got["in_play"][i]) == in_play
        if not in_play:
            assert not got["hands"][i].any() and not got["team"][i].any()
            continue
        assert (got["mover"][i], got["played"][i]) == (seat, played)
        seen += 1
        for v in range(VARIANTS):
            for w in range(WORLDS):
                wkey = DM.world_key(seed, SALT, i, EPISODE, played, w)
                world = VM.world_of(g, wkey, int(words[i, v]))
                hands = [int(world.g.hand[s]) for s in range(4)]
                assert [int(x) for x in got["hands"][i, v, w]] == hands, (i, v, w)
                if v < 2:                                   # a sound word holds in every world
                    for s in range(4):
                        if s != seat:
                            assert not hands[s] & VM.class_cards((int(words[i, v]) >> (5 * s)) & 31), (i, v, w, s)
                plain = DM.world_of(g, wkey)
                constrained[v] += hands != [int(plain.g.hand[s]) for s in range(4)]
                team = int(world.g.team)
                assert int(got["team"][i, v, w]) == team, (i, v, w)
                park = int(got["park"][i, v, w])
                assert park != 254, "the un-owned talon cards sit on different seats"
                if park != 255 and team not in (0, 15):
                    assert not (team >> park) & 1, (i, v, w, team, park)
                q = played
                while not world.done:
                    assert world.step(O.policy_action(wkey, q, world.legal())) >= 0
                    q += 1
                assert [int(x) for x in got["scores"][i, v, w]] == world.scores, (i, v, w)
    assert seen >= 100
    if 13 <= cards <= 34:                       # (at 46 cards one or two cards are unseen: nothing to constrain)
        assert constrained[0] > seen // 4 and constrained[1] > seen, (seen, constrained)


def test_redeal_voids_under_address_and_ub_sanitizers(tmp_path):
    """The same stand-alone program with -fsanitize=address,undefined on 500 games of four mixes."""
    exe = str(tmp_path / "redeal_voids_host_san")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", EMU, "-o", exe, SRC])
    for mix, seed, cards in ((0, 5, 13), (2, 9, 22), (16, 1, 47), (25, 1, 9)):
        words, _ = void_words(seed, 500, mix, cards)
        vpath = str(tmp_path / "v.bin")
        words.tofile(vpath)
        subprocess.check_call([exe, str(seed), "0", "500", str(EPISODE), str(mix), str(cards), "3", vpath, str(tmp_path / "o.bin")])
