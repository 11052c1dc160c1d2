"""TEST INFRASTRUCTURE — the statement of tarok_playout_cards_net_voids and tarok_playout_cards_net_hidden
(include/tarok_env.h) on the CPU oracle.

tests/playout_net_model.py with the world swapped: world w of a game is tests/playout_voids_model.world_of under the
game's void word, or tests/playout_hidden_model.world_for under its word of played cards, for the seat to move.  The keys
are tests/playout_det_model.py's, the playouts are played by playout_net_model.play_out; all of it is imported, nothing
is restated here and nothing comes from the code under test.
"""
import numpy as np

import playout_det_model as DM
import playout_hidden_model as HM
import playout_model as PM
import playout_net_model as NM
import playout_voids_model as VM
from oracle import oracle as O

RANKS = PM.RANKS
KINDS = ("voids", "hidden")


def world_of(kind, game, wkey, word):
    """World wkey of `game` as its mover sees it, under the game's word of the kind."""
    if kind == "voids":
        return VM.world_of(game, wkey, int(word))
    assert kind == "hidden"
    return HM.world_for(game, wkey, int(word), game.seat())


def items_of(kind, lanes, episode, seed, salt, gidx, seats, worlds, word):
    """playout_net_model.items_of in the worlds of `kind`: [(rank j, world w, the world's Game with the candidate
    applied, its playout key)]."""
    game = O.Game.from_lanes(lanes)
    if not PM.takes_part(game, seats):
        return []
    _, _, legal, played = PM.position(game)
    out = []
    for w in range(worlds):
        world = world_of(kind, game, DM.world_key(seed, salt, gidx, episode, played, w), word)
        assert world.legal() == legal and world.seat() == game.seat()
        for j, c in enumerate(PM.cards_of(legal)):
            h = PM.copy_of(world)
            assert h.step(c) >= 0
            out.append((j, w, h, DM.playout_key(seed, salt, gidx, episode, played, c, w, 0)))
    return out


def playout_scores(kind, games, seed, salt, seats, worlds, W, net_seats, words, pick=NM.greedy):
    """games: [(lanes, episode, gidx, seat set or None)], words: one per game -> scores [n, 12, worlds, 4] int64."""
    out = np.zeros((len(games), RANKS, worlds, 4), np.int64)
    where, hs, keys = [], [], []
    for g, (lanes, ep, gidx, s) in enumerate(games):
        for j, w, h, key in items_of(kind, lanes, ep, seed, salt, gidx, seats if s is None else s, worlds, words[g]):
            where.append((g, j, w)); hs.append(h); keys.append(key)
    for (g, j, w), sc in zip(where, NM.play_out(hs, keys, W, net_seats, pick)):
        out[g, j, w] = sc
    return out


def playout_cards(kind, games, seed, salt, seats, worlds, W, net_seats, words, pick=NM.greedy):
    """(sum [n, 12, 4] int64, cards [n] uint8): the whole statement; the card rule is tarok_playout_cards'."""
    sums = playout_scores(kind, games, seed, salt, seats, worlds, W, net_seats, words, pick).sum(axis=2)
    acts = np.array([PM.card_of(lanes, seed, gidx, ep, seats if s is None else s, sums[g])
                     for g, (lanes, ep, gidx, s) in enumerate(games)], np.uint8)
    return sums, acts


def bot_games(kind, seed, episode, mix, n, cards, first=0):
    """What a test env holds after `cards` Bot cards, rebuilt on the oracle: ([(lanes, episode, gidx, None)], the games'
    own words of the kind — tarok_shown_voids' / tarok_played_cards' — and the oracle Games)."""
    games, words, objs = [], [], []
    for gidx in range(first, first + n):
        if kind == "voids":
            g, played, lead = VM.bot_game(seed, gidx, episode, mix, cards)
            word = VM.shown_voids(played, lead) if PM.position(g)[0] else 0
        else:
            g, word = HM.bot_game(seed, gidx, episode, mix, cards)
        games.append((g.lanes(), episode, gidx, None)); words.append(word); objs.append(g)
    return games, words, objs


def constrains(kind, game, word):
    """Does the word change the worlds of this position?  voids: a void of a seat other than the mover; hidden: a
    non-empty hidden discard set ("discards") or live Klop talon cards ("talon"), else None."""
    in_play = PM.position(game)[0]
    if not in_play:
        return None
    if kind == "voids":
        return "voids" if any((int(word) >> (5 * o)) & 31 for o in DM.others_of(game.seat())) else None
    if int(game.g.contract) == HM.KLOP and int(game.g.talon_left) > 0:
        return "talon"
    return "discards" if HM.hidden_discards(game, game.seat(), int(word)) else None
