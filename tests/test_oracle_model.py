"""CPU: the test infrastructure of tests/test_gpu_output_contract.py checked on its own, without a GPU.

  * the per-slot model (tests/oracle_model.py) against the games RECORDED FROM THE REFERENCE
    (tests/golden/traces_v1.npz): its trick, done, reward and history rows are the reference run's;
  * its game_of hook (a slot whose next game is a given one: tests/test_gpu_front_rows.py): nothing changes without it,
    the Bot's line reproduces the synthetic run, a fronted game (tests/front_lines_model.py) changes it;
  * the guard-band checker (tests/guarded.py) reports a flipped byte in either guard and in a padding column;
  * the case table of the GPU file covers every allowed pair of values of two different axes.
"""
import itertools
import os

import numpy as np
import pytest

import output_contract_cases as G
from guarded import SENTINEL_BYTE, Guarded, assert_guards_intact
from oracle import encoder_spec as E
from oracle import oracle as O
from oracle import tarok_spec as S
from oracle_model import SlotModel


@pytest.fixture(scope="module")
def traces(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "traces_v1.npz")))


def trace_game(tr, i):
    g = O.Game(tr["deals"][i], tr["contract"][i], tr["declarer"][i], tr["king"][i])
    if g.g.phase == 1:
        assert g.exchange(tr["choice"][i], tr["discards"][i][: S.N_DISCARD[int(tr["contract"][i])]]) == 0
    return g


@pytest.mark.parametrize("reward_ref", [False, True])
def test_model_rows_are_the_reference_runs(traces, reward_ref):
    """Every recorded game replayed through the model, all ten contracts: the trick row is 0x8000 | trick_value << 4 |
    trick_winner on every 4th card and 0 elsewhere, done is at nsteps - 1, reward is the fixture's scores (with
    reward_ref: rezultat_igre_st_tock of them), the history is the fixture's cards, the observation word carries the
    fixture's next legal mask and seat."""
    tr = traces
    seen = set()
    for i in range(len(tr["contract"])):
        c, decl, ns = int(tr["contract"][i]), int(tr["declarer"][i]), int(tr["nsteps"][i])
        m = SlotModel(0, i, S.MIX_ALL, game=trace_game(tr, i))
        for t in range(ns):
            row = m.card(int(tr["actions"][i, t]), auto=False, reward_ref=reward_ref)
            assert not row.rejected and row.action == tr["actions"][i, t] and row.hist_pos == t, (i, t)
            if t % 4 == 3:
                k = t // 4
                assert row.trick == 0x8000 | (int(tr["trick_value"][i, k]) << 4) | int(tr["trick_winner"][i, k]), (i, t, c)
            else:
                assert row.trick == 0, (i, t)
            assert row.done == (1 if t == ns - 1 else 0), (i, t, c)
            if t < ns - 1:
                assert row.reward is None
                assert row.obs & S.DECK == int(tr["masks"][i, t + 1]) and (row.obs >> 54) & 3 == tr["seats"][i, t + 1], (i, t)
                assert (row.obs >> 56) & 63 == t + 1 and row.obs >> 62 == 0, (i, t)
            else:
                scores = [int(x) for x in tr["scores"][i]]
                left = 12 - ns // 4                        # cards left in every hand when the game ended
                exp = [E.rezultat_igre_st_tock(scores[s], E.TIP_IZBIRE[c], s == decl, left) for s in range(4)] if reward_ref else scores
                assert row.reward == exp, (i, c, row.reward, exp)
                assert row.obs & S.DECK == 0 and (row.obs >> 62) & 1 == 1, i
        assert m.played == ns and m.hist[:ns] == tr["actions"][i, :ns].tolist(), i
        assert m.sum == [int(x) for x in tr["scores"][i]], i    # the score sums stay the plain scores
        # once the game is over every card is rejected: no done, no trick, no history byte, the state as it was
        before = m.g.lanes()
        row = m.card(int(tr["actions"][i, 0]), auto=False, reward_ref=reward_ref)
        assert row.rejected and (row.done, row.trick, row.reward, row.hist_pos) == (0, 0, None, None) and (m.g.lanes() == before).all()
        seen.add(c)
    assert seen == set(range(10))
    berac = np.isin(tr["contract"], (7, 9))
    assert (tr["nsteps"][berac] < 48).any() and (tr["nsteps"][berac] == 48).any()      # both defender rewards of reward_ref occur


def test_model_rejects_illegal_and_garbage_cards(traces):
    """A card outside the legal mask, or no card id at all: done 0, trick 0, no history byte, the error bit, the state
    otherwise unchanged; the next legal card plays on."""
    tr = traces
    for i in range(0, len(tr["contract"]), 97):
        m = SlotModel(0, i, S.MIX_ALL, game=trace_game(tr, i))
        for t in range(min(6, int(tr["nsteps"][i]))):
            legal = int(tr["masks"][i, t])
            for bad in ([b for b in range(54) if not (legal >> b) & 1][0], 54, 200, 255):
                before = m.g.lanes()
                row = m.card(bad)
                after = m.g.lanes()
                assert row.rejected and (row.action, row.done, row.trick, row.reward, row.hist_pos) == (bad, 0, 0, None, None)
                assert row.obs >> 63 == 1 and row.obs & S.DECK == legal
                assert (before[:9] == after[:9]).all() and after[9] == before[9] | np.uint64(1 << 54)
            assert not m.card(int(tr["actions"][i, t])).rejected


def test_model_auto_reset_starts_the_next_game_at_history_row_0():
    """Synthetic slots through several auto-resets: the game after a finish is episode + 1 of the slot, the observation
    word of the finishing card describes it and keeps DONE, and its first card is history row 0 again."""
    for mix in (S.MIX_ALL, S.MIX_FIXED + 7):
        for i in range(40):
            m = SlotModel(9, i, mix)
            finished = 0
            for t in range(160):
                ep = m.ep
                row = m.card(None, auto=True)
                if row.done:
                    finished += 1
                    nxt = O.Game.synth(9, i, ep + 1, mix)
                    assert m.ep == ep + 1 and m.played == 0 and (m.g.lanes() == nxt.lanes()).all()
                    assert row.obs == nxt.obs_word(True) and (row.obs >> 62) & 1 and (row.obs >> 56) & 63 == 0
                    assert m.card(None, auto=True).hist_pos == 0
            assert finished >= 3


def _run_rows(m, cards=144, reward_ref=False):
    """`cards` auto-reset cards of the Bot policy: every field of every row, and the model's state after each card."""
    out = []
    for _ in range(cards):
        r = m.card(None, auto=True, reward_ref=reward_ref)
        out.append((r.action, r.done, r.reward, r.trick, r.obs, r.hist_pos, r.rejected, m.ep, m.played, list(m.sum),
                    [int(x) for x in m.g.lanes()]))
    return out


def test_model_without_a_hook_is_unchanged():
    """game_of=None and a hook that always answers None: the synthetic games, row for row, and the hook is asked once
    per game with the slot's index and the game's episode."""
    for mix in (S.MIX_ALL, S.MIX_BOT):
        for i in (0, 5, 9077):
            asked = []
            plain, hooked = SlotModel(9, i, mix), SlotModel(9, i, mix, game_of=lambda index, ep: asked.append((index, ep)))
            assert _run_rows(plain) == _run_rows(hooked)
            assert asked == [(i, e) for e in range(plain.ep + 1)] and plain.ep >= 3
            assert plain.key == S.game_key(9, i, plain.ep) == hooked.key


def test_model_hook_with_the_bot_line_is_the_synthetic_run():
    """A hook that hands out front_lines_model.bot_line (what deal_into_buffer writes for MIX_BOT) with the line's key:
    the run of the synthetic games, row for row, over three games and more."""
    import front_lines_model as FM
    for i in range(9000, 9012):
        hook = lambda index, ep: (FM.bot_line(9, index, ep, S.MIX_BOT), S.game_key(9, index, ep)) if ep > 0 else None
        plain, hooked = SlotModel(9, i, S.MIX_BOT), SlotModel(9, i, S.MIX_BOT, game_of=hook)
        for reward_ref in (False, True):
            assert _run_rows(plain, 96, reward_ref) == _run_rows(hooked, 96, reward_ref), i
        assert plain.ep >= 3
    with pytest.raises(AssertionError):                     # a game under another key than its line's is refused
        SlotModel(9, 9000, S.MIX_BOT, game_of=lambda index, ep: (FM.bot_line(9, index, ep, S.MIX_BOT), S.game_key(9, index, ep + 1)))


def test_model_hook_with_fronted_games_differs_from_the_bots():
    """A hook that hands out front_lines_model.front_game on the integer weight sets of tests/test_front_lines_cpu.py:
    each game starts as that game, and the run differs from the Bot's."""
    import front_lines_model as FM
    import front_lines_cpu_cases as FC
    bid = dict(W=FC.model_weights(1), scale=70.0, playouts=1, margin=0, contracts=0x3FF, pass_value=False)
    Wx = FC.model_weights(2)
    differ = 0
    for i in (FC.GIDX, FC.GIDX + 1):
        started = {}

        def hook(index, ep):
            if ep == 0:
                return None
            started[ep] = FM.front_game(FC.SEED, index, ep, 15, S.MIX_BOT, bid=bid, exchange=Wx).lanes()
            return FM.front_game(FC.SEED, index, ep, 15, S.MIX_BOT, bid=bid, exchange=Wx), S.game_key(FC.SEED, index, ep)
        plain, hooked = SlotModel(FC.SEED, i, S.MIX_BOT), SlotModel(FC.SEED, i, S.MIX_BOT, game_of=hook)
        rows = []
        for t in range(144):
            ep = hooked.ep
            r = hooked.card(None, auto=True)
            rows.append(r)
            if r.done:                                      # the finishing card's observation word describes the fronted game
                g = O.Game.from_lanes(started[ep + 1])
                assert hooked.ep == ep + 1 and hooked.played == 0 and (hooked.g.lanes() == started[ep + 1]).all()
                assert r.obs == g.obs_word(True)
        assert len(started) >= 3
        mine = [(r.action, r.done, r.reward, r.trick, r.obs) for r in rows]
        bots = [x[:5] for x in _run_rows(plain)]
        first_game = next(t for t, r in enumerate(rows) if r.done)
        assert mine[:first_game] == bots[:first_game], "episode 0 is the slot's own game under either"
        differ += mine != bots
    assert differ > 0


def test_guard_checker_reports_one_flipped_byte():
    """tests/guarded.py on a CPU buffer: intact after legitimate writes into the columns [0, n); one flipped byte in the
    front guard, in the back guard or in a padding column [n, stride) is reported with its place."""
    import torch
    for dt, inner in ((np.uint8, ()), (np.uint16, ()), (np.int16, (4,)), (np.uint64, ())):
        a = Guarded("out", 5, 63, dt, inner=inner, stride=63 + 192, device="cpu")
        assert a.guard_bytes >= 4096 and a.guard_bytes >= a.row_bytes and a.violations() == []
        vals, written = a.host()
        assert vals.shape == (5, 63) + inner and not written.any()
        view = a.payload().view(5, a.stride, a.elem)
        view[:, :63, :] = 0                                    # what a correct launch does: every own column of every row
        view[2, 10, :] = SENTINEL_BYTE                         # ... but one element left alone
        a._host = None
        vals, written = a.host()
        assert a.violations() == [] and written.sum() == 5 * 63 - 1 and not written[2, 10] and (vals[written] == 0).all()
        assert_guards_intact([a, None])
        gb, pb = a.guard_bytes, a.payload_bytes
        for where, off in (("front guard", gb - 1), ("front guard", 0), ("back guard", gb + pb), ("back guard", 2 * gb + pb - 1),
                           ("padding columns", gb + 63 * a.elem), ("padding columns", gb + pb - 1)):
            keep = int(a.raw[off])
            a.raw[off] = keep ^ 0x01
            a._host = None
            v = a.violations()
            assert len(v) == 1 and v[0][0] == "out: " + where and v[0][2] == keep ^ 0x01, (dt, where, off, v)
            with pytest.raises(AssertionError):
                assert_guards_intact([a])
            a.raw[off] = keep
            a._host = None
            assert a.violations() == []
        assert torch.equal(a.raw[:gb], torch.full((gb,), SENTINEL_BYTE, dtype=torch.uint8))


def test_card_output_readers_fail_on_an_unwritten_element_and_a_differing_row():
    """tests/gpu_harness.py's readers on CPU buffers of n = 3 games: fully written outputs read back; one unwritten word of
    sum_out or one unwritten byte of action_out fails; assert_cards_equal passes on equal arrays and fails on one differing
    sum row and on one differing card."""
    import gpu_harness as H
    n = 3

    def written(skip_word=None, skip_byte=None):
        g_sum, g_act = H.card_outputs(n, ("sum", "action"), device="cpu")
        words = g_sum.payload().view(n * 12 * 4, 4)
        for w in range(n * 12 * 4):
            if w != skip_word:
                words[w] = 0
        g_sum.payload()[0] = 7                                 # (game 0, card 0, seat 0: 7 points)
        for g in range(n):
            if g != skip_byte:
                g_act.payload()[g] = 20 + g
        g_sum._host = g_act._host = None
        return g_sum, g_act
    sums, acts = H.read_cards(*written())
    assert sums.shape == (n, 12, 4) and sums.dtype == np.int32 and sums[0, 0, 0] == 7 and sums.sum() == 7
    assert acts.dtype == np.uint8 and acts.tolist() == [20, 21, 22]
    assert H.read_cards(written()[0], None)[1] is None and H.read_cards(None, written()[1])[0] is None
    with pytest.raises(AssertionError, match="a word of sum_out was not written"):
        H.read_cards(*written(skip_word=(1 * 12 + 5) * 4 + 2))
    with pytest.raises(AssertionError, match="a byte of action_out was not written"):
        H.read_cards(*written(skip_byte=2))
    H.assert_cards_equal(sums, sums.copy(), acts, acts.copy(), "equal")
    other = sums.copy()
    other[2, 11, 3] += 1
    with pytest.raises(AssertionError, match="sums differ"):
        H.assert_cards_equal(other, sums, acts, acts, "one sum row")
    card = acts.copy()
    card[1] = 255
    with pytest.raises(AssertionError, match="cards differ"):
        H.assert_cards_equal(sums, sums, card, acts, "one card")


def test_case_table_covers_every_allowed_pair():
    """Every pair of values of two different axes that the API allows (G.allowed over the full cross product) occurs
    in at least one case of the committed table; the cases themselves are allowed, well-formed and distinct."""
    fields = G.FIELDS
    for case in G.CASES:
        assert len(case) == len(fields) and all(v in G.AXES[f] for f, v in zip(fields, case)), case
        assert G.allowed(case), case
    assert len(set(G.CASES)) == len(G.CASES)

    def pairs(case):
        return {(fields[a], case[a], fields[b], case[b]) for a in range(len(fields)) for b in range(a + 1, len(fields))}
    need = set()
    for case in itertools.product(*[G.AXES[f] for f in fields]):
        if G.allowed(case):
            need |= pairs(case)
    have = set()
    for case in G.CASES:
        have |= pairs(case)
    missing = sorted(need - have, key=str)
    assert not missing, "allowed pairs without a case: %s" % missing
    # what the predicate rules out is what the header rules out, no more
    ruled_out = {p for case in itertools.product(*[G.AXES[f] for f in fields]) for p in pairs(case)} - need
    for f1, v1, f2, v2 in ruled_out:
        assert f1 == "kind" and ((f2 == "stride" and v2 == "N+192" and not v1.startswith("krog:")) or
                                 (f2 == "trick" and v2 == "given" and v1.startswith("run:")) or
                                 (f2 == "action" and v2 == "null")), (f1, v1, f2, v2)
    # the sizes that are modelled in full, and the thinned one
    assert all(len(G.modelled_slots(n)) == n for n in (1, 63, 257, 773))
    s = G.modelled_slots(20077)
    assert set(range(64)) <= set(s) and set(range(20077 - 64, 20077)) <= set(s) and set(range(0, 20077, 29)) <= set(s) and len(s) < 900
