"""CPU-side checks of the observation-feature statement (tests/observe_model.py), no GPU in here:

  a. on the 2,880 games recorded from the reference (tests/golden/traces_v1.npz) every region the recording can speak
     about — legal cards, mover, table, trick number, hands, taken cards — is tied to what the reference did;
  b. a census of the positions tests/test_gpu_observe_features.py compares (tests/observe_cases.py): every value of
     every flag field occurs among them, so no comparison there is vacuous;
  c. mutants of the statement, each caught by (a) or on the positions of (b);
  d. TarokVecEnv.expand_feature_words against expand().
"""
import os

import numpy as np
import pytest

import observe_cases as OC
import observe_model as OM
from oracle import oracle as O
from oracle import tarok_spec as S

DECK = OM.DECK
MODEL = OM.Statement()


@pytest.fixture(scope="module")
def traces(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "traces_v1.npz")))


@pytest.fixture(scope="module")
def census():
    return OC.census_positions()


def bits_of(cards):
    m = 0
    for c in cards:
        m |= 1 << int(c)
    return m


def trace_game(tr, i):
    g = O.Game(tr["deals"][i], tr["contract"][i], tr["declarer"][i], tr["king"][i])
    if g.g.phase == OM.PHASE_EXCHANGE:
        assert g.exchange(tr["choice"][i], tr["discards"][i][: S.N_DISCARD[int(tr["contract"][i])]]) == 0
    return g


def check_trace(tr, i, st):
    """Game i of the recording, every step: the words of statement `st` against what the reference recorded."""
    contract, n = int(tr["contract"][i]), int(tr["nsteps"][i])
    talon = [int(c) for c in tr["deals"][i][48:54]]
    nd = S.N_DISCARD[contract]
    g = trace_game(tr, i)
    declarer = int(g.g.declarer)
    taken_now = bits_of(tr["discards"][i][:nd])            # before the first card: the declarer's discards, nothing else
    last_hand, last_card = {}, {}
    for t in range(n):
        before = OC.copy_of(g)
        a = int(tr["actions"][i, t])
        assert g.step(a) == (1 if t == n - 1 else 0)
        w = st.words(before, g)
        flags = [x >> 54 for x in w]
        where = (i, t, contract)
        assert w[1] & DECK == int(tr["masks"][i, t]), ("legal region", where)
        rel = flags[1] & 15
        assert rel in (1, 2, 4, 8) and (declarer - rel.bit_length() + 1) & 3 == int(tr["seats"][i, t]), ("mover", where)
        mover = int(tr["seats"][i, t])
        assert (flags[1] >> 4) & 15 == 1 << (t % 4), ("table count", where)
        assert w[2] & DECK == bits_of(tr["actions"][i, t - t % 4:t]), ("table region", where)
        assert (flags[2] >> 4) & 15 == t // 4, ("trick number", where)
        assert flags[0] == 1 << contract and flags[3] == 1 and (flags[1] >> 9) & 1 == (1 if 1 <= contract <= 3 else 0), ("flags", where)
        assert flags[2] & 15 == ((1 << int(tr["king"][i])) if 1 <= contract <= 3 else 0), ("king suit", where)
        hand = w[0] & DECK
        if mover in last_hand:
            assert last_hand[mover] == hand | (1 << last_card[mover]) and not (hand >> last_card[mover]) & 1, ("hand region", where)
        else:
            assert bin(hand).count("1") == 12, ("hand region", where)
        assert (hand >> a) & 1
        last_hand[mover], last_card[mover] = hand, a
        if t % 4 == 0 and t > 0:                           # a trick was completed: it went to a pile, with Klop's gift
            k = t // 4 - 1
            gift = (1 << talon[5 - k]) if contract == S.KLOP and k < 6 else 0
            taken_now |= bits_of(tr["actions"][i, t - 4:t]) | gift
        assert w[3] & DECK == taken_now, ("taken region", where)
    # the last step plus one: the finished game
    w = st.words(g, None)
    assert g.done and w[1] & DECK == 0 and w[3] >> 54 == 0 and w[2] & DECK == 0, ("finished row", i)
    k = n // 4
    taken_now |= bits_of(tr["actions"][i, n - 4:n]) | ((1 << talon[5 - (k - 1)]) if contract == S.KLOP and k - 1 < 6 else 0)
    assert w[3] & DECK == taken_now == int(np.bitwise_or.reduce(tr["piles"][i])), ("taken at the end", i)
    mover = (declarer - (w[1] >> 54 & 15).bit_length() + 1) & 3
    assert w[0] & DECK == int(tr["hands_end"][i, mover]), ("hand at the end", i)
    others = int(np.bitwise_or.reduce(tr["hands_end"][i]))
    if contract == S.KLOP:
        unowned = bits_of(talon[:max(0, 6 - k)])
    elif nd:
        gs, ch = S.GROUP_SIZE[contract], int(tr["choice"][i])
        unowned = bits_of(talon) & ~bits_of(talon[ch * gs:(ch + 1) * gs])
    else:
        unowned = bits_of(talon)
    assert (w[0] & DECK) | others | (w[3] & DECK) | unowned == DECK, ("the whole deck", i)
    if n == 48:
        assert w[0] & DECK == 0 and (w[3] & DECK) | unowned == DECK and (w[2] >> 58) & 15 == 12, ("after 12 tricks", i)


def check_traces(tr, st, games=None):
    for i in (range(len(tr["contract"])) if games is None else games):
        check_trace(tr, i, st)


def test_statement_on_the_reference_traces(traces):
    """(a) all 2,880 recorded games, every step."""
    check_traces(traces, MODEL)
    assert set(int(c) for c in traces["contract"]) == set(range(10)) and len(traces["contract"]) == 2880


def facts_of(game):
    g = game.g
    nt = int(g.n_in_trick)
    seat = (int(g.leader) + nt) & 3
    return dict(contract=int(g.contract), table=nt, trick=int(g.trick_no), rel=(int(g.declarer) - seat) & 3,
                team=(int(g.team) >> seat) & 1, king=int(g.king), phase=int(g.phase))


def test_census_of_the_compared_positions(census):
    """(b) what the rows of the GPU comparison cover: every value of every field, every (contract, table count) pair."""
    facts = [facts_of(b) for _, b, _ in census]
    play = [f for f in facts if f["phase"] == OM.PHASE_PLAY]
    seen = lambda name, rows=play: set(f[name] for f in rows)
    assert seen("contract") == set(range(10))
    assert seen("table") == {0, 1, 2, 3}
    assert seen("trick") == set(range(12))
    assert set((f["contract"], f["table"]) for f in play) == set((c, k) for c in range(10) for k in range(4))
    assert seen("rel") == {0, 1, 2, 3}
    assert seen("team") == {0, 1}
    assert seen("king") == {-1, 0, 1, 2, 3}
    assert seen("phase", facts) == {OM.PHASE_EXCHANGE, OM.PHASE_PLAY, OM.PHASE_DONE}
    wait = [f for f in facts if f["phase"] == OM.PHASE_EXCHANGE]
    done = [f for f in facts if f["phase"] == OM.PHASE_DONE]
    assert set(f["contract"] for f in wait) == set(range(1, 7))                # every contract with an exchange waits
    assert set(f["contract"] for f in done) == set(range(10))
    assert 12 in set(f["trick"] for f in done) and min(f["trick"] for f in done) < 12   # (a Berac that ended early)
    # the whole-game runs see renewed games' first tricks beside last tricks in one lock-step, and Klop's gifts
    whole = [(what, b, a) for what, b, a in census if what.startswith("whole:")]
    assert any(int(b.g.trick_no) == 11 and int(b.g.n_in_trick) == 3 and int(a.g.trick_no) == 0 for _, b, a in whole)
    assert any(int(b.g.contract) == S.KLOP and 0 < int(b.g.talon_left) < 6 for _, b, _ in whole)


# ---- (c) mutants: one part of the statement replaced by a wrong one
class TableShifted(OM.Statement):
    def table_onehot(self, nt):
        return 1 << ((nt + 1) & 3)


class TrickAfterRenewal(OM.Statement):
    def trick_number(self, game, after):
        return int((game if after is None else after).g.trick_no)


class TeamOfDeclarer(OM.Statement):
    def team_bit(self, game, seat):
        return (int(game.g.team) >> int(game.g.declarer)) & 1


class TakenWithoutGift(OM.Statement):
    def taken(self, game):
        g = game.g
        gifts = 0
        if int(g.contract) == S.KLOP:
            for j in range(int(g.talon_left), 6):
                gifts |= 1 << int(g.talon[j])
        return OM.Statement.taken(self, game) & ~gifts


class LegalWhileWaiting(OM.Statement):
    def legal(self, game):
        g = game.g
        if g.phase == OM.PHASE_EXCHANGE:
            return int(O.lib().to_legal_navadna(int(g.hand[int(g.leader)]), -1))
        return OM.Statement.legal(self, game)


class LiveWhenFinished(OM.Statement):
    def live(self, game):
        return 1 if game.g.phase in (OM.PHASE_PLAY, OM.PHASE_DONE) else 0


def caught_by_traces(tr, st):
    try:
        check_traces(tr, st)
    except AssertionError:
        return True
    return False


def caught_by_census(census, st):
    return any(st.words(b, a) != MODEL.words(b, a) for _, b, a in census)


@pytest.mark.parametrize("mutant,by_traces,by_census", [
    (TableShifted, True, True), (TrickAfterRenewal, True, True), (TeamOfDeclarer, False, True), (TakenWithoutGift, True, True),
    (LegalWhileWaiting, False, True), (LiveWhenFinished, True, True)])
def test_mutants_are_caught(traces, census, mutant, by_traces, by_census):
    """Each wrong statement fails (a), differs from the statement on a position of (b), or both, as listed.  (The
    recording holds no waiting game and says nothing about teams: those two are the census's alone.)"""
    st = mutant()
    assert caught_by_census(census, st) == by_census
    if by_traces:                                          # (a survivor would cost a full pass: not run where none is expected)
        assert caught_by_traces(traces, st)
    assert by_traces or by_census


def test_trick_after_renewal_differs_at_the_last_card(census):
    """The row that mutant is about: the 48th card of a game on an auto-reset env, where the renewed game is at trick 0."""
    st = TrickAfterRenewal()
    rows = [(b, a) for what, b, a in census if a is not None and int(b.g.trick_no) == 11 and int(b.g.n_in_trick) == 3]
    assert rows and all((st.words(b, a)[2] >> 58) & 15 == 0 and (MODEL.words(b, a)[2] >> 58) & 15 == 11 for b, a in rows)


# ---- (d) the expansion
def test_expand_feature_words_equals_expand():
    import torch
    from tarok_amd import TarokVecEnv
    rng = np.random.default_rng(5)
    w = rng.integers(0, 1 << 64, size=(300, 4), dtype=np.uint64)
    w[:20] |= np.uint64(0x3FF << 54)                       # all ten flag bits set
    w[20:24] = 0
    w[24:28] = np.uint64((1 << 64) - 1)
    x = OM.expand(w)
    assert x.shape == (300, 256) and x.dtype == np.float64 and set(np.unique(x)) == {0.0, 1.0}
    assert x[:20].reshape(20, 4, 64)[:, :, 54:].all() and x[24:28].all() and not x[20:24].any()
    for f in (0, 53, 54, 63, 64, 200, 255):                # (spelled out: feature f is bit f % 64 of word f // 64)
        assert (x[:, f] == ((w[:, f // 64] >> np.uint64(f % 64)) & np.uint64(1))).all()
    t = torch.from_numpy(w.view(np.int64))
    for dtype in (torch.bfloat16, torch.float64):
        got = TarokVecEnv.expand_feature_words(t, dtype)
        assert got.dtype == dtype and tuple(got.shape) == (300, 256) and (got.double().numpy() == x).all()
    raw = TarokVecEnv.expand_feature_words(t).view(torch.int16).numpy().view(np.uint16)
    assert (OM.from_bf16(raw) == x).all()
    assert OM.expand([[1, 2, 1 << 63, 0]]).sum() == 3      # lists of Python ints, as the playout models pass them


def test_from_bf16_takes_the_two_patterns_only():
    ok = np.array([[0x0000, 0x3F80] * 128], np.uint16)
    assert (OM.from_bf16(ok) == np.array([[0.0, 1.0] * 128])).all()
    for bad in (0x8000, 0x3F81, 0x3F00, 0x0001, 0xA5A5, 0x7FC0):
        raw = ok.copy()
        raw[0, 77] = bad
        with pytest.raises(AssertionError):
            OM.from_bf16(raw)
