"""GPU: tarok_playout_bids_pass (the value of a pass by determinized playouts, row 19) and tarok_bid_round_pass (the round
with that row as the bar), and the surface built on them, checked exactly — integers against integers — against the
per-game model of tests/playout_pass_model.py.  Rows 0..18 are held byte for byte to tarok_playout_bids at the same
arguments; the round with row 19 zeroed byte for byte to tarok_bid_round.  All outputs sit inside guard bands
(tests/guarded.py).  A library without the new entries FAILS these tests: nothing here skips.

The advantage (tools/playout_pass_advantage.py) is a finding, not a bar: no sign or size is asserted.

Run on the GPU box:  python -m pytest tests/test_gpu_playout_pass.py -m gpu -q
"""
import ctypes as C
import functools

import numpy as np
import pytest

import gpu_harness as H
from gpu_harness import T, U, dev_u8  # noqa: F401  (T: the module fixture)

pytestmark = pytest.mark.gpu

SEED = 2
OFFSET = 3000                            # game offset of the envs: gidx = OFFSET + g
EPISODE = 4                              # the keys' episode field is not zero
DEFAULT, ALL = 0x00F, 0x3FF
_MODEL = {}                              # pass scores of the model, computed once per (deal, seats, sizes, salt)
make_env = functools.partial(H.make_bid_env, seed=SEED, offset=OFFSET)   # (T, n, **kw): NOT reset, bidding comes first
perms_of = functools.partial(H.perms_of, seed=SEED, offset=OFFSET, episode=EPISODE)


def launch_bids(env, worlds, samples, contracts=DEFAULT, deals=None, salt=0, seats=15, per_game=None, episode=EPISODE,
                entry="tarok_playout_bids_pass"):
    """One launch of `entry` into a guarded sum_out: [n, 4, 20] i32."""
    return H.launch_bids(env, worlds, samples, contracts, deals, salt, seats, per_game, episode=episode, entry=entry)


def launch_round(env, sums, playouts, margin=0, contracts=DEFAULT, seats=15, per_game=None, episode=EPISODE,
                 entry="tarok_bid_round_pass"):
    """One launch of `entry` into three guarded outputs: [n, 3] i8 (contract, declarer, king)."""
    return H.launch_round(env, sums, playouts, margin, contracts, seats, per_game, episode=episode, entry=entry)


def model_pass(perms, seats_of, worlds, samples, salt=0, seed=SEED, offset=OFFSET, episode=EPISODE):
    """Row 19 of the model, [n, 4]: every pass playout played on the oracle, once per argument set."""
    import playout_pass_model as PS
    out = np.zeros((len(perms), 4), np.int64)
    for g, perm in enumerate(perms):
        k = (tuple(int(c) for c in perm), int(seats_of[g]) & 15, worlds, samples, salt, seed, offset + g, episode)
        if k not in _MODEL:
            _MODEL[k] = PS.pass_scores(perm, episode, seed, salt, offset + g, k[1], worlds, samples).sum(axis=(1, 2))
        out[g] = _MODEL[k]
    return out


def check(env, perms, seats_of, worlds, samples, contracts=DEFAULT, salt=0, seats=15, per_game=None, deals=None, tag=None):
    """The pass launch: row 19 against the model, rows 0..18 byte for byte against tarok_playout_bids, whose row 19 is 0."""
    got = launch_bids(env, worlds, samples, contracts, deals, salt, seats, per_game)
    plain = launch_bids(env, worlds, samples, contracts, deals, salt, seats, per_game, entry="tarok_playout_bids")
    assert got[:, :, :19].tobytes() == plain[:, :, :19].tobytes(), (tag, "rows 0..18 differ from tarok_playout_bids")
    assert not plain[:, :, 19].any()
    want = model_pass(perms, seats_of, worlds, samples, salt)
    bad = np.nonzero((got[:, :, 19] != want).any(axis=1))[0]
    assert bad.size == 0, (tag, "row 19 differs", bad[:8], got[bad[0], :, 19].tolist(), want[bad[0]].tolist())
    return got


@pytest.mark.parametrize("n,worlds,samples,contracts", [(1, 1, 1, DEFAULT), (5, 4, 2, ALL), (16, 8, 2, DEFAULT), (33, 2, 1, DEFAULT),
                                                        (4, 64, 1, DEFAULT), (6, 2, 2, 0x001)])
def test_row_19_is_the_model_and_the_other_rows_are_tarok_playout_bids(T, n, worlds, samples, contracts):
    """(33 games at (2, 1): 16 lanes per game, 16 games per workgroup, a ragged third one; 0x001: the pass row rides with
    Klop alone.)"""
    env = make_env(T, n)
    try:
        got = check(env, perms_of(n), [15] * n, worlds, samples, contracts, salt=3, tag=(n, worlds, samples, contracts))
        if n >= 4:
            assert got[:, :, 19].any() and got[:, :, 0].any()
    finally:
        env.close()


def test_the_largest_samples(T):
    """2 games at samples = 1024: seat 0 views the first (its forced Klop among the playouts), seat 2 the second."""
    from tarok_amd import karte as K
    per_game = np.array([1, 4], np.uint8)
    env = make_env(T, 2)
    try:
        got = check(env, perms_of(2), per_game, 1, K.PLAYOUT_MAX_SAMPLES, DEFAULT, seats=0, per_game=per_game, tag="1024 samples")
        assert got[0, 0, 19] != 0 and not got[0, 1:].any() and not got[1, [0, 1, 3]].any()
    finally:
        env.close()


def test_deals_given_deals_null_and_an_invalid_row(T):
    n = 12
    rng = np.random.default_rng(5)
    own = np.array(perms_of(n), np.uint8)
    env = make_env(T, n)
    try:
        a = launch_bids(env, 2, 1, DEFAULT, deals=None, salt=2)
        b = launch_bids(env, 2, 1, DEFAULT, deals=own, salt=2)
        assert a.tobytes() == b.tobytes()
        other = np.stack([rng.permutation(54) for _ in range(n)]).astype(np.uint8)
        other[3, 7] = other[3, 8]                                        # a card twice
        other[9, 50] = 54                                                # no such card
        perms = [other[g].tolist() for g in range(n)]
        got = check(env, perms, [15] * n, 2, 1, DEFAULT, salt=2, deals=other, tag="deals given")
        assert not got[3].any() and not got[9].any() and got[0].any() and got[:, :, 19].any()
    finally:
        env.close()


def test_seat_sets_per_game(T):
    """Per-game sets with the empty set, seat 0 alone (the forced Klop) and seat 3 alone among them; bits above the seats
    are ignored."""
    n = 16
    perms = perms_of(n)
    per_game = np.array([0, 1, 8, 15, 6, 9] + [(5 * g + 3) & 15 for g in range(6, n)], np.uint8) | np.uint8(16)
    env = make_env(T, n)
    try:
        got = check(env, perms, per_game, 2, 2, DEFAULT, seats=15, per_game=per_game, tag="per game")
        for g in range(n):
            for v in range(4):
                if not (int(per_game[g]) >> v) & 1:
                    assert not got[g, v].any(), (g, v)
        for seats in (0, 1, 8):
            got = check(env, perms, [seats] * n, 2, 2, DEFAULT, seats=seats, tag=("seats", seats))
            assert got.any() == bool(seats)
        assert check(env, perms, [1] * n, 2, 2, DEFAULT, seats=1, tag="seat 0")[:, 0, 19].any()
    finally:
        env.close()


def test_read_only_deterministic_salted_and_batch_independent(T):
    n = 33
    env = make_env(T, n, history=True)
    try:
        env.reset(episode=1)
        for _ in range(9):
            env.step_random(auto_reset=False)
        before = (env.state().copy(), env.counters(), env.get_history().cpu().numpy())
        a = launch_bids(env, 2, 2, DEFAULT, salt=6)
        r = launch_round(env, a, 4)
        after = (env.state(), env.counters(), env.get_history().cpu().numpy())
        assert (before[0] == after[0]).all() and (before[2] == after[2]).all()
        assert (before[1][0] == after[1][0]).all() and (before[1][1] == after[1][1]).all()
        assert launch_bids(env, 2, 2, DEFAULT, salt=6).tobytes() == a.tobytes()
        assert (launch_round(env, a, 4) == r).all()
        assert (launch_bids(env, 2, 2, DEFAULT, salt=7)[:, :, 19] != a[:, :, 19]).any()
    finally:
        env.close()
    for g in (0, 17, 32):                                                # game g of the 33: the same gidx in an env of one game
        part = make_env(T, 1, offset=OFFSET + g)
        try:
            b = launch_bids(part, 2, 2, DEFAULT, salt=6)
            assert b.tobytes() == a[g:g + 1].tobytes()
            assert (launch_round(part, b, 4) == r[g:g + 1]).all()
        finally:
            part.close()


def model_round(sums, playouts, margin, contracts, seats_of, seed=SEED, offset=OFFSET, episode=EPISODE):
    import playout_pass_model as PS
    from oracle import tarok_spec as S
    return np.array([PS.bid_round(S.game_key(seed, offset + g, episode), sums[g].tolist(), playouts, margin, contracts,
                                  int(seats_of[g]) & 15) for g in range(len(sums))], np.int8)


def test_the_round_on_the_launchs_sums(T):
    n = 16
    env = make_env(T, n)
    try:
        got = check(env, perms_of(n), [15] * n, 8, 2, DEFAULT, salt=3, tag="the sums")       # (the model's run is shared)
        for margin in (-30, 0, 40):
            want = model_round(got, 16, margin, DEFAULT, [15] * n)
            assert (launch_round(env, got, 16, margin) == want).all(), margin
    finally:
        env.close()


def test_the_round_on_hand_made_sums_that_force_every_branch(T):
    """Small sums, so that ties, bids under the pass, negative bids over a more negative pass and holders that stand all
    happen: asserted from the model first.  Then row 19 zeroed against tarok_bid_round, byte for byte."""
    import playout_bids_model as BM
    from oracle import tarok_spec as S
    n = 600
    rng = np.random.default_rng(3)
    sums = rng.integers(-20, 21, size=(n, 4, 20)).astype(np.int32)
    sums[:100, :, :19] -= 25                                             # every bid negative: only a worse pass lets one through
    sums[:100, :, 19] -= 40
    per_game = np.array([(15, 1 << (g & 3), 6, 9, 0)[g % 5] for g in range(n)], np.uint8)
    flat = sums.copy()
    flat[:, :, 19] = 0
    env = make_env(T, n)
    try:
        for contracts in (DEFAULT, ALL, 0x2AB):
            for margin, playouts in ((-30, 1), (0, 1), (40, 1), (1, 7)):
                want = model_round(sums, playouts, margin, contracts, per_game)
                got = launch_round(env, sums, playouts, margin, contracts, seats=0, per_game=per_game)
                bad = np.nonzero((got != want).any(axis=1))[0]
                assert bad.size == 0, (contracts, margin, bad[:8], got[bad[:8]].tolist(), want[bad[:8]].tolist())
                plain = launch_round(env, sums, playouts, margin, contracts, seats=0, per_game=per_game, entry="tarok_bid_round")
                zeroed = launch_round(env, flat, playouts, margin, contracts, seats=0, per_game=per_game)
                assert zeroed.tobytes() == launch_round(env, flat, playouts, margin, contracts, seats=0, per_game=per_game,
                                                        entry="tarok_bid_round").tobytes()
                assert plain.tobytes() == zeroed.tobytes()               # (tarok_bid_round does not read row 19)
                if margin == 0 and contracts == ALL:
                    assert (got != plain).any(axis=1).sum() > 20, "the pass row moves the round"
                    assert len(set(want[:, 0].tolist())) >= 6 and set(want[:, 1].tolist()) == {0, 1, 2, 3}
                    neg = want[:100]
                    assert (neg[:, 0] > 0).any(), "a negative bid clears a more negative pass"
                    key0 = [S.game_key(SEED, OFFSET + g, EPISODE) for g in range(100)]
                    assert any(BM.bid_round(key0[g], sums[g].tolist(), 1, 0, ALL, int(per_game[g]))[:2] != tuple(neg[g, :2]) for g in range(100))
    finally:
        env.close()


def test_the_empty_set_is_the_bots_own_round(T):
    n = 300
    env = make_env(T, n)
    try:
        bid = launch_round(env, None, 1, seats=0)
        assert bid.tobytes() == launch_round(env, None, 1, seats=0, entry="tarok_bid_round").tobytes()
        env.reset(episode=EPISODE)
        meta = env.state()[9]
        contract, declarer, king = (meta >> U(33)) & U(15), (meta >> U(37)) & U(3), (meta >> U(39)) & U(7)
        assert (bid[:, 0] == contract.astype(np.int8)).all() and (bid[:, 1] == declarer.astype(np.int8)).all()
        assert (bid[:, 2] == np.where(king == 7, 0, king).astype(np.int8)).all()
        assert len(set(bid[:, 0].tolist())) == 4 and set(bid[:, 1].tolist()) == {0, 1, 2, 3}
    finally:
        env.close()


def test_every_einval_of_the_three_entries(T):
    """TAROK_EINVAL comes before the env is touched: a fake, never dereferenced handle shows every condition; the
    siblings answer the same arguments the same way."""
    from tarok_amd import _native
    L = _native.lib()
    out = (C.c_int32 * 80)()
    f32 = (C.c_float * 80)()
    o8 = (C.c_int8 * 4)()
    w = (C.c_char * 64)()
    fake = (C.c_char * 4096)()
    h = C.cast(fake, C.c_void_p)
    for name in ("tarok_playout_bids_pass", "tarok_playout_bids"):
        f = getattr(L, name)
        assert f(None, 0, None, 1, 1, 15, 0, 15, None, out, None) == -1
        for worlds, samples, contracts, seats in ((0, 1, 15, 15), (65, 1, 15, 15), (1, 0, 15, 15), (1, 1025, 15, 15), (1, 1, 0, 15),
                                                  (1, 1, 0x400, 15), (1, 1, 15, -1), (1, 1, 15, 16)):
            assert f(h, 0, None, worlds, samples, contracts, 0, seats, None, out, None) == -1, (name, worlds, samples, contracts, seats)
        assert f(h, 0, None, 1, 1, 15, 0, 15, None, None, None) == 0                         # sum_out NULL: nothing is launched
    for name in ("tarok_bid_round_pass", "tarok_bid_round"):
        f = getattr(L, name)
        assert f(None, 0, out, 1, 0, 15, 15, None, o8, o8, o8, None) == -1
        for sums, playouts, contracts, seats, outs in ((out, 0, 15, 15, (o8, o8, o8)), (out, 1, 0, 15, (o8, o8, o8)),
                                                       (out, 1, 0x400, 15, (o8, o8, o8)), (out, 1, 15, 16, (o8, o8, o8)),
                                                       (out, 1, 15, -1, (o8, o8, o8)), (None, 1, 15, 1, (o8, o8, o8)),
                                                       (out, 1, 15, 0, (None, None, None))):
            assert f(h, 0, sums, playouts, 0, contracts, seats, None, outs[0], outs[1], outs[2], None) == -1, (name, playouts, contracts, seats)
        assert f(h, 0, None, 1, 0, 15, 0, o8, o8, o8, o8, None) == -1                         # a seat array without sums
    for name in ("tarok_bid_values_pass", "tarok_bid_values"):
        f = getattr(L, name)
        good = [h, 0, None, w, f32, w, f32, w, f32, 1.0, 15, 15, None, out, f32, None, None]
        assert f(*([None] + good[1:])) == -1
        for i in range(3, 9):                                                                 # a NULL weight or bias
            assert f(*(good[:i] + [None] + good[i + 1:])) == -1, (name, i)
        for scale in (0.0, -1.0, float("nan"), float("inf"), 2.0 ** 20 + 1):
            assert f(*(good[:9] + [scale] + good[10:])) == -1, (name, scale)
        for contracts, seats in ((0, 15), (0x400, 15), (15, -1), (15, 16)):
            assert f(*(good[:10] + [contracts, seats] + good[12:])) == -1, (name, contracts, seats)
        assert f(*(good[:13] + [None, None, None, None])) == -1                              # all three outputs NULL


def test_python_surface(T):
    import torch
    from tarok_amd import karte as K
    from tarok_amd import licitacija as LI
    assert K.BID_PASS_ROW == 19 == LI.BID_PASS_ROW
    n = 40
    env = make_env(T, n)
    try:
        raw = launch_bids(env, 2, 1, ALL, salt=4)
        sums = env.playout_bids(EPISODE, 2, 1, contracts=ALL, salt=4, pass_value=True)
        assert sums.dtype == torch.int32 and tuple(sums.shape) == (n, 4, 20) and (sums.cpu().numpy() == raw).all()
        plain = env.playout_bids(EPISODE, 2, 1, contracts=ALL, salt=4)
        assert (plain[:, :, :19] == sums[:, :, :19]).all() and not plain[:, :, 19].any() and sums[:, :, 19].any()
        for margin in (0, -5):
            got = torch.stack(env.bid_round(EPISODE, sums, 2, threshold=margin, contracts=ALL, pass_value=True), 1).cpu().numpy()
            assert (got == launch_round(env, raw, 2, margin, ALL)).all()
            old = torch.stack(env.bid_round(EPISODE, sums, 2, threshold=margin, contracts=ALL), 1).cpu().numpy()
            assert (old == launch_round(env, raw, 2, margin, ALL, entry="tarok_bid_round")).all()
        with pytest.raises(Exception):
            env.playout_bids(EPISODE, 0, 1, pass_value=True)
        with pytest.raises(Exception):
            env.bid_round(EPISODE, None, 1, seats=1, pass_value=True)
    finally:
        env.close()


def test_evaluate_bidding_vs_bot_with_the_pass_replays_on_the_oracle(T):
    import playout_pass_model as PS
    from tarok_amd import evaluate as E
    n, seed, salt = 32, 3, 2
    inspect = []
    res = E.evaluate_bidding_vs_bot(4, 1, n, 1, seed=seed, salt=salt, inspect=inspect, pass_value=True)
    assert len(inspect) == 5 and res["deals"] == n
    scores = np.zeros((5, n, 4), np.int64)
    for p, rec in enumerate(inspect):
        assert rec["seats"] == E.PASS_SEATS[p]
        for g in range(n):
            c, d, k, actions, sc = PS.replay_pass(seed, g, 0, rec["seats"], 4, 1, salt=salt)
            assert (int(rec["contract"][g]), int(rec["declarer"][g]), int(rec["king_suit"][g])) == (c, d, k), (p, g)
            assert rec["actions"][:, g].tolist() == actions and rec["scores"][g].tolist() == sc, (p, g)
            scores[p, g] = sc
    assert res == E.duplicate_advantage(scores)
    # pass 0 is the Bot's own round: the pass 0 of the evaluation without the front end
    plain = []
    E.evaluate_playout_vs_bot(1, n, 1, seed=seed, inspect=plain, worlds=1)
    assert (plain[0]["scores"] == inspect[0]["scores"]).all() and (plain[0]["start"] == inspect[0]["start"]).all()
