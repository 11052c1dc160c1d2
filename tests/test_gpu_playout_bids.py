"""GPU: tarok_playout_bids (every bid valued by determinized playouts) and tarok_bid_round (the bidding round on the
device), and the surface built on them, checked exactly — integers against integers — against the per-game model of
tests/playout_bids_model.py, which deals every world, plays every playout and runs its own bidding loop on the CPU
oracle.  All outputs sit inside guard bands (tests/guarded.py); every row of sum_out and of the three bid outputs is
compared.

The advantage (tools/playout_bids_advantage.py) is a finding, not a bar: the evaluations are held to exact reproduction of
the model's replay alone, and no sign is asserted.

Run on the GPU box:  python -m pytest tests/test_gpu_playout_bids.py -m gpu -q
"""
import functools

import numpy as np
import pytest

import gpu_harness as H
from gpu_harness import T, U, dev_u8  # noqa: F401  (T: the module fixture)

pytestmark = pytest.mark.gpu

SEED = 2                                 # chosen on the CPU with the model alone: see test_the_default_mask_on_32_games
OFFSET = 3000                            # game offset of the envs: gidx = OFFSET + g
EPISODE = 4                              # the keys' episode field is not zero
DEFAULT, ALL = 0x00F, 0x3FF
make_env = functools.partial(H.make_bid_env, seed=SEED, offset=OFFSET)   # (T, n, **kw): NOT reset, bidding comes first
perms_of = functools.partial(H.perms_of, seed=SEED, offset=OFFSET, episode=EPISODE)


def launch_bids(env, worlds, samples, contracts=DEFAULT, deals=None, salt=0, seats=15, per_game=None, episode=EPISODE):
    """One tarok_playout_bids into a guarded sum_out: [n, 4, 20] i32."""
    return H.launch_bids(env, worlds, samples, contracts, deals, salt, seats, per_game, episode=episode, entry="tarok_playout_bids")


def launch_round(env, sums, playouts, threshold=0, contracts=DEFAULT, seats=15, per_game=None, episode=EPISODE):
    """One tarok_bid_round into three guarded outputs: [n, 3] i8 (contract, declarer, king)."""
    return H.launch_round(env, sums, playouts, threshold, contracts, seats, per_game, episode=episode, entry="tarok_bid_round")


def model_scores(perms, seats_of, worlds, samples, contracts, salt=0, seed=SEED, offset=OFFSET, episode=EPISODE):
    import playout_bids_model as BM
    return [BM.playout_scores(perms[g], episode, seed, salt, offset + g, int(seats_of[g]) & 15, worlds, samples, contracts)
            for g in range(len(perms))]


def check(env, scores, seats_of, worlds, samples, contracts=DEFAULT, salt=0, seats=15, per_game=None, deals=None, threshold=0,
          tag=None, seed=SEED, offset=OFFSET, episode=EPISODE):
    """Both launches against the model: every row of sum_out, then every row of the bid round's outputs on those sums."""
    import playout_bids_model as BM
    from oracle import tarok_spec as S
    want = np.stack([BM.sums_of(sc, worlds, samples) for sc in scores])
    got = launch_bids(env, worlds, samples, contracts, deals, salt, seats, per_game, episode)
    bad = np.nonzero((got != want).any(axis=(1, 2)))[0]
    assert bad.size == 0, (tag, "sums differ", bad[:8], got[bad[0]].tolist(), want[bad[0]].tolist())
    want_bid = np.array([BM.bid_round(S.game_key(seed, offset + g, episode), want[g], worlds * samples, threshold, contracts,
                                      int(seats_of[g]) & 15) for g in range(len(scores))], np.int8)
    got_bid = launch_round(env, got, worlds * samples, threshold, contracts, seats, per_game, episode)
    bad = np.nonzero((got_bid != want_bid).any(axis=1))[0]
    assert bad.size == 0, (tag, "bid rounds differ", bad[:8], got_bid[bad[:8]].tolist(), want_bid[bad[:8]].tolist())
    return got, got_bid


def test_the_full_mask_on_16_games(T):
    env = make_env(T, 16)
    try:
        perms = perms_of(16)
        sc = model_scores(perms, [15] * 16, 2, 1, ALL, salt=3)
        got, bid = check(env, sc, [15] * 16, 2, 1, ALL, salt=3, tag="full mask")
        assert got[:, :, :19].any(axis=(0, 1)).all() and not got[:, :, 19].any()
    finally:
        env.close()


def test_the_default_mask_on_32_games(T):
    """One model run at (3, 2) serves the launches at (3, 2), (2, 1) and (1, 2): w and k do not depend on the sizes.
    Coverage is a condition on the inputs: SEED was chosen with the model alone so that its own bid round over these 32
    games (one playout bidder per game, seat g % 4) shows at least three contracts and a declarer on every seat."""
    import playout_bids_model as BM
    from oracle import tarok_spec as S
    n = 32
    per_game = np.array([1 << (g & 3) for g in range(n)], np.uint8)
    perms = perms_of(n)
    sc = model_scores(perms, per_game, 3, 2, DEFAULT, salt=1)
    sums = [BM.sums_of(s, 3, 2) for s in sc]
    rounds = [BM.bid_round(S.game_key(SEED, OFFSET + g, EPISODE), sums[g], 6, 0, DEFAULT, int(per_game[g])) for g in range(n)]
    assert len({r[0] for r in rounds}) >= 3 and {r[1] for r in rounds} == {0, 1, 2, 3}, rounds
    env = make_env(T, n)
    try:
        for worlds, samples in ((3, 2), (2, 1), (1, 2)):
            got, _ = check(env, sc, per_game, worlds, samples, DEFAULT, salt=1, seats=0, per_game=per_game, tag=(worlds, samples))
            assert not got[:, :, 13:].any()
    finally:
        env.close()
    sc15 = model_scores(perms[:8], [15] * 8, 3, 2, DEFAULT, salt=1)
    env = make_env(T, 8)
    try:
        check(env, sc15, [15] * 8, 3, 2, DEFAULT, salt=1, tag="every seat")
        check(env, sc15, [15] * 8, 3, 2, DEFAULT, salt=1, threshold=-30, tag="threshold -30")
        check(env, sc15, [15] * 8, 3, 2, DEFAULT, salt=1, threshold=40, tag="threshold 40")
    finally:
        env.close()


def test_the_most_worlds(T):
    env = make_env(T, 4)
    try:
        sc = model_scores(perms_of(4), [15] * 4, 64, 1, 0x003)
        check(env, sc, [15] * 4, 64, 1, 0x003, tag="64 worlds")
    finally:
        env.close()


def test_a_single_game_and_a_ragged_last_workgroup(T):
    for n in (1, 17):                    # (2, 1): 16 lanes per game, 16 games per workgroup
        env = make_env(T, n)
        try:
            sc = model_scores(perms_of(n), [15] * n, 2, 1, 0x081)
            check(env, sc, [15] * n, 2, 1, 0x081, tag=n)
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
        sc = model_scores(perms, [15] * n, 2, 1, DEFAULT, salt=2)
        got, _ = check(env, sc, [15] * n, 2, 1, DEFAULT, salt=2, deals=other, tag="deals given")
        assert not got[3].any() and not got[9].any() and got[0].any()
    finally:
        env.close()


def test_seat_sets_per_game_and_a_single_contract(T):
    import playout_bids_model as BM
    n = 16
    perms = perms_of(n)
    per_game = np.array([(5 * g + 3) & 15 for g in range(n)], np.uint8) | np.uint8(16)      # (bits above the seats are ignored)
    env = make_env(T, n)
    try:
        for seats in (0, 1, 6, 8):
            sc = model_scores(perms, [seats] * n, 2, 1, DEFAULT)
            got, _ = check(env, sc, [seats] * n, 2, 1, DEFAULT, seats=seats, tag=("seats", seats))
            for v in range(4):
                assert got[:, v].any() == bool((seats >> v) & 1)
        sc = model_scores(perms, per_game, 2, 1, DEFAULT)
        check(env, sc, per_game, 2, 1, DEFAULT, seats=15, per_game=per_game, tag="per game")
        for contracts in (1 << 7, 1 << 2, 1 << 9):
            sc = model_scores(perms, [15] * n, 1, 2, contracts)
            got, bid = check(env, sc, [15] * n, 1, 2, contracts, tag=("contracts", contracts))
            rows = [r for r in range(19) if (contracts >> BM.row_option(r)[0]) & 1]
            assert got[:, :, rows].any() and not np.delete(got, rows, axis=2).any()
    finally:
        env.close()


def test_the_empty_set_is_the_bots_own_round(T):
    """bid_round(seats = 0, sums = NULL) against a TAROK_MIX_BOT reset's contract, declarer and king read back."""
    n = 300
    env = make_env(T, n)
    try:
        bid = launch_round(env, None, 1, seats=0)
        env.reset(episode=EPISODE)
        meta = env.state()[9]
        contract, declarer, king = (meta >> U(33)) & U(15), (meta >> U(37)) & U(3), (meta >> U(39)) & U(7)
        assert (bid[:, 0] == contract.astype(np.int8)).all() and (bid[:, 1] == declarer.astype(np.int8)).all()
        assert (bid[:, 2] == np.where(king == 7, 0, king).astype(np.int8)).all()
        assert len(set(bid[:, 0].tolist())) == 4 and set(bid[:, 1].tolist()) == {0, 1, 2, 3}
    finally:
        env.close()


def test_the_sums_depend_on_the_viewers_information_set_alone(T):
    """100 deals and their twins, in which the 42 cards the viewer does not hold are shuffled by numpy: identical bytes."""
    n = 100
    rng = np.random.default_rng(11)
    deals = np.stack([rng.permutation(54) for _ in range(n)]).astype(np.uint8)
    twins = deals.copy()
    per_game = np.array([1 << (g & 3) for g in range(n)], np.uint8)
    for g in range(n):
        v = g & 3
        rest = np.r_[0:12 * v, 12 * v + 12:54]
        twins[g, rest] = rng.permutation(deals[g, rest])
    assert (twins != deals).any(axis=1).all()
    env = make_env(T, n)
    try:
        a = launch_bids(env, 3, 1, ALL, deals=deals, seats=0, per_game=per_game)
        b = launch_bids(env, 3, 1, ALL, deals=twins, seats=0, per_game=per_game)
        assert a.tobytes() == b.tobytes() and a.any(axis=(1, 2)).all()
        c = launch_bids(env, 3, 1, ALL, deals=twins, seats=15)          # (the other viewers do see the difference)
        d = launch_bids(env, 3, 1, ALL, deals=deals, seats=15)
        assert (c != d).any()
    finally:
        env.close()


def test_read_only_deterministic_salted_and_batch_independent(T):
    import torch
    n = 24
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
        assert (launch_bids(env, 2, 2, DEFAULT, salt=7) != a).any()
    finally:
        env.close()
    part = make_env(T, 7, offset=OFFSET + 5)
    try:
        b = launch_bids(part, 2, 2, DEFAULT, salt=6)
        assert b.tobytes() == a[5:12].tobytes()
        assert (launch_round(part, b, 4) == r[5:12]).all()
    finally:
        part.close()


def test_python_surface_and_a_reset_from_the_round(T):
    import torch
    from tarok_amd import karte as K
    assert (K.BID_ROWS, K.BID_DEFAULT_CONTRACTS, K.BID_ALL_CONTRACTS) == (20, DEFAULT, ALL)
    assert [K.bid_row(*K.bid_row_option(r)) for r in range(19)] == list(range(19))
    n = 40
    env = make_env(T, n)
    try:
        raw = launch_bids(env, 2, 1, ALL, salt=4)
        sums = env.playout_bids(EPISODE, 2, 1, contracts=ALL, salt=4)
        assert sums.dtype == torch.int32 and tuple(sums.shape) == (n, 4, 20) and sums.is_cuda
        assert (sums.cpu().numpy() == raw).all()
        out = torch.full((n, 4, 20), 7, dtype=torch.int32, device=sums.device)
        assert env.playout_bids(EPISODE, 2, 1, contracts=ALL, salt=4, sum_out=out) is out and (out == sums).all()
        c, d, k = env.bid_round(EPISODE, sums, 2, contracts=ALL)
        want = launch_round(env, raw, 2, contracts=ALL)
        for t, col in zip((c, d, k), want.T):
            assert t.dtype == torch.int8 and tuple(t.shape) == (n,) and (t.cpu().numpy() == col).all()
        assert len(set(want[:, 0].tolist())) >= 3
        env.reset(episode=EPISODE, contract=c, declarer=d, king_suit=k)
        meta = env.state()[9]
        assert not ((meta >> U(54)) & U(1)).any(), "the reset took the round's outputs without an error"
        assert (((meta >> U(33)) & U(15)).astype(np.int8) == want[:, 0]).all()
        assert (((meta >> U(37)) & U(3)).astype(np.int8) == want[:, 1]).all()
        king = (meta >> U(39)) & U(7)
        has_king = (want[:, 0] >= 1) & (want[:, 0] <= 3)
        assert (king[has_king].astype(np.int8) == want[has_king, 2]).all() and (king[~has_king] == 7).all()
        for _ in range(48):
            env.step_random(auto_reset=False)
        assert (((env.state()[9] >> U(52)) & U(3)) == 3).all() and not ((env.state()[9] >> U(54)) & U(1)).any()
        with pytest.raises(Exception):
            env.playout_bids(EPISODE, 0, 1)
        with pytest.raises(Exception):
            env.bid_round(EPISODE, None, 1, seats=1)
        b0 = env.bid_round(EPISODE, None, 1, seats=0)
        assert (torch.stack(b0, 1).cpu().numpy() == launch_round(env, None, 1, seats=0)).all()
    finally:
        env.close()


def test_evaluate_bidding_vs_bot_replays_on_the_oracle(T):
    import playout_bids_model as BM
    from tarok_amd import evaluate as E
    from oracle import tarok_spec as S
    n, seed, salt = 32, 3, 2
    inspect = []
    res = E.evaluate_bidding_vs_bot(2, 1, n, 1, seed=seed, salt=salt, inspect=inspect)
    assert len(inspect) == 5 and res["deals"] == n
    scores = np.zeros((5, n, 4), np.int64)
    for p, rec in enumerate(inspect):
        assert rec["seats"] == E.PASS_SEATS[p]
        for g in range(n):
            c, d, k, actions, sc = BM.replay_pass(seed, g, 0, rec["seats"], 2, 1, salt=salt)
            assert (int(rec["contract"][g]), int(rec["declarer"][g]), int(rec["king_suit"][g])) == (c, d, k), (p, g)
            assert rec["actions"][:, g].tolist() == actions and rec["scores"][g].tolist() == sc, (p, g)
            scores[p, g] = sc
    assert res == E.duplicate_advantage(scores)
    # pass 0 is the Bot's own round: the pass 0 of the evaluation without the front end
    plain = []
    E.evaluate_playout_vs_bot(1, n, 1, seed=seed, inspect=plain, worlds=1)
    assert (plain[0]["scores"] == inspect[0]["scores"]).all() and (plain[0]["start"] == inspect[0]["start"]).all()
    differs = sum(int((inspect[p]["contract"] != inspect[0]["contract"]).sum()) for p in range(1, 5))
    assert differs > 0, "the playout bidder bids otherwise than the Bot somewhere"


def test_evaluate_playout_vs_bot_with_bidding_replays_on_the_oracle(T):
    import playout_bids_model as BM
    from tarok_amd import evaluate as E
    n, seed = 32, 5
    inspect = []
    res = E.evaluate_playout_vs_bot(1, n, 1, seed=seed, worlds=2, bidding=(2, 1), inspect=inspect)
    scores = np.zeros((5, n, 4), np.int64)
    for p, rec in enumerate(inspect):
        for g in range(n):
            c, d, k, actions, sc = BM.replay_pass(seed, g, 0, rec["seats"], 2, 1, cards=(2, 1))
            assert (int(rec["contract"][g]), int(rec["declarer"][g]), int(rec["king_suit"][g])) == (c, d, k), (p, g)
            assert rec["actions"][:, g].tolist() == actions and rec["scores"][g].tolist() == sc, (p, g)
            scores[p, g] = sc
    assert res == E.duplicate_advantage(scores)
    plain = []
    E.evaluate_playout_vs_bot(1, n, 1, seed=seed, worlds=2, inspect=plain)
    assert (plain[0]["scores"] == inspect[0]["scores"]).all() and (plain[0]["actions"] == inspect[0]["actions"]).all()
    with pytest.raises(ValueError):
        E.evaluate_playout_vs_bot(1, n, 1, bidding=(2, 1))
