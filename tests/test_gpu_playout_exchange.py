"""GPU: tarok_playout_exchange (the declarer's talon exchange valued by determinized playouts) and the surface built on
it, checked exactly — integers against integers — against the per-game model of tests/playout_exchange_model.py, which
deals every world, samples every candidate and plays every playout on the CPU oracle.  All three outputs sit inside
guard bands (tests/guarded.py) and every row of each is compared.  The launch helpers are
tests/gpu_harness.py's.

The advantage: tools/playout_exchange_advantage.py (the model alone, 512 deals, (8, 2, 4)) gives evaluate_exchange_vs_bot
+1.27 points per game with a standard error of 0.26 — 4.8 of them, short of five — so no sign is asserted here: the
evaluations are held to exact reproduction of the model's replay alone.

Run on the GPU box:  python -m pytest tests/test_gpu_playout_exchange.py -m gpu -q
"""
import functools

import numpy as np
import pytest

import gpu_harness as H
from gpu_harness import T, U, launch_exchange_bot as launch  # noqa: F401  (T: the module fixture)

pytestmark = pytest.mark.gpu

SEED = 43
OFFSET = 2000                            # game offset of the envs: gidx = OFFSET + g
EPISODE = 5                              # episode the envs are reset to: the keys' episode field is not zero
EXCHANGE_CODES = (1, 2, 3, 4, 5, 6)      # Tri, Dve, Ena, Solo_tri, Solo_dve, Solo_ena


def make_env(T, n, mix, cards=0, defer=True, seed=SEED):
    """An env of n games at EPISODE, waiting for the exchange where the contract has one (defer), after `cards` Bot cards."""
    return H.make_env(T, n, mix, cards, seed=seed, offset=OFFSET, episode=EPISODE, defer_exchange=defer)


def model_scores(env, salt, sets_of_seats, worlds, samples, sets, seed=SEED):
    """Per game: (lanes, episode, seat set, the model's scores [6, sets, worlds, samples, 4]) of the env's current state."""
    import playout_exchange_model as XM
    lanes = env.state()
    ep, _ = env.counters()
    out = []
    for g in range(env.n):
        s = int(sets_of_seats[g]) & 15
        out.append((lanes[:, g].copy(), int(ep[g]), s,
                    XM.playout_scores(lanes[:, g], int(ep[g]), seed, salt, OFFSET + g, s, worlds, samples, sets)))
    return out


def expected(model, worlds, samples, sets, salt, seed=SEED):
    import playout_exchange_model as XM
    sums = np.stack([XM.sums_of(sc, worlds, samples, sets) for _, _, _, sc in model])
    rows = [XM.choice_of(lanes, seed, salt, OFFSET + g, ep, s, sums[g], sets) for g, (lanes, ep, s, _) in enumerate(model)]
    return sums, np.array([r[0] for r in rows], np.int8), np.array([r[1] for r in rows], np.uint8)


def check(env, model, worlds, samples, sets, salt=0, seats=15, per_game=None, tag=None):
    want_sum, want_ch, want_di = expected(model, worlds, samples, sets, salt)
    got_sum, got_ch, got_di = launch(env, worlds, samples, sets, salt, seats, per_game)
    bad = np.nonzero((got_sum != want_sum).any(axis=(1, 2)))[0]
    assert bad.size == 0, (tag, "sums differ", bad[:8], got_sum[bad[0]].tolist(), want_sum[bad[0]].tolist())
    bad = np.nonzero(got_ch != want_ch)[0]
    assert bad.size == 0, (tag, "choices differ", bad[:8], got_ch[bad[:8]], want_ch[bad[:8]])
    bad = np.nonzero((got_di != want_di).any(axis=1))[0]
    assert bad.size == 0, (tag, "discards differ", bad[:8], got_di[bad[:8]].tolist(), want_di[bad[:8]].tolist())
    return got_sum, got_ch, got_di


@pytest.mark.parametrize("code", EXCHANGE_CODES)
def test_every_row_against_the_model(T, code):
    """32 games of one exchange contract; one model run at (3, 2, 2) serves the launches at (2, 1, 2) and (3, 2, 1): d, w
    and k do not depend on the launch's sizes.  The fixed inputs must be able to tell the launch from bot_exchange: the
    MODEL picks another group than 0 in some game (a condition on the inputs, asserted on the model's output)."""
    from oracle import tarok_spec as S
    env = make_env(T, 32, S.MIX_FIXED + code)
    try:
        assert (((env.state()[9] >> U(52)) & U(3)) == 1).all()
        model = model_scores(env, 7, np.full(32, 15), 3, 2, 2)
        for worlds, samples, sets in ((2, 1, 2), (3, 2, 1)):
            _, want_ch, _ = expected(model, worlds, samples, sets, 7)
            assert (want_ch > 0).any(), "the model itself must choose another group than 0 somewhere"
            got_sum, got_ch, got_di = check(env, model, worlds, samples, sets, salt=7, tag=(code, worlds, samples, sets))
            ngroups = 6 // S.GROUP_SIZE[code]
            assert got_sum[:, :ngroups * sets].any() and not got_sum[:, ngroups * sets:].any()
            assert (got_di[:, S.GROUP_SIZE[code]:] == 255).all() and (got_di[:, :S.GROUP_SIZE[code]] < 54).all()
        for one in ("sum", "choice", "discards"):                        # NULL for the two others: the same bytes
            s, c, d = launch(env, 3, 2, 1, 7, want=(one,))
            got = dict(sum=s, choice=c, discards=d)[one]
            assert got.tobytes() == dict(sum=got_sum, choice=got_ch, discards=got_di)[one].tobytes()
        for skip in ("sum", "choice", "discards"):                       # NULL for each output in turn
            keep = tuple(o for o in ("sum", "choice", "discards") if o != skip)
            s, c, d = launch(env, 3, 2, 1, 7, want=keep)
            for o, got in (("sum", s), ("choice", c), ("discards", d)):
                if o != skip:
                    assert got.tobytes() == dict(sum=got_sum, choice=got_ch, discards=got_di)[o].tobytes()
    finally:
        env.close()


def test_the_most_worlds_and_the_most_discard_sets(T):
    """8 games at (64, 1, 1): every world slot of a workgroup belongs to one game, a team of 256 lanes.  8 games at
    (8, 2, 8): 48 rows per game, a team of 64 lanes, more items than lanes."""
    from oracle import tarok_spec as S
    env = make_env(T, 8, S.MIX_NAVADNA3)
    try:
        check(env, model_scores(env, 0, np.full(8, 15), 64, 1, 1), 64, 1, 1, tag=(64, 1, 1))
        check(env, model_scores(env, 3, np.full(8, 15), 8, 2, 8), 8, 2, 8, salt=3, tag=(8, 2, 8))
    finally:
        env.close()


def test_a_single_game_and_a_ragged_last_workgroup(T):
    """n = 1, and n = 21 at (1, 1, 3): 16 teams of 16 lanes per workgroup, so the second workgroup has 5 games."""
    from oracle import tarok_spec as S
    env = make_env(T, 1, S.MIX_FIXED + S.DVE)
    try:
        check(env, model_scores(env, 2, [15], 2, 2, 2), 2, 2, 2, salt=2, tag="n=1")
    finally:
        env.close()
    env = make_env(T, 21, S.MIX_BOT)
    try:
        check(env, model_scores(env, 0, np.full(21, 15), 1, 1, 3), 1, 1, 3, tag="n=21")
    finally:
        env.close()


def test_games_without_an_exchange_in_play_and_finished(T):
    """Klop, Berac and Solo_brez (no exchange), games already in play (the reset made the Bot's exchange) and finished
    games: -1, 255s and zero rows — and the model agrees."""
    from oracle import tarok_spec as S
    for mix, cards, defer in ((S.MIX_FIXED + S.KLOP, 0, True), (S.MIX_FIXED + S.BERAC, 0, True), (S.MIX_FIXED + S.SOLO_BREZ, 0, True),
                              (S.MIX_NAVADNA3, 0, False), (S.MIX_NAVADNA3, 5, False), (S.MIX_ALL, 48, False)):
        env = make_env(T, 24, mix, cards, defer)
        try:
            phases = (env.state()[9] >> U(52)) & U(3)
            assert (phases != 1).all() and (cards != 48 or (phases == 3).all())
            got_sum, got_ch, got_di = check(env, model_scores(env, 0, np.full(24, 15), 2, 1, 2), 2, 1, 2, tag=(mix, cards))
            assert not got_sum.any() and (got_ch == -1).all() and (got_di == 255).all()
        finally:
            env.close()


def test_seat_sets_and_the_bots_exchange_outside_the_set(T):
    """seats = 0, 15, every single seat and a per-game array (bits 4..7 ignored) against the model on a MIX_ALL env with
    the exchange deferred (games that wait beside games in play).  Outside the set the rows ARE the Bot's exchange:
    applied through tarok_exchange on a twin, they leave those games in the state of a twin that called exchange()
    without arrays."""
    import torch
    from oracle import tarok_spec as S
    n = 96
    env, twin_a, twin_b = (make_env(T, n, S.MIX_ALL) for _ in range(3))
    try:
        lanes = env.state()
        waiting = ((lanes[9] >> U(52)) & U(3)) == 1
        declarer = ((lanes[9] >> U(37)) & U(3)).astype(np.int64)
        assert waiting.sum() >= 16 and (~waiting).sum() >= 16
        model15 = model_scores(env, 11, np.full(n, 15), 2, 1, 2)
        for seats in (0, 15, 1, 2, 4, 8):
            model = [(l, ep, seats, sc if (seats >> int(declarer[g])) & 1 else np.zeros_like(sc)) for g, (l, ep, _, sc) in enumerate(model15)]
            got_sum, got_ch, got_di = check(env, model, 2, 1, 2, salt=11, seats=seats, tag=("seats", seats))
            inside = waiting & (((seats >> declarer) & 1) == 1)
            assert not got_sum[~inside].any() and (got_ch[waiting] >= 0).all() and (got_ch[~waiting] == -1).all()
        per = np.array([0, 1, 6, 15], np.uint8)[np.arange(n) % 4] | ((np.arange(n) % 3) << 4).astype(np.uint8)
        model = [(l, ep, int(per[g]) & 15, sc if (int(per[g]) >> int(declarer[g])) & 1 else np.zeros_like(sc))
                 for g, (l, ep, _, sc) in enumerate(model15)]
        got_sum, got_ch, got_di = check(env, model, 2, 1, 2, salt=11, seats=9, per_game=per, tag="per-game sets")
        outside = waiting & (((per.astype(np.int64) >> declarer) & 1) == 0)
        assert outside.sum() >= 4 and (waiting & ~outside).sum() >= 4
        assert (got_ch[outside] == 0).all() and not got_sum[outside].any()
        twin_a.exchange(torch.from_numpy(got_ch), torch.from_numpy(got_di))
        twin_b.exchange()
        sa, sb = twin_a.state(), twin_b.state()
        assert (((sa[9] >> U(52)) & U(3)) != 1).all()                     # one call served the whole mixed table
        assert (((sa[9] >> U(54)) & U(1)) == 0).all(), "an exchange was rejected"
        assert (sa[:, outside] == sb[:, outside]).all() and (sa[:, ~waiting] == sb[:, ~waiting]).all()
        assert (sa[:, waiting & ~outside] != sb[:, waiting & ~outside]).any()
    finally:
        for e in (env, twin_a, twin_b):
            e.close()


def redealt_twin(lanes, rnd):
    """Canonical lanes [10, n] with, in every game that waits for the exchange, the hands of the three seats other than
    the DECLARER re-dealt among them by a numpy permutation.  Returns (the twin's lanes with the ORIGINAL team field,
    the same with the twin's TRUE team: the declarer and the holder of the called king where that card is in a hand)."""
    import playout_model as PM
    a, b = lanes.copy(), lanes.copy()
    changed = 0
    for g in range(lanes.shape[1]):
        m = int(lanes[9, g])
        if (m >> 52) & 3 != 1:
            continue
        declarer = (m >> 37) & 3
        others = [o for o in range(4) if o != declarer]
        pool = [c for o in others for c in PM.cards_of(lanes[o, g])]
        pool = [pool[i] for i in rnd.permutation(len(pool))]
        hands = {}
        for j, o in enumerate(others):
            hands[o] = sum(1 << c for c in pool[12 * j:12 * j + 12])
            changed += hands[o] != int(lanes[o, g])
            a[o, g] = b[o, g] = U(hands[o])
        king, team = (m >> 39) & 7, (m >> 42) & 15
        if king != 7:
            holder = [o for o in others if (hands[o] >> (8 * king + 7)) & 1]
            if holder:
                team = (1 << declarer) | (1 << holder[0])
        b[9, g] = U((m & ~(15 << 42)) | (team << 42))
    return a, b, changed


def test_the_result_depends_on_the_declarers_information_set_alone(T):
    """100 Tri / Dve / Ena games and their twins, in which the three hands the declarer cannot see are re-dealt among
    their seats — once with the team field left as it was (stale), once with the twin's true team: identical bytes."""
    from oracle import tarok_spec as S
    envs = [make_env(T, 100, S.MIX_NAVADNA3) for _ in range(3)]
    try:
        lanes = envs[0].state()
        a, b, changed = redealt_twin(lanes, np.random.RandomState(77))
        assert changed > 250 and (a[9] != b[9]).sum() >= 10              # games whose partner sits elsewhere in the twin
        envs[1].set_state(a)
        envs[2].set_state(b)
        assert (envs[1].state() == a).all() and (envs[2].state() == b).all()
        ref = launch(envs[0], 4, 2, 2, salt=5)
        assert ref[0].any() and (ref[1] > 0).any()
        for e in envs[1:]:
            got = launch(e, 4, 2, 2, salt=5)
            for x, y in zip(ref, got):
                assert x.tobytes() == y.tobytes()
    finally:
        for e in envs:
            e.close()


def test_read_only_deterministic_salted_and_batch_independent(T):
    from oracle import tarok_spec as S
    big, small = make_env(T, 200, S.MIX_BOT), make_env(T, 37, S.MIX_BOT)
    try:
        snap = lambda: (big.state().copy(), big.counters(), big.play_mode)
        before = snap()
        r1 = launch(big, 3, 2, 2)
        after = snap()
        assert (before[0] == after[0]).all() and before[2] == after[2]
        assert (before[1][0] == after[1][0]).all() and (before[1][1] == after[1][1]).all()
        r2 = launch(big, 3, 2, 2)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(r1, r2))
        r3 = launch(big, 3, 2, 2, salt=1)
        assert (r3[0] != r1[0]).any()
        assert (big.state()[:, :37] == small.state()).all()             # another grid, another ragged tail: the same rows
        rs = launch(small, 3, 2, 2)
        assert all((x[:37] == y).all() for x, y in zip(r1, rs))
        big.exchange()                                                   # the env plays on as if nothing had been launched
        small.exchange()
        for _ in range(4):
            big.step_random(auto_reset=False)
            small.step_random(auto_reset=False)
        assert (big.state()[:, :37] == small.state()).all()
    finally:
        big.close()
        small.close()


def test_python_surface(T):
    import torch
    from oracle import tarok_spec as S
    env = make_env(T, 40, S.MIX_BOT)
    try:
        want = launch(env, 2, 2, 4, salt=4)
        sums, choice, disc = env.playout_exchange(2, 2, salt=4)         # discard_sets defaults to 4
        assert sums.dtype == torch.int32 and tuple(sums.shape) == (40, 24, 4)
        assert choice.dtype == torch.int8 and tuple(choice.shape) == (40,)
        assert disc.dtype == torch.uint8 and tuple(disc.shape) == (40, 3)
        for got, w in zip((sums, choice, disc), want):
            assert (got.cpu().numpy() == w).all()
        per = np.arange(40, dtype=np.uint8) % 16
        want = launch(env, 2, 1, 1, per_game=per)
        per_dev = torch.from_numpy(per).to(env.device)
        got = env.playout_exchange(2, 1, 1, seats_per_game=per_dev)
        assert tuple(got[0].shape) == (40, 6, 4) and all((g.cpu().numpy() == w).all() for g, w in zip(got, want))
        mine = torch.empty((40, 6, 4), dtype=torch.int32, device=env.device)
        assert env.playout_exchange(2, 1, 1, seats_per_game=per_dev, sum_out=mine)[0] is mine and (mine.cpu().numpy() == want[0]).all()
        with pytest.raises(Exception):
            env.playout_exchange(2, 1, 9)
    finally:
        env.close()


EVAL_SEED = 5


@functools.lru_cache(maxsize=None)
def bot_everywhere_scores():
    """Pass 0 as the parent commit plays it: the model replay of evaluate_playout_vs_bot(worlds=3) on the 64 deals."""
    import playout_det_model as DM
    from oracle import tarok_spec as S
    return [DM.replay_pass(EVAL_SEED, S.MIX_BOT, i, 0, 0, 3, 1)[1] for i in range(64)]


def replay_and_compare(seen, worlds, samples, sets, cards):
    import playout_exchange_model as XM
    from oracle import tarok_spec as S
    from tarok_amd import evaluate as EV
    assert [p["seats"] for p in seen] == list(EV.PASS_SEATS)
    scores = np.zeros((5, 64, 4), np.int32)
    other_group = 0
    for p, rec in enumerate(seen):
        for i in range(64):
            choice, disc, actions, sc = XM.replay_pass(EVAL_SEED, S.MIX_BOT, i, 0, rec["seats"], worlds, samples, sets, cards=cards)
            assert (int(rec["choice"][i]), rec["discards"][i].tolist()) == (choice, disc), (p, i)
            assert rec["actions"][:, i].tolist() == actions, (p, i)
            assert rec["scores"][i].tolist() == sc, (p, i)
            scores[p, i] = sc
            other_group += choice > 0
    assert other_group > 0
    assert scores[0].tolist() == bot_everywhere_scores(), "pass 0 is the Bot everywhere, as without the exchange front end"
    return EV.duplicate_advantage(scores)


def same_dict(got, want):
    return got == want or (np.isnan(got["stderr"]) and np.isnan(want["stderr"]))


def test_evaluate_exchange_vs_bot_replays_on_the_oracle(T):
    """64 deals at (3, 1, 2): every exchange, every card and every score of every pass equal the model's replay; pass 0
    equals the Bot-everywhere pass.  No sign is asserted (see the module's docstring)."""
    from tarok_amd import evaluate as EV
    seen = []
    got = EV.evaluate_exchange_vs_bot(3, 1, 2, n_games=64, episodes=1, seed=EVAL_SEED, inspect=seen)
    assert same_dict(got, replay_and_compare(seen, 3, 1, 2, cards=False))


def test_evaluate_playout_vs_bot_with_the_exchange_replays_on_the_oracle(T):
    """evaluate_playout_vs_bot(1, 64, 1, worlds=3, exchange=2): both decisions against the model's replay.  The same call
    with exchange=None (the default): the parent's code path, against the existing model replay, with the same pass 0."""
    import playout_det_model as DM
    from oracle import tarok_spec as S
    from tarok_amd import evaluate as EV
    seen = []
    got = EV.evaluate_playout_vs_bot(1, 64, 1, seed=EVAL_SEED, inspect=seen, worlds=3, exchange=2)
    assert same_dict(got, replay_and_compare(seen, 3, 1, 2, cards=True))
    plain = []
    got = EV.evaluate_playout_vs_bot(1, 64, 1, seed=EVAL_SEED, inspect=plain, worlds=3)
    scores = np.zeros((5, 64, 4), np.int32)
    for p, rec in enumerate(plain):
        assert "choice" not in rec
        for i in range(64):
            actions, sc = DM.replay_pass(EVAL_SEED, S.MIX_BOT, i, 0, rec["seats"], 3, 1)
            assert rec["actions"][:, i].tolist() == actions and rec["scores"][i].tolist() == sc, (p, i)
            scores[p, i] = sc
    assert same_dict(got, EV.duplicate_advantage(scores))
    assert plain[0]["scores"].tolist() == seen[0]["scores"].tolist() == bot_everywhere_scores()
