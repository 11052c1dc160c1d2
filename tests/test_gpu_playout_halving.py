"""GPU: tarok_playout_cards_halving and tarok_playout_targets_counts, and the doors built on them.  The launch is checked
exactly — integers against integers — against tests/playout_halving_model.py (sequential halving over the single playouts
of the uniform models on the CPU oracle), and byte for byte against the existing launches where the definition says so.
Outputs sit inside guard bands (tests/guarded.py); the launch helpers are tests/gpu_harness.py's.

Run on the GPU box:  python -m pytest tests/test_gpu_playout_halving.py -m gpu -q
"""
import ctypes
import functools

import numpy as np
import pytest

import gpu_harness as H
import playout_halving_model as HM
from guarded import Guarded
from gpu_harness import T  # noqa: F401  (T: the module fixture)

pytestmark = pytest.mark.gpu
U = np.uint64
SEED, OFFSET, EPISODE = 41, 1000, 3
make_env = functools.partial(H.make_env, seed=SEED, offset=OFFSET, episode=EPISODE)
SCHEDULES = (((1, 1, 1, 1), 1), ((2, 1), 2), ((1, 2, 4, 8), 1))


def launch(kind, env, schedule, samples, words=None, salt=0, seats=15, per_game=None, want=("sum", "count", "action"), untouched=False):
    """One launch into guarded outputs: (sum [n,12,4] i32, count [n,12] i32, action [n] u8), None where not asked for."""
    g_sum, g_act = H.card_outputs(env.n, want)
    g_cnt = Guarded("count_out", 1, env.n, np.int32, inner=(12,), device="cuda") if "count" in want else None
    w = None if kind == "det" else H.words_of(kind, env, words)
    rw = (ctypes.c_int * len(schedule))(*schedule)
    H._launch(env, "tarok_playout_cards_halving", [HM.KINDS.index(kind), w, len(schedule), rw, int(samples), int(salt), int(seats), H.dev_u8(per_game)],
              [g_sum, g_cnt, g_act], None, untouched, (kind, schedule, samples))
    s, a = H.read_cards(g_sum, g_act)
    return s, None if g_cnt is None else H.read_words(g_cnt), a


def uniform(kind, env, worlds, samples, words=None, **kw):
    return H.launch_det(env, worlds, samples, **kw) if kind == "det" else H.launch_worlds(kind, env, worlds, samples, words, **kw)


def model(kind, env, schedule, samples, salt, sets=None, words=None, scores=None):
    """scores: per game the kind's single playouts at (>= the schedule's worlds, >= samples), where the caller has them."""
    lanes = env.state()
    ep, _ = env.counters()
    words = None if kind == "det" else (H.model_words(kind, env) if words is None else words)
    out = [HM.playout_cards_halving(kind, lanes[:, g].copy(), int(ep[g]), SEED, salt, OFFSET + g, 15 if sets is None else int(sets[g]) & 15,
                                    schedule, samples, None if words is None else int(words[g]), None if scores is None else scores[g])
           for g in range(env.n)]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], np.uint8))


def single_playouts(kind, env, worlds, samples, salt, seats=15):
    """Per game the kind's single playouts [12, worlds, samples, 4] on the CPU model: one array serves every schedule."""
    lanes = env.state()
    ep, _ = env.counters()
    words = None if kind == "det" else H.model_words(kind, env)
    return [HM.model_scores(kind, lanes[:, g].copy(), int(ep[g]), SEED, salt, OFFSET + g, seats, worlds, samples,
                            None if words is None else int(words[g])) for g in range(env.n)]


def check(kind, env, schedule, samples, salt=0, seats=15, per_game=None, tag=None, scores=None):
    sets = per_game if per_game is not None else np.full(env.n, seats)
    want = model(kind, env, schedule, samples, salt, sets, scores=scores)
    got = launch(kind, env, schedule, samples, None, salt, seats, per_game)
    H.assert_cards_equal(got[0], want[0], got[2], want[2], (tag, kind, schedule, samples))
    assert (got[1] == want[1]).all(), (tag, kind, "counts differ", np.nonzero((got[1] != want[1]).any(axis=1))[0][:8])
    return got


ALL_SCHEDULES = SCHEDULES + (((16, 16, 16, 16), 1), ((64,), 1))
GAMES = {0: 8, 5: 8, 13: 12, 22: 24, 34: 32, 46: 32}          # per contract: the CPU model plays 64 worlds of every legal card


@pytest.mark.parametrize("kind", HM.KINDS)
@pytest.mark.parametrize("cards", [0, 5, 13, 22, 34, 46])
def test_every_row_against_the_model(T, kind, cards):
    """Games of each of the ten contracts after `cards` Bot cards, all five schedules at every position: every row of sum,
    count and the card.  The late positions give the 1-, 2-, 3- and 5-card chains and natural ties; the early ones the
    12-6-3-2 chain at 64 worlds, where a team is four waves.  The model plays every single playout once per game — 64
    worlds x 1 sample and 3 worlds x 2 samples serve the five schedules — and that sets the games per contract: 32 from
    34 cards on, 24, 12, 8 and 8 at 22, 13, 5 and 0 cards (the fresh deal at full size:
    test_wide_teams_on_a_fresh_deal_against_the_existing_launch)."""
    from oracle import tarok_spec as S
    for code in range(10):
        env = make_env(T, GAMES[cards], S.MIX_FIXED + code, cards, history=True)
        try:
            wide, twice = single_playouts(kind, env, 64, 1, 7), single_playouts(kind, env, 3, 2, 7)
            for schedule, samples in ALL_SCHEDULES:
                check(kind, env, schedule, samples, salt=7, tag=(code, cards), scores=twice if samples == 2 else wide)
        finally:
            env.close()


@pytest.mark.parametrize("kind", HM.KINDS)
def test_wide_teams_on_a_fresh_deal_against_the_existing_launch(T, kind):
    """96 fresh deals of every contract, no CPU model: teams of two waves (W x S = 20 and 24: lg 7) and of four (W = 64:
    lg 8), twelve legal cards.  The expected outputs are rebuilt on the host from the EXISTING launch's rows at the
    cumulative ends: a rank alive in round r has played the worlds below e_r, so its sum there is the existing launch's row
    at worlds = e_r; the survivors are playout_halving_model.survivors on those rows.  Every row, count and card equal; the
    counts follow the 12-6-3-2 chain and the card has the maximal count."""
    from oracle import tarok_spec as S
    env = make_env(T, 96, S.MIX_ALL, 0, history=True)
    try:
        words = env.legal_actions().words.cpu().numpy().view(np.uint64)
        nl = np.array([bin(int(w) & ((1 << 54) - 1)).count("1") for w in words])
        mover = ((words >> U(54)) & U(3)).astype(np.int64)
        assert (nl == 12).sum() >= 64
        for schedule, samples in (((4, 4, 4, 8), 1), ((2, 2, 4, 4), 2), ((16, 16, 16, 16), 1), ((8, 8, 16, 32), 1)):
            ends = np.cumsum(schedule).tolist()
            rows = [uniform(kind, env, e, samples, salt=9) for e in ends]
            want_sum, want_cnt = np.zeros((96, 12, 4), np.int64), np.zeros((96, 12), np.int64)
            want_act = rows[-1][1].copy()
            for g in range(96):
                if nl[g] == 0:
                    continue
                alive = list(range(nl[g]))
                for r, e in enumerate(ends):
                    if r > 0 and len(alive) == 1:
                        break
                    want_sum[g, alive], want_cnt[g, alive] = rows[r][0][g, alive], e * samples
                    if r + 1 < len(ends):
                        alive = HM.survivors(rows[r][0][g, :, mover[g]], alive)
                cards_of = [c for c in range(54) if (int(words[g]) >> c) & 1]
                want_act[g] = cards_of[min(alive, key=lambda j: (-int(want_sum[g, j, mover[g]]), j))]
            got = launch(kind, env, schedule, samples, None, 9)
            H.assert_cards_equal(got[0], want_sum, got[2], want_act, (kind, schedule, samples))
            assert (got[1] == want_cnt).all(), (kind, schedule, "counts differ")
            full = nl == 12
            top = sorted(np.unique(got[1][full], return_counts=True)[1].tolist())
            assert sorted(np.unique(got[1][full]).tolist()) == [e * samples for e in ends]
            assert top == sorted(int(full.sum()) * k for k in (6, 3, 1, 2))          # 12 -> 6 -> 3 -> 2: 6, 3, 1 and 2 ranks leave
            rank = np.array([[c for c in range(54) if (int(w) >> c) & 1].index(int(a)) for w, a in zip(words[full], got[2][full])])
            assert (got[1][full][np.arange(full.sum()), rank] == ends[-1] * samples).all()
    finally:
        env.close()


def test_the_widest_schedules_one_game_and_a_ragged_workgroup(T):
    from oracle import tarok_spec as S
    env = make_env(T, 4, S.MIX_BOT, 40, history=True)
    try:
        check("det", env, (16, 16, 16, 16), 1, salt=3, tag="W=64")
        check("hidden", env, (64,), 1, salt=3, tag="(64,)")
    finally:
        env.close()
    env = make_env(T, 1, S.MIX_FIXED + 2, 30, history=True)
    try:
        check("voids", env, (1, 2), 2, salt=2, tag="n=1")
    finally:
        env.close()
    env = make_env(T, 67, S.MIX_BOT, 42, history=True)             # 67 games, 32 teams of 8 lanes per workgroup at W * S = 2
    try:
        check("det", env, (1, 1), 1, salt=1, tag="ragged")
    finally:
        env.close()


@pytest.mark.parametrize("kind", HM.KINDS)
def test_one_round_is_the_existing_launch_and_rows_are_prefixes(T, kind):
    """rounds = 1 writes the existing launch's bytes; for (2, 1, 2) x 2 every row equals the existing launch's row at the
    cumulative end its count names, and the card is alive at the last end."""
    from oracle import tarok_spec as S
    env = make_env(T, 96, S.MIX_ALL, 9, history=True)
    try:
        s, c, a = launch(kind, env, (5,), 2, salt=4)
        u_sum, u_act = uniform(kind, env, 5, 2, salt=4)
        assert s.any() and s.tobytes() == u_sum.tobytes() and a.tobytes() == u_act.tobytes()
        legal = (s != 0).any(axis=2) | (c != 0)
        assert set(np.unique(c).tolist()) <= {0, 10} and (c[legal] == 10).all()
        s, c, a = launch(kind, env, (2, 1, 2), 2, salt=4)
        assert set(np.unique(c).tolist()) <= {0, 4, 6, 10} and (c == 4).any() and (c == 10).any()
        for e in (2, 3, 5):
            u_sum, _ = uniform(kind, env, e, 2, salt=4)
            at = c == 2 * e
            assert (s[at] == u_sum[at]).all(), e
        assert not s[c == 0].any()
    finally:
        env.close()


def test_zero_words_and_nothing_hidden_give_the_det_bytes(T):
    from oracle import tarok_spec as S
    env = make_env(T, 64, S.MIX_FIXED + 7, 3, history=True)        # Berac: nothing more is hidden
    try:
        d = launch("det", env, (1, 2, 2), 1, salt=5)
        v = launch("voids", env, (1, 2, 2), 1, np.zeros(64, np.uint32), salt=5)
        h = launch("hidden", env, (1, 2, 2), 1, salt=5)
        for x in (v, h):
            assert d[0].any() and all(p.tobytes() == q.tobytes() for p, q in zip(d, x))
    finally:
        env.close()


def test_seat_sets_waiting_and_finished_games_and_each_output_alone(T):
    from oracle import tarok_spec as S
    env = make_env(T, 96, S.MIX_ALL, 22, history=True)
    try:
        phases = (env.state()[9] >> U(52)) & U(3)
        assert (phases == 3).any() and (phases == 2).any()
        s, c, a = check("det", env, (1, 2), 1, salt=4, seats=5, tag="seats=5")
        assert (a[phases == 3] == 255).all() and not s[phases == 3].any() and not c[phases == 3].any()
        sets = np.random.RandomState(3).randint(0, 16, 96).astype(np.uint8)
        full = check("hidden", env, (1, 2), 1, salt=4, seats=0, per_game=sets, tag="per game")
        for i, name in enumerate(("sum", "count", "action")):
            alone = launch("hidden", env, (1, 2), 1, None, 4, 0, sets, want=(name,))
            assert alone[i].tobytes() == full[i].tobytes() and all(alone[k] is None for k in range(3) if k != i)
            rest = launch("hidden", env, (1, 2), 1, None, 4, 0, sets, want=tuple(k for k in ("sum", "count", "action") if k != name))
            assert rest[i] is None and all(rest[k].tobytes() == full[k].tobytes() for k in range(3) if k != i)
    finally:
        env.close()
    env = make_env(T, 96, S.MIX_ALL, 0, history=True, defer_exchange=True)
    try:
        phases = (env.state()[9] >> U(52)) & U(3)
        assert (phases == 1).sum() >= 8
        s, c, a = check("voids", env, (1, 1), 1, salt=4, tag="waiting")
        assert (a[phases == 1] == 255).all() and not s[phases == 1].any() and not c[phases == 1].any()
    finally:
        env.close()


def test_read_only_deterministic_salted_and_independent_of_the_batch(T):
    from oracle import tarok_spec as S
    big, small = make_env(T, 200, S.MIX_BOT, 30, history=True), make_env(T, 77, S.MIX_BOT, 30, history=True)
    try:
        x = launch("hidden", big, (1, 1, 2), 2, untouched=True)
        y = launch("hidden", big, (1, 1, 2), 2)
        assert all(p.tobytes() == q.tobytes() for p, q in zip(x, y))
        assert (launch("hidden", big, (1, 1, 2), 2, salt=1)[0] != x[0]).any()
        z = launch("hidden", small, (1, 1, 2), 2)
        assert all((p[:77] == q).all() for p, q in zip(x, z))
    finally:
        big.close()
        small.close()


def to_bf16_rows(t):
    import torch
    return t.to(torch.float32).cpu().numpy().astype(np.float64)


def test_the_counts_targets_within_the_derived_bound(T):
    """On a halving launch's output and on hand-made counts with zeros: every row within
    playout_halving_model.targets_counts_bound; tau = 0 is the launch's card; with every count equal to `playouts` the rows
    are within the two bounds of tarok_playout_targets' rows."""
    import torch
    import distill_model as DI
    from oracle import tarok_spec as S
    env = make_env(T, 160, S.MIX_ALL, 18)
    try:
        words = env.legal_actions().words.clone()
        sums, counts, act = env.playout_cards_halving((1, 2, 4), 2, salt=6)
        s, c, a, w = sums.cpu().numpy(), counts.cpu().numpy(), act.cpu().numpy(), words.cpu().numpy().view(np.uint64)
        for tau in (8.0, 0.5):
            q, has, card, big = HM.targets_counts_reference(s, c, w, tau, 15)
            got = to_bf16_rows(env.playout_targets_counts(sums, counts, words, tau))
            assert has.sum() > 60 and (np.abs(got - q) <= HM.targets_counts_bound(q, big, tau)).all(), tau
        q, has, card, big = HM.targets_counts_reference(s, c, w, 0.0, 15)
        got = to_bf16_rows(env.playout_targets_counts(sums, counts, words, 0.0))
        assert (got == q).all() and (card[has] == a[has]).all()
        rnd = np.random.RandomState(5)
        c2 = rnd.randint(0, 4, c.shape).astype(np.int32) * (c > 0)
        c2[:8] = 0
        q, has, card, big = HM.targets_counts_reference(s, c2, w, 4.0, 15)
        got = to_bf16_rows(env.playout_targets_counts(sums, torch.from_numpy(c2).cuda(), words, 4.0))
        assert (np.abs(got - q) <= HM.targets_counts_bound(q, big, 4.0)).all() and not got[:8].any()
        u_sum, _ = env.playout_cards_det(3, 2, salt=6)
        same = torch.full_like(counts, 6)
        got = to_bf16_rows(env.playout_targets_counts(u_sum, same, words, 8.0))
        old = to_bf16_rows(env.playout_targets(u_sum, words, 6, 8.0))
        q, has, card, big = HM.targets_counts_reference(u_sum.cpu().numpy(), same.cpu().numpy(), w, 8.0, 15)
        assert (np.abs(got - old) <= HM.targets_counts_bound(q, big, 8.0) + DI.target_bound(q)).all()
    finally:
        env.close()


def test_evaluate_playout_vs_bot_halving_replays_on_the_model(T):
    """64 deals, halving = (1, 2): every card of every pass and the returned dict equal a replay on the model."""
    from oracle import tarok_spec as S
    from tarok_amd import evaluate as EV
    seen = []
    got = EV.evaluate_playout_vs_bot(1, 64, 1, seed=5, inspect=seen, worlds=None, halving=(1, 2))
    scores = np.zeros((5, 64, 4), np.int32)
    for p, rec in enumerate(seen):
        for i in range(64):
            actions, sc = HM.replay_pass(5, S.MIX_BOT, i, 0, rec["seats"], (1, 2), 1)
            assert rec["actions"][:, i].tolist() == actions, (p, i)
            scores[p, i] = sc
    assert got == EV.duplicate_advantage(scores)


def test_a_halving_teacher_in_the_captured_rollout_equals_the_eager_rows(T):
    """SelfPlay(teacher=dict(halving=(1, 1, 2))) on 512 games, T = 4: the captured graph records the eager rollout's bytes,
    the rollout's own outputs are those of a rollout without a teacher, and the rows are a replayed launch's targets."""
    import torch
    from tarok_amd import selfplay as SP
    n, steps, tc = 512, 4, dict(halving=(1, 1, 2), tau=8, salt=11)

    def make(use_graph, teacher=tc):
        env = T.TarokVecEnv(n, seed=6, mix=T.karte.MIX_BOT)
        return env, SP.SelfPlay(env, hidden=256, seed=0, fused_learner=True, teacher=teacher, distill_coef=0.0, use_graph=use_graph)
    ea, a = make(True)
    eb, b = make(False)
    ed, d = make(True, None)
    with torch.no_grad():
        b._alloc(steps)
        b._collect_body(2)                               # (SelfPlay.collect warms up with two lock-steps before it captures)
    bufa, bufb, bufd = a.collect(steps), b.collect(steps), d.collect(steps)
    torch.cuda.synchronize()
    for k in ("obs", "words", "act", "logp", "val", "done", "reward"):
        assert torch.equal(bufa[k], bufb[k]) and torch.equal(bufa[k], bufd[k]), k
    assert torch.equal(bufa["teach"].view(torch.int16), bufb["teach"].view(torch.int16))
    assert bufa["teach"].view(torch.int16).ne(0).any(-1).all()
    ec, c = make(False)
    buf = c.collect(steps)
    twin = T.TarokVecEnv(n, seed=6, mix=T.karte.MIX_BOT)
    twin.reset()
    torch.cuda.synchronize()
    for t in range(steps):
        sums, counts, _ = twin.playout_cards_halving((1, 1, 2), 1, salt=11)
        want = twin.playout_targets_counts(sums, counts, buf["words"][t], 8.0)
        assert torch.equal(buf["teach"][t].view(torch.int16), want.view(torch.int16)), t
        twin.step(buf["act"][t], auto_reset=True)
    for e in (ea, eb, ec, ed, twin):
        e.close()
