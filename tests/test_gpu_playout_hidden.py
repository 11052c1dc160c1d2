"""GPU: tarok_playout_cards_hidden (determinized playouts whose worlds also re-deal Klop's face-down talon and the
declarer's discards) and the surface built on it, checked exactly — integers against integers — against the per-game
model of tests/playout_hidden_model.py, which rebuilds every word of played cards from the history, deals every world
and plays every playout on the CPU oracle.  Outputs sit inside guard bands (tests/guarded.py).  The launch helpers are
tests/gpu_harness.py's.

Run on the GPU box:  python -m pytest tests/test_gpu_playout_hidden.py -m gpu -q
"""
import functools

import numpy as np
import pytest

import gpu_harness as H
from gpu_harness import T, launch_det  # noqa: F401  (T: the module fixture)

pytestmark = pytest.mark.gpu
U = np.uint64
SEED, OFFSET, EPISODE = 41, 1000, 3               # tests/test_gpu_playout_det.py's: the same games
KLOP, DVE, BERAC, SOLO_BREZ = 0, 2, 7, 8
HIDING = (0, 1, 2, 3, 4, 5, 6)                    # Klop and the six contracts with an exchange
make_env = functools.partial(H.make_env, seed=SEED, offset=OFFSET, episode=EPISODE)


def launch(env, worlds, samples, played=None, salt=0, seats=15, per_game=None, want=("sum", "action")):
    """One launch into guarded outputs: (sum [n,12,4] i32 or None, action [n] u8 or None).  played: [n] u64 host array;
    None: the env's own (TarokVecEnv.played_cards)."""
    return H.launch_worlds("hidden", env, worlds, samples, played, salt, seats, per_game, want)


def own_played(env):
    import playout_hidden_model as HM
    lanes, hist = env.state(), env.get_history().cpu().numpy()
    return np.array([HM.played_of_lanes(lanes[:, g], hist[:, g]) for g in range(env.n)], np.uint64)


def model_scores(env, salt, played, worlds, samples, sets=None, seed=SEED):
    import playout_hidden_model as HM
    lanes = env.state()
    ep, _ = env.counters()
    out = []
    for g in range(env.n):
        s = 15 if sets is None else int(sets[g]) & 15
        out.append((lanes[:, g].copy(), int(ep[g]), s,
                    HM.playout_scores(lanes[:, g], int(ep[g]), seed, salt, OFFSET + g, s, worlds, samples, int(played[g]))))
    return out


def check(env, model, worlds, samples, played=None, salt=0, seats=15, per_game=None, tag=None, seed=SEED):
    import playout_hidden_model as HM
    import playout_model as PM
    want_sum = np.stack([HM.sums_of(sc, worlds, samples) for _, _, _, sc in model])
    want_act = np.array([PM.card_of(lanes, seed, OFFSET + g, ep, s, want_sum[g]) for g, (lanes, ep, s, _) in enumerate(model)], np.uint8)
    got_sum, got_act = launch(env, worlds, samples, played, salt, seats, per_game)
    H.assert_cards_equal(got_sum, want_sum, got_act, want_act, tag)
    return got_sum, got_act


@pytest.mark.parametrize("cards", [0, 1, 3, 5, 23, 24, 46])
def test_every_row_against_the_model_on_the_contracts_that_hide(T, cards):
    """32 games each of Klop, Tri, Dve, Ena and the three Solo contracts after `cards` Bot cards, under the games' own
    words (the launch takes TarokVecEnv.played_cards'; the model rebuilds them from the history); one model run at (3, 2)
    serves the launches at (1, 1) and (3, 2).  Where something more is hidden the determinized launch gives other sums."""
    from oracle import tarok_spec as S
    differ = 0
    for code in HIDING:
        env = make_env(T, 32, S.MIX_FIXED + code, cards, history=True)
        try:
            words = own_played(env)
            assert (env.played_cards().cpu().numpy().view(np.uint64) == words).all()
            model = model_scores(env, 7, words, 3, 2)
            for worlds, samples in ((1, 1), (3, 2)):
                got, _ = check(env, model, worlds, samples, None, salt=7, tag=(code, cards, worlds, samples))
            differ += int((got != launch_det(env, 3, 2, salt=7)[0]).any(axis=(1, 2)).sum())
        finally:
            env.close()
    if cards < 24:                                             # (after 24 cards a Klop's talon is gone; discards still differ)
        assert differ > 32, differ


def test_many_worlds_odd_sizes_one_game_and_a_ragged_workgroup(T):
    from oracle import tarok_spec as S
    env = make_env(T, 8, S.MIX_FIXED + KLOP, 4, history=True)
    try:
        check(env, model_scores(env, 3, own_played(env), 64, 1), 64, 1, None, salt=3, tag=(64, 1))
    finally:
        env.close()
    env = make_env(T, 16, S.MIX_BOT, 9, history=True)
    try:
        check(env, model_scores(env, 0, own_played(env), 5, 3), 5, 3, None, tag=(5, 3))
    finally:
        env.close()
    for code, cards in ((KLOP, 9), (DVE, 30)):
        env = make_env(T, 1, S.MIX_FIXED + code, cards, history=True)
        try:
            check(env, model_scores(env, 2, own_played(env), 2, 2), 2, 2, None, salt=2, tag=("n=1", code, cards))
        finally:
            env.close()
    env = make_env(T, 67, S.MIX_BOT, 6, history=True)          # 67 games, 64 teams of 4 lanes per workgroup at (1, 1)
    try:
        check(env, model_scores(env, 1, own_played(env), 1, 1), 1, 1, None, salt=1, tag="ragged")
    finally:
        env.close()


def test_mixed_games_seat_sets_and_each_output_alone(T):
    """96 games of every contract after 22 cards (finished Berac games beside games in play), one seat set for all and
    one per game; games waiting for the exchange take no part; each output NULL in turn gives the same bytes."""
    from oracle import tarok_spec as S
    env = make_env(T, 96, S.MIX_ALL, 22, history=True)
    try:
        words = own_played(env)
        phases = (env.state()[9] >> U(52)) & U(3)
        assert (phases == 3).any() and (phases == 2).any()
        got_sum, got_act = check(env, model_scores(env, 4, words, 2, 2, np.full(96, 5)), 2, 2, None, salt=4, seats=5, tag="seats=5")
        assert (got_act[phases == 3] == 255).all() and not got_sum[phases == 3].any()
        sets = np.random.RandomState(3).randint(0, 16, 96).astype(np.uint8)
        got_sum, got_act = check(env, model_scores(env, 4, words, 2, 2, sets), 2, 2, None, salt=4, seats=0, per_game=sets, tag="per game")
        s_only, _ = launch(env, 2, 2, None, 4, 0, sets, want=("sum",))
        _, a_only = launch(env, 2, 2, None, 4, 0, sets, want=("action",))
        assert s_only.tobytes() == got_sum.tobytes() and a_only.tobytes() == got_act.tobytes()
    finally:
        env.close()
    env = make_env(T, 96, S.MIX_ALL, 0, history=True, defer_exchange=True)
    try:
        phases = (env.state()[9] >> U(52)) & U(3)
        assert (phases == 1).sum() >= 8
        got_sum, got_act = check(env, model_scores(env, 4, own_played(env), 2, 1), 2, 1, None, salt=4, tag="waiting")
        assert (got_act[phases == 1] == 255).all() and not got_sum[phases == 1].any()
    finally:
        env.close()


def test_byte_equality_with_the_determinized_launch_where_nothing_more_is_hidden(T):
    """Berac, Solo_brez, a Klop after its sixth trick, and in the exchange contracts the declarer's own moves: both
    outputs are tarok_playout_cards_det's bytes."""
    from oracle import tarok_spec as S
    for code, cards in ((BERAC, 3), (SOLO_BREZ, 5), (9, 2), (KLOP, 24), (KLOP, 30)):
        env = make_env(T, 64, S.MIX_FIXED + code, cards, history=True)
        try:
            s, a = launch(env, 3, 2, None, salt=5)
            d_sum, d_act = launch_det(env, 3, 2, salt=5)
            assert s.any() and s.tobytes() == d_sum.tobytes() and a.tobytes() == d_act.tobytes(), (code, cards)
        finally:
            env.close()
    env = make_env(T, 256, S.MIX_FIXED + DVE, 5, history=True)
    try:
        m = env.state()[9]
        mover = (((m >> U(27)) & U(3)) + ((m >> U(24)) & U(7))) & U(3)
        own = mover == ((m >> U(37)) & U(3))
        assert own.sum() >= 16
        s, a = launch(env, 3, 2, None, salt=5)
        d_sum, d_act = launch_det(env, 3, 2, salt=5)
        assert (s[own] == d_sum[own]).all() and (a[own] == d_act[own]).all()
        assert (s[~own] != d_sum[~own]).any()
    finally:
        env.close()


def hidden_twin(lanes, words, rnd):
    """Canonical lanes with, in every game in play, everything the mover cannot know re-dealt inside the constraints: the
    hands of the other seats together with a Klop's remaining talon slots, or with the declarer's discards (discardable
    cards only) when the mover is not the declarer; the twin's TRUE team.  Returns (lanes, games changed beyond the hands)."""
    import playout_hidden_model as HM
    import playout_model as PM
    from oracle import oracle as O
    from oracle import tarok_spec as S
    out = lanes.copy()
    wider = 0
    for g in range(lanes.shape[1]):
        m = int(lanes[9, g])
        if (m >> 52) & 3 != 2:
            continue
        game = O.Game.from_lanes(lanes[:, g])
        mover = game.seat()
        others = [o for o in range(4) if o != mover]
        sizes = [S.popcount(int(lanes[o, g])) for o in others]
        pool = 0
        for o in others:
            pool |= int(lanes[o, g])
        contract, declarer, tl = (m >> 33) & 15, (m >> 37) & 3, (m >> 46) & 7
        tal = int(lanes[8, g])
        if contract == KLOP and tl > 0:
            cards = PM.cards_of(pool | HM.mask_of((tal >> (6 * i)) & 63 for i in range(tl)))
            cards = [cards[i] for i in rnd.permutation(len(cards))]
            for i in range(tl):
                tal = (tal & ~(63 << (6 * i))) | (cards[i] << (6 * i))
            wider += tal != int(lanes[8, g])
            out[8, g] = U(tal)
            rest = cards[tl:]
        else:
            disc = HM.hidden_discards(game, mover, int(words[g]))
            cand = PM.cards_of((pool | disc) & S.DISCARDABLE)
            new = HM.mask_of(cand[i] for i in rnd.permutation(len(cand))[:S.popcount(disc)])
            wider += new != disc
            out[4 + declarer, g] = U((int(lanes[4 + declarer, g]) & ~disc) | new)
            rest = PM.cards_of((pool | disc) & ~new)
            rest = [rest[i] for i in rnd.permutation(len(rest))]
        hands, at = {}, 0
        for o, k in zip(others, sizes):
            hands[o] = HM.mask_of(rest[at:at + k])
            out[o, g] = U(hands[o])
            at += k
        assert at == len(rest)
        king, team = (m >> 39) & 7, (m >> 42) & 15
        if king != 7:
            holder = [o for o in others if (hands[o] >> (8 * king + 7)) & 1]
            if holder:
                team = (1 << declarer) | (1 << holder[0])
        out[9, g] = U((m & ~(15 << 42)) | (team << 42))
    return out, wider


@pytest.mark.parametrize("code,cards", [(KLOP, 4), (KLOP, 9), (DVE, 5)])
def test_the_result_depends_on_the_information_set_alone(T, code, cards):
    """100 games and their twins, whose hidden hands and remaining talon slots (Klop) or hidden hands and discards (Dve)
    are re-dealt by numpy inside the constraints (same history, so the same words): identical bytes.  The determinized
    launch, which keeps the talon and the discards, differs on them: this test can fail."""
    from oracle import tarok_spec as S
    envs = [make_env(T, 100, S.MIX_FIXED + code, cards, history=True) for _ in range(2)]
    try:
        lanes = envs[0].state()
        words = own_played(envs[0])
        twin, wider = hidden_twin(lanes, words, np.random.RandomState(100 * code + cards))
        assert wider > 50
        envs[1].set_state(twin)
        assert (envs[1].state() == twin).all() and (own_played(envs[1]) == words).all()
        s0, a0 = launch(envs[0], 4, 2, None, salt=5)
        s1, a1 = launch(envs[1], 4, 2, None, salt=5)
        assert s0.any() and s0.tobytes() == s1.tobytes() and a0.tobytes() == a1.tobytes()
        d0, _ = launch_det(envs[0], 4, 2, salt=5)
        d1, _ = launch_det(envs[1], 4, 2, salt=5)
        assert (d0 != d1).any(axis=(1, 2)).sum() >= 1
    finally:
        for e in envs:
            e.close()


def test_read_only_deterministic_salted_and_independent_of_the_batch(T):
    from oracle import tarok_spec as S
    big, small = make_env(T, 200, S.MIX_BOT, 9, history=True), make_env(T, 77, S.MIX_BOT, 9, history=True)
    try:
        snap = lambda: (big.state().copy(), big.counters(), big.get_history().cpu().numpy().copy(), big.play_mode)
        before = snap()
        s1, a1 = launch(big, 3, 2)
        after = snap()
        assert (before[0] == after[0]).all() and (before[2] == after[2]).all() and before[3] == after[3]
        assert (before[1][0] == after[1][0]).all() and (before[1][1] == after[1][1]).all()
        s2, a2 = launch(big, 3, 2)
        assert s1.tobytes() == s2.tobytes() and a1.tobytes() == a2.tobytes()
        s3, _ = launch(big, 3, 2, salt=1)
        assert (s3 != s1).any()
        assert (big.state()[:, :77] == small.state()).all()
        ss, as_ = launch(small, 3, 2)
        assert (s1[:77] == ss).all() and (a1[:77] == as_).all()
    finally:
        big.close()
        small.close()


def test_python_surface(T):
    """playout_cards_hidden equals the direct C call, with the env's own words and with given ones; the determinized
    method is unchanged; hidden and voids together are refused."""
    import torch
    from oracle import tarok_spec as S
    from tarok_amd import evaluate as EV
    from tarok_amd import selfplay as SP
    env = make_env(T, 64, S.MIX_BOT, 6, history=True)
    try:
        s_c, a_c = launch(env, 3, 2, None, salt=4)
        sums, acts = env.playout_cards_hidden(3, 2, salt=4)
        assert (sums.cpu().numpy() == s_c).all() and (acts.cpu().numpy() == a_c).all()
        words = env.played_cards()
        assert words.dtype == torch.int64 and words.any()
        sums, acts = env.playout_cards_hidden(3, 2, salt=4, played=words)
        assert (sums.cpu().numpy() == s_c).all() and (acts.cpu().numpy() == a_c).all()
        s_d, a_d = launch_det(env, 3, 2, salt=4)
        sums, acts = env.playout_cards_det(3, 2, salt=4)
        assert (sums.cpu().numpy() == s_d).all() and (acts.cpu().numpy() == a_d).all()
        assert (s_d != s_c).any()
        assert env.L.tarok_playout_cards_hidden(env._h, 3, 2, 0, 15, None, None, env._p(sums), env._p(acts), env._stream()) == -1
        with pytest.raises(ValueError):
            EV.evaluate_playout_vs_bot(2, 64, 1, worlds=3, voids=True, hidden=True)
        with pytest.raises(ValueError):
            EV.evaluate_playout_vs_bot(2, 64, 1, hidden=True)
        with pytest.raises(ValueError):
            SP.SelfPlay(env, hidden=256, teacher=dict(worlds=2, samples=1, voids=True, hidden=True))
    finally:
        env.close()


def test_evaluate_playout_vs_bot_hidden_replays_on_the_oracle(T):
    """64 deals, 3 worlds, 2 samples: every card of every pass and the returned dict equal a replay on the oracle with
    the model's cards; the figure is the model's, exactly."""
    import playout_hidden_model as HM
    from oracle import tarok_spec as S
    from tarok_amd import evaluate as EV
    seen = []
    got = EV.evaluate_playout_vs_bot(2, 64, 1, seed=5, inspect=seen, worlds=3, hidden=True)
    assert [p["seats"] for p in seen] == list(EV.PASS_SEATS)
    scores = np.zeros((5, 64, 4), np.int32)
    for p, rec in enumerate(seen):
        for i in range(64):
            actions, sc = HM.replay_pass(5, S.MIX_BOT, i, 0, rec["seats"], 3, 2)
            assert rec["actions"][:, i].tolist() == actions, (p, i)
            assert rec["scores"][i].tolist() == sc, (p, i)
            scores[p, i] = sc
    assert got == EV.duplicate_advantage(scores)


def test_a_hidden_teacher_in_the_captured_rollout_equals_the_eager_rows(T):
    """SelfPlay(teacher=dict(..., hidden=True)) on 512 games, T = 4: the captured graph records the bytes of the eager
    rollout, and the eager rows are the targets of a replayed tarok_played_cards + tarok_playout_cards_hidden launch."""
    import torch
    from tarok_amd import selfplay as SP
    n, steps, tc = 512, 4, dict(worlds=2, samples=1, tau=8, hidden=True, salt=11)

    def make(use_graph):
        env = T.TarokVecEnv(n, seed=6, mix=T.karte.MIX_BOT, history=True)
        return env, SP.SelfPlay(env, hidden=256, seed=0, fused_learner=True, teacher=tc, distill_coef=0.0, use_graph=use_graph)
    ea, a = make(True)
    eb, b = make(False)
    with torch.no_grad():
        b._alloc(steps)
        b._collect_body(2)                               # (SelfPlay.collect warms up with two lock-steps before it captures)
    bufa, bufb = a.collect(steps), b.collect(steps)
    torch.cuda.synchronize()
    for k in ("obs", "words", "act", "logp", "val", "done", "reward"):
        assert torch.equal(bufa[k], bufb[k]), k
    assert torch.equal(bufa["teach"].view(torch.int16), bufb["teach"].view(torch.int16))
    assert bufa["teach"].view(torch.int16).ne(0).any(-1).all()
    ec, c = make(False)
    buf = c.collect(steps)
    twin = T.TarokVecEnv(n, seed=6, mix=T.karte.MIX_BOT, history=True)
    twin.reset()
    torch.cuda.synchronize()
    differ = 0
    for t in range(steps):
        sums, _ = twin.playout_cards_hidden(2, 1, salt=11, played=twin.played_cards())
        want = twin.playout_targets(sums, buf["words"][t], 2, 8.0)
        assert torch.equal(buf["teach"][t].view(torch.int16), want.view(torch.int16)), t
        plain = twin.playout_targets(twin.playout_cards_det(2, 1, salt=11)[0], buf["words"][t], 2, 8.0)
        differ += int(buf["teach"][t].view(torch.int16).ne(plain.view(torch.int16)).any(-1).sum())
        twin.step(buf["act"][t], auto_reset=True)
    assert differ > 0
    for e in (ea, eb, ec, twin):
        e.close()
