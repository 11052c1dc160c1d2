"""GPU: tarok_playout_cards_det (determinized Monte-Carlo playouts: the unseen cards re-dealt per world) and the surface
built on it, checked exactly — integers against integers — against the per-game model of tests/playout_det_model.py,
which deals every world and plays every playout on the CPU oracle.  Outputs sit inside guard bands (tests/guarded.py).
The launch helpers are tests/gpu_harness.py's.

Run on the GPU box:  python -m pytest tests/test_gpu_playout_det.py -m gpu -q
"""
import functools

import numpy as np
import pytest

import gpu_harness as H
from gpu_harness import T, U, launch_det as launch  # noqa: F401  (T: the module fixture)

pytestmark = pytest.mark.gpu

SEED = 41
OFFSET = 1000                            # game offset of the envs: gidx = OFFSET + g
EPISODE = 3                              # episode the envs are reset to: the keys' episode field is not zero
make_env = functools.partial(H.make_env, seed=SEED, offset=OFFSET, episode=EPISODE)


def model_scores(env, salt, sets, worlds, samples, seed=SEED):
    """Per game: (lanes, episode, set, the model's scores [12, worlds, samples, 4]) of the env's current positions."""
    import playout_det_model as DM
    lanes = env.state()
    ep, _ = env.counters()
    out = []
    for g in range(env.n):
        s = int(sets[g]) & 15
        out.append((lanes[:, g].copy(), int(ep[g]), s,
                    DM.playout_scores(lanes[:, g], int(ep[g]), seed, salt, OFFSET + g, s, worlds, samples)))
    return out


def expected(model, worlds, samples, seed=SEED):
    import playout_det_model as DM
    import playout_model as PM
    sums = np.stack([DM.sums_of(sc, worlds, samples) for _, _, _, sc in model])
    acts = np.array([PM.card_of(lanes, seed, OFFSET + g, ep, s, sums[g]) for g, (lanes, ep, s, _) in enumerate(model)], np.uint8)
    return sums, acts


def check(env, model, worlds, samples, salt=0, seats=15, per_game=None, tag=None):
    want_sum, want_act = expected(model, worlds, samples)
    got_sum, got_act = launch(env, worlds, samples, salt, seats, per_game)
    H.assert_cards_equal(got_sum, want_sum, got_act, want_act, tag)
    return got_sum, got_act


@pytest.mark.parametrize("cards", [0, 1, 2, 3, 5, 22, 46, 47])
def test_every_row_against_the_model(T, cards):
    """300 games of every contract after `cards` Bot cards; one model run at (worlds, samples) = (3, 2) serves the
    launches at (1, 1), (3, 1) and (3, 2): world w and sample k do not depend on the launch's sizes."""
    from oracle import tarok_spec as S
    env = make_env(T, 300, S.MIX_ALL, cards)
    try:
        model = model_scores(env, 7, np.full(300, 15), 3, 2)
        phases = (env.state()[9] >> U(52)) & U(3)
        if cards >= 22:
            assert (phases == 3).any() and (phases == 2).any()           # finished games beside games in play
        for worlds, samples in ((1, 1), (3, 1), (3, 2)):
            got_sum, got_act = check(env, model, worlds, samples, salt=7, tag=(cards, worlds, samples))
            assert (got_act[phases == 3] == 255).all() and not got_sum[phases == 3].any()
            assert got_sum[phases == 2].any()
        s_only, _ = launch(env, 3, 2, 7, want=("sum",))                  # one output at a time: the same bytes
        _, a_only = launch(env, 3, 2, 7, want=("action",))
        assert (s_only == got_sum).all() and (a_only == got_act).all()
    finally:
        env.close()


def test_a_whole_workgroup_per_game_and_a_ragged_item_tail(T):
    """70 games at (16, 4) — 64 playouts per card, a team of 256 lanes — and at (20, 4): 80 per card, more items than
    lanes and no power of two.  One model run at (20, 4)."""
    from oracle import tarok_spec as S
    env = make_env(T, 70, S.MIX_ALL, 23)
    try:
        model = model_scores(env, 0, np.full(70, 15), 20, 4)
        for worlds in (16, 20):
            check(env, model, worlds, 4, tag=(worlds, 4))
    finally:
        env.close()


def test_odd_sizes_and_the_most_worlds(T):
    """(5, 3) at 70 games: neither size a power of two, teams of 64 lanes, 20 world slots of a workgroup in use.
    (64, 1) at 8 games: every world slot belongs to one game."""
    from oracle import tarok_spec as S
    env = make_env(T, 70, S.MIX_ALL, 30)
    try:
        check(env, model_scores(env, 3, np.full(70, 15), 5, 3), 5, 3, salt=3, tag=(5, 3))
    finally:
        env.close()
    env = make_env(T, 8, S.MIX_ALL, 38)
    try:
        check(env, model_scores(env, 0, np.full(8, 15), 64, 1), 64, 1, tag=(64, 1))
    finally:
        env.close()


def test_a_single_game(T):
    from oracle import tarok_spec as S
    for cards in (0, 6):
        env = make_env(T, 1, S.MIX_ALL, cards)
        try:
            check(env, model_scores(env, 2, [15], 2, 2), 2, 2, salt=2, tag=("n=1", cards))
        finally:
            env.close()


@pytest.mark.parametrize("code", [0, 7, 3, 8])
def test_fixed_contracts(T, code):
    """Klop (talon gifts, no team), Berac (early ends), Ena (called king: the world's team and the re-parked talon) and
    Solo_brez, 64 games, after 0 and 7 cards."""
    from oracle import tarok_spec as S
    for cards in (0, 7):
        env = make_env(T, 64, S.MIX_FIXED + code, cards)
        try:
            check(env, model_scores(env, 0, np.full(64, 15), 2, 2), 2, 2, tag=(code, cards))
        finally:
            env.close()


def test_games_waiting_for_the_exchange_give_zeros_and_255(T):
    from oracle import tarok_spec as S
    env = make_env(T, 96, S.MIX_ALL, 0, defer_exchange=True)
    try:
        phases = (env.state()[9] >> U(52)) & U(3)
        waiting = phases == 1
        assert waiting.sum() >= 8 and (phases == 2).sum() >= 8
        got_sum, got_act = check(env, model_scores(env, 0, np.full(96, 15), 2, 2), 2, 2, tag="deferred exchange")
        assert not got_sum[waiting].any() and (got_act[waiting] == 255).all()
    finally:
        env.close()


def test_seat_sets(T):
    """seats = 0: tarok_policy_random's bytes and no playout; a per-game array mixing 0, 1, 6 and 15 (bits 4..7 are
    ignored) against the model."""
    from oracle import tarok_spec as S
    env = make_env(T, 300, S.MIX_ALL, 5)
    try:
        bot = env.policy_random(env.legal_actions()).cpu().numpy().copy()
        got_sum, got_act = launch(env, 3, 2, seats=0)
        assert not got_sum.any() and (got_act == bot).all()
        assert (bot != 255).sum() > 200
        per = np.array([0, 1, 6, 15], np.uint8)[np.arange(300) % 4] | ((np.arange(300) % 3) << 4).astype(np.uint8)
        model = model_scores(env, 11, per, 2, 2)
        got_sum, got_act = check(env, model, 2, 2, salt=11, seats=9, per_game=per, tag="per-game sets")
        movers = ((env.legal_actions().words.cpu().numpy().view(U) >> U(54)) & U(3)).astype(np.int64)
        out = ((per.astype(np.int64) >> movers) & 1) == 0
        assert out.sum() > 50 and (~out).sum() > 50
        assert not got_sum[out].any() and (got_act[out] == bot[out]).all()
    finally:
        env.close()


def redealt_twin(lanes, rnd):
    """Canonical lanes [10, n] with, in every game in play, the hands of the three seats other than the seat to move
    re-dealt among them (sizes kept) by a numpy permutation.  Returns (the twin's lanes with the ORIGINAL team field,
    the same with the twin's TRUE team: declarer and holder of the called king where that card is in a hand)."""
    import playout_model as PM
    a, b = lanes.copy(), lanes.copy()
    changed = 0
    for g in range(lanes.shape[1]):
        m = int(lanes[9, g])
        if (m >> 52) & 3 != 2:
            continue
        mover = (((m >> 27) & 3) + ((m >> 24) & 7)) & 3
        others = [o for o in range(4) if o != mover]
        sizes = [bin(int(lanes[o, g])).count("1") for o in others]
        pool = [c for o in others for c in PM.cards_of(lanes[o, g])]
        pool = [pool[i] for i in rnd.permutation(len(pool))]
        at = 0
        hands = {}
        for o, k in zip(others, sizes):
            hands[o] = sum(1 << c for c in pool[at:at + k])
            at += k
            changed += hands[o] != int(lanes[o, g])
            a[o, g] = b[o, g] = U(hands[o])
        king, declarer, team = (m >> 39) & 7, (m >> 37) & 3, (m >> 42) & 15
        if king != 7:
            holder = [o for o in others if (hands[o] >> (8 * king + 7)) & 1]
            if holder:
                team = (1 << declarer) | (1 << holder[0])
        b[9, g] = U((m & ~(15 << 42)) | (team << 42))
    return a, b, changed


@pytest.mark.parametrize("cards", [5, 22])
def test_the_result_depends_on_the_information_set_alone(T, cards):
    """The test that says "fair": 200 games and their twins, in which the three hands the mover cannot see are re-dealt
    among their seats — once with the team field left as it was, once with the twin's true team.  The determinized
    launch at (4, 2) gives the same bytes on all three; the open-hand launch does not (so this test can fail)."""
    from oracle import tarok_spec as S
    envs = [make_env(T, 200, S.MIX_ALL, cards) for _ in range(3)]
    try:
        lanes = envs[0].state()
        a, b, changed = redealt_twin(lanes, np.random.RandomState(100 + cards))
        assert changed > 200
        assert (a[9] != b[9]).sum() >= 5                     # games whose partner sits elsewhere in the twin
        envs[1].set_state(a)
        envs[2].set_state(b)
        assert (envs[1].state() == a).all() and (envs[2].state() == b).all()
        s0, a0 = launch(envs[0], 4, 2, salt=5)
        assert s0.any()
        for e in envs[1:]:
            s, act = launch(e, 4, 2, salt=5)
            assert s.tobytes() == s0.tobytes() and act.tobytes() == a0.tobytes()
        o0, _ = launch(envs[0], None, 8, salt=5)
        o1, _ = launch(envs[2], None, 8, salt=5)
        assert (o0 != o1).any(axis=(1, 2)).sum() >= 1         # the open hands are not a function of the information set
    finally:
        for e in envs:
            e.close()


def test_read_only_deterministic_and_salted(T):
    import torch
    from oracle import tarok_spec as S
    envs = [T.TarokVecEnv(300, seed=SEED, mix=S.MIX_ALL, game_offset=OFFSET, history=True) for _ in range(2)]
    env, twin = envs
    try:
        for e in envs:
            e.reset(episode=EPISODE)
            e.set_play_mode(0.5, 0.25)
            for _ in range(9):
                e.step_random(auto_reset=True)
        snap = lambda: (env.state().copy(), env.counters(), env.get_history().cpu().numpy().copy(), env.play_mode)
        before = snap()
        s1, a1 = launch(env, 3, 2)
        after = snap()
        assert (before[0] == after[0]).all() and (before[2] == after[2]).all() and before[3] == after[3]
        assert (before[1][0] == after[1][0]).all() and (before[1][1] == after[1][1]).all()
        s2, a2 = launch(env, 3, 2)
        assert s1.tobytes() == s2.tobytes() and a1.tobytes() == a2.tobytes()
        s3, _ = launch(env, 3, 2, salt=1)
        assert (s3 != s1).any()
        for e in envs:                                   # the twin never ran a playout: the same games from here on,
            e.run_random(96, auto_reset=True)            # next-game lines included
        torch.cuda.synchronize()
        assert (env.state() == twin.state()).all()
        ce, ct = env.counters(), twin.counters()
        assert (ce[0] == ct[0]).all() and (ce[1] == ct[1]).all()
        assert (env.get_history().cpu().numpy() == twin.get_history().cpu().numpy()).all()
    finally:
        for e in envs:
            e.close()


def test_a_game_does_not_depend_on_the_batch_around_it(T):
    """The first 77 games of an env of 300 and an env of 77 (another grid, another ragged tail): the same rows."""
    from oracle import tarok_spec as S
    big, small = make_env(T, 300, S.MIX_ALL, 9), make_env(T, 77, S.MIX_ALL, 9)
    try:
        assert (big.state()[:, :77] == small.state()).all()
        for worlds, samples in ((2, 1), (6, 2)):
            sb, ab = launch(big, worlds, samples)
            ss, as_ = launch(small, worlds, samples)
            assert (sb[:77] == ss).all() and (ab[:77] == as_).all()
    finally:
        big.close()
        small.close()


def test_python_surface_and_the_open_hand_call_unchanged(T):
    """playout_cards_det equals the direct C call; playout_cards (the open-hand call) still equals tarok_playout_cards
    byte for byte; playout_values with the divisor worlds * samples."""
    from oracle import tarok_spec as S
    import playout_model as PM
    from tarok_amd.env import playout_values
    env = make_env(T, 64, S.MIX_ALL, 6)
    try:
        s_open, a_open = launch(env, None, 3, salt=4)
        sums, acts = env.playout_cards(3, salt=4)
        assert (sums.cpu().numpy() == s_open).all() and (acts.cpu().numpy() == a_open).all()
        s_det, a_det = launch(env, 3, 2, salt=4)
        sums, acts = env.playout_cards_det(3, 2, salt=4)
        assert (sums.cpu().numpy() == s_det).all() and (acts.cpu().numpy() == a_det).all()
        assert (s_det != s_open).any()
        words = env.legal_actions().words
        got = playout_values(sums, words, 6).cpu().numpy()
        want = PM.playout_values_loop(sums.cpu().numpy(), words.cpu().numpy().view(U), 6)
        assert (got.view(np.uint32) == want.view(np.uint32)).all()
    finally:
        env.close()


def test_evaluate_playout_vs_bot_with_worlds_replays_on_the_oracle(T):
    """64 deals, 3 worlds, 2 samples: every card of every pass and the returned dict equal a replay on the oracle with
    the determinized model's cards.  (No threshold on the advantage: DESIGN 8.4 has the model's figure.)"""
    import playout_det_model as DM
    from oracle import tarok_spec as S
    from tarok_amd import evaluate as EV
    seen = []
    got = EV.evaluate_playout_vs_bot(2, 64, 1, seed=5, inspect=seen, worlds=3)
    assert [p["seats"] for p in seen] == list(EV.PASS_SEATS)
    scores = np.zeros((5, 64, 4), np.int32)
    for p, rec in enumerate(seen):
        for i in range(64):
            actions, sc = DM.replay_pass(5, S.MIX_BOT, i, 0, rec["seats"], 3, 2)
            assert rec["actions"][:, i].tolist() == actions, (p, i)
            assert rec["scores"][i].tolist() == sc, (p, i)
            scores[p, i] = sc
    want = EV.duplicate_advantage(scores)
    assert got == want or (np.isnan(got["stderr"]) and np.isnan(want["stderr"]))


SANITY_SUM = 8197        # = advantage 4.00244140625 points per game over 4 * 512 paired scores (stderr 0.45: nine of them)


def test_the_determinized_player_beats_the_bot(T):
    """Sanity, not a bar on play strength: on 512 deals (seed 0, MIX_BOT) at (worlds, samples) = (8, 2) the fair player's
    summed duplicate advantage over the Bot is positive.  SANITY_SUM is that sum as the CPU model ALONE gives it for
    these very arguments (tools/playout_det_advantage.py: tests/playout_det_model.replay_pass over the five passes);
    it is nine standard errors above zero, so the sign is asserted, and the GPU must equal the figure."""
    from tarok_amd import evaluate as EV
    got = EV.evaluate_playout_vs_bot(2, 512, 1, seed=0, worlds=8)
    assert SANITY_SUM > 0
    assert got["deals"] == 512 and got["advantage"] == SANITY_SUM / 2048.0
    assert got["policy_mean"] == -1.02001953125 and got["bot_mean"] == -5.0224609375          # (the model's, likewise)
