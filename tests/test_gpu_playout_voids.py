"""GPU: tarok_playout_cards_voids (determinized playouts whose worlds honour shown voids) and the surface built on it,
checked exactly — integers against integers — against the per-game model of tests/playout_voids_model.py, which rebuilds
every void word from the history, deals every world and plays every playout on the CPU oracle.  Outputs sit inside guard
bands (tests/guarded.py).  The launch helpers are tests/gpu_harness.py's.

Run on the GPU box:  python -m pytest tests/test_gpu_playout_voids.py -m gpu -q
"""
import functools

import numpy as np
import pytest

import gpu_harness as H
from gpu_harness import T, launch_det  # noqa: F401  (T: the module fixture)

pytestmark = pytest.mark.gpu
U = np.uint64
SEED, OFFSET, EPISODE = 41, 1000, 3               # tests/test_gpu_playout_det.py's: the same games
make_env = functools.partial(H.make_env, seed=SEED, offset=OFFSET, episode=EPISODE)


def launch(env, worlds, samples, voids=None, salt=0, seats=15):
    """One launch into guarded outputs: (sum [n,12,4] i32, action [n] u8).  voids: [n] u32 host array; None: the env's own
    (TarokVecEnv.shown_voids)."""
    return H.launch_worlds("voids", env, worlds, samples, voids, salt, seats)


def own_voids(env):
    import playout_voids_model as VM
    lanes, hist = env.state(), env.get_history().cpu().numpy()
    return np.array([VM.voids_of_lanes(lanes[:, g], hist[:, g]) for g in range(env.n)], np.uint32)


def model_scores(env, salt, voids, worlds, samples, seats=15, seed=SEED):
    import playout_voids_model as VM
    lanes = env.state()
    ep, _ = env.counters()
    return [(lanes[:, g].copy(), int(ep[g]), seats,
             VM.playout_scores(lanes[:, g], int(ep[g]), seed, salt, OFFSET + g, seats, worlds, samples, int(voids[g]))) for g in range(env.n)]


def check(env, model, worlds, samples, voids, salt=0, tag=None, seed=SEED):
    import playout_model as PM
    import playout_voids_model as VM
    want_sum = np.stack([VM.sums_of(sc, worlds, samples) for _, _, _, sc in model])
    want_act = np.array([PM.card_of(lanes, seed, OFFSET + g, ep, s, want_sum[g]) for g, (lanes, ep, s, _) in enumerate(model)], np.uint8)
    got_sum, got_act = launch(env, worlds, samples, voids, salt)
    H.assert_cards_equal(got_sum, want_sum, got_act, want_act, tag)
    return got_sum, got_act


def groups(env, voids):
    """Per game in play: how many of the two-seat groups G01, G02, G12 are not empty, and whether a card is forced."""
    import playout_model as PM
    import playout_voids_model as VM
    from oracle import oracle as O
    lanes = env.state()
    two, forced = np.zeros(env.n, int), np.zeros(env.n, bool)
    for g in range(env.n):
        game = O.Game.from_lanes(lanes[:, g])
        if not PM.position(game)[0]:
            continue
        oth = [o for o in range(4) if o != game.seat()]
        pool = 0
        for o in oth:
            pool |= int(game.g.hand[o])
        gr = VM.groups_of(pool, VM.allowed_of(pool, oth, int(voids[g])))
        two[g] = sum(1 for k in ("G01", "G02", "G12") if gr[k])
        forced[g] = any(gr["F"])
    return two, forced


@pytest.mark.parametrize("cards", [5, 13, 22, 34, 46])
def test_every_row_against_the_model_on_every_contract(T, cards):
    """64 games of each of the ten contracts after `cards` Bot cards, under the games' own voids (the launch takes
    TarokVecEnv.shown_voids' words; the model rebuilds them from the history); one model run at (3, 2) serves the
    launches at (3, 1) and (2, 2)."""
    from oracle import tarok_spec as S
    for code in range(10):
        env = make_env(T, 64, S.MIX_FIXED + code, cards, history=True)
        try:
            voids = own_voids(env)
            assert (env.shown_voids().cpu().numpy().view(np.uint32) == voids).all()
            model = model_scores(env, 7, voids, 3, 2)
            for worlds, samples in ((3, 1), (2, 2)):
                check(env, model, worlds, samples, None, salt=7, tag=(code, cards, worlds, samples))
        finally:
            env.close()


def test_the_natural_games_reach_the_two_seat_groups():
    """Counted from the model alone, on the very games of the test above (the Bot's games of SEED, OFFSET, EPISODE): how
    many have at least one two-seat group under their own voids, and how many have two.  The hand-made arrays below
    guarantee every branch whatever the deals; this says the natural ones get there too."""
    import playout_voids_model as VM
    from oracle import tarok_spec as S
    one = two = 0
    for cards in (5, 13, 22, 34, 46):
        for code in range(10):
            for g in range(64):
                game, played, lead = VM.bot_game(SEED, OFFSET + g, EPISODE, S.MIX_FIXED + code, cards)
                if game.done:
                    continue
                oth = [o for o in range(4) if o != game.seat()]
                pool = 0
                for o in oth:
                    pool |= int(game.g.hand[o])
                gr = VM.groups_of(pool, VM.allowed_of(pool, oth, VM.shown_voids(played, lead)))
                k = sum(1 for name in ("G01", "G02", "G12") if gr[name])
                one += k >= 1
                two += k >= 2
    print("natural games with one two-seat group: %d, with two: %d" % (one, two))
    assert one >= 5 and two >= 5, (one, two)


def test_many_worlds_and_a_single_game(T):
    from oracle import tarok_spec as S
    env = make_env(T, 16, S.MIX_ALL, 22, history=True)
    try:
        voids = own_voids(env)
        assert voids.any()
        check(env, model_scores(env, 0, voids, 16, 2), 16, 2, None, tag=(16, 2))
        check(env, model_scores(env, 3, voids, 64, 1), 64, 1, None, salt=3, tag=(64, 1))
    finally:
        env.close()
    for cards in (9, 30):
        env = make_env(T, 1, S.MIX_BOT, cards, history=True)
        try:
            check(env, model_scores(env, 2, own_voids(env), 2, 2), 2, 2, None, salt=2, tag=("n=1", cards))
        finally:
            env.close()


@pytest.mark.parametrize("cards", [13, 34])
def test_hand_made_void_arrays_take_every_branch(T, cards):
    """On 96 games of every contract: the largest sound word of every game (every class a seat truly lacks: forced cards,
    G01 with G02, G12 — asserted from the model), a word that allows a card nowhere (the determinized bytes), random words
    (mostly contradicted by the hands: the fallbacks, some not), and all zeros (tarok_playout_cards_det byte for byte)."""
    import playout_voids_model as VM
    from oracle import oracle as O
    from oracle import tarok_spec as S
    env = make_env(T, 96, S.MIX_ALL, cards, history=True)
    try:
        lanes = env.state()
        true = np.array([VM.true_voids(O.Game.from_lanes(lanes[:, g])) for g in range(96)], np.uint32)
        two, forced = groups(env, true)
        assert forced.sum() >= 5 and (two >= 2).sum() >= 5 and (two == 3).sum() >= 1, (forced.sum(), two)
        check(env, model_scores(env, 5, true, 2, 2), 2, 2, true, salt=5, tag=("true voids", cards))
        rnd = np.random.RandomState(cards)
        words = (rnd.randint(0, 1 << 20, 96) & rnd.randint(0, 1 << 20, 96)).astype(np.uint32) | np.uint32(1 << 27)
        check(env, model_scores(env, 5, words, 2, 2), 2, 2, words, salt=5, tag=("random words", cards))
        d_sum, d_act = launch_det(env, 2, 2, salt=5)
        for tag, w in (("nowhere", np.full(96, (1 << 20) - 1, np.uint32)), ("zeros", np.zeros(96, np.uint32))):
            s, a = launch(env, 2, 2, w, salt=5)
            assert s.tobytes() == d_sum.tobytes() and a.tobytes() == d_act.tobytes(), tag
        s, _ = launch(env, 2, 2, true, salt=5)
        assert (s != d_sum).any()
    finally:
        env.close()


def consistent_twin(lanes, voids, rnd):
    """Canonical lanes with, in every game in play, cards swapped between the hands of the seats other than the mover —
    only swaps after which both cards lie on seats the void word allows — and the twin's TRUE team."""
    import playout_model as PM
    import playout_voids_model as VM
    out = lanes.copy()
    changed = 0
    for g in range(lanes.shape[1]):
        m = int(lanes[9, g])
        if (m >> 52) & 3 != 2:
            continue
        mover = (((m >> 27) & 3) + ((m >> 24) & 7)) & 3
        others = [o for o in range(4) if o != mover]
        hands = {o: int(lanes[o, g]) for o in others}
        bad = {o: VM.class_cards((int(voids[g]) >> (5 * o)) & 31) for o in others}
        for _ in range(60):
            a, b = (others[i] for i in rnd.permutation(3)[:2])
            ca, cb = PM.cards_of(hands[a]), PM.cards_of(hands[b])
            if not ca or not cb:
                continue
            x, y = ca[rnd.randint(len(ca))], cb[rnd.randint(len(cb))]
            if (bad[b] >> x) & 1 or (bad[a] >> y) & 1:
                continue
            hands[a] = hands[a] & ~(1 << x) | (1 << y)
            hands[b] = hands[b] & ~(1 << y) | (1 << x)
        for o in others:
            changed += hands[o] != int(lanes[o, g])
            out[o, g] = U(hands[o])
        king, declarer, team = (m >> 39) & 7, (m >> 37) & 3, (m >> 42) & 15
        if king != 7:
            holder = [o for o in others if (hands[o] >> (8 * king + 7)) & 1]
            if holder:
                team = (1 << declarer) | (1 << holder[0])
        out[9, g] = U((m & ~(15 << 42)) | (team << 42))
    return out, changed


def test_the_result_depends_on_the_information_set_alone(T):
    """128 games after 22 cards and their twins, whose hidden hands are re-dealt consistently with the shown voids (same
    history, so the same words): identical bytes.  The open-hand launch differs, so this test can fail."""
    from oracle import tarok_spec as S
    envs = [make_env(T, 128, S.MIX_ALL, 22, history=True) for _ in range(2)]
    try:
        lanes = envs[0].state()
        voids = own_voids(envs[0])
        twin, changed = consistent_twin(lanes, voids, np.random.RandomState(122))
        assert changed > 128
        envs[1].set_state(twin)
        assert (envs[1].state() == twin).all() and (own_voids(envs[1]) == voids).all()
        s0, a0 = launch(envs[0], 4, 2, None, salt=5)
        s1, a1 = launch(envs[1], 4, 2, None, salt=5)
        assert s0.any() and s0.tobytes() == s1.tobytes() and a0.tobytes() == a1.tobytes()
        o0, _ = launch_det(envs[0], None, 8, salt=5)
        o1, _ = launch_det(envs[1], None, 8, salt=5)
        assert (o0 != o1).any()
    finally:
        for e in envs:
            e.close()


def test_read_only_deterministic_salted_and_independent_of_the_batch(T):
    from oracle import tarok_spec as S
    big, small = make_env(T, 200, S.MIX_ALL, 21, history=True), make_env(T, 77, S.MIX_ALL, 21, history=True)
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
    """playout_cards_voids equals the direct C call, with the env's own words and with given ones; the determinized
    method is unchanged."""
    import torch
    from oracle import tarok_spec as S
    env = make_env(T, 64, S.MIX_ALL, 18, history=True)
    try:
        s_c, a_c = launch(env, 3, 2, None, salt=4)
        sums, acts = env.playout_cards_voids(3, 2, salt=4)
        assert (sums.cpu().numpy() == s_c).all() and (acts.cpu().numpy() == a_c).all()
        words = env.shown_voids()
        assert words.dtype == torch.int32 and words.any()
        sums, acts = env.playout_cards_voids(3, 2, salt=4, voids=words)
        assert (sums.cpu().numpy() == s_c).all() and (acts.cpu().numpy() == a_c).all()
        s_d, a_d = launch_det(env, 3, 2, salt=4)
        sums, acts = env.playout_cards_voids(3, 2, salt=4, voids=torch.zeros_like(words))
        assert (sums.cpu().numpy() == s_d).all() and (acts.cpu().numpy() == a_d).all()
        sums, acts = env.playout_cards_det(3, 2, salt=4)
        assert (sums.cpu().numpy() == s_d).all() and (acts.cpu().numpy() == a_d).all()
        assert (s_d != s_c).any()
    finally:
        env.close()


def test_evaluate_playout_vs_bot_with_voids_replays_on_the_oracle(T):
    """64 deals, 3 worlds, 2 samples: every card of every pass and the returned dict equal a replay on the oracle with
    the void-aware model's cards; the figure is the model's, exactly."""
    import playout_voids_model as VM
    from oracle import tarok_spec as S
    from tarok_amd import evaluate as EV
    seen = []
    got = EV.evaluate_playout_vs_bot(2, 64, 1, seed=5, inspect=seen, worlds=3, voids=True)
    assert [p["seats"] for p in seen] == list(EV.PASS_SEATS)
    scores = np.zeros((5, 64, 4), np.int32)
    for p, rec in enumerate(seen):
        for i in range(64):
            actions, sc = VM.replay_pass(5, S.MIX_BOT, i, 0, rec["seats"], 3, 2)
            assert rec["actions"][:, i].tolist() == actions, (p, i)
            assert rec["scores"][i].tolist() == sc, (p, i)
            scores[p, i] = sc
    want = EV.duplicate_advantage(scores)
    assert got == want
    with pytest.raises(ValueError):
        EV.evaluate_playout_vs_bot(2, 64, 1, voids=True)
