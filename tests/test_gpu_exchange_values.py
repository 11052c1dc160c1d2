"""GPU: tarok_exchange_values (the exchange head: the talon group and the discards from the policy's network),
tarok_exchange_candidates and the surface built on them, against tests/exchange_head_model.py.  All outputs sit inside
guard bands (tests/guarded.py); every row of raw_out, choice_out, discards_out, feature_words_out and cand_out is compared.

The games come from a reset with the exchange deferred whose contract, declarer and king arrays cycle through all ten
contract codes x four declarers x four kings, so Klop, Berac and Solo_brez games sit between the waiting ones.  N = 1,
16 (one workgroup), 17 (a ragged second) and 160 (the whole cycle).

Why equality.  The weight sets are tests/policy_exact_ref.py's: small integers times a power of two on 0/1
features, so every partial sum of a layer is a multiple of one quantum below 2^24 quanta and float32 accumulation is
exact in ANY order; the two bf16 stores are round-to-nearest-even, which the float64 model writes in.  The conditions are
asserted on the launches' own inputs before any output is looked at.

Run on the GPU box:  python -m pytest tests/test_gpu_exchange_values.py -m gpu -q
"""

import numpy as np
import pytest

from gpu_harness import T  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

SEED, OFFSET, EPISODE = 2, 5000, 4
NS = (1, 16, 17, 160)
U = np.uint64


def weight_sets():
    """{name: float64 weight set}: R and two sets P of tests/policy_exact_ref.py, and TIE — set P1 with the value
    row and the score rows of cards 0..19 and 32..39 cut down to their biases: every group ties at 1/4 (the lowest
    wins) and those cards tie at 1/2, above every other card of P1 only where the row says so."""
    import policy_exact_ref as PE
    tie = [t.clone() for t in PE.weights_p(*PE.P_PARAMS[1])]
    tie[4][54] = 0
    tie[5][54] = 0.25
    for c in list(range(20)) + list(range(32, 40)):
        tie[4][c] = 0
        tie[5][c] = 0.5
    return dict(R=PE.weights_r(), P1=PE.weights_p(*PE.P_PARAMS[1]), P8=PE.weights_p(*PE.P_PARAMS[8]), TIE=tie)


@pytest.fixture(scope="module")
def sets(T):
    import policy_exact_ref as PE
    W = weight_sets()
    return W, {k: PE.kernel_weights(T, w) for k, w in W.items()}


def setup_arrays(n, shift=1):
    """contract, declarer, king [n] int8: game g is entry g + shift of the cycle (Klop's declarer is seat 0)."""
    j = np.arange(n) + shift
    contract = (j % 10).astype(np.int8)
    declarer = np.where(contract == 0, 0, (j // 10) % 4).astype(np.int8)
    king = ((j // 40) % 4).astype(np.int8)
    return contract, declarer, king


def make_env(T, n, seed=SEED, offset=OFFSET, shift=1, episode=EPISODE, **kw):
    """An env of n games reset with the exchange deferred on the cycle of setups; returns (env, lanes [n][10])."""
    from oracle import tarok_spec as S
    env = T.TarokVecEnv(n, seed=seed, mix=S.MIX_ALL, game_offset=offset, **kw)
    c, d, k = setup_arrays(n, shift)
    env.reset(episode=episode, contract=c, declarer=d, king_suit=k, defer_exchange=True)
    return env, env.state().T.copy()


def dev_u8(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.uint8)).cuda()


def launch(env, kw, seats=15, per_game=None, outs=("raw", "choice", "disc", "fw")):
    """One tarok_exchange_values into guarded outputs: dict of raw [n,8,64] f32, choice [n] i8, disc [n,3] u8, fw [n,8,4]
    u64 (those asked for; every element of them written, no stray store)."""
    import torch
    from guarded import Guarded, assert_guards_intact
    from tarok_amd import _native
    n = env.n
    g = dict(raw=Guarded("raw_out", 1, n, np.float32, inner=(8, 64), device="cuda") if "raw" in outs else None,
             choice=Guarded("choice_out", 1, n, np.int8, device="cuda") if "choice" in outs else None,
             disc=Guarded("discards_out", 1, n, np.uint8, inner=(3,), device="cuda") if "disc" in outs else None,
             fw=Guarded("feature_words_out", 1, n, np.uint64, inner=(8, 4), device="cuda") if "fw" in outs else None)
    p = dev_u8(per_game)
    ptr = lambda a: None if a is None else a.ptr
    with torch.cuda.device(env.device):
        _native.check(env.L.tarok_exchange_values(env._h, *[env._p(t) for t in kw], int(seats), env._p(p), ptr(g["raw"]), ptr(g["choice"]),
                                                  ptr(g["disc"]), ptr(g["fw"]), env._stream()))
        torch.cuda.synchronize()
    assert_guards_intact(list(g.values()), (n, seats))
    out = {}
    for k, a in g.items():
        if a is not None:
            vals, written = a.host()
            out[k] = vals[0]
            if k in ("raw", "fw"):
                assert a.ptr.value % 16 == 0
                assert (np.ascontiguousarray(vals[0]).view(np.uint32) != 0xA5A5A5A5).all(), "a word of %s was not written" % k
            else:
                assert written.all(), "an element of %s was not written" % k     # (choice 165 = -91 and card 165 do not exist)
    return out


def same(a, b):
    return bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def check(env, lanes, W, kw, seats_of, tag, **kwargs):
    """One launch against the model: every row of every output equal."""
    import exchange_head_model as EM
    raw, choice, disc, words = EM.exchange_values(lanes, W, SEED, OFFSET, EPISODE, seats_of)
    got = launch(env, kw, **kwargs)
    assert (got["fw"] == words).all(), (tag, "feature words", np.nonzero((got["fw"] != words).any(axis=(1, 2)))[0][:8])
    bad = np.nonzero([not same(got["raw"][g], raw[g]) for g in range(len(lanes))])[0]
    assert bad.size == 0, (tag, "raw differs", bad[:8])
    assert (got["choice"] == choice).all(), (tag, "choice", np.nonzero(got["choice"] != choice)[0][:8])
    assert (got["disc"] == disc).all(), (tag, "discards", np.nonzero((got["disc"] != disc).any(axis=1))[0][:8])
    return got


def test_the_inputs_meet_the_exactness_conditions():
    """Before any kernel output: on the rows of 160 oracle games of the cycle every set keeps float32 exact, and the cycle
    holds what the tests lean on: all six exchange contracts, every declarer, and all three places of the called king."""
    import torch
    import exchange_head_model as EM
    import policy_exact_ref as PE
    from oracle import oracle as O
    from oracle import tarok_spec as S
    c, d, k = setup_arrays(160)
    games = [O.Game(S.deal(S.game_key(SEED, OFFSET + g, EPISODE)), int(c[g]), int(d[g]), int(k[g]) if 1 <= c[g] <= 3 else -1)
             for g in range(160)]
    waiting = [g for g in games if EM.XM.waiting(g)]
    assert {int(g.g.contract) for g in waiting} == set(range(1, 7)) and {int(g.g.declarer) for g in waiting} == {0, 1, 2, 3}
    words = np.array([EM.game_words(g) for g in waiting], np.uint64)
    assert {int(w) for w in ((words[:, :, 2] >> U(54)) & U(7)).ravel()} == {0, 1, 2, 4}
    live = words[:, :, 0] != 0
    assert sorted(set(live.sum(1).tolist())) == [2, 3, 6]
    x = torch.from_numpy(EM.expand(words[live]))
    assert 30 <= int(x.sum(1).min()) and int(x.sum(1).max()) <= 80
    for name, w in weight_sets().items():
        r = PE.reference(x, w)
        assert max(PE.exactness(r, w)) < 2 ** 24, name
        assert torch.equal(r["out"].float().double(), r["out"])
        assert (EM.forward(x.numpy(), w)[0] == r["out"].numpy()).all()


@pytest.mark.parametrize("n", NS)
def test_exact_on_every_weight_set(T, sets, n):
    W, KW = sets
    env, lanes = make_env(T, n)
    try:
        for name in ("R", "P1", "P8", "TIE"):
            got = check(env, lanes, W[name], KW[name], [15] * n, (n, name))
            assert got["raw"].any() and (got["choice"] >= 0).any()
    finally:
        env.close()


def test_ties_in_value_and_in_score(T, sets):
    """Set TIE: every group of a game has the same value, so group 0 is chosen; the tied cards go by card number."""
    W, KW = sets
    env, lanes = make_env(T, 160)
    try:
        got = check(env, lanes, W["TIE"], KW["TIE"], [15] * 160, "tie")
        part = got["choice"] >= 0
        assert part.any() and (got["choice"][part] == 0).all()
        assert (got["raw"][part][:, 0, 54] == 0.25).all()
        d, y = got["disc"][part].astype(np.int64), got["raw"][part][:, 0]
        two = np.nonzero(d[:, 1] != 255)[0]
        tied = two[y[two, d[two, 0]] == y[two, d[two, 1]]]
        assert tied.size > 10 and (d[tied, 0] < d[tied, 1]).all()        # a tie in score goes to the lower card
    finally:
        env.close()


def test_nan_and_infinities_still_give_a_valid_exchange(T, sets):
    """b3[54] = NaN: every group's value is -inf after clean(), group 0 wins.  Score biases of +inf, -inf and a W3 row
    holding +inf and -inf (NaN for the rows that light both, else +-inf) still give the model's discards."""
    import policy_exact_ref as PE
    env, lanes = make_env(T, 160)
    try:
        W = [t.clone() for t in sets[0]["P1"]]
        W[5][54] = float("nan")
        W[5][0], W[5][1], W[5][33] = float("inf"), float("-inf"), float("inf")
        W[4][2, 10], W[4][2, 200] = float("inf"), float("-inf")
        W[4][34] = 0
        W[5][34] = float("nan")
        got = check(env, lanes, W, PE.kernel_weights(T, W), [15] * 160, "nan")
        part = got["choice"] >= 0
        assert (got["choice"][part] == 0).all() and np.isnan(got["raw"][part][:, 0, 54]).all()
        assert np.isnan(got["raw"][part][:, 0, 34]).all() and np.isinf(got["raw"][part][:, 0, 0]).all()
        W = [t.clone() for t in sets[0]["P8"]]
        W[5][54] = float("inf")                                           # every group +inf: a tie at the top
        got = check(env, lanes, W, PE.kernel_weights(T, W), [15] * 160, "inf")
        assert (got["choice"][got["choice"] >= 0] == 0).all()
        W[5][54] = float("-inf")
        check(env, lanes, W, PE.kernel_weights(T, W), [15] * 160, "-inf")
    finally:
        env.close()


def test_random_bf16_weights_within_the_derived_bound(T):
    """Gaussian weights rounded to bf16.  raw_out against the float64 forward WITHOUT the bf16 stores, within
    exchange_head_model.forward_bound — derived there from the float32 accumulation length (256 products and a bias per
    output) and the two bf16 stores; choice_out and discards_out equal the kernel's own raw_out pushed through the
    model's selection."""
    import torch
    import exchange_head_model as EM
    import policy_exact_ref as PE
    from oracle import oracle as O
    g = torch.Generator(); g.manual_seed(17)
    bf = lambda t: t.to(torch.bfloat16).double()
    W = [bf(torch.randn(256, 256, generator=g) / 8), torch.randn(256, generator=g).float().double() / 4,
         bf(torch.randn(256, 256, generator=g) / 8), torch.randn(256, generator=g).float().double() / 4,
         bf(torch.randn(64, 256, generator=g) / 8), torch.randn(64, generator=g).float().double() / 4]
    n = 160
    env, lanes = make_env(T, n)
    try:
        got = launch(env, PE.kernel_weights(T, W))
        live = got["fw"][:, :, 0] != 0
        x = EM.expand(got["fw"][live])
        y = EM.forward(x, W, stores=False)[0]
        bound = EM.forward_bound(x, W)
        err = np.abs(got["raw"][live].astype(np.float64) - y)
        print("random weights: max error %.3g, max bound %.3g, max |y| %.3g, worst ratio %.3g" % (err.max(), bound.max(), np.abs(y).max(),
                                                                                                (err / bound).max()))
        assert bound.max() < np.abs(y).max(), "the bound says something"
        assert (err <= bound).all() and not got["raw"][~live].any()
        choice, disc = EM.decisions([O.Game.from_lanes(l) for l in lanes], got["raw"], SEED, OFFSET, EPISODE, [15] * n)
        assert (got["choice"] == choice).all() and (got["disc"] == disc).all()
        assert len(set(got["choice"].tolist())) >= 4
    finally:
        env.close()


def test_seat_sets_and_the_three_cases(T, sets):
    import torch
    W, KW = sets
    n = 160
    env, lanes = make_env(T, n)
    meta = lanes[:, 9]
    waiting = ((meta >> U(52)) & U(3)) == 1
    declarer = ((meta >> U(37)) & U(3)).astype(np.int64)
    assert waiting.sum() == 96
    try:
        for seats in (0, 1, 6, 15):
            got = check(env, lanes, W["P8"], KW["P8"], [seats] * n, ("seats", seats), seats=seats)
            part = waiting & (((seats >> declarer) & 1) == 1)
            assert ((got["fw"][:, 0, 0] != 0) == part).all() and (got["raw"].any(axis=(1, 2)) == part).all()
            assert ((got["choice"] == -1) == ~waiting).all() and (got["disc"][~waiting] == 255).all()
            assert (got["choice"][waiting & ~part] == 0).all() and (got["disc"][waiting, 0] < 54).all()
        per_game = np.array([(5 * g + 3) & 15 for g in range(n)], np.uint8) | np.uint8(16)       # (bits above the seats are ignored)
        check(env, lanes, W["P8"], KW["P8"], per_game, "per game", seats=15, per_game=per_game)
        # seat set 0 is the Bot's own exchange: a twin env's tarok_exchange(NULL, NULL), read back
        bot = launch(env, KW["P8"], seats=0)
        env.exchange(dev_u8(bot["choice"].view(np.uint8)).view(torch.int8), dev_u8(bot["disc"]))
        twin, _ = make_env(T, n)
        try:
            twin.exchange()
            assert (twin.state() == env.state()).all()
        finally:
            twin.close()
    finally:
        env.close()


def test_optional_outputs_read_only_and_deterministic(T, sets):
    import torch
    from tarok_amd import _native
    KW = sets[1]
    n = 40
    env, lanes = make_env(T, n, history=True)
    try:
        before = (env.state().copy(), env.counters(), env.get_history().cpu().numpy())
        full = launch(env, KW["R"])
        after = (env.state(), env.counters(), env.get_history().cpu().numpy())
        assert (before[0] == after[0]).all() and (before[2] == after[2]).all()
        assert (before[1][0] == after[1][0]).all() and (before[1][1] == after[1][1]).all()
        for outs in (("raw",), ("choice",), ("disc",), ("fw",), ("choice", "disc"), ("raw", "fw")):
            part = launch(env, KW["R"], outs=outs)
            assert set(part) == set(outs) and all(part[k].tobytes() == full[k].tobytes() for k in outs)
        assert launch(env, KW["R"], outs=()) == {}                      # all four NULL: TAROK_OK, nothing to write
        again = launch(env, KW["R"])
        assert all(again[k].tobytes() == full[k].tobytes() for k in full)
        assert _native.lib().tarok_exchange_values(env._h, *[env._p(t) for t in KW["R"]], 16, None, None, None, None, None, None) != 0
    finally:
        env.close()
    part, _ = make_env(T, 7, offset=OFFSET + 5, shift=6)               # batch independence: games 5..11 on their own
    try:
        b = launch(part, KW["R"])
        assert all(b[k].tobytes() == full[k][5:12].tobytes() for k in b)
    finally:
        part.close()


def test_the_python_surface_and_a_game_played_to_the_end(T, sets):
    import torch
    KW = sets[1]["P8"]
    n = 160
    env, lanes = make_env(T, n)
    try:
        want = launch(env, KW)
        choice, disc = env.exchange_values(KW)
        assert choice.dtype == torch.int8 and disc.dtype == torch.uint8 and tuple(disc.shape) == (n, 3)
        assert (choice.cpu().numpy() == want["choice"]).all() and (disc.cpu().numpy() == want["disc"]).all()
        c2, d2, raw, fw = env.exchange_values(KW, raw=True, feature_words=True, choice_out=choice, discards_out=disc)
        assert c2 is choice and d2 is disc and same(raw.cpu().numpy(), want["raw"])
        assert fw.dtype == torch.int64 and (fw.cpu().numpy().view(np.uint64) == want["fw"]).all()
        with pytest.raises(Exception):
            env.exchange_values(KW[:5])
        with pytest.raises(Exception):
            env.exchange_values(KW, seats=16)
        env.exchange(choice, disc)
        meta = env.state()[9]
        assert not ((meta >> U(54)) & U(1)).any() and (((meta >> U(52)) & U(3)) == 2).all()
        for _ in range(48):
            env.step_random(auto_reset=False)
        meta = env.state()[9]
        assert (((meta >> U(52)) & U(3)) == 3).all() and not ((meta >> U(54)) & U(1)).any()
    finally:
        env.close()


@pytest.mark.parametrize("sets_d", (1, 4, 8))
def test_candidates_equal_the_model_and_the_teachers_discards(T, sets_d):
    import torch
    from guarded import Guarded, assert_guards_intact
    import exchange_head_model as EM
    from tarok_amd import _native
    n, salt = 160, 9
    env, lanes = make_env(T, n)
    try:
        for seats in (15, 6):
            out = Guarded("cand_out", 1, n, np.uint8, inner=(6 * sets_d, 3), device="cuda")
            with torch.cuda.device(env.device):
                _native.check(env.L.tarok_exchange_candidates(env._h, sets_d, salt, seats, None, out.ptr, env._stream()))
                torch.cuda.synchronize()
            assert_guards_intact([out], (sets_d, seats))
            vals, written = out.host()
            assert written.all()
            want = np.array([EM.candidates(lanes[g], EPISODE, SEED, salt, OFFSET + g, seats, sets_d) for g in range(n)], np.uint8)
            assert (vals[0] == want).all(), np.nonzero((vals[0] != want).any(axis=(1, 2)))[0][:8]
            assert (env.exchange_candidates(sets_d, salt=salt, seats=seats).cpu().numpy() == want).all()
        sums, choice, disc = env.playout_exchange(2, 1, sets_d, salt=salt)
        cand = env.exchange_candidates(sets_d, salt=salt).cpu().numpy()
        sums, choice, disc = sums.cpu().numpy(), choice.cpu().numpy(), disc.cpu().numpy()
        declarer = ((lanes[:, 9] >> U(37)) & U(3)).astype(np.int64)
        took = 0
        for g in range(n):
            if (cand[g] != 255).any():
                own = sums[g, :, declarer[g]]
                rows = (6 // int((cand[g, 0] != 255).sum())) * sets_d
                best = int(np.argmax(own[:rows]))                     # (the first candidate at the maximum)
                assert best // sets_d == choice[g] and (cand[g, best] == disc[g]).all(), g
                took += 1
        assert took == 96
        for bad in ((0, 15), (9, 15), (4, 16), (4, -1)):
            assert _native.lib().tarok_exchange_candidates(env._h, bad[0], 0, bad[1], None, out.ptr, None) != 0
    finally:
        env.close()


def test_evaluate_exchangenet_vs_bot_replays_on_the_oracle(T, sets):
    import exchange_head_model as EM
    from oracle import tarok_spec as S
    from tarok_amd import evaluate as E
    W, KW = sets[0]["P8"], sets[1]["P8"]
    n, seed = 32, 3
    inspect = []
    res = E.evaluate_exchangenet_vs_bot(KW, n, 1, seed=seed, inspect=inspect)
    assert len(inspect) == 5 and res["deals"] == n
    scores = np.zeros((5, n, 4), np.int64)
    for p, rec in enumerate(inspect):
        assert rec["seats"] == E.PASS_SEATS[p]
        for g in range(n):
            choice, disc, actions, sc = EM.replay_pass(seed, S.MIX_BOT, g, 0, rec["seats"], W)
            assert (int(rec["choice"][g]), rec["discards"][g].tolist()) == (choice, disc), (p, g)
            assert rec["actions"][:, g].tolist() == actions and rec["scores"][g].tolist() == sc, (p, g)
            scores[p, g] = sc
    assert res == E.duplicate_advantage(scores)
    # pass 0 is the Bot's own exchange: evaluate_exchange_vs_bot's pass 0 on the same deals
    plain = []
    E.evaluate_exchange_vs_bot(1, 1, 1, n, 1, seed=seed, inspect=plain)
    for k in ("scores", "start", "actions", "choice", "discards"):
        assert (plain[0][k] == inspect[0][k]).all(), k
    differs = sum(int((inspect[p]["discards"] != inspect[0]["discards"]).any(axis=1).sum()) for p in range(1, 5))
    assert differs > 0, "the head exchanges otherwise than the Bot somewhere"
