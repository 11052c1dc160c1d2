"""GPU: tarok_bid_values (the bidding head: tarok_playout_bids' array written by the policy's network from the twelve cards
of each hand) and the surface built on it, against tests/bid_head_model.py.  All outputs sit inside guard bands
(tests/guarded.py); every row of value_out, raw_out and feature_words_out is compared.

Why equality.  The weight sets are tests/policy_exact_ref.py's: small integers times a power of two on 0/1
features, so every partial sum of a layer is a multiple of one quantum below 2^24 quanta and float32 accumulation is
exact in ANY order; the two bf16 stores are round-to-nearest-even, which the float64 model writes in.  Set R rounds a
good share of H2 (many exact ties), the sets P walk the fragment order, and set H — a set P with integer W3 and b3 =
integer + 1/2 — makes every output a half-integer, so at scale 1 rintf's ties-to-even decides every value.  The
conditions are asserted on the launches' own inputs before any output is looked at.

Run on the GPU box:  python -m pytest tests/test_gpu_bid_values.py -m gpu -q
"""

import numpy as np
import pytest

from gpu_harness import T  # noqa: F401  (the module fixture)
from bid_values_cases import weight_sets

pytestmark = pytest.mark.gpu

SEED, OFFSET, EPISODE = 2, 3000, 4
DEFAULT, ALL = 0x00F, 0x3FF
SCALE = 1120.0                            # 16 playouts of 1 / 70 points
NS = (1, 32, 33, 100)                     # 32 games per workgroup: one game and 124 padding rows, one full group, a ragged second, four
SENT32 = 0xA5A5A5A5
U = np.uint64


@pytest.fixture(scope="module")
def sets(T):
    import policy_exact_ref as PE
    W = weight_sets()
    return W, {k: PE.kernel_weights(T, w) for k, w in W.items()}


def make_env(T, n, seed=SEED, offset=OFFSET, **kw):
    """An env of n games that has NOT been reset: bidding comes first."""
    from oracle import tarok_spec as S
    return T.TarokVecEnv(n, seed=seed, mix=S.MIX_BOT, game_offset=offset, **kw)


def dev_u8(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.uint8)).cuda()


def perms_of(n, seed=SEED, offset=OFFSET, episode=EPISODE):
    import bid_head_model as HM
    return [HM.own_deal(seed, offset + g, episode) for g in range(n)]


def launch(env, kw, scale=SCALE, contracts=DEFAULT, deals=None, seats=15, per_game=None, episode=EPISODE,
           outs=("value", "raw", "fw")):
    """One tarok_bid_values into guarded outputs: dict of value [n,4,20] i32, raw [n,4,20] f32, fw [n,4,4] u64 (those
    asked for; every word of them written, no stray store)."""
    import torch
    from guarded import Guarded, assert_guards_intact
    from tarok_amd import _native
    n = env.n
    g = dict(value=Guarded("value_out", 1, n, np.int32, inner=(4, 20), device="cuda") if "value" in outs else None,
             raw=Guarded("raw_out", 1, n, np.float32, inner=(4, 20), device="cuda") if "raw" in outs else None,
             fw=Guarded("feature_words_out", 1, n, np.uint64, inner=(4, 4), device="cuda") if "fw" in outs else None)
    d, p = dev_u8(deals), dev_u8(per_game)
    ptr = lambda a: None if a is None else a.ptr
    with torch.cuda.device(env.device):
        _native.check(env.L.tarok_bid_values(env._h, int(episode), env._p(d), *[env._p(t) for t in kw], float(scale), int(contracts),
                                             int(seats), env._p(p), ptr(g["value"]), ptr(g["raw"]), ptr(g["fw"]), env._stream()))
        torch.cuda.synchronize()
    assert_guards_intact(list(g.values()), (n, contracts, seats))
    out = {}
    for k, a in g.items():
        if a is not None:
            assert a.ptr.value % 16 == 0
            out[k] = a.host()[0][0]
            words = np.ascontiguousarray(out[k]).view(np.uint32)
            assert (words != SENT32).all() if k != "fw" else (out[k] != U(0xA5A5A5A5A5A5A5A5)).all(), "a word of %s was not written" % k
    return out


def check(env, W, kw, perms, seats_of, tag, **kwargs):
    """One launch against the model: feature words, raw and value equal for every row."""
    import bid_head_model as HM
    want_v, want_r, want_w = HM.bid_values(perms, W, kwargs.get("scale", SCALE), kwargs.get("contracts", DEFAULT), seats_of)
    got = launch(env, kw, **kwargs)
    assert (got["fw"] == want_w).all(), (tag, "feature words")
    bad = np.nonzero(~((got["raw"] == want_r) | (np.isnan(got["raw"]) & np.isnan(want_r))).all(axis=(1, 2)))[0]
    assert bad.size == 0, (tag, "raw differs", bad[:8], got["raw"][bad[0]].tolist(), want_r[bad[0]].tolist())
    bad = np.nonzero((got["value"] != want_v).any(axis=(1, 2)))[0]
    assert bad.size == 0, (tag, "values differ", bad[:8], got["value"][bad[0]].tolist(), want_v[bad[0]].tolist())
    return got


def test_the_inputs_meet_the_exactness_conditions():
    """Before any kernel output: on the bidders' own feature rows (100 deals x 4 seats) every set keeps float32 exact, R
    rounds at least 5 % of H2 with at least 1 % ties, H gives half-integers that tie both ways."""
    import torch
    import bid_head_model as HM
    import policy_exact_ref as PE
    words = np.array([HM.game_words(p) for p in perms_of(100)], np.uint64).reshape(-1, 4)
    x = torch.from_numpy(HM.expand(words))
    assert 25 <= int(x.sum(1).min()) and int(x.sum(1).max()) <= 40
    W = weight_sets()
    for name, w in W.items():
        r = PE.reference(x, w)
        assert max(PE.exactness(r, w)) < 2 ** 24, name
        assert torch.equal(r["out"].float().double(), r["out"])
        assert (HM.forward(x.numpy(), w)[0] == r["out"].numpy()).all()
    PE.check_conditions_r(PE.reference(x, W["R"]), W["R"])
    y = PE.reference(x, W["H"])["out"].numpy()[:, :19]
    assert (y - np.floor(y) == 0.5).all()
    v = HM.values(y.astype(np.float32), 1.0)
    assert (v % 2 == 0).all() and (v > y).any() and (v < y).any()
    assert HM.values(np.float32([0.5, 1.5, 2.5, -0.5, -2.5]), 1.0).tolist() == [0, 2, 2, 0, -2]


@pytest.mark.parametrize("n", NS)
def test_exact_on_every_weight_set(T, sets, n):
    W, KW = sets
    perms = perms_of(n)
    env = make_env(T, n)
    try:
        for name in ("R", "P1", "P8"):
            got = check(env, W[name], KW[name], perms, [15] * n, (n, name), contracts=ALL)
            assert got["value"][:, :, :19].any() and not got["value"][:, :, 19].any()
        check(env, W["H"], KW["H"], perms, [15] * n, (n, "H"), contracts=ALL, scale=1.0)
        check(env, W["R"], KW["R"], perms, [15] * n, (n, "R default"))
    finally:
        env.close()


def test_the_clamp_and_the_nan_rule(T, sets):
    """b3 = +-1e30 and +inf end at +-2^30; a W3 row holding +inf and -inf makes NaN for every input (inf - inf, or
    0 x inf), which fmaxf turns into -2^30.  The other rows stay exact."""
    import torch
    import policy_exact_ref as PE
    W = [t.clone() for t in sets[0]["P1"]]
    W[5][0], W[5][1], W[5][2] = 1e30, -1e30, float("inf")
    W[5] = W[5].float().double()
    W[4][3, 10], W[4][3, 200] = float("inf"), float("-inf")
    n = 33
    env = make_env(T, n)
    try:
        got = check(env, W, PE.kernel_weights(T, W), perms_of(n), [15] * n, "clamp", contracts=ALL)
        assert (got["value"][:, :, 0] == 2 ** 30).all() and (got["value"][:, :, 1] == -2 ** 30).all()
        assert (got["value"][:, :, 2] == 2 ** 30).all() and np.isinf(got["raw"][:, :, 2]).all()
        assert np.isnan(got["raw"][:, :, 3]).all() and (got["value"][:, :, 3] == -2 ** 30).all()
        assert np.isfinite(got["raw"][:, :, 4:]).all()
    finally:
        env.close()


def test_random_bf16_weights_within_the_derived_bound(T):
    """Gaussian weights rounded to bf16.  raw_out against the float64 forward WITHOUT the bf16 stores, within
    bid_head_model.forward_bound — derived there from the float32 accumulation length (256 products and a bias per
    output) and the two bf16 stores; value_out equals the kernel's own raw_out pushed through the scaling in numpy."""
    import torch
    import bid_head_model as HM
    import policy_exact_ref as PE
    g = torch.Generator(); g.manual_seed(17)
    bf = lambda t: t.to(torch.bfloat16).double()
    W = [bf(torch.randn(256, 256, generator=g) / 8), torch.randn(256, generator=g).float().double() / 4,
         bf(torch.randn(256, 256, generator=g) / 8), torch.randn(256, generator=g).float().double() / 4,
         bf(torch.randn(64, 256, generator=g) / 8), torch.randn(64, generator=g).float().double() / 4]
    n = 100
    perms = perms_of(n)
    env = make_env(T, n)
    try:
        got = launch(env, PE.kernel_weights(T, W), contracts=ALL)
        x = HM.expand(got["fw"].reshape(n * 4, 4))
        y = HM.forward(x, W, stores=False)[0].reshape(n, 4, 64)[:, :, :19]
        bound = HM.forward_bound(x, W).reshape(n, 4, 64)[:, :, :19]
        err = np.abs(got["raw"][:, :, :19].astype(np.float64) - y)
        print("random weights: max error %.3g, max bound %.3g, max |y| %.3g, worst ratio %.3g" % (err.max(), bound.max(), np.abs(y).max(),
                                                                                                (err / bound).max()))
        assert bound.max() < np.abs(y).max(), "the bound says something"
        assert (err <= bound).all()
        want = np.where(HM.keep(15, ALL)[None], HM.values(got["raw"], SCALE), 0)
        assert (got["value"] == want).all() and np.abs(got["value"]).max() > 1000
    finally:
        env.close()


def test_the_zeros(T, sets):
    import bid_head_model as HM
    W, KW = sets
    n = 40
    perms = perms_of(n)
    env = make_env(T, n)
    try:
        for seats in (0, 1, 6, 15):
            got = check(env, W["P8"], KW["P8"], perms, [seats] * n, ("seats", seats), seats=seats, contracts=ALL)
            for v in range(4):
                assert got["value"][:, v].any() == bool((seats >> v) & 1) and got["raw"][:, v].any() == bool((seats >> v) & 1)
        per_game = np.array([(5 * g + 3) & 15 for g in range(n)], np.uint8) | np.uint8(16)       # (bits above the seats are ignored)
        check(env, W["P8"], KW["P8"], perms, per_game, "per game", seats=15, per_game=per_game, contracts=ALL)
        for contracts in (1, 1 << 2, 1 << 7, 1 << 9, DEFAULT, ALL):
            got = check(env, W["R"], KW["R"], perms, [15] * n, ("contracts", contracts), contracts=contracts)
            rows = np.nonzero(HM.keep(15, contracts)[0])[0]
            assert got["value"][:, :, rows].any() and not np.delete(got["value"], rows, axis=2).any()
        # deals given against deals == NULL, and invalid rows
        own = np.array(perms, np.uint8)
        a = launch(env, KW["R"], contracts=ALL)
        b = launch(env, KW["R"], contracts=ALL, deals=own)
        assert all(a[k].tobytes() == b[k].tobytes() for k in a)
        rng = np.random.default_rng(5)
        other = np.stack([rng.permutation(54) for _ in range(n)]).astype(np.uint8)
        other[3, 7] = other[3, 8]                                        # a card twice
        other[33, 50] = 54                                               # no such card
        got = check(env, W["R"], KW["R"], [other[g].tolist() for g in range(n)], [15] * n, "deals given", deals=other, contracts=ALL)
        for g in (3, 33):
            assert not got["value"][g].any() and not got["raw"][g].any() and (got["fw"][g] == [[U(1) << U(54 + v), 0, 0, 0] for v in range(4)]).all()
        assert got["value"][0].any()
    finally:
        env.close()


def test_the_rows_depend_on_the_viewers_hand_alone(T, sets):
    """100 deals and their twins, in which the 42 cards the viewer does not hold are shuffled by numpy: identical rows
    for the viewer."""
    n = 100
    rng = np.random.default_rng(11)
    deals = np.stack([rng.permutation(54) for _ in range(n)]).astype(np.uint8)
    twins = deals.copy()
    for g in range(n):
        v = g & 3
        rest = np.r_[0:12 * v, 12 * v + 12:54]
        twins[g, rest] = rng.permutation(deals[g, rest])
    assert (twins != deals).any(axis=1).all()
    env = make_env(T, n)
    try:
        a = launch(env, sets[1]["R"], contracts=ALL, deals=deals)
        b = launch(env, sets[1]["R"], contracts=ALL, deals=twins)
        for g in range(n):
            for k in a:
                assert a[k][g, g & 3].tobytes() == b[k][g, g & 3].tobytes()
        assert (a["value"] != b["value"]).any()                          # (the other viewers do see the difference)
    finally:
        env.close()


def test_optional_outputs_read_only_and_deterministic(T, sets):
    KW = sets[1]
    n = 24
    env = make_env(T, n, history=True)
    try:
        env.reset(episode=1)
        for _ in range(9):
            env.step_random(auto_reset=False)
        before = (env.state().copy(), env.counters(), env.get_history().cpu().numpy())
        full = launch(env, KW["R"], contracts=ALL)
        after = (env.state(), env.counters(), env.get_history().cpu().numpy())
        assert (before[0] == after[0]).all() and (before[2] == after[2]).all()
        assert (before[1][0] == after[1][0]).all() and (before[1][1] == after[1][1]).all()
        for outs in (("value",), ("raw",), ("fw",), ("value", "fw"), ("raw", "fw"), ("value", "raw")):
            part = launch(env, KW["R"], contracts=ALL, outs=outs)
            assert set(part) == set(outs) and all(part[k].tobytes() == full[k].tobytes() for k in outs)
        again = launch(env, KW["R"], contracts=ALL)
        assert all(again[k].tobytes() == full[k].tobytes() for k in full)
    finally:
        env.close()
    part = make_env(T, 7, offset=OFFSET + 5)                             # batch independence
    try:
        b = launch(part, KW["R"], contracts=ALL)
        assert all(b[k].tobytes() == full[k][5:12].tobytes() for k in b)
    finally:
        part.close()


def test_the_python_surface(T, sets):
    import torch
    KW = sets[1]["P8"]
    n = 40
    env = make_env(T, n)
    try:
        want = launch(env, KW, contracts=ALL)
        v = env.bid_values(EPISODE, KW, SCALE, contracts=ALL)
        assert v.dtype == torch.int32 and tuple(v.shape) == (n, 4, 20) and v.is_cuda and (v.cpu().numpy() == want["value"]).all()
        out = torch.full((n, 4, 20), 7, dtype=torch.int32, device=v.device)
        v2, raw, fw = env.bid_values(EPISODE, KW, SCALE, contracts=ALL, value_out=out, raw=True, feature_words=True)
        assert v2 is out and (out == v).all()
        assert raw.dtype == torch.float32 and (raw.cpu().numpy() == want["raw"]).all()
        assert fw.dtype == torch.int64 and tuple(fw.shape) == (n, 4, 4) and (fw.cpu().numpy().view(np.uint64) == want["fw"]).all()
        _, none, fw3 = env.bid_values(EPISODE, KW, SCALE, feature_words=True)
        assert none is None and (fw3 == fw).all()
        for bad in (0.0, float("nan"), 2.0 ** 21):
            with pytest.raises(Exception):
                env.bid_values(EPISODE, KW, bad)
        with pytest.raises(Exception):
            env.bid_values(EPISODE, KW[:5], SCALE)
    finally:
        env.close()


def test_interchangeable_with_the_teachers_array(T, sets):
    """tarok_bid_round on value_out against the playout model's round on the MODEL's values, thresholds -30, 0 and 40, one
    head bidder per game (seat g % 4) with the full mask; a reset from the round's outputs plays to the end.  Coverage
    is a condition on the model's rounds: at least four contracts and every declarer."""
    import torch
    import bid_head_model as HM
    import playout_bids_model as BM
    from oracle import tarok_spec as S
    W, KW = sets[0]["P8"], sets[1]["P8"]
    n = 100
    perms = perms_of(n)
    per_game = np.array([1 << (g & 3) for g in range(n)], np.uint8)
    model = HM.bid_values(perms, W, SCALE, ALL, per_game)[0]
    env = make_env(T, n)
    try:
        spg = dev_u8(per_game)
        vals = env.bid_values(EPISODE, KW, SCALE, contracts=ALL, seats=0, seats_per_game=spg)
        assert (vals.cpu().numpy() == model).all()
        for threshold in (-30, 0, 40):
            want = np.array([BM.bid_round(S.game_key(SEED, OFFSET + g, EPISODE), model[g], 16, threshold, ALL, int(per_game[g]))
                             for g in range(n)], np.int8)
            assert len(set(want[:, 0].tolist())) >= 4 and set(want[:, 1].tolist()) == {0, 1, 2, 3}, want.tolist()
            c, d, k = env.bid_round(EPISODE, vals, 16, threshold=threshold, contracts=ALL, seats=0, seats_per_game=spg)
            got = torch.stack((c, d, k), 1).cpu().numpy()
            assert (got == want).all(), (threshold, np.nonzero((got != want).any(axis=1))[0][:8])
            env.reset(episode=EPISODE, contract=c, declarer=d, king_suit=k)
            meta = env.state()[9]
            assert not ((meta >> U(54)) & U(1)).any() and (((meta >> U(33)) & U(15)).astype(np.int8) == want[:, 0]).all()
            for _ in range(48):
                env.step_random(auto_reset=False)
            meta = env.state()[9]
            assert (((meta >> U(52)) & U(3)) == 3).all() and not ((meta >> U(54)) & U(1)).any()
    finally:
        env.close()


def test_evaluate_bidnet_vs_bot_replays_on_the_oracle(T, sets):
    import bid_head_model as HM
    from tarok_amd import evaluate as E
    W, KW = sets[0]["P8"], sets[1]["P8"]
    n, seed = 32, 3
    inspect = []
    res = E.evaluate_bidnet_vs_bot(KW, n, 1, seed=seed, contracts=ALL, inspect=inspect)
    assert len(inspect) == 5 and res["deals"] == n
    scores = np.zeros((5, n, 4), np.int64)
    for p, rec in enumerate(inspect):
        assert rec["seats"] == E.PASS_SEATS[p]
        for g in range(n):
            vals, c, d, k, actions, sc = HM.replay_pass(seed, g, 0, rec["seats"], W, SCALE, 16, contracts=ALL)
            assert (rec["values"][g] == vals).all(), (p, g)
            assert (int(rec["contract"][g]), int(rec["declarer"][g]), int(rec["king_suit"][g])) == (c, d, k), (p, g)
            assert rec["actions"][:, g].tolist() == actions and rec["scores"][g].tolist() == sc, (p, g)
            scores[p, g] = sc
    assert res == E.duplicate_advantage(scores)
    # pass 0 is the Bot's own round: evaluate_bidding_vs_bot's pass 0 on the same deals
    plain = []
    E.evaluate_bidding_vs_bot(1, 1, n, 1, seed=seed, inspect=plain)
    assert (plain[0]["scores"] == inspect[0]["scores"]).all() and (plain[0]["start"] == inspect[0]["start"]).all()
    assert (plain[0]["actions"] == inspect[0]["actions"]).all()
    differs = sum(int((inspect[p]["contract"] != inspect[0]["contract"]).sum()) for p in range(1, 5))
    assert differs > 0, "the head bids otherwise than the Bot somewhere"
