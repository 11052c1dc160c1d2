"""GPU: tarok_bid_values_pass (the bidding head with output 19 as the value of a pass) and BidLearner(pass_value=True),
against tests/bid_head_model.py's float64 forward with the bf16 stores written in.  Row 19 of value_out and raw_out must
EQUAL the model; rows 0..18 are held byte for byte to tarok_bid_values at the same arguments.  All outputs sit inside
guard bands (tests/guarded.py).  A library without the new entry FAILS these tests: nothing here skips.

Why equality: the weight sets are tests/test_gpu_bid_values.py's — small integers times a power of two on 0/1 features,
float32 accumulation exact in any order — and the conditions are asserted on this file's own inputs, output 19 included,
before any kernel output is looked at.

Run on the GPU box:  python -m pytest tests/test_gpu_bid_values_pass.py -m gpu -q
"""

import numpy as np
import pytest

from gpu_harness import T  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

SEED, OFFSET, EPISODE = 2, 3000, 4
DEFAULT, ALL = 0x00F, 0x3FF
SCALE = 1120.0                            # 16 playouts of 1 / 70 points
NS = (1, 16, 17, 160)                     # 32 games per workgroup: one game, half a group, an odd half, five groups
SENT32 = 0xA5A5A5A5
U = np.uint64
PASS = 19


@pytest.fixture(scope="module")
def sets(T):
    import bid_values_cases as BV
    import policy_exact_ref as PE
    W = BV.weight_sets()
    return W, {k: PE.kernel_weights(T, w) for k, w in W.items()}


def make_env(T, n, seed=SEED, offset=OFFSET, **kw):
    from oracle import tarok_spec as S
    return T.TarokVecEnv(n, seed=seed, mix=S.MIX_BOT, game_offset=offset, **kw)


def dev_u8(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.uint8)).cuda()


def perms_of(n, seed=SEED, offset=OFFSET, episode=EPISODE):
    import bid_head_model as HM
    return [HM.own_deal(seed, offset + g, episode) for g in range(n)]


def launch(env, kw, scale=SCALE, contracts=DEFAULT, deals=None, seats=15, per_game=None, episode=EPISODE, entry="tarok_bid_values_pass"):
    """One launch of `entry` into guarded outputs: value [n,4,20] i32, raw [n,4,20] f32, fw [n,4,4] u64, every word written."""
    import torch
    from guarded import Guarded, assert_guards_intact
    from tarok_amd import _native
    n = env.n
    g = dict(value=Guarded("value_out", 1, n, np.int32, inner=(4, 20), device="cuda"),
             raw=Guarded("raw_out", 1, n, np.float32, inner=(4, 20), device="cuda"),
             fw=Guarded("feature_words_out", 1, n, np.uint64, inner=(4, 4), device="cuda"))
    d, p = dev_u8(deals), dev_u8(per_game)
    with torch.cuda.device(env.device):
        _native.check(getattr(env.L, entry)(env._h, int(episode), env._p(d), *[env._p(t) for t in kw], float(scale), int(contracts),
                                            int(seats), env._p(p), g["value"].ptr, g["raw"].ptr, g["fw"].ptr, env._stream()))
        torch.cuda.synchronize()
    assert_guards_intact(list(g.values()), (entry, n, contracts, seats))
    out = {}
    for k, a in g.items():
        out[k] = a.host()[0][0]
        words = np.ascontiguousarray(out[k]).view(np.uint32)
        assert (words != SENT32).all() if k != "fw" else (out[k] != U(0xA5A5A5A5A5A5A5A5)).all(), "a word of %s was not written" % k
    return out


def model_pass_row(perms, W, scale, seats_of):
    """(value [n, 4] int32, raw [n, 4] float32) of row 19: output 19 of the float64 forward with the bf16 stores written
    in, scaled, clamped and rounded as bid_head_model.values does; zeros for a seat outside the set and an invalid deal."""
    import bid_head_model as HM
    import playout_bids_model as BM
    n = len(perms)
    words = np.array([HM.game_words(p) for p in perms], np.uint64)
    y = HM.forward(HM.expand(words.reshape(n * 4, 4)), W, stores=True)[0].reshape(n, 4, 64)[:, :, PASS].astype(np.float32)
    live = np.array([[BM.valid_perm(perms[g]) and bool((int(seats_of[g]) >> v) & 1) for v in range(4)] for g in range(n)])
    return np.where(live, HM.values(y, scale), 0).astype(np.int32), np.where(live, y, np.float32(0))


def check(env, W, kw, perms, seats_of, tag, **kwargs):
    """Row 19 against the model, everything else byte for byte against tarok_bid_values, whose row 19 is zero."""
    got = launch(env, kw, **kwargs)
    plain = launch(env, kw, entry="tarok_bid_values", **kwargs)
    for k in ("value", "raw"):
        assert got[k][:, :, :PASS].tobytes() == plain[k][:, :, :PASS].tobytes(), (tag, k, "rows 0..18 differ from tarok_bid_values")
        assert not plain[k][:, :, PASS].any()
    assert got["fw"].tobytes() == plain["fw"].tobytes()
    want_v, want_r = model_pass_row(perms, W, kwargs.get("scale", SCALE), seats_of)
    r = got["raw"][:, :, PASS]
    bad = np.nonzero(~((r == want_r) | (np.isnan(r) & np.isnan(want_r))).all(axis=1))[0]
    assert bad.size == 0, (tag, "raw row 19 differs", bad[:8], r[bad[0]].tolist(), want_r[bad[0]].tolist())
    bad = np.nonzero((got["value"][:, :, PASS] != want_v).any(axis=1))[0]
    assert bad.size == 0, (tag, "value row 19 differs", bad[:8], got["value"][bad[0], :, PASS].tolist(), want_v[bad[0]].tolist())
    return got


def test_the_inputs_meet_the_exactness_conditions():
    """Before any kernel output: on this file's own feature rows (160 deals x 4 seats) every set keeps float32 exact in
    any order on all 64 outputs, so on output 19; set H makes output 19 a half-integer that ties both ways at scale 1."""
    import torch
    import bid_head_model as HM
    import bid_values_cases as BV
    import policy_exact_ref as PE
    words = np.array([HM.game_words(p) for p in perms_of(160)], np.uint64).reshape(-1, 4)
    x = torch.from_numpy(HM.expand(words))
    W = BV.weight_sets()
    for name, w in W.items():
        r = PE.reference(x, w)
        assert max(PE.exactness(r, w)) < 2 ** 24, name
        assert torch.equal(r["out"].float().double(), r["out"])
        assert (HM.forward(x.numpy(), w)[0] == r["out"].numpy()).all()
        assert len(set(r["out"][:, PASS].tolist())) > 8, (name, "output 19 varies over the rows")
    y = PE.reference(x, W["H"])["out"].numpy()[:, PASS]
    assert (y - np.floor(y) == 0.5).all()
    v = HM.values(y.astype(np.float32), 1.0)
    assert (v % 2 == 0).all() and (v > y).any() and (v < y).any()


@pytest.mark.parametrize("n", NS)
def test_row_19_is_output_19_on_every_weight_set(T, sets, n):
    W, KW = sets
    perms = perms_of(n)
    env = make_env(T, n)
    try:
        for name in ("R", "P1", "P8"):
            got = check(env, W[name], KW[name], perms, [15] * n, (n, name), contracts=ALL)
            assert got["raw"][:, :, PASS].any()
        check(env, W["H"], KW["H"], perms, [15] * n, (n, "H"), contracts=ALL, scale=1.0)
        check(env, W["R"], KW["R"], perms, [15] * n, (n, "R default"))
    finally:
        env.close()


def test_a_nan_and_an_output_beyond_the_clamp_in_output_19(T, sets):
    import policy_exact_ref as PE
    n = 33
    perms = perms_of(n)
    env = make_env(T, n)
    try:
        for b3, raw_is, value in ((1e30, np.isfinite, 2 ** 30), (-1e30, np.isfinite, -2 ** 30), (float("inf"), np.isinf, 2 ** 30)):
            W = [t.clone() for t in sets[0]["P1"]]
            W[5][PASS] = b3
            W[5] = W[5].float().double()
            got = check(env, W, PE.kernel_weights(T, W), perms, [15] * n, ("clamp", b3), contracts=ALL)
            assert (got["value"][:, :, PASS] == value).all() and raw_is(got["raw"][:, :, PASS]).all()
        W = [t.clone() for t in sets[0]["P1"]]
        W[4][PASS, 10], W[4][PASS, 200] = float("inf"), float("-inf")   # inf - inf, or 0 x inf: NaN for every input
        got = check(env, W, PE.kernel_weights(T, W), perms, [15] * n, "nan", contracts=ALL)
        assert np.isnan(got["raw"][:, :, PASS]).all() and (got["value"][:, :, PASS] == -2 ** 30).all()
        assert np.isfinite(got["raw"][:, :, :PASS]).all()
    finally:
        env.close()


def test_the_zeros_and_row_19_does_not_depend_on_contracts(T, sets):
    W, KW = sets
    n = 40
    perms = perms_of(n)
    env = make_env(T, n)
    try:
        for seats in (0, 1, 6, 15):
            got = check(env, W["P8"], KW["P8"], perms, [seats] * n, ("seats", seats), seats=seats, contracts=ALL)
            for v in range(4):
                assert got["raw"][:, v, PASS].any() == bool((seats >> v) & 1)
        per_game = np.array([(5 * g + 3) & 15 for g in range(n)], np.uint8) | np.uint8(16)       # (bits above the seats are ignored)
        check(env, W["P8"], KW["P8"], perms, per_game, "per game", seats=15, per_game=per_game, contracts=ALL)
        full = check(env, W["R"], KW["R"], perms, [15] * n, "all contracts", contracts=ALL)
        for contracts in (1, 1 << 2, 1 << 9, DEFAULT):
            got = check(env, W["R"], KW["R"], perms, [15] * n, ("contracts", contracts), contracts=contracts)
            for k in ("value", "raw"):
                assert got[k][:, :, PASS].tobytes() == full[k][:, :, PASS].tobytes(), (k, contracts)
        rng = np.random.default_rng(5)
        other = np.stack([rng.permutation(54) for _ in range(n)]).astype(np.uint8)
        other[3, 7] = other[3, 8]                                        # a card twice
        other[33, 50] = 54                                               # no such card
        got = check(env, W["R"], KW["R"], [other[g].tolist() for g in range(n)], [15] * n, "deals given", deals=other, contracts=ALL)
        for g in (3, 33):
            assert not got["value"][g].any() and not got["raw"][g].any()
        assert got["value"][0, :, PASS].any()
    finally:
        env.close()


def test_the_python_surface(T, sets):
    import torch
    KW = sets[1]["P8"]
    n = 40
    env = make_env(T, n)
    try:
        want = launch(env, KW, contracts=ALL)
        v, raw, fw = env.bid_values(EPISODE, KW, SCALE, contracts=ALL, raw=True, feature_words=True, pass_value=True)
        assert (v.cpu().numpy() == want["value"]).all() and (raw.cpu().numpy() == want["raw"]).all()
        assert (fw.cpu().numpy().view(np.uint64) == want["fw"]).all()
        old = env.bid_values(EPISODE, KW, SCALE, contracts=ALL)
        assert (old[:, :, :PASS] == v[:, :, :PASS]).all() and not old[:, :, PASS].any() and v[:, :, PASS].any()
        with pytest.raises(Exception):
            env.bid_values(EPISODE, KW, 0.0, pass_value=True)
    finally:
        env.close()


def test_the_learner_with_the_pass_row(T):
    """256 games, 3 iterations: a finite loss, a gradient on output 19, and round() is bid_round(pass_value=True) on the
    learner's own values."""
    import torch
    from tarok_amd import bidding as B
    env = make_env(T, 256)
    try:
        lr = B.BidLearner(env, worlds=4, samples=1, seed=1, pass_value=True)
        for _ in range(3):
            loss = lr.iterate()
            assert np.isfinite(loss)
            gw = lr.net.head.weight.grad
            assert gw[PASS].abs().sum() > 0 and lr.net.head.bias.grad[PASS] != 0
            assert not gw[PASS + 1:].any()
        fw, sums, playouts = lr.collect(7)
        assert playouts == 4 and sums[:, :, PASS].any()
        values = env.bid_values(7, lr.weights(), lr.scale, contracts=lr.contracts, pass_value=True)
        assert values[:, :, PASS].any()
        for margin in (0, -3):
            want = env.bid_round(7, values, lr.playouts_equiv, threshold=margin, contracts=lr.contracts, pass_value=True)
            got = lr.round(7, threshold=margin)
            assert all((a == b).all() for a, b in zip(got, want))
    finally:
        env.close()


def test_without_the_switch_the_learner_is_the_one_it_was(T):
    """BidLearner() against the same three iterations made by hand from the launches and the loss it used before the
    switch existed (playout_bids, bid_values and bid_loss with no pass_value given), on a fixed seed: the same losses,
    weights and round, bit for bit."""
    import torch
    from tarok_amd import bidding as B
    from tarok_amd.selfplay import PolicyNet
    env = make_env(T, 256)
    try:
        lr = B.BidLearner(env, worlds=4, samples=1, seed=5)
        assert lr.pass_value is False
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(5)
            net = PolicyNet(256)
        net.to(env.device)
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)
        for ep in range(3):
            got = lr.iterate()
            sums = env.playout_bids(ep, 4, 1, contracts=DEFAULT, salt=5)
            _, _, fw = env.bid_values(ep, B.pack_weights(net), lr.scale, contracts=DEFAULT, feature_words=True)
            assert not sums[:, :, PASS].any()
            opt.zero_grad(set_to_none=True)
            out = net.forward_raw(env.expand_feature_words(fw.reshape(-1, 4), torch.float32))
            loss = B.bid_loss(out, sums.reshape(-1, 20), 4, 1.0 / 70.0, DEFAULT)
            loss.backward()
            opt.step()
            assert got == float(loss.detach()), (ep, got, float(loss.detach()))
            assert not net.head.weight.grad[PASS:].any()
        assert all(torch.equal(p, q) for p, q in zip(lr.net.parameters(), net.parameters()))
        values = env.bid_values(9, B.pack_weights(net), lr.scale, contracts=DEFAULT)
        want = env.bid_round(9, values, 16, threshold=0, contracts=DEFAULT)
        assert all((a == b).all() for a, b in zip(lr.round(9), want))
    finally:
        env.close()
