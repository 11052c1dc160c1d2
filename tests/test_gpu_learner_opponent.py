"""GPU tests of training against a frozen opponent: tarok_learn_returns_seats (the two returns walks with `known` masked
by the learner's seats) against the float64 per-slot loop of tests/gae_model.py, tarok_learn_select (the compaction of
the known samples) against np.flatnonzero and the numpy model of its three launches (tests/select_model.py), every
output between guard bands, and SelfPlay(opponent=...) end to end.  Build-owned code (the reference has no
policy-gradient learner).

Shapes of the returns tests: those of tests/test_gpu_learner_gae.py, whose arrays and slot patterns (tests/gae_cases.py) are reused — n = 300
slots (two workgroups, the second a ragged one of 44) at T = 12 and T = 13 (not a multiple of the walk's unroll of 4),
one slot at T = 1; slots that never end a game, end one at t = 0 only, at t = T - 1, twice in a row, and slots where
seat 2 never moves.

Run on the GPU box:  python -m pytest tests -m gpu -x -q
"""
import ctypes
import functools

import numpy as np
import pytest

from select_model import known_patterns, rec_of, scratch_bytes, select_model
from gae_cases import F32, SHAPES, arrays, check_bits, launch, model
from opponent_cases import SETS, monte_carlo_known, moves, seat_sets
from gpu_harness import T  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
MODES = [("mc", 1.0, 1.0), ("gae", 1.0, 0.5), ("gae", 0.5, 1.0)]          # exact inputs: gamma and lambda in {1, 1/2}


@pytest.fixture(scope="module")
def envs(T):
    es = {n: T.TarokVecEnv(n, seed=1) for n in (300, 1)}
    yield es
    for e in es.values():
        e.close()


def sets_of(n, which):
    """The learner's seat sets of a case: an int (passed as `seats`, seats_per_game = NULL) or, for the per-slot cycle,
    [n] uint8 (seats_per_game) with noise in bits 4..7 of every other slot, which the kernels ignore."""
    if which != "cycle":
        return int(which)
    return seat_sets(n, which) | np.where(np.arange(n) % 2 == 1, 0xA0, 0).astype(np.uint8)


def seats_call(env, gae, gamma, lam, scale, sets):
    import torch

    def call(dev, rec, stats, scratch):
        kw = dict(seats=sets) if isinstance(sets, int) else dict(seats_per_game=torch.from_numpy(sets).cuda())
        env.learn_returns_seats(dev["done"].shape[0], dev["done"], dev["reward"], dev["words"], dev["logp"], dev["val"], dev["act"],
                                scale, rec, stats, scratch, gae=gae, gamma=gamma, lam=lam, **kw)
    return call


@functools.lru_cache(maxsize=None)
def mc_model(Tn, n, eighths, one_done, scale):
    """The Monte-Carlo walk in float64: ret = the seat's final score of the game the card belongs to times scale (0 where
    no game ends at or after t), known = one does; ret32 = the same product as ONE float32 multiplication (what the
    kernel computes: there is nothing to associate differently)."""
    a = arrays(Tn, n, eighths, one_done)
    cur = np.zeros((n, 4), np.int64)
    score = np.zeros((Tn, n), np.int64)
    for t in range(Tn - 1, -1, -1):
        d = a["done"][t].astype(bool)
        cur[d] = a["reward"][t][d]
        score[t] = cur[np.arange(n), a["seat"][t]]
    known = monte_carlo_known(a["done"])
    ret = score.astype(np.float64) * scale
    return dict(ret=ret, ret32=score.astype(np.float32) * np.float32(scale), known=known, adv=ret - a["val"].astype(np.float64))


def reference(mode, Tn, n, eighths, one_done, gamma, lam, scale):
    """(returns f64, unmasked known, advantages f64, bound of a float32 evaluation) of a case."""
    g = model(Tn, n, eighths, one_done, gamma if mode == "gae" else 1.0, lam if mode == "gae" else 1.0, scale)
    if mode == "gae":
        return g["ret"], g["known"], g["adv"], g["bound"]
    m = mc_model(Tn, n, eighths, one_done, scale)
    # gae_model's bound at gamma = lambda = 1 holds wherever a game ends at or after t (there its return telescopes to the
    # score); elsewhere the return is an exact 0
    return m["ret"], m["known"], m["adv"], np.where(m["known"], g["bound"], 0.0)


def check_stats(s, adv, known, total):
    """stats_out against the float64 mean, 1 / std and known fraction at test_returns_gae_general's tolerances."""
    a = adv[known]
    if a.size == 0:
        assert np.isfinite(s).all() and s[0] == 0 and s[2] == 0 and s[3] == 0
        return
    assert abs(s[0] - a.mean()) < 1e-4
    if a.size >= 2 and a.std() > 0:
        assert abs(s[1] - 1.0 / a.std()) < 1e-3 / a.std()
    else:
        assert np.isfinite(s[1]) and s[1] > 0
    assert abs(s[2] - known.sum() / total) < 1e-6 and s[3] == 0


@pytest.mark.parametrize("mode,gamma,lam", MODES)
@pytest.mark.parametrize("Tn,n", SHAPES)
def test_returns_seats_exact(T, envs, Tn, n, mode, gamma, lam):
    """Values in eighths, scores scaled by 1/64, gamma and lambda in {1, 1/2}: every intermediate is a float32 (the model
    checks it), so the returns must EQUAL the float64 model's — for every sample, the opponent's too; logp and val pass
    through bit for bit; the card is the rollout's and known is the model's AND the seat mask."""
    a = arrays(Tn, n, True, n == 1)
    scale = 1.0 / 64.0
    ret, known, adv, _ = reference(mode, Tn, n, True, n == 1, gamma, lam, scale)
    assert model(Tn, n, True, n == 1, gamma if mode == "gae" else 1.0, lam if mode == "gae" else 1.0, scale)["lossless"].all()
    for which in SETS:
        sets = sets_of(n, which)
        r, written, s, s_written, *_ = launch(envs[n], a, gamma, lam, scale, call=seats_call(envs[n], mode == "gae", gamma, lam, scale, sets))
        assert written.all() and s_written.all()
        assert (r[..., 1].astype(np.float64) == ret).all(), which
        mine = known & moves(a["seat"], seat_sets(n, which))
        check_bits(r, a, dict(known=mine))
        check_stats(s, adv, mine, Tn * n)
        if which == "0":
            assert not mine.any() and s[2] == 0 and np.isfinite(s).all()
        if n > 1 and which not in ("0", "15"):
            assert mine.any() and (known & ~mine).any()


@pytest.mark.parametrize("mode", ["mc", "gae"])
@pytest.mark.parametrize("Tn,n", SHAPES)
def test_returns_seats_general(T, envs, Tn, n, mode):
    """Normal values, gamma = 0.99, lambda = 0.95, scale 1/70 (each as the float32 the ABI passes): every return within
    gae_model's derived bound of a float32 evaluation (Monte-Carlo: also EQUAL to the single float32 product score *
    scale); stats at the tolerances of test_returns_gae_general."""
    gamma, lam, scale = F32(0.99), F32(0.95), F32(1.0 / 70.0)
    a = arrays(Tn, n, False, True)
    ret, known, adv, bound = reference(mode, Tn, n, False, True, gamma, lam, scale)
    for which in SETS:
        sets = sets_of(n, which)
        r, written, s, s_written, *_ = launch(envs[n], a, gamma, lam, scale, call=seats_call(envs[n], mode == "gae", gamma, lam, scale, sets))
        assert written.all() and s_written.all()
        err = np.abs(r[..., 1].astype(np.float64) - ret)
        print(mode, (Tn, n), which, "max error", err.max(), "max error / bound", (err[bound > 0] / bound[bound > 0]).max(initial=0.0))
        assert (err <= bound).all()
        if mode == "mc":
            assert (r[..., 1] == mc_model(Tn, n, False, True, scale)["ret32"]).all()
        mine = known & moves(a["seat"], seat_sets(n, which))
        check_bits(r, a, dict(known=mine))
        print("stats", s, "known", mine.sum())
        check_stats(s, adv, mine, Tn * n)


@pytest.mark.parametrize("mode", ["mc", "gae"])
@pytest.mark.parametrize("Tn,n", SHAPES)
def test_all_seats_is_the_unmasked_function_byte_for_byte(T, envs, Tn, n, mode):
    """seats = 15, seats_per_game = NULL: rec, stats and the scratch rows are the bytes of tarok_learn_returns (gae = 0) /
    tarok_learn_returns_gae (gae = 1) on the same arrays; a per-slot array of 15s and the uniform set 6 against an array
    of 6s give the same bytes too."""
    gamma, lam, scale = F32(0.99), F32(0.95), F32(1.0 / 70.0)
    a = arrays(Tn, n, False, True)
    env = envs[n]

    def plain(dev, rec, stats, scratch):
        args = (Tn, dev["done"], dev["reward"], dev["words"], dev["logp"], dev["val"], dev["act"], scale)
        if mode == "gae":
            env.learn_returns_gae(*args, gamma, lam, rec, stats, scratch)
        else:
            env.learn_returns(*args, rec, stats, scratch)

    same = lambda x, y: x[0].tobytes() == y[0].tobytes() and x[2].tobytes() == y[2].tobytes() and x[4].tobytes() == y[4].tobytes()
    ref = launch(env, a, gamma, lam, scale, call=plain)
    for sets in (15, np.full(n, 15, np.uint8), np.full(n, 0x5F, np.uint8)):
        assert same(ref, launch(env, a, gamma, lam, scale, call=seats_call(env, mode == "gae", gamma, lam, scale, sets)))
    six = launch(env, a, gamma, lam, scale, call=seats_call(env, mode == "gae", gamma, lam, scale, 6))
    assert same(six, launch(env, a, gamma, lam, scale, call=seats_call(env, mode == "gae", gamma, lam, scale, np.full(n, 6, np.uint8))))
    if n > 1:
        assert not same(ref, six)


@pytest.mark.parametrize("mode", ["mc", "gae"])
@pytest.mark.parametrize("Tn,n", SHAPES)
def test_returns_seats_writes_only_its_arrays(T, envs, Tn, n, mode):
    """rec, stats and scratch between guard bands (launch() checks the bands): all of rec and stats is written, of scratch
    exactly the first ceil(n / 256) rows, whose first column is the block's count of the learner's known samples."""
    gamma, lam, scale = F32(0.99), F32(0.95), F32(1.0 / 70.0)
    a = arrays(Tn, n, False, True)
    _, known, _, _ = reference(mode, Tn, n, False, True, gamma, lam, scale)
    sets = sets_of(n, "cycle")
    r, written, s, s_written, c, c_written, blocks = launch(envs[n], a, gamma, lam, scale, spare_rows=5,
                                                            call=seats_call(envs[n], mode == "gae", gamma, lam, scale, sets))
    assert written.all() and s_written.all()
    assert c_written[:blocks].all() and not c_written[blocks:].any()
    mine = (known & moves(a["seat"], seat_sets(n, "cycle"))).reshape(Tn, -1)
    per_block = [mine[:, b * 256:(b + 1) * 256].sum() for b in range(blocks)]
    assert [float(x) for x in c[:blocks, 0]] == [float(x) for x in per_block] and (c[:blocks, 3] == 0).all()


@pytest.mark.parametrize("mode", ["mc", "gae"])
def test_returns_seats_is_reproducible(T, envs, mode):
    a = arrays(13, 300, False, True)
    call = seats_call(envs[300], mode == "gae", F32(0.99), F32(0.95), F32(1.0 / 70.0), sets_of(300, "cycle"))
    one = launch(envs[300], a, 0.0, 0.0, 0.0, call=call)
    two = launch(envs[300], a, 0.0, 0.0, 0.0, call=call)
    assert one[0].tobytes() == two[0].tobytes() and one[2].tobytes() == two[2].tobytes()


def test_returns_seats_rejects_bad_arguments(T, envs):
    """A seat set outside 0..15, gae outside {0, 1}, with gae = 1 a gamma or lambda outside [0, 1] or NaN, a NULL array,
    T < 1: TAROK_EINVAL and nothing is launched (rec, stats and scratch keep their fill).  With gae = 0 gamma and lambda
    are ignored."""
    from tarok_amd import _native
    env = envs[300]
    L = _native.lib()
    a = arrays(12, 300, False, True)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    nan = float("nan")

    def raw(Tn=12, gae=1, gamma=0.99, lam=0.95, seats=1, null=None, want=-1):
        def call(dev, rec, stats, scratch):
            args = [p(dev["done"]), p(dev["reward"]), p(dev["words"]), p(dev["logp"]), p(dev["val"]), p(dev["act"])]
            outs = [p(rec), p(stats), p(scratch)]
            if null is not None:
                (args + outs)[null].value = None
            code = L.tarok_learn_returns_seats(env._h, Tn, *args, 1.0 / 70.0, gae, gamma, lam, seats, None, *outs, env._stream())
            assert code == want, (Tn, gae, gamma, lam, seats, null, code)
        return call

    cases = [raw(gamma=1.5), raw(lam=-0.1), raw(gamma=nan), raw(lam=nan), raw(gamma=-0.01), raw(lam=1.001), raw(Tn=0), raw(Tn=0, gae=0),
             raw(seats=16), raw(seats=-1), raw(seats=16, gae=0), raw(gae=2), raw(gae=-1)]
    cases += [raw(null=k, gae=g) for k in range(9) for g in (0, 1)]
    for call in cases:
        r, written, s, s_written, c, c_written, _ = launch(env, a, 0.0, 0.0, 0.0, call=call)
        assert not written.any() and not s_written.any() and not c_written.any()
    r, written, *_ = launch(env, a, 0.0, 0.0, 0.0, call=raw(gae=0, gamma=nan, lam=7.0, want=0))       # ignored without GAE
    assert written.all()
    with pytest.raises(_native.TarokNativeError):
        launch(env, a, 0.0, 0.0, 0.0, call=seats_call(env, True, 0.99, 0.95, 1.0 / 70.0, 16))
    with pytest.raises(ValueError):
        launch(env, a, 0.0, 0.0, 0.0, call=seats_call(env, True, 0.99, 0.95, 1.0 / 70.0, np.full(299, 1, np.uint8)))


# ---------------------------------------------------------------------------------------------------------------
# compaction


def select_launch(env, rec_np, spare=256):
    """One tarok_learn_select launch on a record (numpy [M,4] f32) with index_out, count_out and scratch between guard
    bands (scratch with `spare` bytes more than tarok_learn_select_scratch_bytes(M)).  Returns (index values, index
    written, count, scratch bytes, scratch written) after checking the bands."""
    import torch
    from guarded import Guarded, assert_guards_intact
    M = rec_np.shape[0]
    need = env.learn_select_scratch_bytes(M)
    rec = torch.from_numpy(rec_np).cuda()
    index = Guarded("index_out", 1, M, np.int64, device="cuda")
    count = Guarded("count_out", 1, 1, np.int64, device="cuda")
    scratch = Guarded("scratch", 1, need + spare, np.uint8, device="cuda")
    env.learn_select(M, rec, index.payload().view(torch.int64), count.payload().view(torch.int64), scratch.payload())
    torch.cuda.synchronize()
    assert_guards_intact([index, count, scratch], M)
    iv, iw = index.host()
    cv, cw = count.host()
    sv, sw = scratch.host()
    assert cw.all()
    return iv[0], iw[0], int(cv[0, 0]), sv[0], sw[0], need


def test_select_tile_is_exported(T):
    from tarok_amd import karte as K
    assert K.LEARN_SELECT_TILE == 2048


@pytest.mark.parametrize("M", ["1", "63", "64", "65", "TILE", "TILE+1", "3*TILE+77"])
def test_select_is_flatnonzero(T, envs, M):
    """index_out[:count] EQUALS np.flatnonzero(known) and count is exact, for every known pattern; the entries from count
    on and the guard bands are untouched; the scratch holds the model's tile prefixes and counts and nothing is written
    past tarok_learn_select_scratch_bytes(M); a second launch gives the same bytes."""
    TILE = T.karte.LEARN_SELECT_TILE
    M = eval(M, {"TILE": TILE})
    env = envs[300]
    for name, known in known_patterns(M, TILE):
        rec = rec_of(known, seed=M)
        want = np.flatnonzero(known)
        iv, iw, count, sv, sw, need = select_launch(env, rec)
        assert need == scratch_bytes(M, TILE)
        assert count == want.size, (M, name, count)
        assert (iv[:count] == want).all() and iw[:count].all(), (M, name)
        assert not iw[count:].any(), (M, name)
        m = select_model(rec, TILE)
        tiles = m["tile_cnt"].size
        assert (sv[:8 * tiles].view(np.int64) == m["tile_off"]).all() and (sv[8 * tiles:12 * tiles].view(np.uint32) == m["tile_cnt"]).all()
        assert not sw[12 * tiles:].any()                         # (nothing past the two arrays; their values: the line above)
        iv2, iw2, count2, sv2, sw2, _ = select_launch(env, rec)
        assert iv2.tobytes() == iv.tobytes() and count2 == count and sv2.tobytes() == sv.tobytes()


def test_select_addresses_2_pow_28_samples(T, envs):
    """M = 2^28, the record of the largest envs (4 GiB: byte offsets past 2^31): known are sample 0, a stretch across
    sample 2^27, the whole last tile and so the last sample.  Checked on the device."""
    import torch
    M = 1 << 28
    env = envs[1]
    TILE = T.karte.LEARN_SELECT_TILE
    want = torch.cat([torch.tensor([0]), torch.arange((1 << 27) - 3000, (1 << 27) + 3000), torch.arange(M - TILE, M)]).cuda()
    rec = torch.zeros((M, 4), dtype=torch.float32, device="cuda")
    rec[:, 3].view(torch.int32)[want] = 256 | 7
    index = torch.full((M,), -1, dtype=torch.int64, device="cuda")
    count = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    scratch = torch.empty(env.learn_select_scratch_bytes(M), dtype=torch.uint8, device="cuda")
    env.learn_select(M, rec, index, count, scratch)
    assert int(count) == want.numel()
    assert torch.equal(index[:want.numel()], want) and bool((index[want.numel():] == -1).all())
    del rec, index
    torch.cuda.empty_cache()


def test_select_rejects_bad_arguments(T, envs):
    import torch
    from tarok_amd import _native
    env = envs[300]
    L = _native.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rec = torch.from_numpy(rec_of(np.ones(64, bool))).cuda()
    index = torch.full((64,), -1, dtype=torch.int64, device="cuda")
    count = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    scratch = torch.full((64,), 0xA5, dtype=torch.uint8, device="cuda")
    good = [p(rec), p(index), p(count), p(scratch)]
    assert L.tarok_learn_select(None, 64, *good, env._stream()) == -1
    for M in (0, -1):
        assert L.tarok_learn_select(env._h, M, *good, env._stream()) == -1
    for k in range(4):
        args = list(good)
        args[k] = None
        assert L.tarok_learn_select(env._h, 64, *args, env._stream()) == -1, k
    torch.cuda.synchronize()
    assert bool((index == -1).all()) and int(count) == -1 and bool((scratch == 0xA5).all())
    with pytest.raises(_native.TarokNativeError):
        env.learn_select(0, rec, index, count, scratch)
    assert L.tarok_learn_select(env._h, 64, *good, env._stream()) == 0
    assert int(count) == 64 and torch.equal(index, torch.arange(64, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------
# end to end

TN, N = 16, 512


@pytest.fixture(scope="module")
def nets(T):
    """Two frozen networks (snapshots of differently seeded learners): the opponent and its replacement."""
    from tarok_amd import selfplay as SP
    env = T.TarokVecEnv(8, seed=3)
    out = [SP.SelfPlay(env, seed=s).snapshot() for s in (5, 9)]
    env.close()
    return out


def fresh(T, made, **kw):
    """SelfPlay on 512 games that stand in the middle of their play (40 random steps: games end inside 16 lock-steps)."""
    from tarok_amd import selfplay as SP
    K = T.karte
    env = T.TarokVecEnv(N, seed=7, mix=K.MIX_ALL)
    sp = SP.SelfPlay(env, seed=0, **kw)
    obs = env.legal_actions()
    for _ in range(40):
        obs, _, _ = env.step(env.policy_random(obs), auto_reset=True)
    sp.obs_words.copy_(obs.words)
    made.append(env)
    return env, sp


def rollout_model(T, sp, buf):
    """(known of the unmasked estimator, the learner-moves mask, done) of a rollout, on the host."""
    from gae_model import gae_model
    K = T.karte
    done = buf["done"].cpu().numpy().astype(bool)
    seat = ((buf["words"][:TN] >> K.OBS_SEAT_SHIFT) & 3).cpu().numpy()
    if sp.gae:
        known = gae_model(done, buf["reward"].cpu().numpy(), seat, buf["val"].cpu().numpy(), sp.gamma, sp.gae_lambda, sp.reward_scale)["known"]
    else:
        known = monte_carlo_known(done)
    return known, moves(seat, sp._seats.cpu().numpy()), done


def bits(t):
    import torch
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def expect_row0(env, sp, learner_w, opponent_w):
    """What row 0 of the next rollout must hold: per slot the card and log-probability of tarok_policy_mlp with the
    mover's network on the observation words the rollout starts from (the env stands exactly there)."""
    import torch
    seat0 = (sp.obs_words >> 54) & 3
    mine = ((sp._seats.long() >> seat0) & 1).bool()
    a_l, lp_l, _ = env.policy_mlp(learner_w, sp.obs_words)
    a_o, lp_o, _ = env.policy_mlp(opponent_w, sp.obs_words)
    assert mine.any() and (~mine).any() and not bool((bits(lp_l) == bits(lp_o)).all())
    return mine, torch.where(mine, a_l, a_o), torch.where(mine, lp_l, lp_o)


@pytest.mark.parametrize("gae", [False, True])
def test_selfplay_against_a_frozen_opponent(T, nets, gae):
    """One SelfPlay(opponent = a snapshot) with the default seats (slot g learns on seat g % 4), Monte-Carlo and GAE
    returns: counts against the model on the rollout it returns, row 0 against tarok_policy_mlp with the mover's
    network, the opponent's tensors untouched by the update, set_opponent() without a new capture, and the torch update
    on a twin env."""
    import torch
    opp, third = nets
    kw = dict(gamma=0.99, gae_lambda=0.95) if gae else {}
    made = []
    env, sp = fresh(T, made, opponent=opp, **kw)
    assert sp.fused_learner and sp._seats.tolist() == [1 << (g % 4) for g in range(N)]
    sp.collect(TN)                                   # (warm-up and graph capture: the next rollout is a plain replay)
    start = sp.snapshot()
    flat0 = sp.flat.clone()
    mine0, act0, logp0 = expect_row0(env, sp, start, opp)
    graph = sp._graph
    st = sp.iterate(T=TN, minibatches=2)
    buf = sp._buf
    assert st["env_errors"] == 0 and np.isfinite(st["loss"])
    known, mover, done = rollout_model(T, sp, buf)
    assert done.any() and (known & mover).any() and (known & ~mover).any()
    assert st["learner_samples"] == (known & mover).sum()
    assert st["known_frac"] == (known & mover).sum() / (TN * N)
    assert st["known_frac"] * (TN * N) == st["learner_samples"]                 # what stats[2] implies (T N is a power of two)
    assert torch.equal(buf["act"][0], act0) and torch.equal(bits(buf["logp"][0]), bits(logp0))
    rw = buf["reward"].cpu().numpy().astype(np.float64)
    w = done[..., None] * ((sp._seats.cpu().numpy()[:, None] >> np.arange(4)) & 1)[None]
    assert abs(st["learner_mean_score"] - (rw * w).sum() / max(1, w.sum())) < 1e-3
    for a, b in zip(sp._opp, opp):
        assert torch.equal(a, b)
    assert not torch.equal(sp.flat, flat0)

    # a new opponent, in place: the same graph plays it
    sp.set_opponent(third)
    for a, b in zip(sp._opp, third):
        assert torch.equal(a, b)
    mine1, act1, logp1 = expect_row0(env, sp, sp.snapshot(), third)
    st1 = sp.iterate(T=TN, minibatches=2)
    assert sp._graph is graph and st1["env_errors"] == 0 and np.isfinite(st1["loss"])
    assert torch.equal(sp._buf["act"][0], act1) and torch.equal(bits(sp._buf["logp"][0]), bits(logp1))

    # the torch update on a twin env: the same rollout, the same count
    env2, sp2 = fresh(T, made, opponent=opp, fused_learner=False, **kw)
    assert not sp2.fused_learner
    sp2.collect(TN)
    st2 = sp2.iterate(T=TN, minibatches=2)
    assert st2["env_errors"] == 0 and np.isfinite(st2["loss"])
    known2, mover2, _ = rollout_model(T, sp2, sp2._buf)
    assert st2["learner_samples"] == (known2 & mover2).sum() and st2["known_frac"] == (known2 & mover2).sum() / (TN * N)
    assert st2["learner_samples"] == st["learner_samples"]
    del sp, sp2
    for e in made:
        e.close()


@pytest.mark.parametrize("gae", [False, True])
def test_the_opponents_samples_have_no_influence(T, nets, gae):
    """Two learners on twin envs, the same seeds, the same collected buffers; in one of them logp, val, act and the
    feature words of every row that another seat than the learner's played are overwritten with garbage (cards stay
    bytes of the legal range).  update_fused leaves BIT-IDENTICAL parameter vectors: no launch of the update reads an
    opponent's sample for anything that reaches the weights."""
    import torch
    opp, _ = nets
    kw = dict(gamma=0.99, gae_lambda=0.95) if gae else {}
    made = []
    (env1, sp1), (env2, sp2) = fresh(T, made, opponent=opp, **kw), fresh(T, made, opponent=opp, **kw)
    b1, b2 = sp1.collect(TN), sp2.collect(TN)
    for k in b1:
        assert torch.equal(b1[k], b2[k]), k
    seat = (b2["words"][:TN] >> 54) & 3
    other = ~((sp2._seats.long().unsqueeze(0) >> seat) & 1).bool()
    assert other.any() and (~other).any()
    g = torch.Generator(device="cuda").manual_seed(1)
    k = int(other.sum())
    b2["logp"][other] = -50.0 * torch.rand(k, device="cuda", generator=g)
    b2["val"][other] = 1e3 * torch.randn(k, device="cuda", generator=g)
    b2["act"][other] = torch.randint(0, 54, (k,), device="cuda", generator=g).to(torch.uint8)
    b2["obs"][other] = torch.randint(-2 ** 62, 2 ** 62, (k, 4), device="cuda", generator=g)
    s1, s2 = sp1.update_fused(b1, 2, 2), sp2.update_fused(b2, 2, 2)
    assert s1["learner_samples"] == s2["learner_samples"] > 0 and s1["loss"] == s2["loss"]
    assert torch.equal(sp1.flat, sp2.flat) and torch.equal(sp1.adam_m, sp2.adam_m) and torch.equal(sp1.adam_v, sp2.adam_v)
    for name in ("w1", "w2", "w3", "w3t", "w2t"):
        assert torch.equal(sp1._wf[name], sp2._wf[name]), name
    del sp1, sp2
    for e in made:
        e.close()


def test_no_learner_seat_no_update(T, nets):
    """learner_seats = 0: the update launches nothing and returns zeros; the default seats follow the env's game offset."""
    import torch
    from tarok_amd import selfplay as SP
    opp, _ = nets
    made = []
    env, sp = fresh(T, made, opponent=opp, learner_seats=0)
    flat0, step0 = sp.flat.clone(), int(sp.adam_step)
    st = sp.iterate(T=TN, minibatches=2)
    assert st["env_errors"] == 0 and st["learner_samples"] == 0 and st["known_frac"] == 0
    assert st["loss"] == 0 and st["pi_loss"] == 0 and st["v_loss"] == 0 and st["entropy"] == 0
    assert torch.equal(sp.flat, flat0) and int(sp.adam_step) == step0
    env8 = T.TarokVecEnv(8, seed=7, game_offset=5)
    made.append(env8)
    assert SP.SelfPlay(env8, opponent=opp)._seats.tolist() == [1 << ((5 + g) % 4) for g in range(8)]
    assert SP.SelfPlay(env8, opponent=opp, learner_seats=6)._seats.tolist() == [6] * 8
    with pytest.raises(RuntimeError):
        SP.SelfPlay(env8).set_opponent(opp)
    del sp
    for e in made:
        e.close()
