"""Training against a frozen opponent, the parts that need no GPU: the seat mask of selfplay.assign_returns /
assign_gae_seats against the float64 per-slot loop of tests/gae_model.py, the numpy model of tarok_learn_select against
np.flatnonzero, SelfPlay's argument rules, and the new entry points' declarations and argument checks.

assign_gae itself keeps its seven parameters (tests/test_gae_cpu.py pins them): the seat mask of the GAE returns is
assign_gae_seats(..., learner=None)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from gae_model import gae_model
from select_model import known_of, known_patterns, rec_of, scratch_bytes, select_model
from tarok_amd import karte as K
from tarok_amd import selfplay as SP
from gae_cases import arrays                                   # the slot patterns of the GAE tests (numpy, no GPU)
from opponent_cases import SETS, monte_carlo_known, moves, seat_sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tt(a, *names):
    return [torch.from_numpy(np.ascontiguousarray(a[k])) for k in names]


@pytest.mark.parametrize("which", SETS)
@pytest.mark.parametrize("gamma,lam", [(1.0, 1.0), (1.0, 0.5), (0.5, 1.0)])
@pytest.mark.parametrize("Tn,n", [(12, 300), (13, 300), (1, 1)])
def test_assign_gae_seats_is_the_model_with_known_masked(Tn, n, gamma, lam, which):
    """Exact inputs (values in eighths, scale 1/64, gamma and lambda in {1, 1/2}): known = the model's AND the seat mask;
    the returns EQUAL the model's for every sample, known or not — the mask changes nothing else."""
    a = arrays(Tn, n, True, n == 1)
    m = gae_model(a["done"], a["reward"], a["seat"], a["val"], gamma, lam, 1.0 / 64.0)
    sets = seat_sets(n, which)
    done, reward, seat, val = tt(a, "done", "reward", "seat", "val")
    ret, known = SP.assign_gae_seats(done.bool(), reward, seat, val, gamma, lam, 1.0 / 64.0, learner=torch.from_numpy(sets))
    assert ret.dtype == torch.float32 and known.dtype == torch.bool
    want = m["known"] & moves(a["seat"], sets)
    assert (known.numpy() == want).all()
    assert (ret.numpy().astype(np.float64) == m["ret"]).all()
    if which == "0":
        assert not known.any()
    if which == "15":
        assert (known.numpy() == m["known"]).all()
    if n > 1 and which != "0":
        assert want.any() and (which == "15" or (m["known"] & ~want).any())


@pytest.mark.parametrize("which", SETS)
@pytest.mark.parametrize("Tn,n", [(12, 300), (13, 300), (1, 1)])
def test_assign_returns_with_learner(Tn, n, which):
    """Monte-Carlo returns: known = (a game ends at or after t) AND the seat mask; the scaled return of every sample it
    knows EQUALS the model's at gamma = lambda = 1 (which telescopes to the seat's final score), masked or not."""
    a = arrays(Tn, n, True, n == 1)
    m = gae_model(a["done"], a["reward"], a["seat"], a["val"], 1.0, 1.0, 1.0 / 64.0)
    sets = seat_sets(n, which)
    done, reward, seat = tt(a, "done", "reward", "seat")
    ret, known = SP.assign_returns(done.bool(), reward, seat, learner=torch.from_numpy(sets))
    mc = monte_carlo_known(a["done"])
    want = mc & moves(a["seat"], sets)
    assert (known.numpy() == want).all()
    assert (m["known"] | ~want).all()                            # what it knows, the model knows
    assert ((ret.numpy().astype(np.float64) / 64.0)[mc] == m["ret"][mc]).all()


@pytest.mark.parametrize("Tn,n", [(12, 300), (1, 1)])
def test_learner_none_is_todays_behaviour(Tn, n):
    a = arrays(Tn, n, False, True)
    done, reward, seat, val = tt(a, "done", "reward", "seat", "val")
    r0, k0 = SP.assign_returns(done.bool(), reward, seat)
    r1, k1 = SP.assign_returns(done.bool(), reward, seat, learner=None)
    r2, k2 = SP.assign_returns(done.bool(), reward, seat, learner=torch.full((n,), 15, dtype=torch.uint8))
    assert torch.equal(r0, r1) and torch.equal(k0, k1) and torch.equal(r0, r2) and torch.equal(k0, k2)
    assert (k0.numpy() == monte_carlo_known(a["done"])).all()
    g0 = SP.assign_gae(done.bool(), reward, seat, val, 0.99, 0.95, 1.0 / 70.0)
    g1 = SP.assign_gae_seats(done.bool(), reward, seat, val, 0.99, 0.95, 1.0 / 70.0)
    g2 = SP.assign_gae_seats(done.bool(), reward, seat, val, 0.99, 0.95, 1.0 / 70.0, learner=torch.full((n,), 0xFF, dtype=torch.uint8))
    for g in (g1, g2):                                           # (bits 4..7 of a set are ignored)
        assert torch.equal(g0[0], g[0]) and torch.equal(g0[1], g[1])
    assert inspect.signature(SP.assign_returns).parameters["learner"].default is None
    assert inspect.signature(SP.assign_gae_seats).parameters["learner"].default is None


def test_learner_moves():
    seat = torch.tensor([[0, 1, 2, 3], [3, 2, 1, 0]])
    sets = torch.tensor([1, 6, 0xF6, 0], dtype=torch.uint8)
    assert SP.learner_moves(seat, sets).tolist() == [[True, True, True, False], [False, True, True, False]]


def test_selfplay_argument_rules():
    """Checked before the env is touched (None stands in for it): learner_seats without an opponent, an opponent without
    the fused policy or the fused step, a seat set outside 0..15."""
    w = [torch.zeros((256, 256), dtype=torch.bfloat16), torch.zeros(256), torch.zeros((256, 256), dtype=torch.bfloat16),
         torch.zeros(256), torch.zeros((64, 256), dtype=torch.bfloat16), torch.zeros(64)]
    for seats in (1, 0, torch.zeros(4, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="opponent"):
            SP.SelfPlay(None, learner_seats=seats)
    for kw in (dict(hidden=128), dict(fused=False), dict(fused_step=False)):
        with pytest.raises(RuntimeError, match="tarok_policy_step_versus"):
            SP.SelfPlay(None, opponent=w, **kw)
    for seats in (16, -1):
        with pytest.raises(ValueError, match="learner_seats"):
            SP.SelfPlay(None, opponent=w, learner_seats=seats)
    sig = inspect.signature(SP.SelfPlay.__init__).parameters
    assert sig["opponent"].default is None and sig["learner_seats"].default is None
    assert hasattr(SP.SelfPlay, "set_opponent")


@pytest.mark.parametrize("tile", [256, K.LEARN_SELECT_TILE])
def test_select_model_is_flatnonzero(tile):
    for M in (1, 63, 64, 65, tile, tile + 1, 3 * tile + 77):
        for name, known in known_patterns(M, tile):
            rec = rec_of(known, seed=M)
            assert (known_of(rec) == known).all()
            m = select_model(rec, tile)
            want = np.flatnonzero(known)
            assert m["count"] == want.size, (M, name)
            assert (m["index"][:want.size] == want).all() and (m["index"][want.size:] == -1).all(), (M, name)
            assert m["tile_cnt"].size == -(-M // tile) and int(m["tile_off"][-1] + m["tile_cnt"][-1]) == want.size


@pytest.fixture(scope="module")
def lib():
    import tarok_amd
    from tarok_amd import _native
    tarok_amd.build()
    return _native.lib()


def test_new_entry_points_are_declared_and_bound(lib):
    from tarok_amd import _native
    src = open(os.path.join(ROOT, "include", "tarok_env.h")).read()
    assert int(re.search(r"#define TAROK_LEARN_SELECT_TILE (\d+)", src).group(1)) == K.LEARN_SELECT_TILE
    assert K.LEARN_SELECT_TILE % 256 == 0
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+tarok_learn_returns_seats\s*\(([^;]*)\)\s*;", src)
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    plain = [" ".join(p.split()) for p in re.search(r"\bint\s+tarok_learn_returns\s*\(([^;]*)\)\s*;", src).group(1).split(",")]
    assert params[:9] == plain[:9] and params[14:] == plain[9:]
    assert params[9:14] == ["int gae", "float gamma", "float lambda", "int seats", "const uint8_t *seats_per_game"]
    assert re.search(r"\bint64_t\s+tarok_learn_select_scratch_bytes\s*\(\s*int64_t M\s*\)\s*;", src)
    m = re.search(r"\bint\s+tarok_learn_select\s*\(([^;]*)\)\s*;", src)
    assert [" ".join(p.split()) for p in m.group(1).split(",")] == [
        "tarok_env *env", "int64_t M", "const float *rec", "int64_t *index_out", "int64_t *count_out", "void *scratch", "void *stream"]
    for name, nargs in (("tarok_learn_returns_seats", 18), ("tarok_learn_select", 7), ("tarok_learn_select_scratch_bytes", 1)):
        assert name in _native.SYMBOLS and len(getattr(lib, name).argtypes) == nargs
    assert lib.tarok_abi_version() == 5                          # additions only
    from tarok_amd.env import TarokVecEnv
    for name in ("learn_returns_seats", "learn_select", "learn_select_scratch_bytes"):
        assert hasattr(TarokVecEnv, name)
    assert list(inspect.signature(TarokVecEnv.learn_select).parameters) == ["self", "M", "rec", "index_out", "count_out", "scratch"]


def test_select_scratch_bytes(lib):
    for M in (1, 2047, 2048, 2049, 3 * 2048 + 77, 48 * 65536, 1 << 28):
        assert lib.tarok_learn_select_scratch_bytes(M) == scratch_bytes(M, K.LEARN_SELECT_TILE)
    assert lib.tarok_learn_select_scratch_bytes(0) == 0 and lib.tarok_learn_select_scratch_bytes(-5) == 0


def test_new_entry_points_reject_bad_arguments_without_a_gpu(lib):
    """Every check comes before the first HIP call: a zeroed stand-in env is never followed."""
    z = ctypes.c_void_p(0)
    buf = ctypes.create_string_buffer(4096)
    q = ctypes.cast(buf, ctypes.c_void_p)
    nan = float("nan")
    fn = lib.tarok_learn_returns_seats

    def call(env=q, Tn=12, gae=1, gamma=0.99, lam=0.95, seats=1, null=None):
        ptrs = [q] * 9                                           # done reward obs logp value action | rec stats scratch
        if null is not None:
            ptrs[null] = z
        return fn(env, Tn, *ptrs[:6], 1.0 / 70.0, gae, gamma, lam, seats, z, *ptrs[6:], z)

    assert call(env=z) == -1 and call(Tn=0) == -1
    for seats in (16, -1, 255):
        assert call(seats=seats) == -1 and call(seats=seats, gae=0) == -1
    for gae in (2, -1):
        assert call(gae=gae) == -1
    for kw in (dict(gamma=1.5), dict(lam=-0.1), dict(gamma=nan), dict(lam=nan), dict(gamma=-0.01), dict(lam=1.001)):
        assert call(**kw) == -1, kw
    for k in range(9):
        assert call(null=k) == -1 and call(null=k, gae=0) == -1, k
    sel = lib.tarok_learn_select
    assert sel(z, 64, q, q, q, q, z) == -1 and sel(q, 0, q, q, q, q, z) == -1 and sel(q, -3, q, q, q, q, z) == -1
    for k in range(4):
        ptrs = [q] * 4
        ptrs[k] = z
        assert sel(q, 64, *ptrs, z) == -1, k
