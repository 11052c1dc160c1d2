"""Host statement of the per-seat GAE(gamma, lambda) returns (no GPU): selfplay.assign_gae against the float64 per-slot
loop of tests/gae_model.py, against assign_returns at gamma = lambda = 1, and the count of samples it cannot use."""
import inspect

import numpy as np
import pytest
import torch

from gae_model import gae_model
from tarok_amd import selfplay as SP


def rollout(seed, T, N, p_done=0.12, eighths=False):
    """Random rollout arrays with the edge slots: 0 never done, 1 done at t = 0 only, 2 done at T - 1, 3 done on two
    consecutive steps, 4: seat 2 never moves.  eighths: values as multiples of 1/8 in [-4, 4]."""
    rnd = np.random.RandomState(seed)
    done = rnd.rand(T, N) < p_done
    done[:, 0] = False
    done[:, 1] = False; done[0, 1] = True
    done[T - 1, 2] = True
    done[T // 2, 3] = True; done[min(T // 2 + 1, T - 1), 3] = True
    reward = np.where(done[..., None], rnd.randint(-90, 91, (T, N, 4)), 0).astype(np.int16)
    seat = rnd.randint(0, 4, (T, N))
    seat[:, 4] = np.where(seat[:, 4] == 2, 3, seat[:, 4])
    val = (rnd.randint(-32, 33, (T, N)) / 8.0 if eighths else rnd.randn(T, N)).astype(np.float32)
    return done, reward, seat, val


def run(done, reward, seat, val, gamma, lam, scale):
    ret, known = SP.assign_gae(torch.from_numpy(done), torch.from_numpy(reward), torch.from_numpy(seat), torch.from_numpy(val),
                               gamma, lam, scale)
    assert ret.dtype == torch.float32 and known.dtype == torch.bool and ret.shape == known.shape == done.shape
    return ret.numpy(), known.numpy()


@pytest.mark.parametrize("gamma,lam", [(0.99, 0.95), (1.0, 1.0), (1.0, 0.0), (0.0, 1.0), (0.6, 0.3)])
def test_assign_gae_matches_a_float64_loop(gamma, lam):
    done, reward, seat, val = rollout(0, 40, 9)
    ret, known = run(done, reward, seat, val, gamma, lam, 1.0 / 70.0)
    m = gae_model(done, reward, seat, val, gamma, lam, 1.0 / 70.0)
    assert (known == m["known"]).all()
    assert (np.abs(ret.astype(np.float64) - m["ret"]) <= 1e-6 * np.abs(m["ret"])).all()
    assert (ret[~known] == val[~known]).all()                    # A = 0 where nothing follows
    assert known.any() and (~known).any()


def test_gamma_lambda_one_is_monte_carlo_where_that_is_known():
    """gamma = lambda = 1 telescopes to the seat's final score: wherever assign_returns knows the return, assign_gae
    knows it too and gives the same one — EQUAL, on values in eighths and scale 1/64, where every partial sum is exact."""
    done, reward, seat, val = rollout(1, 40, 9, eighths=True)
    ret, known = run(done, reward, seat, val, 1.0, 1.0, 1.0 / 64.0)
    mc, mc_known = SP.assign_returns(torch.from_numpy(done), torch.from_numpy(reward), torch.from_numpy(seat))
    mc, mc_known = mc.numpy() / 64.0, mc_known.numpy()
    assert mc_known.any() and not mc_known.all()
    assert known[mc_known].all()
    assert (ret[mc_known] == mc[mc_known]).all()
    assert (known & ~mc_known).any()                             # and it knows more than that


def test_unknown_samples_are_the_last_decision_of_each_seat_of_the_unfinished_game():
    done, reward, seat, val = rollout(2, 37, 40)
    _, known = run(done, reward, seat, val, 0.99, 0.95, 1.0 / 70.0)
    T, N = done.shape
    counts = set()
    for i in range(N):
        ends = np.nonzero(done[:, i])[0]
        tail = range(ends[-1] + 1, T) if len(ends) else range(T)
        movers = {int(seat[t, i]) for t in tail}
        unknown = np.nonzero(~known[:, i])[0]
        assert len(unknown) == len(movers) <= 4, i
        assert {int(seat[t, i]) for t in unknown} == movers                            # one per seat ...
        assert all(t == max(u for u in tail if seat[u, i] == seat[t, i]) for t in unknown)     # ... its last one
        counts.add(len(unknown))
    assert (~known[:, 2]).sum() == 0                             # done at T - 1: nothing is lost
    assert (~known[:, 4]).sum() <= 3                             # a seat that never moves loses nothing
    assert {0, 4} <= counts


def test_selfplay_arguments_default_to_none():
    sig = inspect.signature(SP.SelfPlay.__init__).parameters
    assert sig["gamma"].default is None and sig["gae_lambda"].default is None
    assert list(inspect.signature(SP.assign_gae).parameters) == ["done", "reward", "seat", "val", "gamma", "lam", "reward_scale", "learner"]
    assert inspect.signature(SP.assign_gae).parameters["learner"].default is None
