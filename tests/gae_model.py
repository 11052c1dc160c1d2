"""TEST INFRASTRUCTURE — the per-seat GAE(gamma, lambda) recursion of tarok_learn_returns_gae (include/tarok_env.h) as a
float64 Python loop over one slot at a time, the model that tests/test_gae_cpu.py holds selfplay.assign_gae against and
tests/test_gpu_learner_gae.py the kernel.

Besides the returns it reports, per sample,
  * `lossless`: every intermediate of the recursion (the scaled score, gamma * next_v, the partial sums of delta,
    gamma * lambda, its product with next_adv, A, A + v) survives rounding to float32 unchanged — then a float32
    evaluation in ANY association, fused or not, gives exactly the model's value;
  * `bound`: how far a float32 evaluation may be from the model.  The kernel rounds at most seven times per decision
    (score * scale, gamma * next_v, the two additions of delta, gamma * lambda, its product with next_adv, the addition
    into A), each by at most u = 2^-24 times the magnitude of its result, which never exceeds
    M = |pend_r| + gamma |next_v| + |v| + gamma lambda |next_adv|; the error of next_adv comes in scaled by
    gamma * lambda.  So E(A) <= gamma lambda E(next_adv) + 8 u M (the eighth u covers the second-order terms), and the
    return A + v, rounded once more, is within E(A) + u (|A| + |v|): a bound that grows with the length of the seat's
    chain of decisions, a few float32 ulps of the running magnitude per decision.
"""
import numpy as np

U = 2.0 ** -24


def _f32_exact(x):
    return float(np.float32(x)) == x


def gae_model(done, reward, seat, val, gamma, lam, scale):
    """done [T,N] bool, reward [T,N,4] int, seat [T,N] int, val [T,N] float (numpy); gamma, lam, scale: Python floats,
    used as given (pass float32-representable ones to model the C ABI, whose arguments are floats).
    Returns dict(ret, adv [T,N] f64, known, lossless [T,N] bool, bound [T,N] f64)."""
    done = np.asarray(done).astype(bool)
    reward, seat, val = np.asarray(reward), np.asarray(seat), np.asarray(val, dtype=np.float64)
    T, N = done.shape
    ret, adv, bound = np.zeros((T, N)), np.zeros((T, N)), np.zeros((T, N))
    known, lossless = np.zeros((T, N), bool), np.zeros((T, N), bool)
    gl = gamma * lam
    gl_ok = _f32_exact(gl)
    for i in range(N):
        have = [False] * 4
        nv, na, pr, err = [0.0] * 4, [0.0] * 4, [0.0] * 4, [0.0] * 4
        pr_ok = [True] * 4
        for t in range(T - 1, -1, -1):
            if done[t, i]:
                for s in range(4):
                    pr[s] = float(reward[t, i, s]) * scale
                    pr_ok[s] = _f32_exact(pr[s])
                    nv[s], na[s], err[s], have[s] = 0.0, 0.0, 0.0, True
            s = int(seat[t, i])
            v = float(val[t, i])
            ok = _f32_exact(v)
            if have[s]:
                steps = [pr[s], gamma * nv[s], pr[s] + gamma * nv[s], pr[s] + gamma * nv[s] - v, gl * na[s]]
                a = steps[3] + steps[4]
                ok = ok and pr_ok[s] and gl_ok and all(_f32_exact(x) for x in steps) and _f32_exact(a)
                mag = abs(pr[s]) + gamma * abs(nv[s]) + abs(v) + gl * abs(na[s])
                e = gl * err[s] + 8 * U * mag
                known[t, i] = True
            else:
                a, e = 0.0, 0.0
            ret[t, i], adv[t, i] = a + v, a
            lossless[t, i] = ok and _f32_exact(a + v)
            bound[t, i] = e + U * (abs(a) + abs(v))
            nv[s], na[s], pr[s], err[s], have[s], pr_ok[s] = v, a, 0.0, e, True, True
    return dict(ret=ret, adv=adv, known=known, lossless=lossless, bound=bound)
