"""TEST INFRASTRUCTURE — the slot patterns of the GAE returns tests (tests/test_gpu_learner_gae.py and the opponent tests
built on it): the rollout arrays of a case (numpy, no GPU), the model's returns, the guarded launch and the bit
comparison."""
import functools

import numpy as np

from gae_model import gae_model


SEAT_SHIFT = 54
SHAPES = [(12, 300), (13, 300), (1, 1)]
F32 = lambda x: float(np.float32(x))                      # what the C ABI's float arguments hold


@functools.lru_cache(maxsize=None)
def arrays(Tn, n, eighths, one_done=False):
    """The rollout arrays of one case (numpy, made once and shared; nobody writes to them).  eighths: values are multiples
    of 1/8 in [-4, 4] (the exact test), else standard normal."""
    rnd = np.random.RandomState(1000 * Tn + n + (7 if eighths else 0))
    done = rnd.rand(Tn, n) < 0.15
    seat = rnd.randint(0, 4, (Tn, n))
    if n > 1:
        slot = np.arange(n)
        never = (slot % 7 == 3) | (slot == n - 1)
        first = (slot % 11 == 5) & ~never
        last = ((slot % 13 == 6) | (slot == n - 2)) & ~never & ~first
        twice = (slot % 17 == 8) & ~never & ~first
        done[Tn - 1, last] = True
        done[Tn // 2, twice] = True; done[Tn // 2 + 1, twice] = True
        done[:, first] = False; done[0, first] = True
        done[:, never] = False
        lame = slot % 5 == 2                                                     # seat 2 never moves
        seat[:, lame] = np.where(seat[:, lame] == 2, 3, seat[:, lame])
        assert never.any() and first.any() and last.any() and twice.any() and lame.any() and never[256:].any(), "the slot patterns lack one of the cases the tests name"
    else:
        done[:] = one_done
    reward = rnd.randint(-90, 91, (Tn, n, 4)).astype(np.int16)                   # (read only where done)
    words = (seat.astype(np.int64) << SEAT_SHIFT) | rnd.randint(0, 1 << 50, (Tn, n)).astype(np.int64)
    logp = -rnd.rand(Tn, n).astype(np.float32)
    val = (rnd.randint(-32, 33, (Tn, n)) / 8.0 if eighths else rnd.randn(Tn, n)).astype(np.float32)
    act = rnd.randint(0, 54, (Tn, n)).astype(np.uint8)
    return dict(T=Tn, n=n, done=done.astype(np.uint8), reward=reward, seat=seat, words=words, logp=logp, val=val, act=act)


@functools.lru_cache(maxsize=None)
def model(Tn, n, eighths, one_done, gamma, lam, scale):
    a = arrays(Tn, n, eighths, one_done)
    return gae_model(a["done"], a["reward"], a["seat"], a["val"], gamma, lam, scale)


def launch(env, a, gamma, lam, scale, spare_rows=3, call=None):
    """One tarok_learn_returns_gae launch on the case's arrays with rec, stats and scratch between guard bands (scratch
    with `spare_rows` rows more than the ceil(n / 256) the launch may write).  Returns (rec [T,n,4] f32, stats [4] f32,
    scratch values, scratch written mask) after checking that no byte outside the three arrays changed and that every
    element of rec and stats was written."""
    import torch
    from guarded import Guarded, assert_guards_intact
    Tn, n = a["T"], a["n"]
    dev = {k: torch.from_numpy(a[k]).cuda() for k in ("done", "reward", "words", "logp", "val", "act")}
    blocks = (n + 255) // 256
    rec = Guarded("rec_out", Tn, n, np.float32, inner=(4,), device="cuda")
    stats = Guarded("stats_out", 1, 4, np.float32, device="cuda")
    scratch = Guarded("scratch", blocks + spare_rows, 1, np.float32, inner=(4,), device="cuda")
    view = lambda g: g.payload().view(torch.float32)
    if call is None:
        env.learn_returns_gae(Tn, dev["done"], dev["reward"], dev["words"], dev["logp"], dev["val"], dev["act"], scale, gamma, lam,
                              view(rec), view(stats), view(scratch))
    else:
        call(dev, view(rec), view(stats), view(scratch))
    torch.cuda.synchronize()
    assert_guards_intact([rec, stats, scratch], (Tn, n, gamma, lam))
    r, r_written = rec.host()
    s, s_written = stats.host()
    c, c_written = scratch.host()
    return r, r_written, s[0], s_written[0], c[:, 0], c_written[:, 0], blocks


def check_bits(r, a, m):
    bits = np.ascontiguousarray(r[..., 3]).view(np.uint32)
    assert ((bits & 255) == a["act"]).all() and (((bits >> 8) & 1).astype(bool) == m["known"]).all() and (bits >> 9 == 0).all(), "the packed word is not (act, known) of the case"
    assert (np.ascontiguousarray(r[..., 0]).view(np.uint32) == a["logp"].view(np.uint32)).all(), "the record's logp is not the case's, bit for bit"
    assert (np.ascontiguousarray(r[..., 2]).view(np.uint32) == a["val"].view(np.uint32)).all(), "the record's value is not the case's, bit for bit"
