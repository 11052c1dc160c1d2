"""GPU: tarok_front_lines (the bid and exchange heads on the dealt-ahead games) and tarok_get_lines.

n = 300 (two step groups, the second partial), K.MIX_BOT, auto-reset.  Every line of get_lines() is looked at; count_out,
contract_hist_out and the scratch sit inside guard bands (tests/guarded.py).  The reference is a TWIN env (same seed,
offset, n) taken through the heads' existing chain at the line's episode — bid_values[_pass] -> bid_round[_pass] ->
reset(E, contract, declarer, king, defer_exchange=True) -> exchange_values -> exchange — one chain per distinct episode:
a line must hold that game, lane for lane, under the twin's key.  Every comparison is of integers.

Run on the GPU box:  python -m pytest tests/test_gpu_front_lines.py -m gpu -q
"""

import numpy as np
import pytest

from gpu_harness import T  # noqa: F401  (the module fixture)
from front_lines_cases import (OFFSET, SEED, AHEAD, N, assert_lines_are_twins, front, make_env, random_weights, sets_tensor, split,
                               twin_chain, valid_lines)

pytestmark = pytest.mark.gpu

EINVAL = -1


@pytest.fixture(scope="module")
def W(T):
    return dict(bid=random_weights(11, 4.0), exchange=random_weights(12, 4.0))


def test_empty_set_keeps_the_bytes_and_marks(T, W):
    env = make_env(T)
    before = env.get_lines()
    _, _, nep0, mark0 = split(before)
    assert valid_lines(env, nep0).all() and (mark0 == 0).all(), "reset + prefetch: 14 valid, unmarked lines a slot"
    count, hist = front(env, bid=W["bid"], exchange=W["exchange"], scale=70.0, seats=0)
    after = env.get_lines()
    assert count == AHEAD * N and hist.sum() == count
    assert (after[:, :, :5] == before[:, :, :5]).all(), "bytes 0..39 of every line"
    _, _, nep, mark = split(after)
    assert (nep == nep0).all() and (mark == nep).all()
    count, hist = front(env, bid=W["bid"], exchange=W["exchange"], scale=70.0, seats=0)
    assert count == 0 and (hist == 0).all()
    assert (env.get_lines() == after).all()
    env.reset(episode=0)                                  # a reset clears the marks: the same episodes are fronted again
    env.prefetch()
    count, _ = front(env, exchange=W["exchange"], seats=0)
    assert count == AHEAD * N
    env.close()


CASES = [dict(seats=15), dict(seats=5), dict(per_game=True), dict(seats=15, pass_value=True, margin=3, playouts=4),
         dict(per_game=True, pass_value=True, contracts=0x3FF), dict(seats=15, contracts=0x3FF, margin=-2),
         dict(seats=15, bid_only=True), dict(seats=10, exchange_only=True)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join("%s=%s" % kv for kv in sorted(c.items())))
def test_lines_equal_the_twin_chain(T, W, case):
    env = make_env(T)
    kw = dict(scale=70.0, seats=case.get("seats", 15), contracts=case.get("contracts", 0xF), margin=case.get("margin", 0),
              playouts=case.get("playouts", 1), pass_value=case.get("pass_value", False))
    if not case.get("exchange_only"):
        kw["bid"] = W["bid"]
    if not case.get("bid_only"):
        kw["exchange"] = W["exchange"]
    if case.get("per_game"):
        kw["seats_per_game"] = sets_tensor(N)
    count, hist = front(env, **kw)
    assert count == AHEAD * N
    lines, lanes = env.get_lines(lanes=True)
    assert (np.bincount(((lanes[9] >> np.uint64(33)) & np.uint64(15)).astype(np.int64).reshape(-1), minlength=10) == hist).all()
    assert_lines_are_twins(T, env, np.ones((N, AHEAD), bool), kw)
    if case.get("per_game"):
        assert (hist > 0).sum() >= 2, "tables of every make-up, the Bots' alone among them: more than one contract occurs"
    env.close()


def test_exchange_only_on_a_fixed_mix(T, W):
    from tarok_amd import karte as K
    mix = K.MIX_FIXED + 2
    env = make_env(T, mix=mix)
    kw = dict(exchange=W["exchange"], seats_per_game=sets_tensor(N))
    count, hist = front(env, **kw)
    assert count == AHEAD * N and hist[2] == count
    assert_lines_are_twins(T, env, np.ones((N, AHEAD), bool), kw, mix=mix)
    env.close()


def test_integer_weights_equal_the_cpu_model(T):
    """The weight sets of tests/policy_exact_ref.py (sums exact in float32 in any order): lines equal
    tests/front_lines_model.py's game, every seventh slot, three lines each, per-slot seat sets, with and without the pass."""
    import front_lines_model as FM
    import policy_exact_ref as PE
    from oracle import tarok_spec as S
    Wb, Wx = PE.weights_p(*PE.P_PARAMS[1]), PE.weights_p(*PE.P_PARAMS[8])
    env = make_env(T)
    sets = sets_tensor(N)
    for pass_value in (False, True):
        env.reset(episode=0)
        env.prefetch()
        contracts = 0x3FF if pass_value else 0x7F             # (with all ten nearly every round ends in a Berac: no exchange)
        count, _ = front(env, bid=PE.kernel_weights(T, Wb), exchange=PE.kernel_weights(T, Wx), scale=64.0, contracts=contracts,
                         seats_per_game=sets, pass_value=pass_value, margin=1)
        assert count == AHEAD * N
        lines, lanes = env.get_lines(lanes=True)
        nep, seats = split(lines)[2], sets.cpu().numpy()
        bid = dict(W=Wb, scale=64.0, playouts=1, margin=1, contracts=contracts, pass_value=pass_value)
        for j in range(0, N, 7):
            for b in (0, 5, 13):
                g = FM.front_game(SEED, OFFSET + j, int(nep[j, b]), int(seats[j]), S.MIX_BOT, bid=bid, exchange=Wx)
                assert [int(x) for x in g.lanes()] == [int(x) for x in lanes[:, j, b]], (pass_value, j, b)
    env.close()


def test_rollout_with_a_call_every_16_launches(T, W):
    """64 policy_step launches, front_lines every 16: every game a slot started is the fronted one; lines dealt since the
    last call are unmarked and the Bot's; stale lines are not touched by a call."""
    import torch
    env = make_env(T)
    kw = dict(bid=W["bid"], exchange=W["exchange"], scale=70.0, seats=15, contracts=0x3FF)
    pol = random_weights(13)
    words = [env.legal_actions().words.clone(), torch.empty(N, dtype=torch.int64, device="cuda")]
    act = torch.empty(N, dtype=torch.uint8, device="cuda")
    done = torch.empty(N, dtype=torch.uint8, device="cuda")
    started = {}                                          # episode -> (slots, lanes at the start of that game)
    ep_before = env.counters()[0]
    for t in range(64):
        if t % 16 == 0:
            stale = ~valid_lines(env, split(env.get_lines())[2])
            before = env.get_lines()
            count, _ = front(env, **kw)
            after = env.get_lines()
            assert (after[stale] == before[stale]).all(), "a line with a stale tag is skipped"
            assert count == int((split(before)[3] != split(before)[2])[~stale].sum())
        env.policy_step(pol, words[t & 1], words[~t & 1], act, done_out=done)
        ep = env.counters()[0]
        new = np.nonzero(ep != ep_before)[0]
        if len(new):
            assert (ep[new] == ep_before[new] + 1).all()
            lanes = env.state()
            for e in np.unique(ep[new]):
                j = new[ep[new] == e]
                started.setdefault(int(e), []).append((j, lanes[:, j]))
        ep_before = ep
    assert len(np.unique(ep_before)) > 2, "episodes have spread"
    for e, parts in started.items():
        want, _ = twin_chain(T, e, kw)
        for j, lanes in parts:
            assert (lanes == want[:, j]).all(), ("a slot started an unfronted game", e)
    lines, lanes = env.get_lines(lanes=True)
    _, _, nep, mark = split(lines)
    fresh = valid_lines(env, nep) & (mark != nep)
    assert fresh.any(), "lines dealt since the last call"
    for e in np.unique(nep[fresh]):
        want, _ = twin_chain(T, int(e), dict(seats=0))     # the Bot's line
        j, b = np.nonzero(fresh & (nep == e))
        assert (lanes[:, j, b] == want[:, j]).all()
    env.close()


def test_a_captured_call_reads_the_weights_in_place(T, W):
    import torch
    env = make_env(T)
    wb, wx = [t.clone() for t in random_weights(21, 4.0)], [t.clone() for t in random_weights(22, 4.0)]
    kw = dict(bid=wb, exchange=wx, scale=70.0, seats=15, contracts=0x3FF)
    env.front_lines_scratch()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        env.front_lines(**kw)                             # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        env.front_lines(**kw)
    for dst, src in zip(wb + wx, W["bid"] + W["exchange"]):
        dst.copy_(src)
    env.reset(episode=0)
    env.prefetch()
    g.replay()
    torch.cuda.synchronize()
    assert_lines_are_twins(T, env, np.ones((N, AHEAD), bool), dict(kw, bid=W["bid"], exchange=W["exchange"]))
    env.close()


def test_every_einval(T, W):
    import torch
    from tarok_amd import karte as K
    env = make_env(T)
    fixed = make_env(T, mix=K.MIX_FIXED + 1)
    before = env.get_lines()
    scratch = torch.empty(int(env.L.tarok_front_lines_scratch_bytes(N)), dtype=torch.uint8, device="cuda")
    b, x, none = [env._p(t) for t in W["bid"]], [env._p(t) for t in W["exchange"]], [None] * 6

    def call(h=None, bid=b, scale=70.0, playouts=1, contracts=0xF, exch=x, seats=15, scr=scratch, nbytes=None):
        return env.L.tarok_front_lines(env._h if h is None else h, *bid, scale, playouts, 0, contracts, 0, *exch, seats, None,
                                       None if scr is None else env._p(scr), scratch.numel() if nbytes is None else nbytes, None, None,
                                       env._stream())
    assert call(h=0) == EINVAL
    assert call(bid=none, exch=none) == EINVAL
    for k in range(6):
        assert call(bid=b[:k] + [None] + b[k + 1:]) == EINVAL and call(exch=x[:k] + [None] + x[k + 1:]) == EINVAL
    for scale in (0.0, -1.0, float("nan"), 2.0 ** 20 + 1):
        assert call(scale=scale) == EINVAL
    assert call(playouts=0) == EINVAL
    for contracts in (0, 0x400, -1):
        assert call(contracts=contracts) == EINVAL
    for seats in (-1, 16):
        assert call(seats=seats) == EINVAL
    assert call(scr=None) == EINVAL and call(nbytes=scratch.numel() - 1) == EINVAL
    assert call(h=fixed._h) == EINVAL, "bid weights on an env whose mix is not the Bot's round"
    assert call(h=fixed._h, bid=none) == 0, "the exchange weights alone go with any mix"
    assert env.L.tarok_front_lines_scratch_bytes(0) < 0
    torch.cuda.synchronize()
    assert (env.get_lines() == before).all(), "a refused call launches nothing"
    env.close()
    fixed.close()
