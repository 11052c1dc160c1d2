"""GPU: tarok_playout_bids_net_list (every bid's — and the pass's — net playouts on a compacted item list) checked exactly —
bytes against bytes: sum_out against tarok_playout_bids_net (depth None / 13 without the pass) and tarok_playout_bids_net_value
(every other depth and pass_value; the pass to the end is depth 13 there) on random bf16 weights and on the exactly summable
integer sets of tests/playout_net_value_cases.py, at net_seats 15, 10 and 0 (there also tarok_playout_bids / _pass); the list
read back from the scratch against the dense grid; empty lists; a scan of more than 256 blocks; the minimal scratch of one
viewer; determinism, salt, batch independence; a captured FIRST call; the learner and the evaluation.  Every launch writes
into guard bands (tests/guarded.py) over a guarded scratch of exactly the header's size and leaves the env as it was.

Run on the GPU box:  python -m pytest tests/test_gpu_playout_bids_net_list.py -m gpu -q
"""
import functools

import numpy as np
import pytest

import front_list_cases as F
import gpu_harness as H
import playout_front_net_value_cases as C
from gpu_harness import T, random_net  # noqa: F401  (T: the module fixture)

pytestmark = pytest.mark.gpu
SEED, OFFSET, EPISODE = C.B_SEED, C.B_OFFSET, C.B_EPISODE
make_env = functools.partial(H.make_bid_env, seed=SEED, offset=OFFSET)   # (T, n, **kw): NOT reset, bidding comes first
DEPTHS = (None, 13, 12, 1)


@pytest.fixture(scope="module")
def nets(T):
    """The integer set R as a kernel set, and one random bf16 set."""
    import policy_exact_ref as PE
    return dict(R=PE.kernel_weights(T, C.weight_sets()["R"]), random=random_net(T, 19))


def both(env, kw, worlds, net_seats, depth, pass_value, tag, contracts=F.DEFAULT, **kw_launch):
    """The list launch and the dense launch of the same arguments: equal sums, and the list is the dense grid compacted."""
    a, b = [], []
    want = F.bids_dense(env, kw, EPISODE, worlds, net_seats, depth, pass_value, contracts=contracts, scratch_out=a, **kw_launch)
    got = F.bids_list(env, kw, EPISODE, worlds, net_seats, depth, pass_value, contracts=contracts, scratch_out=b, **kw_launch)
    assert got.tobytes() == want.tobytes(), (tag, np.nonzero((got != want).any(axis=(1, 2)))[0][:8])
    n = env.n
    bound = F.bid_bound(n, worlds, contracts, kw_launch.get("seats", 15), kw_launch.get("per_game") is not None, pass_value)
    total, on, base, counts = F.assert_list_is_the_dense_grid_compacted(b[0], a[0], bound, n * 80 * worlds, 4 * n, 40 * n)
    assert set(np.unique(on).tolist()) <= {0, F.bid_rows(contracts, pass_value)}
    assert (base == np.concatenate([[0], np.cumsum(counts * worlds)[:-1]])).all(), "base is the exclusive prefix sum"
    return got, total


@pytest.mark.parametrize("n,worlds,contracts", [(2, 1, F.DEFAULT), (5, 3, F.ALL), (65, 2, F.DEFAULT)])
def test_bytes_of_the_dense_launches(T, nets, n, worlds, contracts):
    """n = 2, W = 1; n = 5, W = 3 with all ten contracts; n = 65, W = 2 (260 units: across the 256-unit scan block): every
    depth, the pass both ways, net_seats 15, 10 and 0 on both weight sets; at net_seats = 0 to the end also the Bot's
    launches."""
    env = make_env(T, n)
    try:
        passes = 0
        for k, depth in enumerate(DEPTHS):
            for pass_value in (0, 1):
                for net_seats in (15, 10, 0):
                    kw = nets["R" if (k + pass_value + net_seats) & 1 else "random"]
                    got, total = both(env, kw, worlds, net_seats, depth, pass_value, (n, depth, pass_value, net_seats), contracts)
                    assert total == F.bid_bound(n, worlds, contracts, 15, False, pass_value) and got[:, :, :13].any()
                    assert pass_value or not got[:, :, 19].any()
                    passes += int(got[:, :, 19].any())
                    if net_seats == 0 and F.to_the_end(depth):
                        bot = H.launch_bids(env, worlds, 1, contracts, None, 3, 15, None, episode=EPISODE,
                                            entry="tarok_playout_bids_pass" if pass_value else "tarok_playout_bids")
                        assert got.tobytes() == bot.tobytes(), ("bot", depth, pass_value)
        assert passes >= 4
    finally:
        env.close()


def test_seat_sets_a_deals_array_and_empty_lists(T, nets):
    """seats 1 and 6, per-game sets, a `deals` array with an invalid row; then the empty seat set and a `deals` array of
    invalid rows only: total 0 and zeros."""
    n, worlds, kw = 8, 2, nets["random"]
    env = make_env(T, n)
    try:
        per = np.array([(5 * g + 3) & 15 for g in range(n)], np.uint8) | np.uint8(16)
        rng = np.random.default_rng(5)
        other = np.stack([rng.permutation(54) for _ in range(n)]).astype(np.uint8)
        other[3, 7] = other[3, 8]                                        # a card twice
        for depth, pass_value in ((None, 0), (1, 1), (None, 1)):
            for seats, per_game in ((1, None), (6, None), (9, per)):
                got, total = both(env, kw, worlds, 15, depth, pass_value, ("sets", depth, seats), salt=11, seats=seats, per_game=per_game)
                sets = per if per_game is not None else np.full(n, seats, np.uint8)
                assert all(got[g, v].any() == bool((int(sets[g]) >> v) & 1) for g in range(n) for v in range(4))
            got, total = both(env, kw, worlds, 15, depth, pass_value, ("deals", depth), deals=other, salt=2)
            assert not got[3].any() and got[0].any() and total == (n - 1) * 4 * F.popc(F.bid_rows(F.DEFAULT, pass_value)) * worlds
            got, total = both(env, kw, worlds, 15, depth, pass_value, ("empty set", depth), seats=0)
            assert total == 0 and not got.any()
            got, total = both(env, kw, worlds, 15, depth, pass_value, ("no valid deal", depth), deals=np.zeros((n, 54), np.uint8))
            assert total == 0 and not got.any()
    finally:
        env.close()


def test_a_scan_of_more_than_256_blocks(T, nets):
    """n = 16,385 (65,540 units: the scan kernel's second pass, with its carry), W = 1, seats = 1, depth 1."""
    n = 16385
    env = make_env(T, n)
    try:
        got, total = both(env, nets["random"], 1, 15, 1, 0, "multi-pass scan", seats=1)
        assert total == n * 13 and got[:, 0].any() and not got[:, 1:].any()
    finally:
        env.close()


def test_the_minimal_scratch_of_one_viewer(T, nets):
    """seats = 1: the scratch is a quarter of the all-seats size (in items), the launch equals the dense one, and one 16-byte
    step less is TAROK_EINVAL."""
    import torch
    n, worlds, kw = 5, 3, nets["R"]
    env = make_env(T, n)
    try:
        one = F.bid_scratch(n, worlds, seats=1)
        assert one == (48 * n * 13 * worlds + 72 * n + 4 + 4 + 15) // 16 * 16                 # 13 rows, 20 units: one scan block
        assert 4 * F.bid_bound(n, worlds, F.DEFAULT, 1, False, False) == F.bid_bound(n, worlds, F.DEFAULT, 15, False, False)
        both(env, kw, worlds, 15, None, 0, "minimal", seats=1)            # (bids_list's scratch is exactly `one`)
        scr = torch.empty(one, dtype=torch.uint8, device="cuda")
        out = torch.empty((n, 4, 20), dtype=torch.int32, device="cuda")
        p = env._p
        rc = lambda size, seats: env.L.tarok_playout_bids_net_list(env._h, EPISODE, None, worlds, F.DEFAULT, 0, seats, None, 15, 0, 70.0, 0,
                                                                   *[p(t) for t in kw], p(scr), size, p(out), env._stream())
        assert rc(one - 16, 1) == -1 and rc(one, 3) == -1 and rc(one, 1) == 0
        torch.cuda.synchronize()
    finally:
        env.close()


def test_determinism_salt_and_batch_independence(T, nets):
    kw = nets["random"]
    env, two = make_env(T, 5), make_env(T, 2)
    try:
        a, b = [], []
        full = F.bids_list(env, kw, EPISODE, 3, 15, 1, 1, scratch_out=a)
        again = F.bids_list(env, kw, EPISODE, 3, 15, 1, 1, scratch_out=b)
        assert again.tobytes() == full.tobytes() and a[0].tobytes() == b[0].tobytes(), "two launches, the whole scratch"
        salted = F.bids_list(env, kw, EPISODE, 3, 15, 1, 1, salt=4)
        assert salted.tobytes() != full.tobytes() and salted.tobytes() == F.bids_dense(env, kw, EPISODE, 3, 15, 1, 1, salt=4).tobytes()
        assert F.bids_list(two, kw, EPISODE, 3, 15, 1, 1).tobytes() == full[:2].tobytes()
    finally:
        env.close()
        two.close()


def test_a_captured_first_launch_replays_with_the_weights_in_place(T, nets):
    """The FIRST launch of an env captured into a graph — nothing is allocated in the call —, then the weights changed in
    place: the replay gives the eager launch's bytes for the NEW weights."""
    import torch
    env, twin = make_env(T, 16), make_env(T, 16)
    try:
        kw, other = [t.clone() for t in nets["random"]], random_net(T, 31)
        env.playout_bids_net_list_scratch(2, pass_value=True)      # allocated before the capture
        out = torch.zeros((16, 4, 20), dtype=torch.int32, device="cuda")
        old = twin.playout_bids_net_value(kw, EPISODE, 2, 2, 0.5, pass_value=True, salt=4).cpu()
        stream = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(stream):
            with torch.cuda.graph(graph, stream=stream):
                env.playout_bids_net_list(kw, EPISODE, 2, 2, 0.5, pass_value=True, salt=4, sum_out=out)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), old)
        for t, o in zip(kw, other):
            t.copy_(o)
        graph.replay()
        torch.cuda.synchronize()
        new = twin.playout_bids_net_list(other, EPISODE, 2, 2, 0.5, pass_value=True, salt=4).cpu()
        assert torch.equal(out.cpu(), new) and not torch.equal(new, old)
    finally:
        env.close()
        twin.close()


def test_the_python_surface_the_learner_and_the_evaluation(T, nets):
    """playout_bids_net_list equals the direct C call; BidLearner(net_list=True, pass_value=True) without a depth collects the
    eager list launch's rows and steps; evaluate_bidding_vs_bot(net=, net_list=True) returns the numbers of net_list=False."""
    import torch
    from oracle import tarok_spec as S
    from tarok_amd import evaluate as EV
    from tarok_amd.bidding import BidLearner
    kw = nets["random"]
    env = make_env(T, 5)
    try:
        want = F.bids_list(env, kw, EPISODE, 3, 10, 2, 1, scale=0.5, contracts=F.ALL, salt=2)
        got = env.playout_bids_net_list(kw, EPISODE, 3, 2, 0.5, pass_value=True, net_seats=10, contracts=F.ALL, salt=2)
        assert got.dtype == torch.int32 and tuple(got.shape) == (5, 4, 20) and (got.cpu().numpy() == want).all()
        assert torch.equal(env.playout_bids_net(kw, EPISODE, 3, salt=2), env.playout_bids_net_list(kw, EPISODE, 3, salt=2))
        with pytest.raises(ValueError):
            env.playout_bids_net_list(kw, EPISODE, 3, 14)
    finally:
        env.close()
    env, twin = T.TarokVecEnv(64, seed=8, mix=S.MIX_BOT), T.TarokVecEnv(64, seed=8, mix=S.MIX_BOT)
    try:
        learner = BidLearner(env, worlds=2, seed=5, net=kw, net_seats=15, net_list=True, pass_value=True)
        fw, sums, playouts = learner.collect(3)
        assert playouts == 2 and tuple(sums.shape) == (64, 4, 20) and sums[:, :, 19].any()
        assert torch.equal(sums, twin.playout_bids_net_list(kw, 3, 2, pass_value=True, net_seats=15, salt=5))
        assert torch.equal(sums, twin.playout_bids_net_value(kw, 3, 2, 13, pass_value=True, net_seats=15, salt=5))
        assert np.isfinite(learner.step(fw, sums, playouts))
    finally:
        env.close()
        twin.close()
    for depth, pass_value in ((None, False), (2, True)):
        a = EV.evaluate_bidding_vs_bot(2, None, 32, 1, seed=3, net=kw, net_list=True, net_depth=depth, pass_value=pass_value)
        b = EV.evaluate_bidding_vs_bot(2, None, 32, 1, seed=3, net=kw, net_list=False, net_depth=depth, pass_value=pass_value)
        assert a == b, depth
