"""CPU: tarok_playout_exchange_net_halving / tarok_playout_bids_net_halving without a GPU — the model's one-round and prefix
properties on the games of tests/playout_front_net_model.py, the value rounding, both scratch formulas of the header against
their restatement (tests/playout_front_halving_model.py), every TAROK_EINVAL before any HIP call (a zeroed stand-in for an
env), the signatures (net_halving directly before net_list), the ValueErrors, and the call sequences of the four doors."""
import ctypes
import inspect
import re
import struct

import numpy as np
import pytest

import playout_front_halving_model as M
from playout_net_cases import weights

DEFAULT, ALL = 0x00F, 0x3FF


@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401  -- before the dlopen: one HIP runtime
    import tarok_amd
    from tarok_amd import _native
    tarok_amd.build()
    return _native.lib()


def stand_in_env(n=0):
    """A zeroed stand-in for an env with its game count written where tarok_env keeps it (an int, padding, then int64 n)."""
    buf = ctypes.create_string_buffer(1 << 16)
    struct.pack_into("<q", buf, 8, n)
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def arr(schedule):
    return len(schedule), (ctypes.c_int * max(1, len(schedule)))(*schedule)


# ---- the model
def test_the_survivor_rule_and_the_value_rounding():
    assert M.survivors([5, 9, 5, 1], [0, 1, 2, 3]) == [0, 1] and M.survivors([5, 9, 5, 1], [0, 2, 3]) == [0, 2]
    assert M.survivors([1, 1, 1], [0, 1, 2]) == [0, 1] and M.survivors([3], [0]) == [0] and M.keep_of(1) == 1 and M.keep_of(13) == 7
    assert [M.value_of(s, 4, c) for s, c in ((6, 4), (3, 2), (-3, 2), (1, 3), (-1, 3), (5, 0))] == [6, 6, -6, 1, -1, 0]
    assert M.value_of(1, 1, 2) == 1 and M.value_of(-1, 1, 2) == -1 and M.value_of(3, 16, 12) == 4                   # halves away from zero
    for s in range(-40, 41):
        for W in (1, 4, 16, 64):
            for c in range(1, W + 1):
                v = M.value_of(s, W, c)
                assert abs(2 * (v * c - s * W)) <= c and (W % c or v * c == s * W * 1)


def front_games():
    """The Bot-played single playouts [rows, worlds, 4] of waiting games of tests/playout_front_net_model.py, per game with its
    arms and declarer."""
    import playout_exchange_model as XM
    import playout_front_net_model as FN
    from oracle import tarok_spec as S
    seed, salt, sets, worlds = 11, 3, 2, 4
    out = []
    for code in (S.TRI, S.ENA):
        games = [(XM.deferred_game(seed, gidx, 0, S.MIX_FIXED + code).lanes(), 0, gidx, None) for gidx in range(2)]
        scores = FN.exchange_scores(games, seed, salt, 15, worlds, sets, None, 0)
        for g, (lanes, _, _, _) in enumerate(games):
            out.append((list(range((6 // S.GROUP_SIZE[code]) * sets)), int((int(lanes[9]) >> 37) & 3), scores[g]))
    return out


def test_one_round_and_prefix_properties_on_the_front_models_games():
    """A one-round walk gives the uniform sums with every count W; for any schedule a row whose count is e holds the uniform
    row at worlds = e.  On the model's games, and on seeded integer playouts with ties for up to 48 arms."""
    cases = front_games()
    rng = np.random.default_rng(7)
    for k in (2, 3, 4, 6, 12, 13, 24, 48):
        sc = rng.integers(-3, 4, size=(48, 16, 4)).astype(np.int64)
        cases.append((list(range(k)), int(rng.integers(4)), sc))
    for arms, declarer, sc in cases:
        W = sc.shape[1]
        at = lambda e: sc[:, :e].sum(axis=1)
        s, c, best, cuts, alive = M.exchange_game(arms, declarer, at, (W,), sc.shape[0])
        assert (s == at(W) * np.isin(np.arange(sc.shape[0]), arms)[:, None]).all() and set(c[arms].tolist()) == {W} and not cuts
        assert best == min(arms, key=lambda j: (-int(at(W)[j, declarer]), j))
        for schedule in ((1, 1, 2), (1, 3), (2, 2), (1, 1, 1, 1)):
            if sum(schedule) > W:
                continue
            s, c, best, cuts, alive = M.exchange_game(arms, declarer, at, schedule, sc.shape[0])
            for j in range(sc.shape[0]):
                assert (s[j] == (at(int(c[j]))[j] if c[j] else 0)).all()
            assert len(alive) >= 1 and best in alive and c[alive].max() == c.max()
            keep = len(arms)
            for before, values, after in cuts:
                assert len(before) == keep and len(after) == M.keep_of(keep)
                keep = len(after)
    # the bids' pass row: played in every round its unit plays
    sums_at = lambda e: np.arange(20) * e
    s, c, v, cuts, alive = M.bid_unit(M.bid_row_mask(DEFAULT), True, sums_at, (1, 1, 2))
    assert c[19] == 4 and c[:13].max() == 4 and sorted(set(c[:13].tolist())) == [1, 2, 4] and v[19] == s[19] and alive == [9, 10, 11, 12]
    s, c, v, cuts, alive = M.bid_unit(1, True, sums_at, (2, 2, 4))
    assert c[0] == 2 and c[19] == 2 and v[19] == 19 * 2 * 4 and alive == [0]


# ---- the header's formulas
def test_the_scratch_formulas_of_the_header(L):
    fx, fb = L.tarok_playout_exchange_net_halving_scratch_bytes, L.tarok_playout_bids_net_halving_scratch_bytes
    assert M.exchange_bounds(10, (2, 2, 4, 8), 4) == [480, 240, 240, 240] and M.bid_bounds(10, (2, 2, 4, 8), DEFAULT, 15, False, True) == [1120, 640, 800, 960]
    for n in (1, 17, 43, 300, 65536):
        keep, env = stand_in_env(n)
        for schedule in ((1,), (64,), (1, 1, 2), (2, 2, 4, 8), (4, 4, 4, 4), (1, 3), (1, 1, 1, 61)):
            r, a = arr(schedule)
            for sets in range(1, 9):
                assert fx(env, r, a, sets) == M.exchange_scratch(n, schedule, sets), (n, schedule, sets)
            for contracts in (DEFAULT, ALL, 1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 0x3F0):
                for seats in (0, 1, 8, 6, 9, 15):                     # sets of 0, 1, 2 and 4 seats
                    for per_game in (0, 1):
                        for pas in (0, 1):
                            assert fb(env, r, a, contracts, seats, per_game, pas) == M.bid_scratch(n, schedule, contracts, seats, per_game, pas), \
                                (n, schedule, contracts, seats, per_game, pas)
    keep, env = stand_in_env(4096)
    r, a = arr((2, 2))
    assert fx(None, r, a, 2) == -1 and fb(None, r, a, 15, 15, 0, 0) == -1 and fx(env, r, None, 2) == -1 and fb(env, r, None, 15, 15, 0, 0) == -1
    for schedule in ((), (1, 1, 1, 1, 1), (0, 2), (2, -1), (60, 5)):
        r2, a2 = arr(schedule)
        assert fx(env, r2, a2, 2) == -1 and fb(env, r2, a2, 15, 15, 0, 0) == -1, schedule
    assert fx(env, r, a, 0) == -1 and fx(env, r, a, 9) == -1
    for bad in ((0, 15, 0, 0), (0x400, 15, 0, 0), (15, 16, 0, 0), (15, -1, 0, 0), (15, 15, 2, 0), (15, 15, -1, 0), (15, 15, 0, 2), (15, 15, 0, -1)):
        assert fb(env, r, a, *bad) == -1, bad
    # a round bound that reaches 2^31 items
    keep, env = stand_in_env(1 << 20)
    r, a = arr((64,))
    assert fx(env, r, a, 8) == -1 and fb(env, r, a, ALL, 15, 0, 1) == -1 and fb(env, r, a, ALL, 1, 1, 1) == -1
    r, a = arr((1, 63))                                           # the later round is the large one: 2^20 x 24 x 63 < 2^31 <= 2^20 x 40 x 63
    assert fx(env, r, a, 8) == M.exchange_scratch(1 << 20, (1, 63), 8) > 0 and fb(env, r, a, ALL, 15, 0, 1) == -1
    assert fb(env, r, a, ALL, 1, 0, 1) == M.bid_scratch(1 << 20, (1, 63), ALL, 1, False, True) > 0


def test_the_launches_validate_before_any_hip_call(L):
    z = ctypes.c_void_p(0)
    keep, env = stand_in_env(0)
    big_keep, big = stand_in_env(1 << 20)
    buf = ctypes.create_string_buffer(512)
    out = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    off = ctypes.c_void_p(out.value + 8)
    r, a = arr((1, 1))
    need = L.tarok_playout_exchange_net_halving_scratch_bytes(env, r, a, 2)
    assert need == 16 == L.tarok_playout_bids_net_halving_scratch_bytes(env, r, a, 15, 15, 0, 1)
    ok = dict(env=env, sched=(1, 1), sets=2, contracts=15, seats=15, per=z, net=15, depth=1, scale=70.0, pas=1, w=[out] * 6, scr=out, size=need,
              outs=[out] * 4)

    def rx(**c):
        q = dict(ok, **c)
        r, a = (q["sched"], None) if isinstance(q["sched"], int) else arr(q["sched"])
        return L.tarok_playout_exchange_net_halving(q["env"], r, a, q["sets"], 0, q["seats"], q["per"], q["net"], q["depth"], q["scale"], *q["w"],
                                                    q["scr"], q["size"], *q["outs"][:4], z)

    def rb(**c):
        q = dict(ok, **c)
        r, a = (q["sched"], None) if isinstance(q["sched"], int) else arr(q["sched"])
        return L.tarok_playout_bids_net_halving(q["env"], 0, z, r, a, q["contracts"], 0, q["seats"], q["per"], q["net"], q["depth"], q["scale"],
                                                q["pas"], *q["w"], q["scr"], q["size"], *q["outs"][:3], z)
    common = [dict(env=None), dict(sched=()), dict(sched=(1,) * 5), dict(sched=(0, 1)), dict(sched=(-1,)), dict(sched=(64, 1)), dict(sched=2),
              dict(seats=16), dict(seats=-1), dict(net=16), dict(net=-1), dict(depth=-1), dict(depth=14), dict(scale=0.0), dict(scale=-70.0),
              dict(scale=float("inf")), dict(scale=float("nan")), dict(scr=z), dict(scr=off), dict(size=need - 1), dict(size=-1), dict(outs=[z] * 4)]
    common += [dict(w=[out] * i + [z] + [out] * (5 - i)) for i in range(6)]
    for depth in (0, 1, 12, 13):
        for c in common:
            if "depth" not in c:
                c = dict(c, depth=depth)
            assert rx(**c) == -1, ("exchange", c)
            assert rb(**c) == -1, ("bids", c)
    for c in (dict(sets=0), dict(sets=9), dict(env=big, sched=(64,), sets=8, size=1 << 62)):
        assert rx(**c) == -1, c
    for c in (dict(contracts=0), dict(contracts=0x400), dict(pas=2), dict(pas=-1), dict(env=big, sched=(64,), contracts=0x3FF, size=1 << 62),
              dict(env=big, sched=(64,), contracts=0x3FF, seats=1, per=out, size=1 << 62)):
        assert rb(**c) == -1, c


# ---- the Python surface
def test_the_surface():
    from tarok_amd import _native
    from tarok_amd import evaluate as EV
    from tarok_amd import karte as K
    from tarok_amd.bidding import BidLearner
    from tarok_amd.env import TarokVecEnv
    from tarok_amd.exchange import ExchangeLearner
    for s in ("tarok_playout_exchange_net_halving_scratch_bytes", "tarok_playout_exchange_net_halving",
              "tarok_playout_bids_net_halving_scratch_bytes", "tarok_playout_bids_net_halving"):
        assert s in _native.SYMBOLS
    sig = inspect.signature(TarokVecEnv.playout_exchange_net_halving).parameters
    assert list(sig)[1:10] == ["weights", "round_worlds", "discard_sets", "depth", "value_scale", "net_seats", "salt", "seats", "seats_per_game"]
    assert [sig[k].default for k in list(sig)[3:]] == [4, None, 70.0, 15, 0, 15] + [None] * 6
    sig = inspect.signature(TarokVecEnv.playout_bids_net_halving).parameters
    assert list(sig)[1:13] == ["weights", "episode", "round_worlds", "depth", "value_scale", "pass_value", "net_seats", "contracts", "deals", "salt",
                               "seats", "seats_per_game"]
    assert [sig[k].default for k in list(sig)[4:]] == [None, 70.0, False, 15, K.BID_DEFAULT_CONTRACTS, None, 0, 15] + [None] * 5
    assert list(inspect.signature(TarokVecEnv.playout_exchange_net_halving_scratch).parameters)[1:] == ["round_worlds", "discard_sets"]
    assert list(inspect.signature(TarokVecEnv.playout_bids_net_halving_scratch).parameters)[1:] == ["round_worlds", "contracts", "seats", "per_game",
                                                                                                    "pass_value"]
    for fn in (ExchangeLearner.__init__, BidLearner.__init__, EV.evaluate_exchange_net_vs_bot, EV.evaluate_bidding_vs_bot):
        names = list(inspect.signature(fn).parameters)
        assert names[-4:] == ["net_halving", "net_list", "net_depth", "net_value_scale"], fn
        assert inspect.signature(fn).parameters["net_halving"].default is None


def test_the_value_errors():
    from tarok_amd import evaluate as EV
    from tarok_amd.bidding import BidLearner
    from tarok_amd.exchange import ExchangeLearner
    w = weights()
    h = (1, 1, 2)
    for make in (lambda: ExchangeLearner(None, net_halving=h), lambda: BidLearner(None, net_halving=h),                # needs net=
                 lambda: EV.evaluate_bidding_vs_bot(None, None, 8, 1, net_halving=h),
                 lambda: EV.evaluate_exchange_net_vs_bot(None, None, 2, 8, 1, net_halving=h),
                 lambda: ExchangeLearner(None, net=w, net_halving=h, net_list=True), lambda: BidLearner(None, net=w, net_halving=h, net_list=True),
                 lambda: EV.evaluate_bidding_vs_bot(None, None, 8, 1, net=w, net_halving=h, net_list=True),
                 lambda: EV.evaluate_exchange_net_vs_bot(w, None, 2, 8, 1, net_halving=h, net_list=True),
                 lambda: ExchangeLearner(None, net=w, net_halving=h, worlds=3), lambda: BidLearner(None, net=w, net_halving=h, worlds=5),
                 lambda: EV.evaluate_bidding_vs_bot(3, None, 8, 1, net=w, net_halving=h),
                 lambda: EV.evaluate_exchange_net_vs_bot(w, 5, 2, 8, 1, net_halving=h),
                 lambda: ExchangeLearner(None, net=w, net_halving=h, samples=2), lambda: BidLearner(None, net=w, net_halving=h, samples=2),
                 lambda: EV.evaluate_bidding_vs_bot(None, 2, 8, 1, net=w, net_halving=h),
                 lambda: ExchangeLearner(None, net=w, net_halving=()), lambda: BidLearner(None, net=w, net_halving=(1, 0)),
                 lambda: BidLearner(None, net=w, net_halving=(60, 5)), lambda: ExchangeLearner(None, net=w, net_halving=(1,) * 5),
                 lambda: ExchangeLearner(None, net=w, net_halving=h, net_depth=14), lambda: BidLearner(None, net=w, net_halving=h, net_depth=0)):
        with pytest.raises(ValueError):
            make()
    a = BidLearner(None, net=w, net_halving=h, pass_value=True)                   # the pass needs no net_depth
    assert a.net_halving == h and a.worlds == 4 and a.pass_value and a.net_depth is None and not a.net_list
    b = ExchangeLearner(None, net=w, net_halving=[2, 2], worlds=4, samples=1, net_depth=3)
    assert b.net_halving == (2, 2) and b.worlds == 4 and b.net_depth == 3
    assert ExchangeLearner(None).net_halving is None and ExchangeLearner(None).worlds == 8 and BidLearner(None).worlds == 8


def test_the_targets_divide_by_the_counts():
    import torch
    from tarok_amd.bidding import bid_loss
    from tarok_amd.exchange import exchange_targets
    g = torch.Generator(); g.manual_seed(3)
    out = torch.randn((6, 64), generator=g)
    sums = torch.randint(-300, 300, (6, 20), generator=g, dtype=torch.int32)
    for pass_value in (False, True):
        same = bid_loss(out, sums, torch.full((6, 20), 4, dtype=torch.int32), 1 / 70.0, DEFAULT, pass_value)
        assert abs(float(same) - float(bid_loss(out, sums, 4, 1 / 70.0, DEFAULT, pass_value))) < 1e-6
        counts = torch.tensor([4, 4, 2, 1, 0, 4, 2, 1, 1, 4, 0, 0, 2] + [0] * 6 + [4], dtype=torch.int32).repeat(6, 1)
        on = (counts > 0) & torch.tensor([True] * 13 + [False] * 6 + [pass_value])
        target = sums.double() / counts.clamp(min=1).double() / 70.0
        ref = torch.nn.functional.huber_loss(out[:, :20].double()[on], target[on], reduction="mean", delta=1.0)
        assert abs(float(bid_loss(out, sums, counts, 1 / 70.0, DEFAULT, pass_value)) - float(ref)) < 1e-6
    fw = torch.zeros((2, 8, 4), dtype=torch.int64)
    fw[0, :3, 0] = (1 << 56) | 1                                  # three live rows, declarer 2
    xs = torch.randint(-300, 300, (2, 12, 4), generator=g, dtype=torch.int32)
    cands = torch.full((2, 12, 3), 255, dtype=torch.uint8)
    counts = torch.tensor([[4, 1, 2, 4, 1, 1, 0, 0, 0, 0, 0, 0], [0] * 12], dtype=torch.int32)
    live, value, _, _ = exchange_targets(fw, xs, cands, counts, 1 / 70.0)
    assert live.tolist() == [[True, True, True, False, False, False], [False] * 6]
    for i in range(3):
        mean = sum(float(xs[0, 2 * i + d, 2]) / float(counts[0, 2 * i + d]) for d in range(2)) / 2 / 70.0
        assert abs(float(value[0, i]) - mean) < 1e-5
    a, b = exchange_targets(fw, xs, cands, 4, 1 / 70.0), exchange_targets(fw, xs, cands, torch.full((2, 12), 4, dtype=torch.int32), 1 / 70.0)
    assert torch.equal(a[0], b[0]) and torch.allclose(a[1], b[1], atol=1e-6)


def test_the_doors_swap_exactly_one_launch():
    """On the stand-in env: with net_halving= the one playout_*_net_list call becomes playout_*_net_halving, the bid round's
    playouts become the schedule's sum, and nothing else changes."""
    import evaluate_calls_cases as EC
    from tarok_amd import evaluate as EV
    new = {
        "x_list": ("evaluate_exchange_net_vs_bot", ("W", 4, 2), dict(net_list=True, net_depth=2), True),
        "x_half": ("evaluate_exchange_net_vs_bot", ("W", None, 2), dict(net_halving=(1, 1, 2), net_depth=2), True),
        "b_list": ("evaluate_bidding_vs_bot", (4, None), dict(net="W", net_list=True, net_depth=2, pass_value=True), False),
        "b_half": ("evaluate_bidding_vs_bot", (None, None), dict(net="W", net_halving=(1, 1, 2), net_depth=2, pass_value=True), False),
    }
    EC.CASES.update(new)
    try:
        traces = {k: EC.run_case(EV, k)[0].calls for k in new}
    finally:
        for k in new:
            del EC.CASES[k]
    for door, old, name in (("x", "playout_exchange_net_list(", "playout_exchange_net_halving("), ("b", "playout_bids_net_list(", "playout_bids_net_halving(")):
        was, now = traces[door + "_list"], traces[door + "_half"]
        assert len(was) == len(now), door
        swapped = rounds = 0
        anon = lambda c: re.sub(r"T\d+\[", "T[", c)            # the halving fronts hold more buffers: tensors are compared by shape and type
        for k, (a, b) in enumerate(zip(was, now)):
            if a.startswith(old):
                swapped += 1
                assert b.startswith(name) and "(1, 1, 2)" in b and not any(c.startswith(old) for c in now), (a, b)
                if door == "b":
                    value = re.search(r"value_out=(T\d+\[[^\]]*\]\w+@\d+)", b).group(1)
                    assert re.search(r"sum_out=(T\d+\[[^\]]*\]\w+@\d+)", b).group(1) != value and "count_out=T" in b, b
                    assert now[k + 1].startswith("bid_round(") and value in now[k + 1], (b, now[k + 1])      # the round reads value_out
                    less = re.sub(r"count_out=T\[[^\]]*\]\w+@\d+, ", "", re.sub(r"sum_out=T\[[^\]]*\]\w+@\d+, ", "", anon(b))).replace("value_out=", "sum_out=")
                    assert less.replace(", (1, 1, 2), 2, ", ", 4, 2, ") == anon(a).replace(old, name), (a, b)
                else:
                    less = re.sub(r"count_out=T\[[^\]]*\]\w+@\d+, ", "", anon(b))
                    assert less.replace(", (1, 1, 2), 2, 2, ", ", 4, 2, 2, ") == anon(a).replace(old, name), (a, b)
                    choice = re.search(r"choice_out=(T\d+\[[^\]]*\]\w+@\d+)", b).group(1)
                    assert now[k + 1].startswith("exchange(") and choice in now[k + 1], (b, now[k + 1])     # exchange() gets the launch's choice
            elif a.startswith("bid_round("):
                rounds += 1
                assert anon(a) == anon(b) and ", 4, " in a, (a, b)            # playouts = W = 4 on both sides
            else:
                assert anon(a) == anon(b), (a, b)
        assert swapped == 5 * EC.EPISODES and (door == "x" or rounds == swapped), (door, swapped, rounds)


def test_the_learners_collect_the_counts():
    """collect() on a stand-in env: one halving launch in the teacher's place, the counts returned in the place of playouts."""
    from tarok_amd.bidding import BidLearner
    from tarok_amd.exchange import ExchangeLearner
    w = weights()

    class Env:
        device = "cpu"

        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            def method(*a, **k):
                self.calls.append(name)
                return {"playout_exchange_net_halving": ("S", "C", None, None), "playout_bids_net_halving": ("S", "C", "V"),
                        "exchange_values": (None, None, None, "FW"), "bid_values": (None, None, "FW"), "exchange_candidates": "K"}.get(name)
            return method
    x = ExchangeLearner(None, net=w, net_halving=(1, 1, 2), discard_sets=2)
    x.env = Env()
    x.weights = lambda: None
    assert x.collect(0) == ("FW", "S", "K", "C") and x.env.calls == ["reset", "playout_exchange_net_halving", "exchange_candidates", "exchange_values"]
    b = BidLearner(None, net=w, net_halving=(1, 1, 2), pass_value=True)
    b.env = Env()
    b.weights = lambda: None
    assert b.collect(0) == ("FW", "S", "C") and b.env.calls == ["playout_bids_net_halving", "bid_values"]
