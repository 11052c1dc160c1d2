"""CPU: the scratch formulas of tarok_playout_exchange_net_list / tarok_playout_bids_net_list against their Python
restatement (tests/front_list_cases.py), every TAROK_EINVAL of the four entry points before any HIP call (a zeroed stand-in
for an env), the parameter lists of the four env methods, net_list in the four callers, their ValueErrors, and the call
sequences of the two evaluations on the stand-in env of tests/evaluate_calls_cases.py.  No GPU involved."""
import ctypes
import inspect
import json
import struct

import pytest

import front_list_cases as F
from playout_net_cases import weights


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


def test_the_restatement_itself():
    assert F.bid_row_mask(F.DEFAULT) == 0x1FFF and F.popc(F.bid_rows(F.DEFAULT, False)) == 13 and F.popc(F.bid_rows(F.ALL, True)) == 20
    assert F.bid_scratch(1, 1, seats=1) == (48 * 13 + 72 + 4 + 4 + 15) // 16 * 16
    assert F.bid_bound(4096, 8, F.DEFAULT, 1, False, False) * 48 == 4096 * 8 * 624         # 48 x 13 x W a game for one viewer, against 3,840 x W


def test_the_scratch_formulas_of_the_header(L):
    fx, fb = L.tarok_playout_exchange_net_list_scratch, L.tarok_playout_bids_net_list_scratch
    for n in (1, 17, 42, 43, 64, 65, 300, 65536):
        keep, env = stand_in_env(n)
        for worlds in (1, 3, 64):
            for sets in (1, 2, 4, 8):
                assert fx(env, worlds, sets) == F.exchange_scratch(n, worlds, sets), (n, worlds, sets)
            for contracts in (F.DEFAULT, F.ALL, 1, 0x3F0, 0x2):
                for seats in (0, 1, 8, 6, 9, 15):                    # sets of 0, 1, 2 and 4 seats
                    for per_game in (0, 1):
                        for pas in (0, 1):
                            assert fb(env, worlds, contracts, seats, per_game, pas) == F.bid_scratch(n, worlds, contracts, seats, per_game, pas), \
                                (n, worlds, contracts, seats, per_game, pas)
    keep, env = stand_in_env(4096)
    assert fb(env, 8, F.DEFAULT, 1, 0, 0) == 4096 * 8 * 624 + 4096 * 72 + 4 * 64 + 16 and fb(env, 8, F.DEFAULT, 15, 0, 0) > 4 * 4096 * 8 * 624
    assert fx(None, 1, 1) == -1 and fb(None, 1, 1, 15, 0, 0) == -1
    for a in ((0, 2), (65, 2), (2, 0), (2, 9)):
        assert fx(env, *a) == -1, a
    for a in ((0, 15, 15, 0, 0), (65, 15, 15, 0, 0), (2, 0, 15, 0, 0), (2, 0x400, 15, 0, 0), (2, 15, 16, 0, 0), (2, 15, -1, 0, 0), (2, 15, 15, 2, 0),
              (2, 15, 15, -1, 0), (2, 15, 15, 0, 2), (2, 15, 15, 0, -1)):
        assert fb(env, *a) == -1, a
    # a bound that reaches 2^31 items
    keep, env = stand_in_env(1 << 20)                        # 2^20 games x 48 rows x 64 worlds = 3 x 2^30
    assert fx(env, 64, 8) == -1 and fx(env, 32, 8) == F.exchange_scratch(1 << 20, 32, 8) > 0
    assert fb(env, 64, F.ALL, 15, 0, 1) == -1 and fb(env, 64, F.ALL, 1, 0, 1) == F.bid_scratch(1 << 20, 64, F.ALL, 1, False, True) > 0
    assert fb(env, 64, F.ALL, 1, 1, 1) == -1                 # per-game sets: four viewers whatever `seats`
    keep, env = stand_in_env((1 << 31) // 6 + 1)             # n x 6 x 1 x 1 just reaches 2^31
    assert fx(env, 1, 1) == -1
    keep, env = stand_in_env((1 << 31) // 6)
    assert fx(env, 1, 1) == F.exchange_scratch((1 << 31) // 6, 1, 1)


def test_the_launches_validate_before_any_hip_call(L):
    """Every refusal comes before the first HIP call: a zeroed stand-in for an env (no GPU, no tarok_create) is enough."""
    z = ctypes.c_void_p(0)
    keep, env = stand_in_env(0)
    big_keep, big = stand_in_env(1 << 20)
    buf = ctypes.create_string_buffer(512)
    out = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    off = ctypes.c_void_p(out.value + 8)
    need = L.tarok_playout_exchange_net_list_scratch(env, 2, 2)
    assert need == 16 == L.tarok_playout_bids_net_list_scratch(env, 2, 15, 15, 0, 1)
    ok = dict(env=env, worlds=2, sets=2, contracts=15, seats=15, per=z, net=15, depth=1, scale=70.0, pas=1, w=[out] * 6, scr=out, size=need, sum=out,
              ch=out, di=out)

    def rx(**c):
        a = dict(ok, **c)
        return L.tarok_playout_exchange_net_list(a["env"], a["worlds"], a["sets"], 0, a["seats"], a["per"], a["net"], a["depth"], a["scale"], *a["w"],
                                                 a["scr"], a["size"], a["sum"], a["ch"], a["di"], z)

    def rb(**c):
        a = dict(ok, **c)
        return L.tarok_playout_bids_net_list(a["env"], 0, z, a["worlds"], a["contracts"], 0, a["seats"], a["per"], a["net"], a["depth"], a["scale"],
                                             a["pas"], *a["w"], a["scr"], a["size"], a["sum"], z)
    common = [dict(env=None), dict(worlds=0), dict(worlds=65), dict(seats=16), dict(seats=-1), dict(net=16), dict(net=-1), dict(depth=-1),
              dict(depth=14), dict(scale=0.0), dict(scale=-70.0), dict(scale=float("inf")), dict(scale=float("nan")), dict(scr=z), dict(scr=off),
              dict(size=need - 1), dict(size=-1)]
    common += [dict(w=[out] * i + [z] + [out] * (5 - i)) for i in range(6)]
    for depth in (0, 1, 12, 13):
        for c in common:
            if "depth" not in c:
                c = dict(c, depth=depth)
            assert rx(**c) == -1, ("exchange", c)
            assert rb(**c) == -1, ("bids", c)
    for c in (dict(sets=0), dict(sets=9), dict(sum=z, ch=z, di=z), dict(env=big, worlds=64, sets=8, size=1 << 62)):
        assert rx(**c) == -1, c
    for c in (dict(contracts=0), dict(contracts=0x400), dict(pas=2), dict(pas=-1), dict(sum=z), dict(env=big, worlds=64, contracts=0x3FF, size=1 << 62),
              dict(env=big, worlds=64, contracts=0x3FF, seats=1, per=out, size=1 << 62)):
        assert rb(**c) == -1, c


def test_the_surface():
    from tarok_amd import _native
    from tarok_amd import evaluate as EV
    from tarok_amd import karte as K
    from tarok_amd.bidding import BidLearner
    from tarok_amd.env import TarokVecEnv
    from tarok_amd.exchange import ExchangeLearner
    for s in ("tarok_playout_exchange_net_list_scratch", "tarok_playout_exchange_net_list", "tarok_playout_bids_net_list_scratch",
              "tarok_playout_bids_net_list"):
        assert s in _native.SYMBOLS
    sig = inspect.signature(TarokVecEnv.playout_exchange_net_list).parameters
    assert list(sig)[1:] == ["weights", "worlds", "discard_sets", "depth", "value_scale", "net_seats", "salt", "seats", "seats_per_game", "sum_out",
                             "choice_out", "discards_out"]
    assert [sig[k].default for k in list(sig)[3:]] == [4, None, 70.0, 15, 0, 15, None, None, None, None]
    sig = inspect.signature(TarokVecEnv.playout_exchange_net_list_scratch).parameters
    assert list(sig)[1:] == ["worlds", "discard_sets"] and sig["discard_sets"].default == 4
    sig = inspect.signature(TarokVecEnv.playout_bids_net_list).parameters
    assert list(sig)[1:] == ["weights", "episode", "worlds", "depth", "value_scale", "pass_value", "net_seats", "contracts", "deals", "salt", "seats",
                             "seats_per_game", "sum_out"]
    assert [sig[k].default for k in list(sig)[4:]] == [None, 70.0, False, 15, K.BID_DEFAULT_CONTRACTS, None, 0, 15, None, None]
    sig = inspect.signature(TarokVecEnv.playout_bids_net_list_scratch).parameters
    assert list(sig)[1:] == ["worlds", "contracts", "seats", "per_game", "pass_value"]
    assert [sig[k].default for k in list(sig)[2:]] == [K.BID_DEFAULT_CONTRACTS, 15, False, False]
    for fn in (ExchangeLearner.__init__, BidLearner.__init__, EV.evaluate_exchange_net_vs_bot, EV.evaluate_bidding_vs_bot):
        names = list(inspect.signature(fn).parameters)
        assert names[-3:] == ["net_list", "net_depth", "net_value_scale"], fn
        assert inspect.signature(fn).parameters["net_list"].default is False


def test_the_value_errors():
    from tarok_amd import evaluate as EV
    from tarok_amd.bidding import BidLearner
    from tarok_amd.exchange import ExchangeLearner
    w = weights()
    for make in (lambda: ExchangeLearner(None, net_list=True), lambda: BidLearner(None, net_list=True),
                 lambda: EV.evaluate_bidding_vs_bot(2, 1, 8, 1, net_list=True),
                 lambda: EV.evaluate_exchange_net_vs_bot(None, 2, 2, 8, 1, net_list=True),
                 # the existing ones, unchanged
                 lambda: BidLearner(None, net=w, pass_value=True), lambda: BidLearner(None, net_depth=2), lambda: ExchangeLearner(None, net_depth=2),
                 lambda: BidLearner(None, net=w, net_list=True, samples=2), lambda: ExchangeLearner(None, net=w, net_list=True, net_seats=16),
                 lambda: BidLearner(None, net=w, net_list=True, net_depth=14), lambda: ExchangeLearner(None, net=w, net_list=True, net_depth=0),
                 lambda: EV.evaluate_bidding_vs_bot(2, 1, 8, 1, net_depth=2), lambda: EV.evaluate_bidding_vs_bot(2, None, 8, 1, net=w, pass_value=True),
                 lambda: EV.evaluate_bidding_vs_bot(2, None, 8, 1, net=w, net_list=True, pass_value=True),
                 lambda: EV.evaluate_bidding_vs_bot(2, 2, 8, 1, net=w, net_list=True),
                 lambda: EV.evaluate_exchange_net_vs_bot(w, 2, 2, 8, 1, net_list=True, net_depth=14)):
        with pytest.raises(ValueError):
            make()
    a = BidLearner(None, net=w, net_list=True, pass_value=True)                  # the list launch values the pass at any depth
    assert a.net_list and a.pass_value and a.net_depth is None
    assert ExchangeLearner(None, net=w, net_list=True).net_list and not ExchangeLearner(None, net=w).net_list and not BidLearner(None).net_list


def test_the_env_methods_issue_the_launches():
    """The two env methods on a stand-in: the scratch asked for at the launch's shape, depth 0 for None, the pass as 0 / 1."""
    import torch
    from playout_net_cases import Calls, no_device
    from tarok_amd.env import TarokVecEnv

    class Env:
        n, device, _h = 4, torch.device("cpu"), 77
        check_mlp_weights = staticmethod(TarokVecEnv.check_mlp_weights)
        _list_value = staticmethod(TarokVecEnv._list_value)
        _dev, _empty = TarokVecEnv._dev, TarokVecEnv._empty

        def __init__(self):
            self.L, self.asked = Calls(), []

        def playout_exchange_net_list_scratch(self, *a):
            self.asked.append(("x",) + a)
            return torch.zeros(1000, dtype=torch.uint8)

        def playout_bids_net_list_scratch(self, *a):
            self.asked.append(("b",) + a)
            return torch.zeros(2000, dtype=torch.uint8)

        def _p(self, t):
            return None if t is None else "%s%s" % (str(t.dtype).replace("torch.", ""), list(t.shape))

        def _seat_sets(self, s):
            return s

        def _stream(self):
            return "stream"
    net = weights()
    w = "'bfloat16[256, 256]', 'float32[256]', 'bfloat16[256, 256]', 'float32[256]', 'bfloat16[64, 256]', 'float32[64]'"
    with no_device():
        env = Env()
        TarokVecEnv.playout_exchange_net_list(env, net, 3, 2, net_seats=5, salt=3, seats=9)
        TarokVecEnv.playout_exchange_net_list(env, net, 3, 2, 12, 0.5)
        assert env.asked == [("x", 3, 2)] * 2
        assert env.L.calls[0] == "tarok_playout_exchange_net_list(77, 3, 2, 3, 9, None, 5, 0, 70.0, %s, 'uint8[1000]', 1000, 'int32[4, 12, 4]', " \
            "'int8[4]', 'uint8[4, 3]', 'stream')" % w, env.L.calls[0]
        assert ", None, 15, 12, 0.5, " in env.L.calls[1]
        env = Env()
        TarokVecEnv.playout_bids_net_list(env, net, 7, 3, pass_value=True, net_seats=5, salt=3, seats=1)
        TarokVecEnv.playout_bids_net_list(env, net, 7, 3, 1, 0.5, contracts=0x3FF, seats_per_game=torch.zeros(4, dtype=torch.uint8))
        assert env.asked == [("b", 3, 15, 1, False, True), ("b", 3, 0x3FF, 15, True, False)]
        assert env.L.calls[0] == "tarok_playout_bids_net_list(77, 7, None, 3, 15, 3, 1, None, 5, 0, 70.0, 1, %s, 'uint8[2000]', 2000, " \
            "'int32[4, 4, 20]', 'stream')" % w, env.L.calls[0]
        assert "tarok_playout_bids_net_list(77, 7, None, 3, 1023, 0, 15, 'uint8[4]', 15, 1, 0.5, 0, " in env.L.calls[1]
        for bad in (dict(net_seats=16), dict(depth=0), dict(depth=14), dict(depth=1, value_scale=0.0)):
            with pytest.raises(ValueError):
                TarokVecEnv.playout_exchange_net_list(Env(), net, 3, 2, **bad)
            with pytest.raises(ValueError):
                TarokVecEnv.playout_bids_net_list(Env(), net, 7, 3, **bad)


def test_the_evaluations_change_one_call_name():
    """On the stand-in env: with net_list=True every playout_*_net[_value] call becomes playout_*_net_list with the same
    arguments and nothing else changes; with net_list=False the calls are those of the call without the keyword, and the
    golden records hold."""
    import evaluate_calls_cases as EC
    from tarok_amd import evaluate as EV
    xa, ba = (2, 2), (2, None)
    new = {}
    for tag, kw in (("plain", {}), ("deep", dict(net_depth=2, net_value_scale=35.0)), ("own", dict(net_seats="own", cards="W"))):
        for mode, extra in (("none", {}), ("off", dict(net_list=False)), ("on", dict(net_list=True))):
            new["x_%s_%s" % (tag, mode)] = ("evaluate_exchange_net_vs_bot", ("W",) + xa, dict(kw, **extra), True)
            new["b_%s_%s" % (tag, mode)] = ("evaluate_bidding_vs_bot", ba, dict(kw, net="W", **extra), True)
    new["b_pass_none"] = ("evaluate_bidding_vs_bot", ba, dict(net="W", net_depth=3, pass_value=True), False)
    new["b_pass_on"] = ("evaluate_bidding_vs_bot", ba, dict(net="W", net_depth=3, pass_value=True, net_list=True), False)
    EC.CASES.update(new)
    try:
        traces = {k: EC.run_case(EV, k)[0].calls for k in new}
    finally:
        for k in new:
            del EC.CASES[k]
    dense = {"x": ("playout_exchange_net(", "playout_exchange_net_value("), "b": ("playout_bids_net(", "playout_bids_net_value(")}
    for k in new:
        if k.endswith("_off"):
            assert traces[k] == traces[k[:-4] + "_none"], k
        if k.endswith("_on"):
            on, none = traces[k], traces[k[:-3] + "_none"]
            old = dense[k[0]][0 if "plain" in k or "own" in k else 1]
            name = "playout_exchange_net_list(" if k[0] == "x" else "playout_bids_net_list("
            assert len(on) == len(none), k
            swapped = 0
            for a, b in zip(on, none):
                if b.startswith(old):
                    swapped += 1
                    assert a == name + b[len(old):], (k, a, b)
                else:
                    assert a == b, (k, a, b)
            assert swapped == 5 * EC.EPISODES and not any(c.startswith(dense[k[0]]) for c in on), k
    with open(EC.FIXTURE) as f:
        golden = json.load(f)
    assert json.loads(json.dumps(EC.record_all(EV))) == golden
