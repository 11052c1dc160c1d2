"""TEST INFRASTRUCTURE — the recorded calls of the evaluate_* drivers (tests/test_evaluate_calls_cpu.py and the CPU tests of
the playout players): the stand-in env that records every launch, the cases, and the packing of a recorded trace.
No GPU."""
import contextlib
import os
import re

import numpy as np
import torch


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "evaluate_calls_v1.json")
N, EPISODES = 2, 2
FILLED = ("start", "scores", "contract", "declarer", "king_suit")    # inspect arrays whose content the stand-in decides


class Trace:
    """The record of one case: the calls, the tensors seen (kept alive: a freed storage's address could come back) and
    the number of close() calls.  fail_at: the name of a method that raises."""

    def __init__(self, fail_at=None):
        self.calls, self.storages, self.keep, self.closed, self.fail_at = [], {}, [], 0, fail_at
        self.tuples = {}                    # a tuple of tensors (six weights) is written out once and named W<i> in the calls

    def show(self, x):
        if torch.is_tensor(x):
            self.keep.append(x)
            i = self.storages.setdefault(x.untyped_storage().data_ptr(), len(self.storages))
            return "T%d%s%s@%d" % (i, list(x.shape), str(x.dtype).replace("torch.", "").replace("float", "f").replace("uint", "u").replace("int", "i"), x.storage_offset())
        if isinstance(x, (tuple, list)):
            text = "(%s)" % ", ".join(self.show(v) for v in x)
            return self.tuples.setdefault(text, "W%d" % len(self.tuples)) if any(torch.is_tensor(v) for v in x) else text
        assert "@" not in repr(x), "not true: \"@\" not in repr(x)"
        return repr(x)

    def call(self, name, args, kwargs):
        shown = [self.show(a) for a in args] + ["%s=%s" % (k, self.show(v)) for k, v in sorted(kwargs.items())]
        self.calls.append("%s(%s)" % (name, ", ".join(shown)))
        if name == self.fail_at:
            raise RuntimeError("the stand-in's %s fails" % name)
        return len(self.calls) - 1


def stand_in(trace):
    """A class to put in evaluate.TarokVecEnv's place: it has what evaluate reads of an env, records every call in
    `trace` and returns what evaluate reads back, filled with the call's ordinal."""
    from tarok_amd import karte as K
    from tarok_amd.env import TarokVecEnv

    class Env:
        check_mlp_weights = staticmethod(TarokVecEnv.check_mlp_weights)

        def __init__(self, n_games, device=0, seed=0, mix=K.MIX_ALL, history=False):
            trace.call("TarokVecEnv", (n_games,), dict(device=device, seed=seed, mix=mix, history=history))
            self.n, self.device_index, self.device = int(n_games), int(device), torch.device("cpu")
            self.obs_words = torch.zeros(self.n, dtype=torch.int64)

        def close(self):
            trace.closed += 1

        def __getattr__(self, name):
            if name.startswith("_"):
                raise AttributeError(name)

            def method(*args, **kwargs):
                k = trace.call(name, args, kwargs)
                if name == "bid_round":
                    out = tuple(torch.full((self.n,), (3 * k + j) % 127, dtype=torch.int8) for j in range(3))
                    trace.keep.extend(out)
                    return out
                if name == "state":
                    return np.full((10, self.n), k, np.uint64)
                if name == "counters":
                    return np.zeros(self.n, np.int64), (1000 * k + np.arange(4 * self.n, dtype=np.int32)).reshape(self.n, 4)
                return None
            return method
    return Env


def weights():
    return [torch.zeros((256, 256), dtype=torch.bfloat16), torch.zeros(256), torch.zeros((256, 256), dtype=torch.bfloat16),
            torch.zeros(256), torch.zeros((64, 256), dtype=torch.bfloat16), torch.zeros(64)]


# name -> (function of evaluate, arguments after which n_games and episodes go, keyword arguments, takes inspect)
CASES = {
    "vs_bot": ("evaluate_vs_bot", ("W",), {}, False),
    "vs_bot_greedy_epsilon": ("evaluate_vs_bot", ("W",), dict(temperature=0, epsilon=0.25), False),
    "vs_policy": ("evaluate_vs_policy", ("W", "V"), dict(seed=3), False),
    "play_passes_inspect": ("_play_passes", ("W",), dict(seed=5, mix=2, device=0), True),
    "playout_open": ("evaluate_playout_vs_bot", (4,), {}, False),
    "playout_worlds": ("evaluate_playout_vs_bot", (4,), dict(worlds=3, salt=7), False),
    "playout_voids": ("evaluate_playout_vs_bot", (2,), dict(worlds=3, voids=True), False),
    "playout_hidden_exchange_bidding": ("evaluate_playout_vs_bot", (2,), dict(worlds=3, hidden=True, exchange=4, bidding=(2, 1),
                                                                             pass_value=True, threshold=5), True),
    "playout_net_own": ("evaluate_playout_vs_bot", (None,), dict(worlds=3, net="W", net_seats="own"), False),
    "playout_net_set": ("evaluate_playout_vs_bot", (None,), dict(worlds=2, net="W", net_seats=5), True),
    "exchange": ("evaluate_exchange_vs_bot", (3, 2, 4), dict(salt=1), False),
    "exchange_inspect": ("evaluate_exchange_vs_bot", (3, 2, 4), {}, True),
    "exchangenet_inspect": ("evaluate_exchangenet_vs_bot", ("W",), {}, True),
    "bidding_pass_value_inspect": ("evaluate_bidding_vs_bot", (3, 2), dict(pass_value=True, threshold=2, contracts=0x1F), True),
    "bidnet_inspect": ("evaluate_bidnet_vs_bot", ("W",), dict(playouts_equiv=8, pass_value=True), True),
}


def run_case(EV, name, trace=None):
    """One case on module EV with the stand-in env: (trace, scores [5, EPISODES * N, 4], the inspect list or None).
    duplicate_advantage is replaced by the identity, so that a public function hands back the score array itself."""
    trace = trace or Trace()
    fn, args, kwargs, takes_inspect = CASES[name]
    named = dict(W=weights(), V=weights())
    args = [named.get(a, a) if isinstance(a, str) else a for a in args]
    kwargs = {k: named.get(v, v) if isinstance(v, str) else v for k, v in kwargs.items()}
    record = [] if takes_inspect else None
    if takes_inspect:
        kwargs["inspect"] = record
    saved = EV.TarokVecEnv, EV.duplicate_advantage, torch.cuda.device
    EV.TarokVecEnv, EV.duplicate_advantage, torch.cuda.device = stand_in(trace), (lambda s: s), (lambda d: contextlib.nullcontext())
    try:
        if fn == "_play_passes":
            scores = EV._play_passes(*args, N, EPISODES, kwargs.pop("seed"), kwargs.pop("mix"), kwargs.pop("device"), **kwargs)
        else:
            scores = getattr(EV, fn)(*args, N, EPISODES, **kwargs)
    finally:
        EV.TarokVecEnv, EV.duplicate_advantage, torch.cuda.device = saved
    return trace, scores, record


def describe(record):
    """The inspect dicts in a form JSON holds: scalars as they are, arrays as [dtype, shape] and, where the stand-in
    filled them, their first element (the buffers of torch.empty hold whatever was there)."""
    out = []
    for d in record:
        row = {}
        for key, v in d.items():
            if isinstance(v, np.ndarray):
                row[key] = [str(v.dtype), list(v.shape)] + ([int(v.flat[0])] if key in FILLED else [])
            else:
                row[key] = v
        out.append(row)
    return out


OFFSET = re.compile(r"@(\d+)")


def _split(line):
    return OFFSET.sub("@", line), [int(x) for x in OFFSET.findall(line)]


def _shift(line, steps, r):
    it = iter(steps)
    return OFFSET.sub(lambda m: "@%d" % (int(m.group(1)) + r * next(it)), line)


def pack(calls):
    """Run-length code: a plain line, or [count, block, steps] for `count` repeats of the lines of `block`, repeat r with
    the offsets of line j moved by r * steps[j]."""
    out, i = [], 0
    while i < len(calls):
        best = None
        for period in (1, 2):
            block = [_split(c) for c in calls[i:i + period]]
            nxt = [_split(c) for c in calls[i + period:i + 2 * period]]
            if len(nxt) < period or [b[0] for b in block] != [b[0] for b in nxt]:
                continue
            steps = [[y - x for x, y in zip(b[1], c[1])] for b, c in zip(block, nxt)]
            count = 2
            while [_shift(c, s, count) for c, s in zip(calls[i:i + period], steps)] == calls[i + count * period:i + (count + 1) * period]:
                count += 1
            if best is None or count * period > best[0] * len(best[1]):
                best = [count, calls[i:i + period], steps]
        if best is None:
            out.append(calls[i])
            i += 1
        else:
            out.append(best)
            i += best[0] * len(best[1])
    return out


def unpack(packed):
    calls = []
    for item in packed:
        if isinstance(item, str):
            calls.append(item)
        else:
            count, block, steps = item
            calls.extend(_shift(c, s, r) for r in range(count) for c, s in zip(block, steps))
    return calls


def record_all(EV):
    out = {}
    for name in CASES:
        trace, scores, record = run_case(EV, name)
        assert unpack(pack(trace.calls)) == trace.calls, "not true: unpack(pack(trace.calls)) == trace.calls"
        out[name] = dict(calls=pack(trace.calls), tuples=trace.tuples, inspect=None if record is None else describe(record))
    return out


REFUSALS = [
    (dict(net="W"), "net= plays the determinized player's playouts: give worlds= as well"),
    (dict(net="W", worlds=2, samples=1), "net= runs one playout per (card, world): samples is not taken (pass None)"),
    (dict(net="W", worlds=2, samples=None, voids=True), "net= composes with nothing else yet: no voids, hidden, exchange or bidding"),
    (dict(net="W", worlds=2, samples=None, hidden=True), "net= composes with nothing else yet: no voids, hidden, exchange or bidding"),
    (dict(net="W", worlds=2, samples=None, exchange=2), "net= composes with nothing else yet: no voids, hidden, exchange or bidding"),
    (dict(net="W", worlds=2, samples=None, bidding=(1, 1)), "net= composes with nothing else yet: no voids, hidden, exchange or bidding"),
    (dict(net="W", worlds=2, samples=None, net_seats=16), 'net_seats: a 4-bit seat set, 0..15, or "own"'),
    (dict(net="W", worlds=2, samples=None, net_seats="all"), 'net_seats: a 4-bit seat set, 0..15, or "own"'),
    (dict(voids=True), "voids=True constrains the re-deals: give worlds= as well"),
    (dict(hidden=True), "hidden=True widens the re-deals: give worlds= as well"),
    (dict(hidden=True, voids=True, worlds=2), "hidden=True is not built together with voids=True: give one of the two"),
    (dict(exchange=4), "exchange=D is the fair player's front end: give worlds= as well"),
    (dict(bidding=(2, 1)), "bidding=(W, S) is the fair player's front end: give worlds= as well"),
    (dict(bidding=(2, 1), worlds=2, mix=0), "bidding=(worlds, samples) replaces the Bot's bidding round: it goes with mix=K.MIX_BOT"),
]
