"""CPU-side checks of the value-bootstrapped net playouts (tarok_playout_cards_net_value): the model of
tests/playout_net_value_model.py against the models it extends (depth 12), its stop rule at depth 1, the mutants it must
tell apart on the GPU tests' own positions, the guards against a vacuous GPU comparison on the model alone, every new
ValueError, the launches the Python surface issues on stand-in envs, and the C entry point's argument checks, which come
before any HIP call.  The plan of the GPU comparison (positions, weight sets, seat sets, depths) is
tests/playout_net_value_cases.py's, shared with tests/test_gpu_playout_net_value.py.  No GPU in here."""
import ctypes
import inspect

import numpy as np
import pytest

import playout_net_model as NM
import playout_net_value_model as VM
import playout_net_worlds_model as WM
from oracle import tarok_spec as S
from playout_net_cases import Calls, NoHistory, WithHistory, no_device, weights, zero_net
from playout_net_value_cases import CASES, EPISODE, OFFSET, SALT, SCALES, SEED, model, plan, weight_sets


def logits(k):
    v = np.arange(54, dtype=np.float64) / 64
    W = zero_net(v[::-1].copy() if k else v)
    return W


@pytest.mark.parametrize("kind", VM.KINDS)
@pytest.mark.parametrize("cards", [0, 9, 24, 40, 44])
def test_depth_12_is_the_existing_model(kind, cards):
    """depth = 12 never stops an item: the sums and cards of playout_net_model / playout_net_worlds_model, for any scale."""
    games, words, _ = WM.bot_games("voids" if kind == "det" else kind, SEED, EPISODE, S.MIX_ALL, 5, cards, first=OFFSET)
    W = logits(cards & 1)
    if kind == "det":
        want_sum, want_act = NM.playout_cards(games, SEED, SALT, 15, 3, W, 15)
    else:
        want_sum, want_act = WM.playout_cards(kind, games, SEED, SALT, 15, 3, W, 15, words)
    got_sum, got_act, info = VM.playout_cards(kind, games, SEED, SALT, 15, 3, W, 15, 12, 1e9, None if kind == "det" else words)
    assert (cards == 44 or want_sum.any()) and (got_sum == want_sum).all() and (got_act == want_act).all()
    assert not any(d["stopped"] for _, d in info)


def test_depth_1_stops_at_the_viewers_next_decision():
    """At 44 cards the candidate is the viewer's last card: no item stops.  At 40 cards every unfinished item stops.  And
    from any position an item is live for at most 7 card rounds (6 cards and the stop round), as the header states."""
    W = weight_sets()["P"]
    for cards, kind in ((44, "det"), (40, "det"), (0, "det"), (9, "voids"), (24, "hidden"), (5, "det")):
        games, words, _ = WM.bot_games("voids" if kind == "det" else kind, SEED, EPISODE, S.MIX_ALL, 5, cards, first=OFFSET)
        _, _, info = VM.playout_cards(kind, games, SEED, SALT, 15, 2, W, 15, 1, 1.0, None if kind == "det" else words)
        assert info
        live = [d for _, d in info if d["rounds"]]
        assert max([d["rounds"] for d in live], default=0) <= 7, cards
        if cards == 44:
            assert not any(d["stopped"] for _, d in info)
        elif cards == 40:                             # (from earlier positions a Berac or a Klop may end inside the six cards)
            assert live and all(d["stopped"] for d in live), cards
        if cards == 0:
            assert max(d["rounds"] for d in live) == 7            # the bound is reached


def test_points_follows_the_float32_steps():
    P = VM.points
    assert [P(v, 1.0) for v in (0.5, 1.5, 2.5, -0.5, -2.5, 3.49, float("nan"), float("inf"), -float("inf"))] == [0, 2, 2, 0, -2, 3, 0, 32767, -32767]
    assert [P(v, 1.0, half_even=False) for v in (0.5, 1.5, 2.5, -0.5, -2.5)] == [1, 2, 3, -1, -3]
    assert P(3.0, 0.5) == 2 and P(5.0, 0.5) == 2 and P(1e-3, 1e9) == 32767 and P(-1e-3, 1e9) == -32767 and P(0.0, 1e9) == 0
    assert P(40000.0, 1.0) == 32767 and P(3e38, 1e9) == 32767          # (the float32 product overflows to inf first)


def run_plan(cases):
    """The model alone over `cases` at the plan's launches: (tags seen, games whose depth-limited card differs from the
    depth-12 card)."""
    sets = weight_sets()
    tags, moved = set(), 0
    for kind, at in cases:
        for n, worlds, depth, name, choice in plan(kind, at):
            games, words, net_seats, sums, acts, info = model(kind, at, n, worlds, depth, sets[name], choice)
            for scale in SCALES:
                tags |= VM.seen([(w, dict(d, V=VM.points(d["v"], scale) if d["stopped"] else None)) for w, d in info], scale)
            _, full, _ = VM.playout_cards(kind, games, SEED, SALT, 15, worlds, sets[name], net_seats, 12, 1.0, words)
            moved += int((acts != full).sum())
    return tags, moved


GUARD_CASES = [("det", 0), ("det", 2), ("voids", 1)]           # enough for every tag, on the model alone


def test_the_plan_is_not_vacuous_on_the_model_alone():
    """Over a part of the GPU comparison's plan the model has seen stopped and finished items in one launch, positive,
    negative and differing V, a tie that half-even and half-away round differently, a clamped value, and a game whose
    chosen card differs from the depth-12 card."""
    tags, moved = run_plan(GUARD_CASES)
    assert tags >= {"mixed", "signs", "tie", "clamped"}, tags
    assert moved >= 1
    seen_depths = {(d, s, c) for k, a in CASES for _, _, d, s, c in plan(k, a)}
    assert {d for d, _, _ in seen_depths} == {1, 2, 3} and {s for _, s, _ in seen_depths} == {"R", "P", "V"}
    assert {c for _, _, c in seen_depths} == {15, 0, "no viewer"}


@pytest.mark.parametrize("rule", [r for r in VM.RULES if r != "spec"])
def test_the_model_tells_the_mutants_apart(rule):
    """On the GPU tests' own positions the statement and each mutant give different sums (at the scale where the mutant
    can show: 0.5 makes ties for "away")."""
    sets = weight_sets()
    differ = 0
    for kind, at in GUARD_CASES:
        n, worlds, depth, name, choice = plan(kind, at)[0]
        scale = 0.5 if rule == "away" else 1.0
        _, _, _, want, _, _ = model(kind, at, n, worlds, depth, sets[name], choice, scale)
        _, _, _, got, _, _ = model(kind, at, n, worlds, depth, sets[name], choice, scale, rule=rule)
        differ += int((got != want).any(axis=(1, 2)).sum())
    assert differ >= 1, rule


def test_new_refusals_and_defaults():
    """Every new ValueError, before any env is made or touched, and the new keywords' defaults."""
    from tarok_amd import _native, evaluate as EV, karte as K, selfplay as SP
    from tarok_amd.env import TarokVecEnv
    assert "tarok_playout_cards_net_value" in _native.SYMBOLS and K.PLAYOUT_MAX_DEPTH == 12
    sig = inspect.signature(TarokVecEnv.playout_cards_net_value).parameters
    assert list(sig)[1:5] == ["weights", "worlds", "depth", "value_scale"] and sig["value_scale"].default == 70.0
    assert inspect.signature(EV.evaluate_playout_vs_bot).parameters["net_depth"].default is None
    assert inspect.signature(EV.evaluate_playout_vs_bot).parameters["net_value_scale"].default == 70.0
    assert inspect.signature(SP.SelfPlay.evaluate).parameters["playout_net_depth"].default is None
    net = weights()
    for depth, scale in ((0, 70.0), (13, 70.0), (-1, 70.0), (1.5, 70.0), (True, 70.0), (1, 0.0), (1, -1.0), (1, float("inf")), (1, float("nan"))):
        with pytest.raises(ValueError):
            TarokVecEnv.playout_cards_net_value(WithHistory(), net, 2, depth, scale)
    for kw in (dict(worlds=2, net_depth=1), dict(net=net, worlds=2, net_depth=0), dict(net=net, worlds=2, net_depth=13),
               dict(net=net, worlds=2, net_depth=1.0), dict(net=net, worlds=2, net_depth=1, net_value_scale=0.0),
               dict(net=net, worlds=2, net_depth=1, net_value_scale=float("inf"))):
        with pytest.raises(ValueError):
            EV.evaluate_playout_vs_bot(None if "net" in kw else 2, 8, 1, **kw)
    for tc in (dict(worlds=2, samples=1, depth=1), dict(net=True, worlds=2, depth=0), dict(net=True, worlds=2, depth=13),
               dict(net=True, worlds=2, depth=2.0)):
        with pytest.raises(ValueError):
            SP.SelfPlay(WithHistory(), hidden=256, teacher=tc)
    for kw in (dict(playout_worlds=2, versus_playout=1, playout_net_depth=1), dict(playout_net=True, playout_worlds=2, playout_net_depth=0),
               dict(playout_net=True, playout_worlds=2, playout_net_depth=13)):
        with pytest.raises(ValueError):
            SP.SelfPlay.evaluate(object(), **kw)


def test_the_env_method_issues_the_value_launch():
    """TarokVecEnv.playout_cards_net_value on a stand-in env: depth=None issues playout_cards_net's calls; an integer depth
    issues tarok_playout_cards_net_value with the kind as a number, the words (or None) before net_seats, and depth and
    value_scale after it — after the words launch where the env's own words are asked for."""
    import torch
    from tarok_amd.env import TarokVecEnv

    class Env:
        n, device, _h = 4, torch.device("cpu"), 77
        check_mlp_weights = staticmethod(TarokVecEnv.check_mlp_weights)
        shown_voids, played_cards, _dev = TarokVecEnv.shown_voids, TarokVecEnv.played_cards, TarokVecEnv._dev
        _cards, _empty = TarokVecEnv._cards, TarokVecEnv._empty          # the one dispatcher under the public methods, its outputs

        def __init__(self, history):
            self.L, self.history, self.scratch = Calls(), history, torch.zeros(4 * 12 * 2 * 48, dtype=torch.uint8)

        def playout_net_scratch(self, worlds):
            return self.scratch

        def _p(self, t):
            return None if t is None else "%s%s" % (str(t.dtype).replace("torch.", ""), list(t.shape))

        def _seat_sets(self, s):
            return s

        def _stream(self):
            return "stream"
    net = weights()
    w = "'bfloat16[256, 256]', 'float32[256]', 'bfloat16[256, 256]', 'float32[256]', 'bfloat16[64, 256]', 'float32[64]'"
    tail = "%s, 'uint8[4608]', 4608, 'int32[4, 12, 4]', 'uint8[4]', 'stream')" % w
    with no_device():
        old, new = Env(False), Env(False)
        TarokVecEnv.playout_cards_net(old, net, 2, net_seats=5, salt=3, seats=9)
        TarokVecEnv.playout_cards_net_value(new, net, 2, None, net_seats=5, salt=3, seats=9)
        assert new.L.calls == old.L.calls == ["tarok_playout_cards_net(77, 2, 3, 9, None, 5, " + tail]
        env = Env(False)
        TarokVecEnv.playout_cards_net_value(env, net, 2, 3, 0.5, net_seats=5, salt=3, seats=9)
        assert env.L.calls == ["tarok_playout_cards_net_value(77, 2, 3, 9, None, 0, None, 5, 3, 0.5, " + tail], env.L.calls
        for kind, num, words_fn, dtype in (("voids", 1, "tarok_shown_voids", torch.int32), ("hidden", 2, "tarok_played_cards", torch.int64)):
            name = str(dtype).replace("torch.", "") + "[4]"
            env = Env(True)
            TarokVecEnv.playout_cards_net_value(env, net, 2, 1, net_seats=5, salt=3, seats=9, words=torch.zeros(4, dtype=dtype), **{kind: True})
            assert env.L.calls == ["%s(77, '%s', 'stream')" % (words_fn, name),
                                   "tarok_playout_cards_net_value(77, 2, 3, 9, None, %d, '%s', 5, 1, 70.0, %s" % (num, name, tail)], env.L.calls
            env = Env(False)
            TarokVecEnv.playout_cards_net_value(env, net, 2, 12, 2.0, net_seats=5, salt=3, seats=9, **{kind: torch.zeros(4, dtype=dtype)})
            assert env.L.calls == ["tarok_playout_cards_net_value(77, 2, 3, 9, None, %d, '%s', 5, 12, 2.0, %s" % (num, name, tail)], env.L.calls


def test_evaluate_issues_the_value_launch():
    """evaluate_playout_vs_bot(net=, net_depth=) on the stand-in env of tests/evaluate_calls_cases.py: None makes the
    calls of the call without it; a depth makes the same calls with playout_cards_net_value(W, worlds, depth, scale, ...) in
    playout_cards_net's place, in the worlds of net_worlds."""
    import evaluate_calls_cases as EC
    from tarok_amd import evaluate as EV
    new = dict(nd_none=("evaluate_playout_vs_bot", (None,), dict(worlds=2, net="W", net_seats=5), False),
               nd_off=("evaluate_playout_vs_bot", (None,), dict(worlds=2, net="W", net_seats=5, net_depth=None, net_value_scale=3.0), False),
               nd_det=("evaluate_playout_vs_bot", (None,), dict(worlds=2, net="W", net_seats=5, net_depth=2, net_value_scale=35.0), False),
               nd_voids=("evaluate_playout_vs_bot", (None,), dict(worlds=2, net="W", net_seats=5, net_worlds="voids", net_depth=1), False),
               nv_voids=("evaluate_playout_vs_bot", (None,), dict(worlds=2, net="W", net_seats=5, net_worlds="voids"), False))
    EC.CASES.update(new)
    try:
        traces = {k: EC.run_case(EV, k)[0].calls for k in new}
    finally:
        for k in new:
            del EC.CASES[k]
    assert traces["nd_off"] == traces["nd_none"]
    for deep, plain, args in (("nd_det", "nd_none", "2, 35.0"), ("nd_voids", "nv_voids", "1, 70.0")):
        assert len(traces[deep]) == len(traces[plain])
        launches = 0
        for a, b in zip(traces[deep], traces[plain]):
            if b.startswith("playout_cards_net("):
                launches += 1
                head, rest = b.split(", 2, ", 1)                  # playout_cards_net(<weights>, 2, <keywords>)
                assert a == head.replace("playout_cards_net(", "playout_cards_net_value(") + ", 2, " + args + ", " + rest, (a, b)
            else:
                assert a == b
        assert launches >= 5 * EC.EPISODES


def test_the_teacher_issues_the_value_launch():
    """SelfPlay's teacher with depth=D on a stand-in: the normalised teacher keeps the key only where it was given, and a
    lock-step's teacher is playout_cards_net_value at (worlds, D, 1 / reward_scale) on the live weights, then
    playout_targets as before."""
    import torch
    from tarok_amd import selfplay as SP

    class Env(Calls):
        n, history = 4, True
    for depth in (None, 2):
        tc = dict(net=True, worlds=2, tau=8.0, salt=11, net_worlds="voids")
        if depth is not None:
            tc["depth"] = depth
        sp = SP.SelfPlay.__new__(SP.SelfPlay)
        try:
            sp.__init__(WithHistory(), hidden=256, teacher=tc, reward_scale=0.25)
        except (AttributeError, TypeError):                      # (the stand-in is no env: the teacher is read first)
            pass
        assert sp.teacher.get("depth") == depth and ("depth" in sp.teacher) == (depth is not None)
        sp.env, sp.device, sp.fused, sp._w, sp._seats, sp.reward_scale = Env(), torch.device("cpu"), True, weights(), None, 0.25
        sp._alloc(3)
        del sp.env.calls[:]
        sp._teach(1)
        assert len(sp.env.calls) == 2 and sp.env.calls[1].startswith("playout_targets(int32[4, 12, 4], int64[4], 2, 8.0,")
        kw = "action_out=uint8[4], net_seats=15, salt=11, seats_per_game=None, sum_out=int32[4, 12, 4], voids=True, words=int32[4])"
        if depth is None:
            assert sp.env.calls[0].startswith("playout_cards_net(") and sp.env.calls[0].endswith("], 2, " + kw), sp.env.calls[0][-200:]
        else:
            assert sp.env.calls[0].startswith("playout_cards_net_value(") and sp.env.calls[0].endswith("], 2, 2, 4.0, " + kw), sp.env.calls[0][-200:]


@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401  -- before the dlopen: one HIP runtime
    import tarok_amd
    from tarok_amd import _native
    tarok_amd.build()
    return _native.lib()


def test_the_entry_point_validates_before_any_hip_call(L):
    """Every refusal comes before the first HIP call: a zeroed stand-in for an env (no GPU, no tarok_create) is enough."""
    z = ctypes.c_void_p(0)
    env = ctypes.cast(ctypes.create_string_buffer(1 << 16), ctypes.c_void_p)
    buf = ctypes.create_string_buffer(512)
    out = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    f = L.tarok_playout_cards_net_value
    for kind in (0, 1, 2):
        ok = dict(env=env, worlds=4, seats=15, kind=kind, words=z if kind == 0 else out, net=15, depth=1, scale=70.0, w=[out] * 6, scr=out,
                  size=0, sum=out, act=out)

        def rc(**ch):
            a = dict(ok, **ch)
            return f(a["env"], a["worlds"], 0, a["seats"], z, a["kind"], a["words"], a["net"], a["depth"], a["scale"], *a["w"], a["scr"],
                     a["size"], a["sum"], a["act"], z)
        bad = [dict(env=None), dict(worlds=0), dict(worlds=65), dict(worlds=-2), dict(seats=16), dict(seats=-1), dict(net=16), dict(net=-1),
               dict(scr=z), dict(scr=ctypes.c_void_p(out.value + 8)), dict(size=-1), dict(sum=z, act=z),
               dict(words=out if kind == 0 else z), dict(kind=3, words=out), dict(kind=-1, words=z), dict(depth=0), dict(depth=13), dict(depth=-1),
               dict(scale=0.0), dict(scale=-1.0), dict(scale=float("inf")), dict(scale=float("nan"))]
        bad += [dict(w=[out] * i + [z] + [out] * (5 - i)) for i in range(6)]
        for ch in bad:
            assert rc(**ch) == -1, (kind, ch)
