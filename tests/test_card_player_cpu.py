"""The playout card player behind its four doors, pinned on the CPU against the code from BEFORE tarok_amd/playout.py: the
native calls of TarokVecEnv's card methods, what SelfPlay(teacher=...) keeps and launches, the launch sequence of
evaluate_playout_vs_bot, what SelfPlay.evaluate(playout_*=...) hands on, and every refusal — each for the ten player
kinds of KINDS, compared record for record with tests/golden/card_player_calls_v1.json.  Every env method is a deterministic
function of the env's state and its arguments, so the same calls with the same arguments compute the same bytes.

The fixture was recorded from the env.py, selfplay.py and evaluate.py of the commit before the module, loaded beside the
package under other names, never from the code under test:

    mkdir /tmp/parent && for f in env selfplay evaluate; do git show 5509796:tarok_amd/$f.py > /tmp/parent/$f.py; done
    PYTHONPATH=. python tests/test_card_player_cpu.py /tmp/parent > tests/golden/card_player_calls_v1.json

Calls are written as tests/evaluate_calls_cases.py (the evaluation: Trace, stand_in, run_case, pack) and
tests/playout_net_cases.py (everything else: Calls — a tensor is its dtype and shape) write them."""
import contextlib
import importlib.util
import json
import os
import sys

import pytest
import torch

import evaluate_calls_cases as EC
from playout_net_cases import Calls, no_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "card_player_calls_v1.json")
VOIDS, HIDDEN = ("voids", torch.int32), ("hidden", torch.int64)
# name -> (worlds, samples, the kind's words (name, dtype) or None, net, depth)
KINDS = dict(open=(None, 2, None, False, None), det=(3, 2, None, False, None), voids=(3, 2, VOIDS, False, None),
             hidden=(3, 2, HIDDEN, False, None), net_det=(2, 1, None, True, None), net_voids=(2, 1, VOIDS, True, None),
             net_hidden=(2, 1, HIDDEN, True, None), value_det=(2, 1, None, True, 1), value_voids=(2, 1, VOIDS, True, 2),
             value_hidden=(2, 1, HIDDEN, True, 12))


class Rec(Calls):
    """Calls whose lists (six weights) are written element by element."""

    def show(self, x):
        return "[%s]" % ", ".join(self.show(v) for v in x) if isinstance(x, (list, tuple)) else Calls.show(self, x)


def rec_env(history=True):
    return type("Env", (Rec,), dict(n=4, history=history, device=torch.device("cpu"), device_index=0))()


def raised(f):
    """The name of the exception type f() ends with (None: it returned)."""
    try:
        f()
    except Exception as e:                            # noqa: BLE001 -- the type is what is recorded
        return type(e).__name__
    return None


# ---- the env: the native call of every public method of a kind
def env_door(ENV):
    TV, out = ENV.TarokVecEnv, {}

    class Env(TV):
        def __init__(self):
            self.n, self.device, self._h, self.history, self.L, self._net_scratch = 4, torch.device("cpu"), 77, True, Rec(), {}

        def close(self):
            pass

        def _p(self, t):
            return None if t is None else self.L.show(t)

        def _stream(self):
            return "stream"
    for name, (worlds, samples, words, net, depth) in KINDS.items():
        w = [] if words is None else [("tensor", {words[0]: torch.zeros(4, dtype=words[1])}),
                                     ("own", {words[0]: True, "words": torch.zeros(4, dtype=words[1])})]
        fair = [("fair_" + k, "playout_cards_fair", (worlds, samples), kw) for k, kw in w[1:] + [("new", {words[0]: True})]] if words else \
            [("fair", "playout_cards_fair", (worlds, samples), {})] + ([] if worlds else [("fair0", "playout_cards_fair", (0, samples), {})])
        if net:
            head = (EC.weights(), worlds) + (() if depth is None else (depth, 0.5))
            ways = [(k, "playout_cards_net" if depth is None else "playout_cards_net_value", head, dict(kw, net_seats=5)) for k, kw in w or [("plain", {})]]
        elif words:
            given = {"voids": "voids", "hidden": "played"}[words[0]]
            ways = [("tensor", "playout_cards_" + words[0], (worlds, samples), {given: torch.zeros(4, dtype=words[1])}),
                    ("own", "playout_cards_" + words[0], (worlds, samples), {})] + fair
        else:
            ways = [("plain", "playout_cards" if worlds is None else "playout_cards_det", (samples,) if worlds is None else (worlds, samples), {})] + fair
        for way, method, args, kw in ways:
            for sets in (dict(seats=9), dict(seats_per_game=torch.zeros(4, dtype=torch.uint8))):
                for outs in ({}, dict(sum_out=torch.zeros((4, 12, 4), dtype=torch.int32), action_out=torch.zeros(4, dtype=torch.uint8))):
                    env = Env()
                    with no_device():
                        got = getattr(env, method)(*args, salt=3, **kw, **sets, **outs)
                    assert not outs or (got[0] is outs["sum_out"] and got[1] is outs["action_out"])
                    out["%s/%s/%s/%s" % (name, way, "+".join(sets), "given" if outs else "new")] = env.L.calls + [env.L.show(list(got))]
    return out


# ---- the teacher: what SelfPlay keeps of teacher=dict(...) and what _alloc and _teach call
def teacher_of(name, **more):
    worlds, samples, words, net, depth = KINDS[name]
    tc = dict(worlds=worlds or 0, tau=8.0, salt=11, **more)
    if net:
        tc.update(dict(net=True, net_seats=5), **({"net_worlds": words[0]} if words else {}), **({} if depth is None else {"depth": depth}))
    else:
        tc.update(dict(samples=samples), **({words[0]: True} if words else {}))
    return tc


def make_teacher(SP, env, tc, **kw):
    sp = SP.SelfPlay.__new__(SP.SelfPlay)
    try:
        sp.__init__(env, hidden=256, teacher=tc, reward_scale=0.25, **kw)
    except (AttributeError, TypeError):               # (the stand-in is no env: the teacher is read first)
        pass
    return sp


def teacher_door(SP):
    out = {}
    for name in KINDS:
        for seats in (None, torch.zeros(4, dtype=torch.uint8)):
            for every in (1, 2):
                env = rec_env()
                sp = make_teacher(SP, env, teacher_of(name, **({} if every == 1 else dict(every=every))))
                row = dict(teacher=dict(sp.teacher), init=list(env.calls))
                sp.env, sp.device, sp.fused, sp.fused_step, sp._w, sp._seats, sp.reward_scale = env, torch.device("cpu"), True, True, EC.weights(), seats, 0.25
                sp._pool_k, sp._opp = 0, None
                del env.calls[:]
                sp._alloc(3)
                row["alloc"], row["words"] = list(env.calls), None if sp._teach_words is None else env.show(sp._teach_words)
                del env.calls[:]
                if every == 1:
                    sp._teach(1)
                else:
                    sp._rollout_body(2)
                row["calls"] = list(env.calls)
                out["%s/%s/every%d" % (name, "all" if seats is None else "seats", every)] = row
    return out


# ---- the evaluation: evaluate_playout_vs_bot's launch sequence
def evaluation_cases():
    cases = {}
    for name, (worlds, samples, words, net, depth) in KINDS.items():
        kw = {} if worlds is None else dict(worlds=worlds)
        if not net:
            cases[name] = ("evaluate_playout_vs_bot", (samples,), dict(kw, salt=7, **({words[0]: True} if words else {})), False)
            continue
        kw.update(dict(net="W"), **({"net_worlds": words[0]} if words else {}), **({} if depth is None else dict(net_depth=depth, net_value_scale=4.0)))
        for seats in (5, "own"):
            cases["%s_%s" % (name, seats)] = ("evaluate_playout_vs_bot", (None,), dict(kw, net_seats=seats), False)
    return cases


def evaluation_door(EV):
    cases, out = evaluation_cases(), {}
    EC.CASES.update(cases)
    try:
        for name in cases:
            trace = EC.run_case(EV, name)[0]
            assert EC.unpack(EC.pack(trace.calls)) == trace.calls
            out[name] = dict(calls=EC.pack(trace.calls), tuples=trace.tuples, closed=trace.closed)
    finally:
        for name in cases:
            del EC.CASES[name]
    return out


# ---- SelfPlay.evaluate: what it hands to evaluate_vs_bot and evaluate_playout_vs_bot
@contextlib.contextmanager
def recorded_evaluations(rec):
    from tarok_amd import evaluate
    names = ("evaluate_vs_bot", "evaluate_playout_vs_bot", "evaluate_vs_policy", "evaluate_vs_pool")
    saved = [getattr(evaluate, k) for k in names]
    for k in names:
        setattr(evaluate, k, getattr(rec, k))
    try:
        yield
    finally:
        for k, f in zip(names, saved):
            setattr(evaluate, k, f)


def evaluate_of(name, **more):
    worlds, samples, words, net, depth = KINDS[name]
    kw = dict(versus_playout=samples, **({} if worlds is None else dict(playout_worlds=worlds)), **more)
    if net:
        kw.update(dict(playout_net=True, playout_net_seats=5), **({"playout_net_worlds": words[0]} if words else {}),
                  **({} if depth is None else dict(playout_net_depth=depth)))
    elif words:
        kw["playout_" + words[0]] = True
    return kw


def call_evaluate(SP, rec, fused=True, **kw):
    sp = SP.SelfPlay.__new__(SP.SelfPlay)
    sp.fused, sp.fused_learner, sp._w, sp.reward_scale, sp.env = fused, True, EC.weights(), 0.25, rec_env()
    with recorded_evaluations(rec):
        return sp.evaluate(n_games=2, episodes=2, **kw)


def selfplay_evaluate_door(SP):
    out = {}
    for name in KINDS:
        rec = Rec()
        call_evaluate(SP, rec, **evaluate_of(name))
        out[name] = rec.calls
    return out


# ---- the refusals, one case per rule of the three validators before the module (and of the env's dispatchers)
INF, W = float("inf"), "W"
TEACHER_REFUSALS = [
    (dict(samples=1, shuffle=1), {}), (dict(worlds=2), {}), (dict(samples=1, net_seats=3), {}), (dict(net=True, worlds=2, net_worlds="both"), {}),
    (dict(samples=1, worlds=2, net_worlds="voids"), {}), (dict(samples=1, worlds=2, depth=1), {}), (dict(net=True, worlds=2, depth=13), {}),
    (dict(net=True, worlds=2, depth=0), {}), (dict(net=True, worlds=2, depth=True), {}), (dict(net=True, worlds=2, depth=2.0), {}),
    (dict(net=True, worlds=2, depth=1), dict(reward_scale=INF)), (dict(net=True, worlds=2, samples=2), {}), (dict(net=True), {}),
    (dict(net=True, worlds=2, voids=True), {}), (dict(net=True, worlds=2, hidden=True), {}), (dict(net=True, worlds=2, net_seats=16), {}),
    (dict(net=True, worlds=2), dict(hidden=128)), (dict(net=True, worlds=2, net_worlds="voids"), dict(history=False)),
    (dict(net=True, worlds=2, net_worlds="hidden"), dict(history=False)), (dict(samples=1, worlds=65), {}), (dict(samples=0), {}),
    (dict(samples=1025), {}), (dict(samples=1, every=0), {}), (dict(samples=1, tau=-1.0), {}), (dict(samples=1, tau=INF), {}),
    (dict(samples=1, voids=True), {}), (dict(samples=1, worlds=2, voids=True), dict(history=False)), (dict(samples=1, hidden=True), {}),
    (dict(samples=1, worlds=2, hidden=True, voids=True), {}), (dict(samples=1, worlds=2, hidden=True), dict(history=False)),
    (None, dict(distill_coef=0.5)),
]
EVALUATION_REFUSALS = [dict(kw) for kw, _ in EC.REFUSALS] + [
    dict(worlds=2, net_depth=1), dict(net=W, worlds=2, samples=None, net_depth=0), dict(net=W, worlds=2, samples=None, net_depth=13),
    dict(net=W, worlds=2, samples=None, net_depth=1.0), dict(net=W, worlds=2, samples=None, net_depth=True),
    dict(net=W, worlds=2, samples=None, net_depth=1, net_value_scale=0.0), dict(net=W, worlds=2, samples=None, net_depth=1, net_value_scale=INF),
    dict(net=W, worlds=2, samples=None, net_worlds="both"), dict(worlds=2, net_worlds="voids"),
]
SELFPLAY_EVALUATE_REFUSALS = [
    dict(versus_playout=1, playout_worlds=2, playout_net_depth=1), dict(versus_playout=1, playout_worlds=2, playout_net=True, playout_net_depth=0),
    dict(versus_playout=1, playout_worlds=2, playout_net=True, playout_net_depth=13), dict(versus_playout=1, playout_worlds=2, playout_net=True, playout_net_worlds="both"),
    dict(versus_playout=1, playout_worlds=2, playout_net_worlds="voids"), dict(versus_playout=1, playout_net=True),
    dict(versus_playout=1, playout_worlds=2, playout_net=True, playout_voids=True), dict(versus_playout=1, playout_worlds=2, playout_net=True, playout_hidden=True),
    dict(versus_playout=1, playout_worlds=2, playout_net=True, playout_exchange=2), dict(versus_playout=1, playout_worlds=2, playout_net=True, playout_bidding=(2, 1)),
    dict(versus_playout=2, playout_worlds=2, playout_net=True), dict(versus_playout=2, playout_bidding=(2, 1)), dict(versus_playout=2, playout_exchange=4),
    dict(playout_worlds=2), dict(versus_playout=2, playout_voids=True), dict(versus_playout=2, playout_hidden=True),
    dict(versus_playout=2, playout_worlds=2, playout_hidden=True, playout_voids=True), dict(versus_playout=2, opponent=W),
    dict(greedy=True, temperature=0.5), dict(fused=False),
]
ENV_REFUSALS = [("playout_cards_fair", (3, 2), dict(voids=True, hidden=True), True), ("playout_cards_net", (W, 2), dict(voids=True, hidden=True), True),
                ("playout_cards_net", (W, 2), dict(voids=True), False), ("playout_cards_net", (W, 2), dict(hidden=True), False),
                ("playout_cards_net", (W, 2), dict(net_seats=16), True), ("playout_cards_voids", (3, 2), {}, False),
                ("playout_cards_hidden", (3, 2), {}, False), ("playout_cards_net_value", (W, 2, 0), {}, True),
                ("playout_cards_net_value", (W, 2, 13), {}, True), ("playout_cards_net_value", (W, 2, True), {}, True),
                ("playout_cards_net_value", (W, 2, 1.5), {}, True), ("playout_cards_net_value", (W, 2, 1, 0.0), {}, True),
                ("playout_cards_net_value", (W, 2, 1, INF), {}, True), ("playout_cards_net_value", (W, 2, 1, float("nan")), {}, True)]


def named(kw):
    return {k: EC.weights() if v == W else v for k, v in kw.items()}


def refusals(ENV, SP, EV):
    """Per door a list of [the case, the exception type, nothing was called and nothing closed]."""
    out = dict(teacher=[], evaluation=[], selfplay_evaluate=[], env=[])
    for tc, kw in TEACHER_REFUSALS:
        kw, env = dict(kw), rec_env(kw.get("history", True))
        kw.pop("history", None)
        hidden = kw.pop("hidden", 256)
        sp = SP.SelfPlay.__new__(SP.SelfPlay)
        out["teacher"].append([repr((tc, kw)), raised(lambda: sp.__init__(env, hidden=hidden, teacher=tc, **kw)), env.calls == []])
    for kw in EVALUATION_REFUSALS:
        for public in (False, True):
            trace, kw_ = EC.Trace(), named(kw)
            samples, mix = kw_.pop("samples", 2), kw_.pop("mix", 2)
            saved, EV.TarokVecEnv = EV.TarokVecEnv, EC.stand_in(trace)
            try:
                how = raised((lambda: EV.evaluate_playout_vs_bot(samples, EC.N, EC.EPISODES, mix=mix, **kw_)) if public else
                             (lambda: EV._playout_passes(samples, EC.N, EC.EPISODES, 0, mix, 0, **kw_)))
            finally:
                EV.TarokVecEnv = saved
            out["evaluation"].append([repr(kw), public, how, trace.calls == [] and trace.closed == 0])
    for kw in SELFPLAY_EVALUATE_REFUSALS:
        rec = Rec()
        out["selfplay_evaluate"].append([repr(kw), raised(lambda: call_evaluate(SP, rec, **named(kw))), rec.calls == []])
    for method, args, kw, history in ENV_REFUSALS:
        env = type("Env", (ENV.TarokVecEnv,), dict(__init__=lambda self: None, close=lambda self: None, n=4, _h=77, history=history,
                                                   device=torch.device("cpu"), L=Rec(), _net_scratch={}))()
        args = [EC.weights() if a == W else a for a in args]
        out["env"].append([method, repr((args[1:] if method.startswith("playout_cards_net") else args, kw, history)),
                           raised(lambda: getattr(env, method)(*args, **kw)), env.L.calls == []])
    return out


def record_all(ENV, SP, EV):
    return json.loads(json.dumps(dict(env=env_door(ENV), teacher=teacher_door(SP), evaluation=evaluation_door(EV),
                                      selfplay_evaluate=selfplay_evaluate_door(SP), refusals=refusals(ENV, SP, EV))))


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def got():
    from tarok_amd import env, evaluate, selfplay
    return record_all(env, selfplay, evaluate)


def test_the_fixture_holds_every_kind_at_every_door(golden):
    assert {k.split("/")[0] for k in golden["env"]} == {k.split("/")[0] for k in golden["teacher"]} == set(golden["selfplay_evaluate"]) == set(KINDS)
    assert set(golden["evaluation"]) == set(evaluation_cases()) and len(golden["evaluation"]) == 4 + 2 * 6
    assert len(golden["env"]) >= 4 * len(KINDS) and len(golden["teacher"]) == 4 * len(KINDS)
    for door, rows in golden["refusals"].items():
        assert rows and all(r[-2] in ("ValueError", "RuntimeError") and r[-1] is True for r in rows), door
    assert [r[-2] for r in golden["refusals"]["selfplay_evaluate"]].count("RuntimeError") == 1
    for name, g in golden["evaluation"].items():
        assert 400 < len(EC.unpack(g["calls"])) < 2500 and g["closed"] == 1, name


@pytest.mark.parametrize("door", ["env", "teacher", "selfplay_evaluate"])
def test_the_doors_calls_are_those_of_the_fixture(got, golden, door):
    assert sorted(got[door]) == sorted(golden[door])
    for key, want in golden[door].items():
        assert got[door][key] == want, "%s: %s differs" % (door, key)


@pytest.mark.parametrize("name", sorted(evaluation_cases()))
def test_the_evaluations_calls_are_those_of_the_fixture(got, golden, name):
    have, want = EC.unpack(got["evaluation"][name]["calls"]), EC.unpack(golden["evaluation"][name]["calls"])
    for i, (a, b) in enumerate(zip(have, want)):
        assert a == b, "%s: call %d differs" % (name, i)
    assert len(have) == len(want)
    assert got["evaluation"][name]["tuples"] == golden["evaluation"][name]["tuples"] and got["evaluation"][name]["closed"] == 1


@pytest.mark.parametrize("door", ["teacher", "evaluation", "selfplay_evaluate", "env"])
def test_the_refusals_are_those_of_the_fixture(got, golden, door):
    assert len(got["refusals"][door]) == len(golden["refusals"][door])
    for have, want in zip(got["refusals"][door], golden["refusals"][door]):
        assert have == want, "%s: %s" % (door, want[0])


if __name__ == "__main__":
    # record the fixture from the three files in the directory given (the parent commit's), loaded beside the package's own modules
    sys.path.insert(0, ROOT)
    mods = []
    for name in ("env", "selfplay", "evaluate"):
        spec = importlib.util.spec_from_file_location("tarok_amd.%s_recorded" % name, os.path.join(sys.argv[1], name + ".py"))
        mods.append(importlib.util.module_from_spec(spec))
        spec.loader.exec_module(mods[-1])
    tight = lambda x: json.dumps(x, separators=(",", ":"))
    doors = []
    for door, rows in record_all(*mods).items():                      # one line per key or refusal
        body = ",\n".join("%s:%s" % (tight(k), tight(v)) for k, v in rows.items()) if door != "refusals" else \
            ",\n".join("%s:[\n%s]" % (tight(k), ",\n".join(tight(r) for r in v)) for k, v in rows.items())
        doors.append("%s:{\n%s}" % (tight(door), body))
    sys.stdout.write("{%s}\n" % ",\n".join(doors))
