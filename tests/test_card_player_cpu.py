"""The playout card player behind its four doors, pinned on the CPU against the code from BEFORE tarok_amd/playout.py: the
native calls of TarokVecEnv's card methods, what SelfPlay(teacher=...) keeps and launches, the launch sequence of
evaluate_playout_vs_bot, what SelfPlay.evaluate(playout_*=...) hands on, and every refusal — each for the ten player
kinds of KINDS, compared record for record with tests/golden/card_player_calls_v1.json.  Every env method is a deterministic
function of the env's state and its arguments, so the same calls with the same arguments compute the same bytes.

The fixture was recorded from the env.py, selfplay.py and evaluate.py of the commit before the module, loaded beside the
package under other names, never from the code under test:

    mkdir /tmp/parent && for f in env selfplay evaluate; do git show 5509796:tarok_amd/$f.py > /tmp/parent/$f.py; done
    PYTHONPATH=. python tests/test_card_player_cpu.py /tmp/parent > tests/golden/card_player_calls_v1.json

The kinds added since — halving, net_halving, versus, versus with halving and sampled: the thirteen of KINDS_V2 — are pinned
the same way at the same doors by tests/golden/card_player_calls_v2.json, recorded from the commit before the five player
classes became the one CardPlayer and the env's net card methods got their one launcher.  That commit's env.py, selfplay.py
and evaluate.py import its own playout.py, so the whole of its tarok_amd/*.py is loaded as a package under another name (a
scratch copy: nothing of it is committed, nothing under tarok_amd/ reads it):

    mkdir -p /tmp/parent/tarok_parent
    for f in $(git ls-tree --name-only 2494921 tarok_amd/ | grep '[.]py$'); do git show 2494921:$f > /tmp/parent/tarok_parent/$(basename $f); done
    PYTHONPATH=. python tests/test_card_player_cpu.py v2 /tmp/parent/tarok_parent > tests/golden/card_player_calls_v2.json

v2 also holds the scratch-size calls of the net-played launches, a halving schedule as the host array it is passed as, a
sampled teacher's teacher_modes() and launches under two play modes of the env (the opponent's mode, left open, is bound
late to env.play_mode), and one refusal per rule of card_player() that names halving, net_halving, net_versus or
net_sampled, in each door's spelling, with the env methods', the teacher's and evaluate's own rules of those options.

Calls are written as tests/evaluate_calls_cases.py (the evaluation: Trace, stand_in, run_case, pack) and
tests/playout_net_cases.py (everything else: Calls — a tensor is its dtype and shape) write them."""
import contextlib
import ctypes
import importlib
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
    """Calls whose lists (six weights) are written element by element, a host array (a halving schedule) as c_int[...]."""

    def show(self, x):
        if isinstance(x, ctypes.Array):
            return "c_int%s" % list(x)
        return "[%s]" % ", ".join(self.show(v) for v in x) if isinstance(x, (list, tuple)) else Calls.show(self, x)


def rec_env(history=True, **more):
    return type("Env", (Rec,), dict(n=4, history=history, device=torch.device("cpu"), device_index=0, **more))()


def raised(f):
    """The name of the exception type f() ends with (None: it returned)."""
    try:
        f()
    except Exception as e:                            # noqa: BLE001 -- the type is what is recorded
        return type(e).__name__
    return None


# ---- the env: the native call of every public method of a kind
def door_env(TV):
    """TarokVecEnv with a recorder in its library's place: a pointer is the tensor's dtype and shape."""
    class Env(TV):
        def __init__(self):
            self.n, self.device, self._h, self.history, self.L, self._net_scratch = 4, torch.device("cpu"), 77, True, Rec(), {}

        def close(self):
            pass

        def _p(self, t):
            return None if t is None else self.L.show(t)

        def _stream(self):
            return "stream"
    return Env


def crossed(Env, out, name, way, method, args, kw, counts=False):
    """One way into a method, crossed with seats= / seats_per_game= and outputs given / new: the native calls and what came back."""
    for sets in (dict(seats=9), dict(seats_per_game=torch.zeros(4, dtype=torch.uint8))):
        given = dict(sum_out=torch.zeros((4, 12, 4), dtype=torch.int32), action_out=torch.zeros(4, dtype=torch.uint8),
                     **(dict(count_out=torch.zeros((4, 12), dtype=torch.int32)) if counts else {}))
        for outs in ({}, given):
            env = Env()
            with no_device():
                got = getattr(env, method)(*args, salt=3, **kw, **sets, **outs)
            assert not outs or (got[0] is outs["sum_out"] and got[-1] is outs["action_out"] and (not counts or got[1] is outs["count_out"]))
            out["%s/%s/%s/%s" % (name, way, "+".join(sets), "given" if outs else "new")] = env.L.calls + [env.L.show(list(got))]


def env_door(ENV):
    Env, out = door_env(ENV.TarokVecEnv), {}
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
            crossed(Env, out, name, way, method, args, kw)
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


def evaluation_door(EV, cases=None):
    cases, out = evaluation_cases() if cases is None else cases, {}
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
def recorded_evaluations(rec, package="tarok_amd"):
    evaluate = importlib.import_module(package + ".evaluate")      # (the module SelfPlay.evaluate's `from .evaluate import` finds)
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
    with recorded_evaluations(rec, SP.__package__):
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


# ---- v2: the kinds added after the module, at the same doors
FIXTURE_V2 = os.path.join(ROOT, "tests", "golden", "card_player_calls_v2.json")


def kind2(launch, words=None, worlds=None, samples=1, schedule=None, depth=None, roles=None, opponent=True, modes=None):
    """launch: the env method's family; words: the kind's (name, dtype) or None; schedule: the worlds of every round of a
    halving launch; roles: (own_rel, opp_rel) of a two-network launch, opponent: whether its six tensors are given; modes:
    the play-mode keys of a sampled launch as the doors spell them."""
    return dict(launch=launch, words=words, worlds=worlds, samples=samples, schedule=schedule, depth=depth, roles=roles,
                opponent=opponent and roles is not None, modes=modes)


KINDS_V2 = dict(
    halving_det=kind2("halving", samples=2, schedule=(1, 2)), halving_voids=kind2("halving", VOIDS, samples=2, schedule=(1, 2)),
    halving_hidden=kind2("halving", HIDDEN, samples=2, schedule=(1, 2)),
    net_halving_det=kind2("net_halving", schedule=(1, 2)), net_halving_hidden=kind2("net_halving", HIDDEN, schedule=(1, 2), depth=2),
    versus_det=kind2("versus", worlds=2, roles=(1, 14)), versus_voids=kind2("versus", VOIDS, worlds=2, roles=(3, 8), depth=2),
    versus_alone=kind2("versus", worlds=2, roles=(15, 0), opponent=False),
    versus_halving_hidden=kind2("versus", HIDDEN, schedule=(1, 2), roles=(1, 14)),
    sampled_det=kind2("sampled", worlds=2, samples=2, modes=dict(temperature=0.5, epsilon=0.25)),
    sampled_hidden=kind2("sampled", HIDDEN, worlds=2, samples=2, depth=2, modes=dict(temperature=0.0)),
    sampled_versus_given=kind2("sampled", HIDDEN, worlds=2, samples=2, roles=(1, 14),
                               modes=dict(temperature=0.5, epsilon=0.25, opp_temperature=2.0, opp_epsilon=0.5)),
    sampled_versus_open=kind2("sampled", worlds=2, samples=3, roles=(1, 14), modes=dict(temperature=0.5)))
FAMILIES_V2 = ("halving", "net_halving", "versus", "versus_halving", "sampled")
PLAY_MODES = ((1.0, 0.0), (0.0, 0.5))                 # two play modes of the env a teacher's open opponent mode binds to


def family(key):
    """The family of a v2 key: its longest prefix among FAMILIES_V2."""
    return max((f for f in FAMILIES_V2 if key.startswith(f + "_")), key=len)


def env_door_v2(ENV):
    Env, out = door_env(ENV.TarokVecEnv), {}
    for name, k in KINDS_V2.items():
        words, schedule = k["words"], k["schedule"]
        ways = [("plain", {})] if words is None else [("tensor", {words[0]: torch.zeros(4, dtype=words[1])}), ("new", {words[0]: True}),
                                                      ("own", {words[0]: True, "words": torch.zeros(4, dtype=words[1])})]
        value = {} if k["depth"] is None else dict(depth=k["depth"], value_scale=0.5)
        nets = (EC.weights(), EC.weights() if k["opponent"] else None)
        for way, kw in ways:
            if k["launch"] == "halving":
                crossed(Env, out, name, way, "playout_cards_halving", (schedule, k["samples"]), kw, counts=True)
            elif k["launch"] == "net_halving":
                crossed(Env, out, name, way, "playout_cards_net_halving", (nets[0], schedule, 5), dict(kw, **value), counts=True)
            elif k["launch"] == "sampled":
                crossed(Env, out, name, way, "playout_cards_net_sampled", nets + (k["worlds"], k["samples"]) + (k["roles"] or ()),
                        dict(kw, **value, **k["modes"]))
            elif schedule is None:
                crossed(Env, out, name, way, "playout_cards_net_versus", nets + (k["worlds"],) + k["roles"], dict(kw, **value))
            else:                                     # worlds None, and worlds the schedule's sum
                crossed(Env, out, name, way, "playout_cards_net_versus", nets + (None,) + k["roles"], dict(kw, halving=schedule, **value), counts=True)
                crossed(Env, out, name, way + "_sum", "playout_cards_net_versus", nets + (sum(schedule),) + k["roles"],
                        dict(kw, halving=list(schedule), **value), counts=True)
    return out


def teacher_of_v2(k, **more):
    words, tc = k["words"], dict(tau=8.0, salt=11, **more)
    if k["worlds"]:
        tc["worlds"] = k["worlds"]
    if k["launch"] == "halving":
        return dict(tc, halving=k["schedule"], samples=k["samples"], **({words[0]: True} if words else {}))
    tc.update(dict(net=True), **({"net_worlds": words[0]} if words else {}), **({} if k["depth"] is None else {"depth": k["depth"]}))
    if k["schedule"]:
        tc["net_halving"] = k["schedule"]
    if k["roles"]:
        tc["versus"] = k["roles"]
    elif not k["modes"]:
        tc["net_seats"] = 5
    return dict(tc, samples=k["samples"], **k["modes"]) if k["modes"] else tc


def teacher_door_v2(SP):
    """As teacher_door; a versus teacher has a frozen opponent (its six tensors are the launch's network B), and a sampled
    teacher is launched under both PLAY_MODES of the env: `late` holds teacher_modes() and the calls under the second."""
    out = {}
    for name, k in KINDS_V2.items():
        opp = EC.weights() if k["roles"] else None
        for seats in (None, torch.zeros(4, dtype=torch.uint8)):
            for every in (1, 2) if seats is None else (1,):           # (the rollout body once per kind: the fixture's size)
                env = rec_env(play_mode=PLAY_MODES[0])
                sp = make_teacher(SP, env, teacher_of_v2(k, **({} if every == 1 else dict(every=every))), **({} if opp is None else dict(opponent=opp)))
                row = dict(teacher=dict(sp.teacher), init=list(env.calls))
                sp.env, sp.device, sp.fused, sp.fused_step, sp._w, sp._seats, sp.reward_scale = env, torch.device("cpu"), True, True, EC.weights(), seats, 0.25
                sp._pool_k, sp._opp = 0, opp
                del env.calls[:]
                sp._alloc(3)
                row["alloc"], row["words"] = list(env.calls), None if sp._teach_words is None else env.show(sp._teach_words)
                row["counts"] = env.show(sp._teach_counts) if hasattr(sp, "_teach_counts") else None
                for mode in PLAY_MODES if k["modes"] else PLAY_MODES[:1]:
                    type(env).play_mode = mode
                    del env.calls[:]
                    if every == 1:
                        sp._teach(1)
                    else:
                        sp._rollout_body(2)
                    if mode == PLAY_MODES[0]:
                        row["calls"] = list(env.calls)
                    else:
                        row["late"] = dict(modes=list(sp.teacher_modes()), calls=list(env.calls))
                out["%s/%s/every%d" % (name, "all" if seats is None else "seats", every)] = row
    return out


def evaluation_cases_v2():
    cases = {}
    for name, k in KINDS_V2.items():
        words = k["words"]
        if k["launch"] == "halving":
            cases[name] = ("evaluate_playout_vs_bot", (k["samples"],), dict(halving=k["schedule"], salt=7, **({words[0]: True} if words else {})), False)
            continue
        kw = dict(net="W", **({"worlds": k["worlds"]} if k["worlds"] else {}), **({"net_worlds": words[0]} if words else {}),
                  **({} if k["depth"] is None else dict(net_depth=k["depth"], net_value_scale=4.0)),
                  **({"net_halving": k["schedule"]} if k["schedule"] else {}), **({"net_versus": k["roles"]} if k["roles"] else {}),
                  **({"net_opponent": V} if k["opponent"] else {}))
        if k["launch"] == "net_halving":
            kw["net_seats"] = 5 if words is None else "own"
        if k["modes"]:
            kw.update({"net_" + key: v for key, v in k["modes"].items()}, net_samples=k["samples"])
        cases[name] = ("evaluate_playout_vs_bot", (None,), kw, False)
    return cases


def evaluate_of_v2(k):
    """SelfPlay.evaluate's spelling of a kind (None: it has none — the two-network launches)."""
    words = k["words"]
    if k["launch"] == "halving":
        return dict(versus_playout=k["samples"], playout_halving=k["schedule"], **({"playout_" + words[0]: True} if words else {}))
    if k["roles"]:
        return None
    kw = dict(versus_playout=1, playout_net=True, **({"playout_worlds": k["worlds"]} if k["worlds"] else {}),
              **({"playout_net_worlds": words[0]} if words else {}), **({} if k["depth"] is None else dict(playout_net_depth=k["depth"])))
    if k["launch"] == "net_halving":
        return dict(kw, playout_net_seats=5, playout_net_halving=k["schedule"])
    return dict(kw, playout_net_samples=k["samples"], **{"playout_net_" + key: v for key, v in k["modes"].items()})


def selfplay_evaluate_door_v2(SP):
    out = {}
    for name, k in KINDS_V2.items():
        if evaluate_of_v2(k) is not None:
            rec = Rec()
            call_evaluate(SP, rec, **evaluate_of_v2(k))
            out[name] = rec.calls
    return out


# the refusals: one case per rule of card_player() that names halving, net_halving, net_versus or net_sampled, in each door's
# spelling, and the doors' own rules of those options.  "W" / "V": six tensors; "C": a count tensor; "_private": the case is
# one that only _playout_passes can spell (the public function has no net_sampled dict)
V, NET, HALF = "V", dict(net=True, worlds=2), dict(temperature=0.5)
TEACHER_REFUSALS_V2 = [
    (dict(NET, temperature=3e6), {}), (dict(NET, epsilon=-0.5), {}), (dict(NET, temperature=0.5, opp_epsilon=2.0), {}),
    (dict(NET, temperature=0.5, samples=0), {}), (dict(NET, temperature=0.5, samples=1025), {}), (dict(net=True, temperature=0.5, net_halving=(1, 2)), {}),
    (dict(NET, temperature=0.5, net_seats=3), {}), (dict(NET, versus=(1, 1)), dict(opponent=W)), (dict(NET, versus=(16, 0)), dict(opponent=W)),
    (dict(NET, versus=(1, 14), net_seats=1), dict(opponent=W)), (dict(worlds=2, samples=1, versus=(1, 14)), dict(opponent=W)),
    (dict(NET, versus=(1, 14), temperature=0.5, net_seats=1), dict(opponent=W)),
    (dict(halving=(0, 2)), {}), (dict(halving=(1, 1, 1, 1, 1)), {}), (dict(halving=(1, 64)), {}), (dict(halving=(1, 2), net=True), {}),
    (dict(halving=(1, 2), worlds=4), {}), (dict(net=True, net_halving=(1, 2.0)), {}), (dict(net_halving=(1, 2), samples=1), {}),
    (dict(net=True, net_halving=(1, 2), worlds=4), {}), (dict(net=True, net_halving=(1, 2), samples=2), {}),
    (dict(halving=(1, 2), hidden=True), dict(history=False)), (dict(net=True, net_halving=(1, 2), net_worlds="voids"), dict(history=False)),
    # the teacher's own: play-mode keys without net; versus without opponent=, and with a pool
    (dict(worlds=2, samples=1, temperature=0.5), {}), (dict(worlds=2, samples=1, opp_epsilon=0.5), {}), (dict(NET, versus=(1, 14)), {}),
    (dict(NET, versus=(1, 14)), dict(opponent=[W, W])), (dict(NET, versus=(1, 14)), dict(opponent=[W])),
]
NETW = dict(net=W, worlds=2, samples=None)
EVALUATION_REFUSALS_V2 = [
    dict(NETW, net_sampled=dict(tempo=1.0), _private=True), dict(NETW, net_sampled=5, _private=True), dict(NETW, net_sampled=dict(samples=0)),
    dict(NETW, net_sampled=dict(samples=1025)), dict(NETW, net_sampled=dict(samples=True)), dict(NETW, net_sampled=dict(temperature=-1.0)),
    dict(NETW, net_sampled=dict(epsilon=2.0)), dict(NETW, net_sampled=dict(temperature=0.5, opp_temperature=1e7)),
    dict(NETW, net_sampled=dict(temperature=float("nan"))), dict(worlds=2, net_sampled=HALF), dict(net=W, samples=None, net_halving=(1, 2), net_sampled=HALF),
    dict(NETW, exchange=2, net_sampled=HALF), dict(NETW, bidding=(1, 1), net_sampled=HALF), dict(NETW, net_seats=5, net_sampled=HALF),
    dict(NETW, net_versus=(1, 14), net_opponent=V, net_seats=5, net_sampled=HALF),
    dict(NETW, net_versus=(1, 1), net_opponent=V), dict(NETW, net_versus=(16, 0)), dict(NETW, net_versus=(1, 2, 4), net_opponent=V),
    dict(worlds=2, net_versus=(1, 14), net_opponent=V), dict(NETW, net_versus=(1, 14), net_opponent=V, net_seats=1),
    dict(NETW, net_versus=(1, 14), net_opponent=V, net_seats="own"), dict(NETW, net_versus=(1, 14), net_opponent=V, exchange=2),
    dict(halving=(0, 2)), dict(halving=(1, 2, 3, 4, 5)), dict(halving=(32, 33)), dict(halving=(1, 2), net=W, samples=None),
    dict(halving=(1, 2), exchange=2), dict(halving=(1, 2), bidding=(1, 1)), dict(halving=(1, 2), worlds=4),
    dict(net=W, samples=None, net_halving=(1, True)), dict(net_halving=(1, 2)), dict(net=W, samples=None, net_halving=(1, 2), worlds=4),
    dict(net=W, samples=None, net_halving=(1, 2), exchange=2),
    # evaluate's own: net_opponent without net_versus; opp_rel non-zero without net_opponent
    dict(NETW, net_opponent=V), dict(NETW, net_versus=(1, 14)), dict(NETW, net_versus=(0, 8), net_sampled=HALF),
]
SPE = dict(versus_playout=1, playout_worlds=2, playout_net=True)
SELFPLAY_EVALUATE_REFUSALS_V2 = [
    dict(versus_playout=1, playout_worlds=2, playout_net_temperature=0.5), dict(versus_playout=1, playout_net=True, playout_net_halving=(1, 2), playout_net_samples=2),
    dict(SPE, playout_net_seats=5, playout_net_epsilon=0.5), dict(SPE, playout_net_temperature=-1.0), dict(SPE, playout_net_epsilon=1.5),
    dict(SPE, playout_net_samples=0), dict(SPE, playout_net_samples=1025), dict(SPE, playout_exchange=2, playout_net_samples=2),
    dict(SPE, playout_bidding=(2, 1), playout_net_temperature=0.5),
    dict(versus_playout=2, playout_halving=(0, 2)), dict(versus_playout=2, playout_halving=(1, 64)), dict(versus_playout=1, playout_halving=(1, 2), playout_net=True),
    dict(versus_playout=2, playout_halving=(1, 2), playout_worlds=4), dict(versus_playout=2, playout_halving=(1, 2), playout_exchange=4),
    dict(versus_playout=2, playout_halving=(1, 2), playout_bidding=(2, 1)), dict(playout_halving=(1, 2)),
    dict(versus_playout=1, playout_net=True, playout_net_halving=(1, 65)), dict(versus_playout=1, playout_net_halving=(1, 2)),
    dict(versus_playout=1, playout_net=True, playout_net_halving=(1, 2), playout_worlds=4),
    dict(versus_playout=1, playout_net=True, playout_net_halving=(1, 2), playout_exchange=2),
]
ENV_REFUSALS_V2 = [
    ("playout_cards_net_versus", (W, V, 3), dict(count_out="C"), True), ("playout_cards_net_versus", (W, V, 4), dict(halving=(1, 2)), True),
    ("playout_cards_net_versus", (W, None, 3), {}, True), ("playout_cards_net_versus", (W, None, 3, 15, 8), {}, True),
    ("playout_cards_net_versus", (W, V, 3, 3, 1), {}, True), ("playout_cards_net_versus", (W, V, 3, 16, 0), {}, True),
    ("playout_cards_net_versus", (W, V, 3), dict(halving=(0, 2)), True), ("playout_cards_net_versus", (W, V, 3), dict(voids=True, hidden=True), True),
    ("playout_cards_net_versus", (W, V, 3), dict(hidden=True), False), ("playout_cards_net_versus", (W, V, 3), dict(depth=13), True),
    ("playout_cards_net_versus", (W, V, 3), dict(depth=1, value_scale=0.0), True), ("playout_cards_net_versus", (W, V, 0), {}, True),
    ("playout_cards_net_sampled", (W, None, 3, 2, 1, 14), {}, True), ("playout_cards_net_sampled", (W, V, 3, 2, 3, 6), {}, True),
    ("playout_cards_net_sampled", (W, V, 3, 2), dict(temperature=-1.0), True), ("playout_cards_net_sampled", (W, V, 3, 2), dict(epsilon=1.5), True),
    ("playout_cards_net_sampled", (W, V, 3, 2), dict(opp_temperature=1e7), True), ("playout_cards_net_sampled", (W, V, 3, 2), dict(opp_epsilon=2.0), True),
    ("playout_cards_net_sampled", (W, V, 3, 0), {}, True), ("playout_cards_net_sampled", (W, V, 3, 1025), {}, True),
    ("playout_cards_net_sampled", (W, V, 65, 2), {}, True), ("playout_cards_net_sampled", (W, V, 3, 2), dict(voids=True), False),
    ("playout_cards_net_sampled", (W, V, 3, 2), dict(depth=0), True),
    ("playout_cards_net_halving", (W, (1, 2)), dict(net_seats=16), True), ("playout_cards_net_halving", (W, (0, 2)), {}, True),
    ("playout_cards_net_halving", (W, (1, 2)), dict(depth=0), True), ("playout_cards_net_halving", (W, (1, 2)), dict(hidden=True), False),
    ("playout_cards_net_halving", (W, (1, 2)), dict(voids=True, hidden=True), True),
    ("playout_cards_halving", ((1, 64),), {}, True), ("playout_cards_halving", ((1, 2),), dict(voids=True, hidden=True), True),
    ("playout_cards_halving", ((1, 2),), dict(voids=True), False), ("playout_cards_halving", ([],), {}, True),
]


def named_v2(x):
    """`x` with "W" / "V" replaced by six tensors and "C" by a count tensor, inside lists and dicts too."""
    if isinstance(x, dict):
        return {k: named_v2(v) for k, v in x.items()}
    if isinstance(x, list):
        return [named_v2(v) for v in x]
    return EC.weights() if x in (W, V) else torch.zeros((4, 12), dtype=torch.int32) if x == "C" else x


def refusals_v2(ENV, SP, EV):
    """As refusals(), with the rows written from the cases as the tables spell them."""
    out = dict(teacher=[], evaluation=[], selfplay_evaluate=[], env=[])
    for tc, kw in TEACHER_REFUSALS_V2:
        kw_, env = named_v2(dict(kw)), rec_env(kw.get("history", True))
        kw_.pop("history", None)
        sp = SP.SelfPlay.__new__(SP.SelfPlay)
        out["teacher"].append([repr((tc, kw)), raised(lambda: sp.__init__(env, hidden=256, teacher=tc, **kw_)), env.calls == []])
    for kw in EVALUATION_REFUSALS_V2:
        for public in (False,) if kw.get("_private") else (False, True):
            trace, kw_ = EC.Trace(), named_v2({k: v for k, v in kw.items() if k != "_private"})
            samples, mix = kw_.pop("samples", 2), kw_.pop("mix", 2)
            if public:                                # the public function spells the dict as net_samples=, net_temperature=, ..
                kw_.update({"net_" + k: v for k, v in kw_.pop("net_sampled", {}).items()})
            saved, EV.TarokVecEnv = EV.TarokVecEnv, EC.stand_in(trace)
            try:
                how = raised((lambda: EV.evaluate_playout_vs_bot(samples, EC.N, EC.EPISODES, mix=mix, **kw_)) if public else
                             (lambda: EV._playout_passes(samples, EC.N, EC.EPISODES, 0, mix, 0, **kw_)))
            finally:
                EV.TarokVecEnv = saved
            out["evaluation"].append([repr(kw), public, how, trace.calls == [] and trace.closed == 0])
    for kw in SELFPLAY_EVALUATE_REFUSALS_V2:
        rec = Rec()
        out["selfplay_evaluate"].append([repr(kw), raised(lambda: call_evaluate(SP, rec, **kw)), rec.calls == []])
    for method, args, kw, history in ENV_REFUSALS_V2:
        env = type("Env", (ENV.TarokVecEnv,), dict(__init__=lambda self: None, close=lambda self: None, n=4, _h=77, history=history,
                                                   device=torch.device("cpu"), L=Rec(), _net_scratch={}))()
        args_, kw_ = [named_v2(a) for a in args], named_v2(kw)
        out["env"].append([method, repr((args, kw, history)), raised(lambda: getattr(env, method)(*args_, **kw_)), env.L.calls == []])
    return out


def record_all_v2(ENV, SP, EV):
    return json.loads(json.dumps(dict(env=env_door_v2(ENV), teacher=teacher_door_v2(SP), evaluation=evaluation_door(EV, evaluation_cases_v2()),
                                      selfplay_evaluate=selfplay_evaluate_door_v2(SP), refusals=refusals_v2(ENV, SP, EV))))


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def got():
    from tarok_amd import env, evaluate, selfplay
    return record_all(env, selfplay, evaluate)


@pytest.fixture(scope="module")
def golden_v2():
    with open(FIXTURE_V2) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def got_v2():
    from tarok_amd import env, evaluate, selfplay
    return record_all_v2(env, selfplay, evaluate)


def refusals_all_raised(golden):
    for door, rows in golden["refusals"].items():
        assert rows and all(r[-2] in ("ValueError", "RuntimeError") and r[-1] is True for r in rows), door


def same_calls(got, golden, door):
    assert sorted(got[door]) == sorted(golden[door])
    for key, want in golden[door].items():
        assert got[door][key] == want, "%s: %s differs" % (door, key)


def same_evaluation(got, golden, name):
    have, want = EC.unpack(got["evaluation"][name]["calls"]), EC.unpack(golden["evaluation"][name]["calls"])
    for i, (a, b) in enumerate(zip(have, want)):
        assert a == b, "%s: call %d differs" % (name, i)
    assert len(have) == len(want)
    assert got["evaluation"][name]["tuples"] == golden["evaluation"][name]["tuples"] and got["evaluation"][name]["closed"] == 1


def same_refusals(got, golden, door):
    assert len(got["refusals"][door]) == len(golden["refusals"][door])
    for have, want in zip(got["refusals"][door], golden["refusals"][door]):
        assert have == want, "%s: %s" % (door, want[0])


def test_the_fixture_holds_every_kind_at_every_door(golden):
    assert {k.split("/")[0] for k in golden["env"]} == {k.split("/")[0] for k in golden["teacher"]} == set(golden["selfplay_evaluate"]) == set(KINDS)
    assert set(golden["evaluation"]) == set(evaluation_cases()) and len(golden["evaluation"]) == 4 + 2 * 6
    assert len(golden["env"]) >= 4 * len(KINDS) and len(golden["teacher"]) == 4 * len(KINDS)
    refusals_all_raised(golden)
    assert [r[-2] for r in golden["refusals"]["selfplay_evaluate"]].count("RuntimeError") == 1
    for name, g in golden["evaluation"].items():
        assert 400 < len(EC.unpack(g["calls"])) < 2500 and g["closed"] == 1, name


def test_the_v2_fixture_holds_every_kind_at_every_door(golden_v2):
    g = golden_v2
    assert {k.split("/")[0] for k in g["env"]} == {k.split("/")[0] for k in g["teacher"]} == set(g["evaluation"]) == set(KINDS_V2)
    assert {family(k) for k in KINDS_V2} == set(FAMILIES_V2)
    # SelfPlay.evaluate spells no two-network launch: every kind with one network, and those alone
    assert set(g["selfplay_evaluate"]) == {name for name, k in KINDS_V2.items() if k["roles"] is None}
    assert {family(k) for k in g["selfplay_evaluate"]} == {"halving", "net_halving", "sampled"}
    # the env's door: every way to the words, both seat spellings, outputs given and new; a two-network halving launch with
    # and without its worlds; the scratch's size asked of the library by every net-played launch
    for name, k in KINDS_V2.items():
        keys = [key for key in g["env"] if key.split("/")[0] == name]
        ways = (3 if k["words"] else 1) * (2 if k["launch"] == "versus" and k["schedule"] else 1)
        assert len(keys) == 4 * ways and len(g["env"][keys[0]]) >= 2, name
        for key in keys:
            assert (k["launch"] == "halving") == (not any("scratch" in c for c in g["env"][key])), key
            assert g["env"][key][-1].count("int32[4, 12]") == (1 if k["schedule"] else 0), key      # (count_out comes back with a schedule alone)
    method = dict(halving="tarok_playout_cards_halving(", net_halving="tarok_playout_cards_net_halving(", sampled="tarok_playout_cards_net_sampled(")
    for key, calls in g["env"].items():
        k = KINDS_V2[key.split("/")[0]]
        want = method.get(k["launch"], "tarok_playout_cards_net_versus_halving(" if k["schedule"] else "tarok_playout_cards_net_versus(")
        assert calls[-2].startswith(want), key
    # the teacher's door: both seat spellings at every 1, the rollout body at every 2; a sampled teacher under both play modes of the env, and where it seats
    # an opponent whose mode it left open the launch's modes follow the env's
    assert len(g["teacher"]) == 3 * len(KINDS_V2) and sum(key.endswith("/all/every2") for key in g["teacher"]) == len(KINDS_V2)
    for key, row in g["teacher"].items():
        k = KINDS_V2[key.split("/")[0]]
        assert ("late" in row) == (k["modes"] is not None) and (row["counts"] is not None) == (k["schedule"] is not None), key
        assert ("versus" in row["teacher"]) == (k["roles"] is not None) and ("temperature" in row["teacher"]) == (k["modes"] is not None), key
        if k["modes"]:
            opens = k["roles"] is not None and "opp_temperature" not in k["modes"]
            assert (row["late"]["modes"][2:] == list(PLAY_MODES[1])) == opens and (row["late"]["calls"] != row["calls"]) == opens, key
    assert sum("late" in row and row["late"]["calls"] != row["calls"] for row in g["teacher"].values()) == 3
    refusals_all_raised(g)
    for name, e in g["evaluation"].items():
        assert 400 < len(EC.unpack(e["calls"])) < 2500 and e["closed"] == 1, name


@pytest.mark.parametrize("door", ["env", "teacher", "selfplay_evaluate"])
def test_the_doors_calls_are_those_of_the_fixture(got, golden, door):
    same_calls(got, golden, door)


@pytest.mark.parametrize("door", ["env", "teacher", "selfplay_evaluate"])
def test_the_v2_doors_calls_are_those_of_the_fixture(got_v2, golden_v2, door):
    same_calls(got_v2, golden_v2, door)


@pytest.mark.parametrize("name", sorted(evaluation_cases()))
def test_the_evaluations_calls_are_those_of_the_fixture(got, golden, name):
    same_evaluation(got, golden, name)


@pytest.mark.parametrize("name", sorted(evaluation_cases_v2()))
def test_the_v2_evaluations_calls_are_those_of_the_fixture(got_v2, golden_v2, name):
    same_evaluation(got_v2, golden_v2, name)


@pytest.mark.parametrize("door", ["teacher", "evaluation", "selfplay_evaluate", "env"])
def test_the_refusals_are_those_of_the_fixture(got, golden, door):
    same_refusals(got, golden, door)


@pytest.mark.parametrize("door", ["teacher", "evaluation", "selfplay_evaluate", "env"])
def test_the_v2_refusals_are_those_of_the_fixture(got_v2, golden_v2, door):
    same_refusals(got_v2, golden_v2, door)


def write_fixture(doors_rows):
    """One line per key or refusal, tight separators."""
    tight = lambda x: json.dumps(x, separators=(",", ":"))
    doors = []
    for door, rows in doors_rows.items():
        body = ",\n".join("%s:%s" % (tight(k), tight(v)) for k, v in rows.items()) if door != "refusals" else \
            ",\n".join("%s:[\n%s]" % (tight(k), ",\n".join(tight(r) for r in v)) for k, v in rows.items())
        doors.append("%s:{\n%s}" % (tight(door), body))
    sys.stdout.write("{%s}\n" % ",\n".join(doors))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    if sys.argv[1] == "v2":
        # record v2 from a whole package in the directory given (the parent commit's tarok_amd/*.py under another name): its env,
        # selfplay and evaluate import their own playout, never the one under test
        sys.path.insert(0, os.path.dirname(os.path.abspath(sys.argv[2])))
        package = os.path.basename(os.path.abspath(sys.argv[2]))
        assert package != "tarok_amd"
        write_fixture(record_all_v2(*[importlib.import_module("%s.%s" % (package, name)) for name in ("env", "selfplay", "evaluate")]))
    else:
        # record v1 from the three files in the directory given (the parent commit's), loaded beside the package's own modules
        mods = []
        for name in ("env", "selfplay", "evaluate"):
            spec = importlib.util.spec_from_file_location("tarok_amd.%s_recorded" % name, os.path.join(sys.argv[1], name + ".py"))
            mods.append(importlib.util.module_from_spec(spec))
            spec.loader.exec_module(mods[-1])
        write_fixture(record_all(*mods))
