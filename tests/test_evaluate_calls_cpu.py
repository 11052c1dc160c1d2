"""The launch sequence of tarok_amd.evaluate, pinned on the CPU.  Every TarokVecEnv method is a deterministic function of
the env's state and its arguments, so an evaluation that makes the same calls with the same arguments — and hands the
same buffers to the same places — computes the same scores.  The tests swap evaluate.TarokVecEnv for a stand-in that
records every call and compare the record, call for call, with tests/golden/evaluate_calls_v1.json.

The fixture was recorded from the evaluate.py of the commit BEFORE the duplicate-pass driver (six separate pass loops),
never from the module under test:

    git show 0adb785:tarok_amd/evaluate.py > /tmp/evaluate_parent.py
    python tests/test_evaluate_calls_cpu.py /tmp/evaluate_parent.py > tests/golden/evaluate_calls_v1.json

A call is one line: name(arguments), keyword arguments sorted by name.  A tensor argument is T<i><shape><dtype>@<offset>,
i counting storages in order of first appearance, so the line says WHICH buffer (row t of `actions`, the side of the
word ping-pong) was passed.  Runs of calls that differ only by a constant step of the offsets are stored as
[count, first block, offset steps per line] (the 48 lock-steps of a pass are one entry)."""
import importlib.util
import json
import re
import sys

import numpy as np
import pytest

from evaluate_calls_cases import (EPISODES, CASES, FIXTURE, N, REFUSALS, ROOT, Trace, describe, record_all, run_case, stand_in, unpack,
                                  weights)


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def EV():
    from tarok_amd import evaluate
    return evaluate


def test_the_fixture_holds_every_case(golden):
    assert sorted(golden) == sorted(CASES)
    for name, g in golden.items():
        assert 400 < len(unpack(g["calls"])) < 2500, name          # 10 passes of 48 lock-steps, one or two calls each


@pytest.mark.parametrize("name", sorted(CASES))
def test_calls_are_those_of_the_fixture(EV, golden, name):
    trace, scores, record = run_case(EV, name)
    want = unpack(golden[name]["calls"])
    for i, (a, b) in enumerate(zip(trace.calls, want)):
        assert a == b, "%s: call %d differs" % (name, i)
    assert len(trace.calls) == len(want)
    assert trace.tuples == golden[name]["tuples"] and trace.closed == 1
    # the score sums of pass p of episode e — the stand-in's carry the ordinal of their counters() call — at [p, e*N:(e+1)*N]
    scores = np.asarray(scores)
    assert scores.dtype == np.int32 and scores.shape == (5, EPISODES * N, 4)
    counters = [i for i, c in enumerate(trace.calls) if c.startswith("counters(")]
    assert len(counters) == 5 * EPISODES
    for j, k in enumerate(counters):
        e, p = divmod(j, 5)
        assert (scores[p, e * N:(e + 1) * N] == (1000 * k + np.arange(4 * N)).reshape(N, 4)).all(), (name, e, p)
    assert (None if record is None else describe(record)) == golden[name]["inspect"]


@pytest.mark.parametrize("name", sorted(n for n in CASES if CASES[n][3]))
def test_inspect_keys(EV, name):
    fn, _, kwargs, _ = CASES[name]
    keys = {"episode", "seats", "start", "actions", "scores"}
    if "exchange" in fn or "exchange" in kwargs:
        keys |= {"choice", "discards"}
    if "bid" in fn or "bidding" in kwargs:
        keys |= {"contract", "declarer", "king_suit"}
    if "bidnet" in fn:
        keys |= {"values"}
    record = run_case(EV, name)[2]
    assert len(record) == 5 * EPISODES
    for j, d in enumerate(record):
        assert set(d) == keys, (name, j)
        assert (d["episode"], d["seats"]) == (j // 5, EV.PASS_SEATS[j % 5])
        assert d["actions"].dtype == np.uint8 and d["actions"].shape == (EV.GAME_CARDS, N)
        assert d["scores"].dtype == np.int32 and d["scores"].shape == (N, 4)
        assert d["start"].dtype == np.uint64 and d["start"].shape == (10, N)


def test_start_is_read_only_for_inspect_and_before_the_exchange(EV):
    for name in CASES:
        calls = run_case(EV, name)[0].calls
        states = [i for i, c in enumerate(calls) if c.startswith("state(")]
        assert len(states) == (5 * EPISODES if CASES[name][3] else 0), name
        for i in states:
            assert calls[i - 1].startswith("reset("), (name, i)


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("fail_at", ["reset", "counters"])
def test_the_env_is_closed_once_when_a_call_raises(EV, name, fail_at):
    trace = Trace(fail_at)
    with pytest.raises(RuntimeError, match="the stand-in's %s fails" % fail_at):
        run_case(EV, name, trace)
    assert trace.closed == 1 and trace.calls[-1].startswith(fail_at + "(")


@pytest.mark.parametrize("kwargs,message", REFUSALS)
def test_playout_passes_refuses_before_an_env_is_made(EV, monkeypatch, kwargs, message):
    trace = Trace()
    monkeypatch.setattr(EV, "TarokVecEnv", stand_in(trace))
    kwargs = dict(kwargs)
    if "net" in kwargs:
        kwargs["net"] = weights()
    samples, mix = kwargs.pop("samples", 2), kwargs.pop("mix", 2)
    with pytest.raises(ValueError, match=re.escape(message)):
        EV._playout_passes(samples, N, EPISODES, 0, mix, 0, **kwargs)
    with pytest.raises(ValueError, match=re.escape(message)):
        EV.evaluate_playout_vs_bot(samples, N, EPISODES, mix=mix, **kwargs)
    assert trace.calls == [] and trace.closed == 0


def test_evaluate_vs_policy_refuses_before_an_env_is_made(EV, monkeypatch):
    trace = Trace()
    monkeypatch.setattr(EV, "TarokVecEnv", stand_in(trace))
    for bad in (None, weights()[:5], tuple(weights()) + (1,), [0] * 6):
        with pytest.raises(ValueError, match=re.escape("weights: six tensors (w1, b1, w2, b2, w3, b3)")):
            EV.evaluate_vs_policy(bad, weights(), N, EPISODES)
        with pytest.raises(ValueError, match=re.escape("opponent: six tensors (w1, b1, w2, b2, w3, b3)")):
            EV.evaluate_vs_policy(weights(), bad, N, EPISODES)
    assert trace.calls == [] and trace.closed == 0


if __name__ == "__main__":
    # record the fixture from the evaluate.py given (the parent commit's), loaded beside the package's own modules
    sys.path.insert(0, ROOT)
    spec = importlib.util.spec_from_file_location("tarok_amd.evaluate_recorded", sys.argv[1])
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    tight = lambda x: json.dumps(x, separators=(",", ":"))
    cases = []
    for name, case in record_all(module).items():                    # one line per call or run of calls
        calls = ",\n".join(tight(c) for c in case.pop("calls"))
        cases.append('%s:{"calls":[\n%s],\n%s}' % (tight(name), calls, ",\n".join("%s:%s" % (tight(k), tight(v)) for k, v in case.items())))
    sys.stdout.write("{%s}\n" % ",\n".join(cases))
