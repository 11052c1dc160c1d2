"""CPU-side checks of the net-played card playouts in the void-aware and hidden-card worlds
(tarok_playout_cards_net_voids, tarok_playout_cards_net_hidden): the model of tests/playout_net_worlds_model.py against
the models it is made of where they must agree, the positions the GPU tests use (they do constrain the worlds), the
ValueErrors old and new, the launches the three Python entry points issue on stand-in envs, and the C entry points'
argument checks, which come before any HIP call.  No GPU in here."""
import ctypes
import inspect

import numpy as np
import pytest

import playout_hidden_model as HM
import playout_net_model as NM
import playout_net_worlds_model as WM
import playout_voids_model as VM
from oracle import tarok_spec as S
from playout_net_cases import Calls, NoHistory, WithHistory, no_device, weights, zero_net

SEED, EPISODE, OFFSET = 41, 3, 1000               # tests/test_gpu_playout_det.py's: the GPU tests' envs
KLOP, DVE = 0, 2


def logits(k):
    """54 distinct card logits, reversed for k = 1: a network that prefers high cards, or low ones."""
    v = np.arange(54, dtype=np.float64) / 64
    return zero_net(v[::-1].copy() if k else v)


@pytest.mark.parametrize("cards", [0, 9, 24, 44])
def test_zero_void_words_are_the_net_model(cards):
    games, words, _ = WM.bot_games("voids", SEED, EPISODE, S.MIX_ALL, 5, cards, first=OFFSET)
    W = logits(0)
    want_sum, want_act = NM.playout_cards(games, SEED, 3, 15, 3, W, 15)
    got_sum, got_act = WM.playout_cards("voids", games, SEED, 3, 15, 3, W, 15, [0] * 5)
    assert want_sum.any() and (got_sum == want_sum).all() and (got_act == want_act).all()


@pytest.mark.parametrize("kind", WM.KINDS)
@pytest.mark.parametrize("cards", [0, 9, 24, 44])
def test_no_net_seat_is_the_bot_played_model(kind, cards):
    """net_seats = 0: playout_voids_model / playout_hidden_model at samples = 1, under the games' own words."""
    M = VM if kind == "voids" else HM
    games, words, _ = WM.bot_games(kind, SEED, EPISODE, S.MIX_ALL, 5, cards, first=OFFSET)
    got_sum, got_act = WM.playout_cards(kind, games, SEED, 7, 15, 3, logits(0), 0, words)
    for g, (lanes, ep, gidx, _) in enumerate(games):
        want_sum, want_act = M.playout_cards(lanes, ep, SEED, 7, gidx, 15, 3, 1, words[g])
        assert (got_sum[g] == want_sum).all() and got_act[g] == want_act, (kind, cards, g)
    assert got_sum.any()


def gpu_positions(kind):
    return ([(S.MIX_ALL, 5), (S.MIX_ALL, 24), (S.MIX_ALL, 44)] if kind == "voids"
            else [(S.MIX_FIXED + KLOP, 5), (S.MIX_FIXED + DVE, 24), (S.MIX_ALL, 44)])


@pytest.mark.parametrize("kind", WM.KINDS)
def test_the_gpu_tests_positions_constrain_the_worlds(kind):
    """The positions of tests/test_gpu_playout_net_worlds.py, rebuilt on the oracle: a void word for a seat other than
    the mover; live Klop talon cards (the first hidden position: a Klop inside its first six tricks) and a non-empty
    hidden discard set with a non-declarer to move (the second: Dve); and the network's playouts in those worlds give
    other sums than in the determinized ones, for two networks that give each other's too."""
    seen, differ, nets_differ = [], 0, 0
    for mix, cards in gpu_positions(kind):
        games, words, objs = WM.bot_games(kind, SEED, EPISODE, mix, 5, cards, first=OFFSET)
        seen.append({WM.constrains(kind, g, w) for g, w in zip(objs, words)})
        new, _ = WM.playout_cards(kind, games, SEED, 3, 15, 3, logits(0), 15, words)
        det, _ = NM.playout_cards(games, SEED, 3, 15, 3, logits(0), 15)
        other, _ = WM.playout_cards(kind, games, SEED, 3, 15, 3, logits(1), 15, words)
        differ += int((new != det).any(axis=(1, 2)).sum())
        nets_differ += int((new != other).any(axis=(1, 2)).sum())
    if kind == "voids":
        assert all("voids" in s for s in seen), seen
    else:
        assert seen[0] == {"talon"} and "discards" in seen[1], seen
        games, _, objs = WM.bot_games(kind, SEED, EPISODE, S.MIX_FIXED + DVE, 5, 24, first=OFFSET)
        assert any(g.seat() != int(g.g.declarer) for g in objs) and any(g.seat() == int(g.g.declarer) for g in objs)
    assert differ >= 3 and nets_differ >= 3


def test_new_and_old_refusals():
    """Every new ValueError, before any env is made or touched; and the old spellings keep raising (the pinned tests of
    tests/test_playout_net_cpu.py and tests/test_evaluate_calls_cpu.py are the authority on those)."""
    from tarok_amd import _native, evaluate as EV, selfplay as SP
    from tarok_amd.env import TarokVecEnv
    assert "tarok_playout_cards_net_voids" in _native.SYMBOLS and "tarok_playout_cards_net_hidden" in _native.SYMBOLS
    sig = inspect.signature(TarokVecEnv.playout_cards_net).parameters
    assert list(sig)[1:] == ["weights", "worlds", "net_seats", "salt", "seats", "seats_per_game", "sum_out", "action_out", "voids",
                             "hidden", "words"]
    assert sig["voids"].default is False and sig["hidden"].default is False and sig["words"].default is None
    assert inspect.signature(EV.evaluate_playout_vs_bot).parameters["net_worlds"].default == "det"
    assert inspect.signature(SP.SelfPlay.evaluate).parameters["playout_net_worlds"].default == "det"
    net = weights()
    for kw in (dict(net=net, worlds=2, net_worlds="both"), dict(net=net, worlds=2, net_worlds=True), dict(worlds=2, net_worlds="voids"),
               dict(net=net, net_worlds="voids"), dict(net=net, worlds=2, net_worlds="voids", exchange=2),
               dict(net=net, worlds=2, net_worlds="hidden", bidding=(2, 1)),
               dict(net=net, worlds=2, voids=True), dict(net=net, worlds=2, hidden=True),                 # the old spellings
               dict(net=net, worlds=2, voids=True, net_worlds="voids"), dict(net=net, worlds=2, hidden=True, net_worlds="hidden")):
        with pytest.raises(ValueError):
            EV.evaluate_playout_vs_bot(None if "net" in kw else 2, 8, 1, **kw)
    with pytest.raises(ValueError):
        EV.evaluate_playout_vs_bot(2, 8, 1, net=net, worlds=2, net_worlds="voids")               # samples is not taken
    for env, tc in ((WithHistory, dict(net=True, worlds=2, net_worlds="both")), (WithHistory, dict(worlds=2, samples=1, net_worlds="voids")),
                    (NoHistory, dict(net=True, worlds=2, net_worlds="voids")), (NoHistory, dict(net=True, worlds=2, net_worlds="hidden")),
                    (WithHistory, dict(net=True, worlds=2, net_worlds="voids", samples=2)),
                    (WithHistory, dict(net=True, worlds=2, voids=True)), (WithHistory, dict(net=True, worlds=2, hidden=True)),   # old
                    (WithHistory, dict(net=True, worlds=2, voids=True, net_worlds="voids"))):
        with pytest.raises(ValueError):
            SP.SelfPlay(env(), hidden=256, teacher=tc)
    with pytest.raises(ValueError):
        SP.SelfPlay(WithHistory(), hidden=128, teacher=dict(net=True, worlds=2, net_worlds="voids"))
    for kw in (dict(playout_net=True, playout_worlds=2, playout_net_worlds="both"), dict(playout_worlds=2, versus_playout=1, playout_net_worlds="voids"),
               dict(playout_net=True, playout_net_worlds="voids"), dict(playout_net=True, playout_worlds=2, playout_voids=True),
               dict(playout_net=True, playout_worlds=2, playout_hidden=True, playout_net_worlds="hidden")):
        with pytest.raises(ValueError):
            SP.SelfPlay.evaluate(object(), **kw)
    for env, kw in ((WithHistory, dict(voids=True, hidden=True)), (NoHistory, dict(voids=True)), (NoHistory, dict(hidden=True))):
        with pytest.raises(ValueError):
            TarokVecEnv.playout_cards_net(type("Env", (env,), dict(_cards=TarokVecEnv._cards))(), net, 2, **kw)


def test_the_env_method_issues_the_launch_of_the_kind():
    """TarokVecEnv.playout_cards_net on a stand-in env: the defaults issue tarok_playout_cards_net alone; voids=True /
    hidden=True the words launch into the caller's scratch tensor and then the launch of the kind with that tensor before
    net_seats; a tensor in their place is the words: no words launch, and no history needed."""
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
        env = Env(False)
        TarokVecEnv.playout_cards_net(env, net, 2, net_seats=5, salt=3, seats=9)
        assert env.L.calls == ["tarok_playout_cards_net(77, 2, 3, 9, None, 5, " + tail]
        for kind, words_fn, dtype in (("voids", "tarok_shown_voids", torch.int32), ("hidden", "tarok_played_cards", torch.int64)):
            name = str(dtype).replace("torch.", "") + "[4]"
            env = Env(True)
            TarokVecEnv.playout_cards_net(env, net, 2, net_seats=5, salt=3, seats=9, words=torch.zeros(4, dtype=dtype), **{kind: True})
            assert env.L.calls == ["%s(77, '%s', 'stream')" % (words_fn, name),
                                   "tarok_playout_cards_net_%s(77, 2, 3, 9, None, '%s', 5, %s" % (kind, name, tail)], env.L.calls
            env = Env(False)
            TarokVecEnv.playout_cards_net(env, net, 2, net_seats=5, salt=3, seats=9, **{kind: torch.zeros(4, dtype=dtype)})
            assert env.L.calls == ["tarok_playout_cards_net_%s(77, 2, 3, 9, None, '%s', 5, %s" % (kind, name, tail)], env.L.calls


def test_evaluate_issues_the_launch_of_the_kind():
    """evaluate_playout_vs_bot(net=, net_worlds=) on the stand-in env of tests/evaluate_calls_cases.py: "det" makes the
    calls of the call without it; "voids" / "hidden" make an env that keeps its history and hand every lock-step's
    playout_cards_net the kind and one words tensor of the kind's dtype, everything else the same."""
    import re
    import evaluate_calls_cases as EC
    from tarok_amd import evaluate as EV
    EC.CASES.update(nw_none=("evaluate_playout_vs_bot", (None,), dict(worlds=2, net="W", net_seats=5), False),
                    nw_det=("evaluate_playout_vs_bot", (None,), dict(worlds=2, net="W", net_seats=5, net_worlds="det"), False),
                    nw_voids=("evaluate_playout_vs_bot", (None,), dict(worlds=2, net="W", net_seats="own", net_worlds="voids"), False),
                    nw_hidden=("evaluate_playout_vs_bot", (None,), dict(worlds=2, net="W", net_seats=5, net_worlds="hidden"), False))
    try:
        traces = {k: EC.run_case(EV, k)[0] for k in ("nw_none", "nw_det", "nw_voids", "nw_hidden")}
    finally:
        for k in ("nw_none", "nw_det", "nw_voids", "nw_hidden"):
            del EC.CASES[k]
    assert traces["nw_det"].calls == traces["nw_none"].calls and "history=False" in traces["nw_none"].calls[0]
    plain = [c for c in traces["nw_none"].calls if c.startswith("playout_cards_net(")]
    assert len(plain) >= 5 * EC.EPISODES and not any("voids" in c or "hidden" in c or "words" in c for c in plain)
    for kind, dtype in (("voids", "i32"), ("hidden", "i64")):
        calls = traces["nw_" + kind].calls
        assert calls[0].startswith("TarokVecEnv(") and "history=True" in calls[0]
        launches = [c for c in calls if c.startswith("playout_cards_net(")]
        assert len(launches) == len(plain) and len(calls) == len(traces["nw_none"].calls)
        words = set()
        for c in launches:
            m = re.search(r", words=(T\d+\[2\]%s@0)\)$" % dtype, c)
            assert m and ("%s=True" % kind) in c and ("voids" if kind == "hidden" else "hidden") not in c, c
            words.add(m.group(1))
        assert len(words) == 1                                    # one scratch tensor for the whole evaluation
    own = [c for c in traces["nw_voids"].calls if c.startswith("playout_cards_net(")]
    assert all(re.search(r"net_seats=(\d+), salt=0, seats=\1,", c) for c in own)


def test_the_teacher_issues_one_chain_per_lock_step():
    """SelfPlay._alloc and ._teach on a stand-in: the words scratch is _teach_words (int32 for voids, int64 for hidden,
    none for "det"), and a lock-step's teacher is playout_cards_net with the kind, that tensor and the learner's live
    rollout weights, then playout_targets at `worlds` playouts."""
    import torch
    from tarok_amd import selfplay as SP

    class Env(Calls):
        n, history = 4, True
    for kind, dtype in (("det", None), ("voids", torch.int32), ("hidden", torch.int64)):
        tc = dict(net=True, worlds=2, tau=8.0, salt=11)
        if kind != "det":
            tc["net_worlds"] = kind
        sp = SP.SelfPlay.__new__(SP.SelfPlay)
        try:
            sp.__init__(WithHistory(), hidden=256, teacher=tc)
        except (AttributeError, TypeError):                      # (the stand-in is no env: the teacher is read first)
            pass
        assert sp.teacher == dict(worlds=2, samples=1, tau=8.0, every=1, salt=11, voids=False, hidden=False, net=True, net_seats=15,
                                  net_worlds=kind)
        sp.env, sp.device, sp.fused, sp._w, sp._seats = Env(), torch.device("cpu"), True, weights(), None
        sp._alloc(3)
        assert sp.env.calls == ["playout_net_scratch(2)"]
        assert (sp._teach_words is None) if dtype is None else (sp._teach_words.dtype == dtype and tuple(sp._teach_words.shape) == (4,))
        del sp.env.calls[:]
        sp._teach(1)
        want = dict(action_out="uint8[4]", net_seats="15", salt="11", seats_per_game="None", sum_out="int32[4, 12, 4]")
        if kind != "det":
            want.update({kind: "True", "words": "%s[4]" % str(dtype).replace("torch.", "")})
        assert len(sp.env.calls) == 2
        assert sp.env.calls[1] == "playout_targets(int32[4, 12, 4], int64[4], 2, 8.0, seats_per_game=None, target_out=bfloat16[4, 64])"
        assert sp.env.calls[0].startswith("playout_cards_net(") and sp.env.calls[0].endswith(
            "], 2, %s)" % ", ".join("%s=%s" % kv for kv in sorted(want.items()))), sp.env.calls[0][-200:]


@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401  -- before the dlopen: one HIP runtime
    import tarok_amd
    from tarok_amd import _native
    tarok_amd.build()
    return _native.lib()


@pytest.mark.parametrize("kind", WM.KINDS)
def test_the_entry_points_validate_before_any_hip_call(L, kind):
    """Every refusal comes before the first HIP call: a zeroed stand-in for an env (no GPU, no tarok_create, no history)
    is enough — and the words being an argument, the missing history is no refusal of its own."""
    z = ctypes.c_void_p(0)
    env = ctypes.cast(ctypes.create_string_buffer(1 << 16), ctypes.c_void_p)
    buf = ctypes.create_string_buffer(512)
    out = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    f = getattr(L, "tarok_playout_cards_net_" + kind)
    ok = dict(env=env, worlds=4, seats=15, words=out, net=15, w=[out] * 6, scr=out, size=0, sum=out, act=out)

    def rc(**ch):
        a = dict(ok, **ch)
        return f(a["env"], a["worlds"], 0, a["seats"], z, a["words"], a["net"], *a["w"], a["scr"], a["size"], a["sum"], a["act"], z)
    bad = [dict(env=None), dict(worlds=0), dict(worlds=65), dict(worlds=-2), dict(seats=16), dict(seats=-1), dict(words=z), dict(net=16),
           dict(net=-1), dict(scr=z), dict(scr=ctypes.c_void_p(out.value + 8)), dict(size=-1), dict(sum=z, act=z)]
    bad += [dict(w=[out] * i + [z] + [out] * (5 - i)) for i in range(6)]
    for ch in bad:
        assert rc(**ch) == -1, ch
