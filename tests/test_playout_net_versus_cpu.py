"""CPU: the statement of tarok_playout_cards_net_versus (tests/playout_net_versus_model.py) on the plan of
tests/playout_net_versus_cases.py — the versus rows against both single-network results, and the three mutants —, every
TAROK_EINVAL of the two new entry points (before any HIP call), every ValueError of playout.card_player(net_versus=...),
evaluate_playout_vs_bot(net_versus=...) and SelfPlay(teacher=dict(versus=...)), the new surface, and what card_player
returns without the keyword.  No GPU involved."""
import ctypes
import inspect
import struct

import numpy as np
import pytest

import playout_net_versus_cases as XC
import playout_net_versus_model as XM
from playout_net_cases import Calls, WithHistory, no_device, weights

SEEN = dict(mutants=set())


@pytest.fixture(scope="module")
def W():
    return XC.weight_sets()


def test_the_role_function_of_the_model():
    assert [XM.role(v, v, 1, 14) for v in range(4)] == [XM.A] * 4
    assert [XM.role(v, (v + r) & 3, 1, 14) for v in range(4) for r in (1, 2, 3)] == [XM.B] * 12
    assert [XM.role(2, s, 3, 8) for s in range(4)] == [XM.BOT, XM.B, XM.A, XM.A]          # r = 2, 3, 0, 1
    assert [XM.role(2, s, 3, 8, "absolute") for s in range(4)] == [XM.A, XM.A, XM.BOT, XM.B]
    assert XM.viewer_net(14) == XM.A and XM.viewer_net(1) == XM.B and XM.viewer_net(0) == XM.A
    for m in range(16):
        for v in range(4):
            assert [XM.role(v, s, XC.rotate(m, v), 0) for s in range(4)] == [(m >> s) & 1 for s in range(4)]
    with pytest.raises(AssertionError):
        XM.role(0, 0, 3, 1)


@pytest.mark.parametrize("kind,at", XC.CASES)
def test_versus_rows_differ_from_both_single_network_results(W, kind, at):
    """(1, 14) at depth 1, five games and three worlds of every case, against (15, 0) — A alone — and (0, 15) — B alone.
    After the candidate the seats other than the viewer play B in (1, 14) and in (0, 15), A in (15, 0); the viewer plays A
    in (1, 14) and (15, 0), B in (0, 15), and its stop value comes from its own network.  So wherever a card is left to
    choose or an item stops, the versus rows differ from both — asserted for every case with at least two tricks to play.
    After 44 cards the candidate opens the last trick: every later card is forced and the viewer never moves again, so no
    item stops and the three launches are provably EQUAL; that is asserted instead."""
    cards = XC.POSITIONS[kind][at][1]
    games, words, sums, acts, info = XC.model(kind, at, 5, 3, W, 1, 14, 1)
    _, _, only_a, _, _ = XC.model(kind, at, 5, 3, W, 15, 0, 1)
    _, _, only_b, _, _ = XC.model(kind, at, 5, 3, W, 0, 15, 1)
    assert sums.any()
    if cards >= 44:
        assert not any(d["stopped"] for _, d in info)
        assert (sums == only_a).all() and (sums == only_b).all()
        return
    assert (sums != only_a).any(axis=(1, 2)).sum() >= 1, "no game tells (1, 14) from A alone"
    assert (sums != only_b).any(axis=(1, 2)).sum() >= 1, "no game tells (1, 14) from B alone"
    assert any(d["stopped"] for _, d in info)
    for rule in XM.RULES[1:]:
        _, _, mutant, _, _ = XC.model(kind, at, 5, 3, W, 1, 14, 1, rule=rule)
        if (mutant != sums).any():
            SEEN["mutants"].add((rule, kind, at))


def test_each_mutant_changes_some_row():
    """Over the cases above: absolute roles, swapped networks and the stop value from the other network each change a row
    of (1, 14) at depth 1.  (Absolute roles ARE the relative ones in a case whose viewers all sit on seat 0 — the fresh
    deals led by seat 0 —, so no single case is asked to show all three; the swap and the other network's value change a
    row in every case with at least two tricks to play.)"""
    cases = {(kind, at) for kind, at in XC.CASES if XC.POSITIONS[kind][at][1] < 44}
    if {(k, a) for _, k, a in SEEN["mutants"]} != cases:
        return                                        # (a partial run: the guard is the whole module's)
    for rule in XM.RULES[1:]:
        assert any(r == rule for r, _, _ in SEEN["mutants"]), rule
    for rule in ("swapped", "other"):
        assert {(k, a) for r, k, a in SEEN["mutants"] if r == rule} == cases, rule


def test_mixed_roles_meet_both_networks_and_depth_0_never_stops(W):
    """(3, 8) after 9 cards: some item meets positions of A and of B and a Bot seat; depth 0 stops nothing and depth 12
    gives its rows; (14, 1) takes the stop value from B, (1, 14) from A."""
    games, words, sums0, _, info0 = XC.model("det", 1, 5, 3, W, 3, 8, 0)
    assert any(d["both"] for _, d in info0) and not any(d["stopped"] for _, d in info0)
    _, _, sums12, _, _ = XC.model("det", 1, 5, 3, W, 3, 8, 12)
    assert (sums0 == sums12).all()
    _, _, _, _, a = XC.model("det", 1, 5, 3, W, 1, 14, 1)
    _, _, _, _, b = XC.model("det", 1, 5, 3, W, 14, 1, 1)
    va = [d["v"] for _, d in a if d["stopped"]]
    vb = [d["v"] for _, d in b if d["stopped"]]
    assert len(va) >= 4 and len(vb) >= 4
    # A's value row has b3[54] = 3.5 and |W3[54]| <= 2^-7 over 256 bf16 activations of set R; B's has b3[54] = -2.25 on 0 / 1
    # activations, at most 256 * 2^-7 = 2 away from it: B's values are negative, and never a value of A's
    assert all(v < 0 for v in vb) and not set(va) & set(vb)


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


def role_refusals(z):
    """What both entries refuse of the roles and of B, as changes of a good argument set."""
    bad = [dict(own=16), dict(own=-1), dict(opp=16), dict(opp=-1), dict(own=1, opp=1), dict(own=15, opp=8), dict(own=3, opp=6)]
    return bad + [dict(b=i) for i in range(6)]


def test_the_dense_launch_validates_before_any_hip_call(L):
    """Every refusal comes before the first HIP call: a zeroed stand-in for an env (no GPU, no tarok_create) is enough."""
    z = ctypes.c_void_p(0)
    keep, env = stand_in_env(0)
    buf = ctypes.create_string_buffer(512)
    out = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    f = L.tarok_playout_cards_net_versus
    for kind in (0, 1, 2):
        ok = dict(env=env, worlds=3, seats=15, kind=kind, words=z if kind == 0 else out, own=1, opp=14, depth=1, scale=70.0, a=[out] * 6,
                  b=[out] * 6, scr=out, size=0, sum=out, act=out)

        def rc(**ch):
            a = dict(ok, **ch)
            if isinstance(a["b"], int):
                a["b"] = [out] * a["b"] + [z] + [out] * (5 - a["b"])
            return f(a["env"], a["worlds"], 0, a["seats"], z, a["kind"], a["words"], a["own"], a["opp"], a["depth"], a["scale"], *a["a"], *a["b"],
                     a["scr"], a["size"], a["sum"], a["act"], z)
        bad = [dict(env=None), dict(worlds=0), dict(worlds=65), dict(seats=16), dict(seats=-1), dict(kind=3, words=out), dict(kind=-1, words=z),
               dict(depth=-1), dict(depth=13), dict(scale=float("nan")), dict(scale=float("inf")), dict(scale=0.0), dict(scale=-1.0),
               dict(scale=0.0, depth=0), dict(scr=z), dict(scr=ctypes.c_void_p(out.value + 8)), dict(size=-1), dict(sum=z, act=z)]
        bad += [dict(words=out)] if kind == 0 else [dict(words=z)]
        bad += [dict(a=[out] * i + [z] + [out] * (5 - i)) for i in range(6)] + role_refusals(z)
        bad += [dict(own=15, opp=0, a=[out] * i + [z] + [out] * (5 - i), b=[z] * 6) for i in range(6)]
        for ch in bad:
            assert rc(**ch) == -1, (kind, ch)
        big_keep, big = stand_in_env(1 << 20)
        assert rc(env=big, size=(1 << 20) * 12 * 3 * 48 - 1) == -1, kind                 # a short scratch


def test_the_halving_launch_validates_before_any_hip_call(L):
    z = ctypes.c_void_p(0)
    keep, env = stand_in_env(0)
    buf = ctypes.create_string_buffer(512)
    out = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    arr = lambda *w: (ctypes.c_int * len(w))(*w)
    f = L.tarok_playout_cards_net_versus_halving
    need = L.tarok_playout_net_halving_scratch_bytes(env, 2, arr(2, 2))
    assert need == 16
    for kind in (0, 1, 2):
        ok = dict(env=env, kind=kind, words=z if kind == 0 else out, rounds=2, rw=arr(2, 2), seats=15, own=1, opp=14, a=[out] * 6, b=[out] * 6,
                  depth=1, scale=70.0, scr=out, size=need, sum=out, cnt=out, act=out)

        def rc(**ch):
            a = dict(ok, **ch)
            if isinstance(a["b"], int):
                a["b"] = [out] * a["b"] + [z] + [out] * (5 - a["b"])
            return f(a["env"], a["kind"], a["words"], a["rounds"], a["rw"], 0, a["seats"], z, a["own"], a["opp"], *a["a"], *a["b"], a["depth"],
                     a["scale"], a["scr"], a["size"], a["sum"], a["cnt"], a["act"], z)
        bad = [dict(env=None), dict(rounds=0), dict(rounds=5, rw=arr(1, 1, 1, 1, 1)), dict(rw=z), dict(rw=arr(2, 0)), dict(rw=arr(2, -1)),
               dict(rw=arr(32, 33)), dict(rounds=1, rw=arr(65)), dict(kind=3, words=out), dict(kind=-1, words=z),
               dict(words=out if kind == 0 else z), dict(seats=16), dict(seats=-1), dict(depth=-1), dict(depth=13),
               dict(scale=float("nan")), dict(scale=float("inf")), dict(scale=0.0), dict(scale=-1.0), dict(scr=z),
               dict(scr=ctypes.c_void_p(out.value + 8)), dict(size=need - 1), dict(size=-1), dict(sum=z, cnt=z, act=z)]
        bad += [dict(a=[out] * i + [z] + [out] * (5 - i)) for i in range(6)] + role_refusals(z)
        for ch in bad:
            assert rc(**ch) == -1, (kind, ch)
        big_keep, big = stand_in_env(1 << 24)
        assert rc(env=big, rounds=1, rw=arr(16), size=1 << 62) == -1, kind           # a round bound at or above 2^31


def test_the_card_player_rules_and_the_surface():
    from tarok_amd import _native
    from tarok_amd import evaluate as EV
    from tarok_amd import playout as P
    from tarok_amd import selfplay as SP
    from tarok_amd.env import TarokVecEnv
    assert "tarok_playout_cards_net_versus" in _native.SYMBOLS and "tarok_playout_cards_net_versus_halving" in _native.SYMBOLS
    sig = inspect.signature(TarokVecEnv.playout_cards_net_versus).parameters
    assert list(sig)[1:] == ["weights", "opponent", "worlds", "own_rel", "opp_rel", "depth", "value_scale", "voids", "hidden", "words", "halving",
                             "salt", "seats", "seats_per_game", "sum_out", "action_out", "count_out"]
    assert [sig[k].default for k in list(sig)[4:]] == [1, 14, None, 70.0, False, False, None, None, 0, 15, None, None, None, None]
    assert inspect.signature(P.card_player).parameters["net_versus"].default is None
    for fn in (EV.evaluate_playout_vs_bot, EV._playout_passes):
        assert inspect.signature(fn).parameters["net_versus"].default is None and inspect.signature(fn).parameters["net_opponent"].default is None
    # what the call returns without the keyword: the parent's tuples, field for field
    assert P.CardPlayer._fields[:8] == ("kind", "worlds", "samples", "net", "net_seats", "depth", "value_scale", "salt")
    assert P.CardPlayer._fields[8:10] == ("halving", "versus") and P.CardPlayer._fields[10:] == ("modes",)      # one class holds them all
    assert P.card_player(4) == P.CardPlayer("open", None, 4, False, 15, None, 70.0, 0)
    assert P.card_player(2, 3, voids=True, salt=5) == P.CardPlayer("voids", 3, 2, False, 15, None, 70.0, 5)
    assert P.card_player(None, 3, net=True) == P.CardPlayer("det", 3, 1, True, 15, None, 70.0, 0)
    assert P.card_player(None, 3, net=True, net_versus=None) == P.card_player(None, 3, net=True)
    p = P.card_player(None, 3, net=True, net_seats="own", net_worlds="hidden", net_depth=2, net_value_scale=35.0)
    assert p.launch_kind == "net_value" and p == ("hidden", 3, 1, True, "own", 2, 35.0, 0, None, None, None)
    p = P.card_player(None, None, net=True, net_halving=(1, 2), net_seats=5)
    assert p.launch_kind == "net_halving" and p == ("det", 3, 1, True, 5, None, 70.0, 0, (1, 2), None, None)
    p = P.card_player(2, None, halving=(1, 2), hidden=True)
    assert p.launch_kind == "halving" and p == ("hidden", 3, 2, False, 15, None, 70.0, 0, (1, 2), None, None)
    # with it
    p = P.card_player(None, 3, net=True, net_versus=(1, 14), net_worlds="voids", net_depth=3, salt=7)
    assert p.launch_kind == "versus" and p == ("voids", 3, 1, True, 15, 3, 70.0, 7, None, (1, 14), None)
    assert p.needs_history and p.playouts == 3 and p.halving is None
    p = P.card_player(None, None, net=True, net_versus=[3, 8], net_halving=(1, 2))
    assert p.launch_kind == "versus" and p.counts and (p.worlds, p.halving, p.versus, p.kind) == (3, (1, 2), (3, 8), "det")
    net = dict(net=True, worlds=3)
    for kw in (dict(net_versus=(1, 14), worlds=3, samples=1),                                   # requires net=
               dict(net, net_versus=(1, 1)), dict(net, net_versus=(15, 8)), dict(net, net_versus=(16, 0)), dict(net, net_versus=(0, -1)),
               dict(net, net_versus=(1,)), dict(net, net_versus=(1, 2, 4)), dict(net, net_versus=5), dict(net, net_versus=(1.0, 14)),
               dict(net, net_versus=(True, 14)), dict(net, net_versus="own"),
               dict(net, net_versus=(1, 14), net_seats=1), dict(net, net_versus=(1, 14), net_seats="own"),
               dict(net, net_versus=(1, 14), samples=2), dict(net, net_versus=(1, 14), front=True), dict(net, net_versus=(1, 14), voids=True),
               dict(net, net_versus=(1, 14), hidden=True), dict(net, net_versus=(1, 14), net_worlds="hidden", history=False),
               dict(net, net_versus=(1, 14), net_depth=0), dict(net, net_versus=(1, 14), fused=False),
               dict(net=True, net_versus=(1, 14)),                                              # no worlds
               dict(net, net_versus=(1, 14), net_halving=(1, 1)), dict(net, net_versus=(1, 14), halving=(1, 2))):
        with pytest.raises(ValueError):
            P.card_player(**kw)
    w = weights()
    for kw in (dict(net_versus=(1, 14), net_opponent=w), dict(net=w, worlds=2, net_opponent=w), dict(net=w, worlds=2, net_versus=(1, 14)),
               dict(net=w, worlds=2, net_versus=(1, 1), net_opponent=w), dict(net=w, worlds=2, net_versus=(1, 14), net_opponent=w, net_seats=1),
               dict(net=w, worlds=2, net_versus=(1, 14), net_opponent=w, exchange=2), dict(net=w, worlds=2, net_versus=(1, 14), net_opponent=w[:5])):
        with pytest.raises(ValueError):
            EV.evaluate_playout_vs_bot(None if "net" in kw else 1, 8, 1, **kw)
    snap = weights()
    for tc, more in ((dict(net=True, worlds=2, versus=(1, 14)), {}),                            # no opponent
                     (dict(net=True, worlds=2, versus=(1, 14)), dict(opponent=[snap, snap])),   # a pool
                     (dict(net=True, worlds=2, versus=(1, 14)), dict(opponent=[snap])),         # a pool of one is a pool
                     (dict(net=True, worlds=2, versus=(1, 1)), dict(opponent=snap)),
                     (dict(net=True, worlds=2, versus=(1, 14), net_seats=1), dict(opponent=snap)),
                     (dict(worlds=2, samples=1, versus=(1, 14)), dict(opponent=snap)),          # requires net=True
                     (dict(net=True, versus=(1, 14)), dict(opponent=snap)),                     # no worlds
                     (dict(net=True, worlds=2, versus=(1, 14), net_halving=(1, 2)), dict(opponent=snap))):
        with pytest.raises(ValueError):
            SP.SelfPlay(WithHistory(), hidden=256, teacher=tc, **more)


def test_the_env_method_issues_the_launch():
    """TarokVecEnv.playout_cards_net_versus on a stand-in env: the dense entry with the kind as a number, depth 0 for None,
    A's six pointers before B's, the cached scratch at its size; halving= issues the second entry with the schedule as a
    host array and the count output; opponent None gives six NULLs where opp_rel is 0."""
    import torch
    from tarok_amd.env import TarokVecEnv

    class Env:
        n, device, _h = 4, torch.device("cpu"), 77
        check_mlp_weights = staticmethod(TarokVecEnv.check_mlp_weights)
        shown_voids, played_cards, _dev, _empty = TarokVecEnv.shown_voids, TarokVecEnv.played_cards, TarokVecEnv._dev, TarokVecEnv._empty

        def __init__(self, history):
            self.L, self.history, self.asked = Calls(), history, []

        def playout_net_scratch(self, worlds):
            self.asked.append(worlds)
            return torch.zeros(500, dtype=torch.uint8)

        def playout_net_halving_scratch(self, schedule):
            self.asked.append(schedule)
            return torch.zeros(1000, dtype=torch.uint8)

        def _p(self, t):
            return None if t is None else "%s%s" % (str(t.dtype).replace("torch.", ""), list(t.shape))

        def _seat_sets(self, s):
            return s

        def _stream(self):
            return "stream"
    a, b = weights(), weights()
    w = "'bfloat16[256, 256]', 'float32[256]', 'bfloat16[256, 256]', 'float32[256]', 'bfloat16[64, 256]', 'float32[64]'"
    with no_device():
        env = Env(False)
        out = TarokVecEnv.playout_cards_net_versus(env, a, b, 3, salt=3, seats=9)
        assert len(out) == 2 and env.asked == [3] and env.L.calls == [
            "tarok_playout_cards_net_versus(77, 3, 3, 9, None, 0, None, 1, 14, 0, 70.0, %s, %s, 'uint8[500]', 500, 'int32[4, 12, 4]', 'uint8[4]', "
            "'stream')" % (w, w)], env.L.calls
        env = Env(False)
        TarokVecEnv.playout_cards_net_versus(env, a, None, 2, 15, 0, depth=3, value_scale=0.5)
        assert env.L.calls[0].startswith("tarok_playout_cards_net_versus(77, 2, 0, 15, None, 0, None, 15, 0, 3, 0.5, %s, %s, 'uint8[500]'"
                                         % (w, ", ".join(["None"] * 6))), env.L.calls
        env = Env(True)
        out = TarokVecEnv.playout_cards_net_versus(env, a, b, None, 3, 8, voids=True, halving=[2, 2, 4], words=torch.zeros(4, dtype=torch.int32))
        assert len(out) == 3 and env.asked == [(2, 2, 4)] and env.L.calls[0] == "tarok_shown_voids(77, 'int32[4]', 'stream')"
        assert env.L.calls[1].startswith("tarok_playout_cards_net_versus_halving(77, 1, 'int32[4]', 3, <")
        assert env.L.calls[1].endswith(">, 0, 15, None, 3, 8, %s, %s, 0, 70.0, 'uint8[1000]', 1000, 'int32[4, 12, 4]', 'int32[4, 12]', 'uint8[4]', "
                                       "'stream')" % (w, w)), env.L.calls[1]
        for bad in (dict(own_rel=3, opp_rel=1), dict(own_rel=16), dict(opp_rel=-1), dict(voids=True, hidden=True), dict(depth=0), dict(depth=13),
                    dict(value_scale=0.0, depth=1), dict(halving=(0, 2)), dict(halving=(1, 1)), dict(count_out=torch.zeros(4, 12, dtype=torch.int32))):
            with pytest.raises(ValueError):
                TarokVecEnv.playout_cards_net_versus(Env(True), a, b, 3, **bad)
        with pytest.raises(ValueError):
            TarokVecEnv.playout_cards_net_versus(Env(True), a, None, 3)                          # opp_rel = 14 without an opponent
        with pytest.raises(ValueError):
            TarokVecEnv.playout_cards_net_versus(Env(False), a, b, 3, hidden=True)               # no history


def test_the_doors_issue_the_launch():
    """A versus player's launch, evaluate's wiring and SelfPlay's teacher on stand-ins: playout_cards_net_versus with A, then B,
    the roles, the kind and the schedule; the teacher reads the rollout weights as A and the opponent's own tensors as B."""
    import torch
    from tarok_amd import playout as P
    from tarok_amd import selfplay as SP

    class Env(Calls):
        n, history = 4, True
    env = Env()
    p = P.card_player(None, 3, net=True, net_versus=(1, 14), net_worlds="hidden", net_depth=2, net_value_scale=35.0, salt=7)
    p.prepare(env)
    p.launch(env, ("A", "B"), dict(seats=4), "W", "S", "C")
    assert env.calls == ["playout_net_scratch(3)",
                         "playout_cards_net_versus('A', 'B', 3, 1, 14, action_out='C', depth=2, halving=None, hidden=True, salt=7, seats=4, "
                         "sum_out='S', value_scale=35.0, voids=False, words='W')"], env.calls
    env = Env()
    p = P.card_player(None, None, net=True, net_versus=(3, 8), net_halving=(1, 2))
    p.prepare(env)
    p.launch(env, ("A", "B"), dict(seats_per_game="G"), None, "S", "C", count_out="N")
    assert env.calls == ["playout_net_halving_scratch((1, 2))",
                         "playout_cards_net_versus('A', 'B', 3, 3, 8, action_out='C', count_out='N', depth=None, halving=(1, 2), hidden=False, "
                         "salt=0, seats_per_game='G', sum_out='S', value_scale=70.0, voids=False, words=None)"], env.calls
    tc = dict(net=True, worlds=2, versus=(1, 14), tau=8.0, salt=11, depth=2)
    sp = SP.SelfPlay.__new__(SP.SelfPlay)
    try:
        sp.__init__(WithHistory(), hidden=256, teacher=tc, reward_scale=0.25, opponent=weights())
    except (AttributeError, TypeError):                      # (the stand-in is no env: the teacher is read first)
        pass
    assert sp.teacher == dict(worlds=2, samples=1, tau=8.0, every=1, salt=11, voids=False, hidden=False, net=True, net_seats=15, net_worlds="det",
                              depth=2, versus=(1, 14))
    sp2 = SP.SelfPlay.__new__(SP.SelfPlay)
    try:
        sp2.__init__(WithHistory(), hidden=256, teacher=dict(net=True, worlds=2, tau=8.0), opponent=weights())
    except (AttributeError, TypeError):
        pass
    assert "versus" not in sp2.teacher and sp2._player.versus is None and sp2._player.launch_kind == "net"      # without the key: as before
    opp = [torch.zeros(1)] * 6
    sp.env, sp.device, sp.fused, sp._w, sp._opp, sp._seats, sp.reward_scale = Env(), torch.device("cpu"), True, weights(), opp, None, 0.25
    sp._alloc(3)
    assert sp.env.calls == ["playout_net_scratch(2)"]
    del sp.env.calls[:]
    sp._teach(1)
    assert len(sp.env.calls) == 2 and sp.env.calls[1].startswith("playout_targets(int32[4, 12, 4], int64[4], 2, 8.0,")
    six = "[" + ", ".join(["tensor([0.])"] * 6) + "]"                 # (a list is shown by its repr: the opponent's own six tensors)
    assert sp.env.calls[0].startswith("playout_cards_net_versus([tensor(") and sp.env.calls[0].endswith(
        "], %s, 2, 1, 14, action_out=uint8[4], depth=2, halving=None, hidden=False, salt=11, seats_per_game=None, sum_out=int32[4, 12, 4], "
        "value_scale=4.0, voids=False, words=None)" % six), sp.env.calls[0][-300:]
