"""CPU: the statement of tarok_playout_cards_net_halving (tests/playout_net_halving_model.py) on the CPU net model's games,
every TAROK_EINVAL of the two new entry points (before any HIP call), the scratch formula of the header, the rules of
playout.card_player(net_halving=...), the new signatures and the call sequences of the three doors with the launch stubbed.
No GPU involved."""
import ctypes
import inspect
import struct

import numpy as np
import pytest

import playout_halving_model as HM
import playout_model as PM
import playout_net_halving_model as NH
import playout_net_model as NM
from oracle import oracle as O
from oracle import tarok_spec as S
from playout_net_cases import Calls, WithHistory, no_device, weights, zero_net

SEED, EPISODE = 41, 3


def games(mix, n, cards, first=0):
    out = []
    for gidx in range(first, first + n):
        g = O.Game.synth(SEED, gidx, EPISODE, mix)
        key = O.game_key(SEED, gidx, EPISODE)
        for q in range(cards):
            if g.done:
                break
            assert g.step(O.policy_action(key, q, g.legal())) >= 0
        out.append((g.lanes(), EPISODE, gidx, None))
    return out


def test_one_round_and_prefix_properties_on_the_net_models_games():
    """Five games after 30 cards, the net model's single playouts at 7 worlds: a one-round schedule is the uniform sums and
    the uniform card; under (1, 2, 4) a row whose count is e is the uniform row at worlds = e, the counts are cumulative
    ends, the survivors shrink by halves, and the card is alive at the end."""
    gs = games(S.MIX_ALL, 5, 30)
    b3 = np.linspace(0.0, 1.0, 54)
    scores = NM.playout_scores(gs, SEED, 7, 15, 7, zero_net(b3), 15)            # [n, 12, 7, 4]
    assert scores.any()
    took_part = 0
    for g, (lanes, ep, gidx, _) in enumerate(gs):
        game = O.Game.from_lanes(lanes)
        if not PM.takes_part(game, 15):
            continue
        took_part += 1
        _, mover, legal, _ = PM.position(game)
        nlegal = len(PM.cards_of(legal))
        uniform = {e: scores[g, :, :e].sum(axis=1) for e in range(1, 8)}
        s, c, alive, flags = NH.walk([uniform[7]], nlegal, mover, (7,))
        assert (s == uniform[7]).all() and c[:nlegal].tolist() == [7] * nlegal and not c[nlegal:].any() and alive == list(range(nlegal))
        assert NH.card_rank(s, alive, mover) == min(range(nlegal), key=lambda j: (-int(uniform[7][j, mover]), j))
        s, c, alive, flags = NH.walk([uniform[1], uniform[3], uniform[7]], nlegal, mover, (1, 2, 4))
        want = HM.halve(scores[g][:, :, None, :], nlegal, mover, (1, 2, 4), 1)
        assert (s == want[0]).all() and (c == want[1]).all() and alive == want[2]
        for j in range(12):
            assert int(c[j]) in (0, 1, 3, 7) and (s[j] == (uniform[int(c[j])][j] if c[j] else 0)).all()
        assert all(c[j] == c.max() for j in alive) and flags["early"] == (nlegal <= 4) == (c.max() < 7)     # 4 -> 2 -> 1: no third round
    assert took_part >= 3
    assert NH.ALIVE_BOUNDS == (12, 6, 3, 2)
    assert abs(NH.item_fraction(12, (2, 2, 4, 8)) - 64 / 192) < 1e-12 and abs(NH.item_fraction(12, (4, 4, 4, 4)) - 92 / 192) < 1e-12


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


def formula(n, schedule):
    bound = max(n * a * w for a, w in zip((12, 6, 3, 2), schedule))
    return (48 * bound + 252 * n + 4 * ((n + 255) // 256) + 4 + 15) // 16 * 16


def test_the_scratch_bytes_formula_of_the_header(L):
    f = L.tarok_playout_net_halving_scratch_bytes
    arr = lambda *w: (ctypes.c_int * len(w))(*w)
    for n in (1, 17, 256, 257, 300, 65536):
        keep, env = stand_in_env(n)
        for schedule in ((1,), (16,), (2, 2, 4, 8), (4, 4, 4, 4), (1, 1), (1, 2, 4), (16, 16, 16, 16), (1, 1, 1, 61), (64,)):
            assert f(env, len(schedule), arr(*schedule)) == formula(n, schedule), (n, schedule)
    keep, env = stand_in_env(65536)
    assert f(env, 4, arr(2, 2, 4, 8)) == 48 * 65536 * 24 + 252 * 65536 + 4 * 256 + 16         # round 0 and round 1 tie at 24 a game
    assert f(None, 1, arr(1)) == -1
    for rounds, rw in ((0, arr(1)), (5, arr(1, 1, 1, 1, 1)), (2, arr(2, 0)), (2, arr(2, -1)), (2, arr(32, 33)), (1, arr(65)), (1, None)):
        assert f(env, rounds, rw) == -1, (rounds, list(rw) if rw else rw)
    keep, env = stand_in_env(1 << 24)                    # 2^24 games x 12 ranks x 16 worlds = 3 x 2^30 items: at least 2^31
    assert f(env, 1, arr(16)) == -1 and f(env, 1, arr(10)) > 0 and f(env, 2, arr(1, 22)) == -1
    keep, env = stand_in_env((1 << 31) // 12 + 1)        # the bound itself: n x 12 x 1 just reaches 2^31
    assert f(env, 1, arr(1)) == -1
    keep, env = stand_in_env((1 << 31) // 12)
    assert f(env, 1, arr(1)) == formula((1 << 31) // 12, (1,))


def test_the_launch_validates_before_any_hip_call(L):
    """Every refusal comes before the first HIP call: a zeroed stand-in for an env (no GPU, no tarok_create) is enough."""
    z = ctypes.c_void_p(0)
    keep, env = stand_in_env(0)
    buf = ctypes.create_string_buffer(512)
    out = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    arr = lambda *w: (ctypes.c_int * len(w))(*w)
    f = L.tarok_playout_cards_net_halving
    need = L.tarok_playout_net_halving_scratch_bytes(env, 2, arr(2, 2))
    assert need == 16
    for kind in (0, 1, 2):
        ok = dict(env=env, kind=kind, words=z if kind == 0 else out, rounds=2, rw=arr(2, 2), seats=15, net=15, w=[out] * 6, depth=1, scale=70.0,
                  scr=out, size=need, sum=out, cnt=out, act=out)

        def rc(**ch):
            a = dict(ok, **ch)
            return f(a["env"], a["kind"], a["words"], a["rounds"], a["rw"], 0, a["seats"], z, a["net"], *a["w"], a["depth"], a["scale"], a["scr"],
                     a["size"], a["sum"], a["cnt"], a["act"], z)
        bad = [dict(env=None), dict(rounds=0), dict(rounds=5, rw=arr(1, 1, 1, 1, 1)), dict(rw=z), dict(rw=arr(2, 0)), dict(rw=arr(2, -1)),
               dict(rw=arr(32, 33)), dict(rounds=1, rw=arr(65)), dict(kind=3, words=out), dict(kind=-1, words=z),
               dict(words=out if kind == 0 else z), dict(net=16), dict(net=-1), dict(seats=16), dict(seats=-1), dict(depth=-1), dict(depth=13),
               dict(scale=float("nan")), dict(scale=float("inf")), dict(scale=0.0), dict(scale=-1.0), dict(scr=z),
               dict(scr=ctypes.c_void_p(out.value + 8)), dict(size=need - 1), dict(size=-1), dict(sum=z, cnt=z, act=z)]
        bad += [dict(w=[out] * i + [z] + [out] * (5 - i)) for i in range(6)]
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
    assert "tarok_playout_cards_net_halving" in _native.SYMBOLS and "tarok_playout_net_halving_scratch_bytes" in _native.SYMBOLS
    sig = inspect.signature(TarokVecEnv.playout_cards_net_halving).parameters
    assert list(sig)[1:] == ["weights", "round_worlds", "net_seats", "voids", "hidden", "words", "depth", "value_scale", "salt", "seats",
                             "seats_per_game", "scratch", "sum_out", "count_out", "action_out"]
    assert [sig[k].default for k in list(sig)[3:]] == [15, False, False, None, None, 70.0, 0, 15, None, None, None, None, None]
    assert inspect.signature(P.card_player).parameters["net_halving"].default is None
    assert inspect.signature(EV.evaluate_playout_vs_bot).parameters["net_halving"].default is None
    assert inspect.signature(EV._playout_passes).parameters["net_halving"].default is None
    assert inspect.signature(SP.SelfPlay.evaluate).parameters["playout_net_halving"].default is None
    assert P.CardPlayer._fields[:8] == ("kind", "worlds", "samples", "net", "net_seats", "depth", "value_scale", "salt")
    assert P.CardPlayer._fields[8:] == ("halving", "versus", "modes")          # one class: the schedule is a field of every player
    p = P.card_player(None, None, net=True, net_halving=(2, 2, 4, 8), net_worlds="hidden", net_depth=3, net_seats=5, salt=3)
    assert isinstance(p, P.CardPlayer) and p.launch_kind == "net_halving" and p.counts
    assert (p.kind, p.worlds, p.samples, p.net, p.net_seats, p.depth, p.halving, p.salt, p.needs_history) == \
        ("hidden", 16, 1, True, 5, 3, (2, 2, 4, 8), 3, True)
    assert P.card_player(1, 16, net=True, net_halving=[2, 2, 4, 8]).kind == "det" and P.card_player(None, 0, net=True, net_halving=(3,)).worlds == 3
    assert P.card_player(None, 3, net=True) == P.CardPlayer("det", 3, 1, True, 15, None, 70.0, 0)      # without the keyword: as before
    assert P.card_player(None, None, net=True, net_halving=(1, 2), net_seats="own").net_seats == "own"
    net = dict(net=True, samples=None)
    for kw in (dict(net_halving=(1, 2)), dict(net_halving=(1, 2), worlds=3, samples=1),                    # net_halving requires net
               dict(net, net_halving=()), dict(net, net_halving=(1, 1, 1, 1, 1)), dict(net, net_halving=(0, 2)), dict(net, net_halving=(2.0, 1)),
               dict(net, net_halving=(True, 1)), dict(net, net_halving=3), dict(net, net_halving=(32, 33)),
               dict(net, net_halving=(1, 2), worlds=4), dict(net, net_halving=(1, 2), samples=2), dict(net, net_halving=(1, 2), front=True),
               dict(net, net_halving=(1, 2), voids=True), dict(net, net_halving=(1, 2), hidden=True),
               dict(net, net_halving=(1, 2), net_worlds="hidden", history=False), dict(net, net_halving=(1, 2), net_depth=0),
               dict(net, net_halving=(1, 2), net_seats=16), dict(net, net_halving=(1, 2), fused=False),
               dict(net, halving=(1, 2), worlds=3), dict(net, halving=(1, 2), net_halving=(1, 2))):        # halving= with net= keeps raising
        with pytest.raises(ValueError):
            P.card_player(**kw)
    w = weights()
    for kw in (dict(net_halving=(1, 2)), dict(net=w, net_halving=(1, 2), exchange=2), dict(net=w, net_halving=(1, 2), bidding=(2, 1)),
               dict(net=w, net_halving=(1, 2), worlds=2), dict(net=w, halving=(1, 2))):
        with pytest.raises(ValueError):
            EV.evaluate_playout_vs_bot(None if "net" in kw else 1, 8, 1, **kw)
    for kw in (dict(playout_net_halving=(1, 2), versus_playout=1), dict(playout_net=True, playout_net_halving=(1, 2), playout_worlds=2),
               dict(playout_net=True, playout_halving=(1, 2), versus_playout=1)):
        with pytest.raises(ValueError):
            SP.SelfPlay.evaluate(object(), **kw)
    for tc in (dict(net_halving=(1, 2), samples=1), dict(net=True, net_halving=(1, 2), worlds=2), dict(net=True, halving=(1, 2))):
        with pytest.raises(ValueError):
            SP.SelfPlay(WithHistory(), hidden=256, teacher=tc)


def test_the_env_method_issues_the_launch():
    """TarokVecEnv.playout_cards_net_halving on a stand-in env: the words launch where the env's own words are asked for,
    then tarok_playout_cards_net_halving with the kind as a number, the schedule as a host array, depth 0 for None, and the
    caller's scratch or the cached one at its size."""
    import torch
    from tarok_amd.env import TarokVecEnv

    class Env:
        n, device, _h = 4, torch.device("cpu"), 77
        check_mlp_weights = staticmethod(TarokVecEnv.check_mlp_weights)
        shown_voids, played_cards, _dev, _empty = TarokVecEnv.shown_voids, TarokVecEnv.played_cards, TarokVecEnv._dev, TarokVecEnv._empty

        def __init__(self, history):
            self.L, self.history, self.asked = Calls(), history, []

        def playout_net_halving_scratch(self, schedule):
            self.asked.append(schedule)
            return torch.zeros(1000, dtype=torch.uint8)

        def _p(self, t):
            return None if t is None else "%s%s" % (str(t.dtype).replace("torch.", ""), list(t.shape))

        def _seat_sets(self, s):
            return s

        def _stream(self):
            return "stream"
    net = weights()
    w = "'bfloat16[256, 256]', 'float32[256]', 'bfloat16[256, 256]', 'float32[256]', 'bfloat16[64, 256]', 'float32[64]'"
    outs = "'int32[4, 12, 4]', 'int32[4, 12]', 'uint8[4]', 'stream')"
    with no_device():
        env = Env(False)
        TarokVecEnv.playout_cards_net_halving(env, net, (1, 2), net_seats=5, salt=3, seats=9)
        assert env.asked == [(1, 2)] and len(env.L.calls) == 1
        head, rest = env.L.calls[0].split(", <", 1)
        assert head == "tarok_playout_cards_net_halving(77, 0, None, 2" and rest.split(">, ", 1)[1] == \
            "3, 9, None, 5, %s, 0, 70.0, 'uint8[1000]', 1000, %s" % (w, outs), env.L.calls[0]
        env = Env(True)
        TarokVecEnv.playout_cards_net_halving(env, net, [2, 2, 4], voids=True, depth=3, value_scale=0.5, words=torch.zeros(4, dtype=torch.int32),
                                              scratch=torch.zeros(64, dtype=torch.uint8))
        assert env.asked == [] and env.L.calls[0] == "tarok_shown_voids(77, 'int32[4]', 'stream')"
        assert env.L.calls[1].startswith("tarok_playout_cards_net_halving(77, 1, 'int32[4]', 3, <")
        assert env.L.calls[1].endswith(">, 0, 15, None, 15, %s, 3, 0.5, 'uint8[64]', 64, %s" % (w, outs)), env.L.calls[1]
        for bad in (dict(voids=True, hidden=True), dict(net_seats=16), dict(depth=0), dict(depth=13), dict(value_scale=0.0, depth=1)):
            with pytest.raises(ValueError):
                TarokVecEnv.playout_cards_net_halving(Env(True), net, (1, 2), **bad)
        with pytest.raises(ValueError):
            TarokVecEnv.playout_cards_net_halving(Env(False), net, (1, 2), hidden=True)
        with pytest.raises(ValueError):
            TarokVecEnv.playout_cards_net_halving(Env(False), net, (0, 2))


def test_evaluate_issues_the_launch():
    """evaluate_playout_vs_bot(net=, net_halving=) on the stand-in env of tests/evaluate_calls_cases.py: the calls of the call
    without the keyword, with playout_cards_net_halving(W, schedule, net_seats, ..., count_out=...) in playout_cards_net's
    place; net_halving=None makes the calls as they were."""
    import evaluate_calls_cases as EC
    from tarok_amd import evaluate as EV
    new = dict(nh_none=("evaluate_playout_vs_bot", (None,), dict(worlds=3, net="W", net_seats=5), False),
               nh_off=("evaluate_playout_vs_bot", (None,), dict(worlds=3, net="W", net_seats=5, net_halving=None), False),
               nh_on=("evaluate_playout_vs_bot", (None,), dict(net="W", net_seats=5, net_halving=(1, 2)), False),
               nh_hidden=("evaluate_playout_vs_bot", (None,), dict(worlds=3, net="W", net_seats="own", net_halving=(1, 2), net_worlds="hidden",
                                                                  net_depth=2, net_value_scale=35.0), False))
    EC.CASES.update(new)
    try:
        traces = {k: EC.run_case(EV, k)[0].calls for k in new}
    finally:
        for k in new:
            del EC.CASES[k]
    assert traces["nh_off"] == traces["nh_none"]
    assert len(traces["nh_on"]) == len(traces["nh_none"])
    launches = 0
    for a, b in zip(traces["nh_on"], traces["nh_none"]):
        if b.startswith("playout_cards_net("):
            launches += 1
            assert a.startswith("playout_cards_net_halving(W0, (1, 2), 5, ") and "count_out=T" in a and "depth=None" in a and "salt=0" in a, a
            assert "hidden=False" in a and "voids=False" in a and "value_scale=70.0" in a and "words=None" in a
        else:
            assert a == b
    assert launches == 5 * EC.EPISODES * 48
    assert "history=True" in traces["nh_hidden"][0] and "history=False" in traces["nh_on"][0]
    deep = [c for c in traces["nh_hidden"] if c.startswith("playout_cards_net_halving(")]
    assert len(deep) == launches and all("depth=2" in c and "hidden=True" in c and "value_scale=35.0" in c and "words=T" in c for c in deep)
    assert {c.split(", ")[3] for c in deep} == {"0", "1", "2", "4", "8"}                   # "own": the pass's seat set


def test_selfplay_doors_issue_the_launch():
    """SelfPlay(teacher=dict(net=True, net_halving=...)) on a stand-in: the normalised teacher, the scratch and the counts
    buffer asked for in _alloc, and a lock-step's teacher = playout_cards_net_halving on the live weights, then
    playout_targets_counts.  SelfPlay.evaluate(playout_net=True, playout_net_halving=...) hands the schedule on."""
    import torch
    from tarok_amd import evaluate as EV
    from tarok_amd import selfplay as SP

    class Env(Calls):
        n, history = 4, True
    tc = dict(net=True, net_halving=(1, 2), worlds=None, tau=8.0, salt=11, net_worlds="voids", depth=2, net_seats=3)
    sp = SP.SelfPlay.__new__(SP.SelfPlay)
    try:
        sp.__init__(WithHistory(), hidden=256, teacher=tc, reward_scale=0.25)
    except (AttributeError, TypeError):                      # (the stand-in is no env: the teacher is read first)
        pass
    assert sp.teacher == dict(worlds=3, samples=1, tau=8.0, every=1, salt=11, voids=False, hidden=False, net=True, net_seats=3, net_worlds="voids",
                              depth=2, net_halving=(1, 2))
    sp.env, sp.device, sp.fused, sp._w, sp._seats, sp.reward_scale = Env(), torch.device("cpu"), True, weights(), None, 0.25
    sp._alloc(3)
    assert sp.env.calls == ["playout_net_halving_scratch((1, 2))"] and tuple(sp._teach_counts.shape) == (4, 12)
    del sp.env.calls[:]
    sp._teach(1)
    assert len(sp.env.calls) == 2 and sp.env.calls[1].startswith("playout_targets_counts(int32[4, 12, 4], int32[4, 12], int64[4], 8.0,")
    assert sp.env.calls[0].startswith("playout_cards_net_halving(") and sp.env.calls[0].endswith(
        "], (1, 2), 3, action_out=uint8[4], count_out=int32[4, 12], depth=2, hidden=False, salt=11, seats_per_game=None, "
        "sum_out=int32[4, 12, 4], value_scale=4.0, voids=True, words=int32[4])"), sp.env.calls[0][-260:]
    seen = []

    class Learner:
        fused, fused_learner, _w, reward_scale = True, True, weights(), 0.5
        env = type("E", (), dict(device_index=0))()
        is_pool = staticmethod(lambda o: False)
    saved = EV.evaluate_vs_bot, EV.evaluate_playout_vs_bot
    EV.evaluate_vs_bot = lambda *a, **k: "own"
    EV.evaluate_playout_vs_bot = lambda *a, **k: seen.append((a, k)) or "playout"
    try:
        out = SP.SelfPlay.evaluate.__wrapped__(Learner(), 8, 1, versus_playout=1, playout_net=True, playout_net_halving=(1, 2), playout_net_depth=2)
    finally:
        EV.evaluate_vs_bot, EV.evaluate_playout_vs_bot = saved
    assert out == ("own", "playout") and len(seen) == 1
    a, k = seen[0]
    assert a[0] is None and k["net_halving"] == (1, 2) and k["worlds"] is None and k["net_depth"] == 2 and k["net_value_scale"] == 2.0
    assert "halving" not in k
