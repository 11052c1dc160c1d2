"""CPU: the statement of tarok_playout_cards_net_sampled (tests/playout_net_sampled_model.py) on the plan of
tests/playout_net_sampled_cases.py — the mutants, and the ambiguity cap of the GPU test's own cases from the model alone —,
every TAROK_EINVAL of the new entry and of its scratch function (before any HIP call), the ValueErrors of
playout.card_player(net_sampled=...), evaluate_playout_vs_bot(net_samples=...), SelfPlay.evaluate and SelfPlay(teacher=...),
and what card_player returns without the keyword.  No GPU involved."""
import ctypes
import inspect
import struct

import numpy as np
import pytest

import playout_net_sampled_cases as SC
import playout_net_sampled_model as SM
from playout_net_cases import Calls, WithHistory, weights


@pytest.fixture(scope="module")
def W():
    return SC.weight_sets()


def test_each_mutant_changes_some_row(W):
    """Six games after 24 cards, 2 worlds x 2 samples, (1, 14) with A at temperature 1 and B at 0.5: the draw on the Bot's
    counter, `played` off by one, B's mode for A and the key without its sample bits each change a row; and with the sample
    bits dropped every row is even, two equal samples — the playout is then a function of the world alone."""
    games, words = SC.games_at("det", 24, 6)
    case = ("det", 24, 2, 2, (1, 14), (1.0, 0.0), (0.5, 0.0), 0)
    only = tuple(range(6))
    spec, _, margin, info = SC.model_rows(case, games, words, W, only=only)
    assert spec.any() and sum(d["draws"] for _, d in info) > 100
    for rule in SM.RULES[1:]:
        mutant, _, _, _ = SC.model_rows(case, games, words, W, rule=rule, only=only)
        assert (mutant != spec).any(), rule
    halves, _, _, _ = SC.model_rows(case, games, words, W, rule="nosample", only=only)
    assert (halves % 2 == 0).all() and (spec % 2 != 0).any()


def test_the_models_own_equalities(W):
    """What the header promises, on the model: epsilon 1 on both networks is the Bot's playout under the item's key (the sum of
    playout_model.one_playout over worlds x samples); temperature 0 at samples S is S times the samples = 1 rows."""
    import playout_det_model as DM
    import playout_model as PM
    from oracle import oracle as O
    games, words = SC.games_at("det", 24, 4)
    only = tuple(range(4))
    bot, _, margin, _ = SC.model_rows(("det", 24, 2, 3, (1, 14), (0.5, 1.0), (2.0, 1.0), 0), games, words, W, only=only)
    assert np.isinf(margin).all()
    want = np.zeros_like(bot)
    for g, (lanes, ep, gidx, _) in enumerate(games):
        game = O.Game.from_lanes(lanes)
        _, _, legal, played = PM.position(game)
        for w in range(2):
            world = DM.world_of(game, DM.world_key(SC.SEED, SC.SALT, gidx, ep, played, w))
            for j, c in enumerate(PM.cards_of(legal)):
                for k in range(3):
                    want[g, j] += PM.one_playout(world, c, DM.playout_key(SC.SEED, SC.SALT, gidx, ep, played, c, w, k), played)
    assert (bot == want).all()
    one, _, _, _ = SC.model_rows(("det", 24, 2, 1, (15, 0), (0.0, 0.0), (0.0, 0.0), 0), games, words, W, only=only)
    three, _, _, _ = SC.model_rows(("det", 24, 2, 3, (15, 0), (0.0, 0.0), (0.0, 0.0), 0), games, words, W, only=only)
    assert one.any() and (three == 3 * one).all()


@pytest.mark.parametrize("at", range(len(SC.TEMPERED)))
def test_the_ambiguity_stays_under_the_cap_from_the_model_alone(W, at):
    """For every case of the GPU test, on its own games: the rows that have a tempered draw within NEAR of a CDF edge are at
    most CAP of the rows with a card left to choose; after 44 cards nothing is left out (no draw decides a card)."""
    case = SC.TEMPERED[at]
    games, words = SC.games_at(case[0], case[1])
    sums, _, margin, info = SC.model_rows(case, games, words, W)
    out, choice = SC.left_out(case, games, margin)
    assert sums.any()
    if case[1] >= 44:
        assert not out.any() and not choice.any() and np.isinf(margin).all()
        return
    assert choice.sum() >= 20 and sum(d["draws"] for _, d in info) >= 500, "the case draws too little to mean anything"
    assert out.sum() <= SC.CAP * choice.sum(), (case, int(out.sum()), int(choice.sum()))


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


def test_the_scratch_function(L):
    keep, env = stand_in_env(300)
    f = L.tarok_playout_cards_net_sampled_scratch
    assert f(env, 2, 3) == 300 * 12 * 2 * 3 * 48 and f(env, 64, 1024) == 300 * 12 * 64 * 1024 * 48
    for worlds, samples in ((0, 1), (65, 1), (1, 0), (1, 1025), (-1, 1), (1, -1)):
        assert f(env, worlds, samples) == -1, (worlds, samples)
    assert f(None, 1, 1) == -1
    keep2, big = stand_in_env(1 << 20)
    assert f(big, 16, 10) == (1 << 20) * 12 * 160 * 48          # 2,013,265,920 items: under 2^31
    assert f(big, 16, 11) == -1 and f(big, 64, 1024) == -1      # 2^31 items and more


def test_the_launch_validates_before_any_hip_call(L):
    """Every refusal comes before the first HIP call: a zeroed stand-in for an env (no GPU, no tarok_create) is enough."""
    z = ctypes.c_void_p(0)
    keep, env = stand_in_env(0)
    buf = ctypes.create_string_buffer(512)
    out = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    f = L.tarok_playout_cards_net_sampled
    nan, inf = float("nan"), float("inf")
    for kind in (0, 1, 2):
        ok = dict(env=env, worlds=3, samples=2, seats=15, kind=kind, words=z if kind == 0 else out, own=1, opp=14, depth=1, scale=70.0,
                  ta=1.0, ea=0.0, tb=0.5, eb=0.25, a=[out] * 6, b=[out] * 6, scr=out, size=0, sum=out, act=out)

        def rc(**ch):
            a = dict(ok, **ch)
            if isinstance(a["b"], int):
                a["b"] = [out] * a["b"] + [z] + [out] * (5 - a["b"])
            return f(a["env"], a["worlds"], a["samples"], 0, a["seats"], z, a["kind"], a["words"], a["own"], a["opp"], a["depth"], a["scale"],
                     a["ta"], a["ea"], a["tb"], a["eb"], *a["a"], *a["b"], a["scr"], a["size"], a["sum"], a["act"], z)
        # everything the versus entry refuses
        bad = [dict(env=None), dict(worlds=0), dict(worlds=65), dict(seats=16), dict(seats=-1), dict(kind=3, words=out), dict(kind=-1, words=z),
               dict(depth=-1), dict(depth=13), dict(scale=nan), dict(scale=inf), dict(scale=0.0), dict(scale=-1.0),
               dict(scale=0.0, depth=0), dict(scr=z), dict(scr=ctypes.c_void_p(out.value + 8)), dict(size=-1), dict(sum=z, act=z)]
        bad += [dict(words=out)] if kind == 0 else [dict(words=z)]
        bad += [dict(a=[out] * i + [z] + [out] * (5 - i)) for i in range(6)] + [dict(b=i) for i in range(6)]
        bad += [dict(own=16), dict(own=-1), dict(opp=16), dict(opp=-1), dict(own=1, opp=1), dict(own=15, opp=8), dict(own=3, opp=6)]
        # samples, and what tarok_set_play_mode refuses, for either network (B's also where no seat plays it)
        bad += [dict(samples=0), dict(samples=-1), dict(samples=1025)]
        for t, e in (("ta", "ea"), ("tb", "eb")):
            bad += [{t: nan}, {t: -1.0}, {t: 1e-7}, {t: 2e6}, {t: inf}, {e: nan}, {e: -0.25}, {e: 1.5}, {e: inf}]
        bad += [dict(own=15, opp=0, tb=-1.0), dict(own=15, opp=0, b=[z] * 6, eb=2.0)]
        for ch in bad:
            assert rc(**ch) == -1, (kind, ch)
        big_keep, big = stand_in_env(1 << 20)
        assert rc(env=big, size=(1 << 20) * 12 * 3 * 2 * 48 - 1) == -1, kind            # a short scratch
        assert rc(env=big, worlds=16, samples=11, size=1 << 62) == -1, kind             # 2^31 items


def test_tarok_set_play_mode_refuses_the_same_modes(L):
    """The entry's mode checks are tarok_set_play_mode's: the same values pass and fail on a stand-in env."""
    keep, env = stand_in_env(0)
    nan, inf = float("nan"), float("inf")
    for t, e, ok in ((1.0, 0.0, True), (0.0, 1.0, True), (1e-6, 0.5, True), (1e6, 0.0, True), (nan, 0.0, False), (-1.0, 0.0, False),
                     (1e-7, 0.0, False), (2e6, 0.0, False), (inf, 0.0, False), (1.0, nan, False), (1.0, -0.25, False), (1.0, 1.5, False)):
        assert (L.tarok_set_play_mode(env, t, e) == 0) == ok, (t, e)
        from tarok_amd import playout as P
        if ok:
            assert P.check_play_mode(t, e) == (t, e)
        else:
            with pytest.raises(ValueError):
                P.check_play_mode(t, e)


def test_the_card_player_rules_and_the_surface():
    from tarok_amd import _native
    from tarok_amd import evaluate as EV
    from tarok_amd import playout as P
    from tarok_amd import selfplay as SP
    from tarok_amd.env import TarokVecEnv
    assert "tarok_playout_cards_net_sampled" in _native.SYMBOLS and "tarok_playout_cards_net_sampled_scratch" in _native.SYMBOLS
    sig = inspect.signature(TarokVecEnv.playout_cards_net_sampled).parameters
    assert list(sig)[1:] == ["weights", "opponent", "worlds", "samples", "own_rel", "opp_rel", "temperature", "epsilon", "opp_temperature",
                             "opp_epsilon", "depth", "value_scale", "voids", "hidden", "words", "salt", "seats", "seats_per_game", "sum_out",
                             "action_out"]
    assert [sig[k].default for k in list(sig)[5:]] == [15, 0, 1.0, 0.0, None, None, None, 70.0, False, False, None, 0, 15, None, None, None]
    # without the keyword: the parent's tuples, field for field
    assert inspect.signature(P.card_player).parameters["net_sampled"].default is None
    assert P.card_player(None, 3, net=True) == P.CardPlayer("det", 3, 1, True, 15, None, 70.0, 0)
    assert P.card_player(None, 3, net=True, net_sampled=None) == P.card_player(None, 3, net=True)
    p = P.card_player(None, 3, net=True, net_versus=(1, 14))
    assert p.launch_kind == "versus" and p == ("det", 3, 1, True, 15, None, 70.0, 0, None, (1, 14), None)
    assert P.CardPlayer._fields[8:] == ("halving", "versus", "modes") and len(P.CardPlayer._fields) == 11
    # with it
    p = P.card_player(None, 3, net=True, net_sampled=dict(samples=4, temperature=0.5))
    assert p.launch_kind == "sampled" and p == ("det", 3, 4, True, 15, None, 70.0, 0, None, (15, 0), (0.5, 0.0, 0.5, 0.0))
    assert p.playouts == 12 and p.halving is None and not p.needs_history
    p = P.card_player(None, 2, net=True, net_versus=(1, 14), net_worlds="hidden", net_depth=3, salt=7,
                      net_sampled=dict(epsilon=0.25, opp_temperature=2, opp_epsilon=0))
    assert p.launch_kind == "sampled" and p == ("hidden", 2, 1, True, 15, 3, 70.0, 7, None, (1, 14), (1.0, 0.25, 2.0, 0.0)) and p.needs_history
    net = dict(net=True, worlds=3)
    for kw in (dict(worlds=3, samples=1, net_sampled=dict(samples=2)),                                   # requires net=
               dict(net, net_sampled=dict(samples=0)), dict(net, net_sampled=dict(samples=1025)), dict(net, net_sampled=dict(samples=2.0)),
               dict(net, net_sampled=dict(samples=True)), dict(net, net_sampled=3), dict(net, net_sampled=dict(sample=2)),
               dict(net, net_sampled=dict(temperature=-1)), dict(net, net_sampled=dict(temperature=1e-7)), dict(net, net_sampled=dict(temperature=2e6)),
               dict(net, net_sampled=dict(temperature=float("nan"))), dict(net, net_sampled=dict(temperature="1")),
               dict(net, net_sampled=dict(epsilon=1.5)), dict(net, net_sampled=dict(epsilon=-0.1)), dict(net, net_sampled=dict(opp_temperature=-1)),
               dict(net, net_sampled=dict(opp_epsilon=2)),
               dict(net, net_sampled={}, net_seats=1), dict(net, net_sampled={}, net_seats="own"), dict(net, net_sampled={}, samples=2),
               dict(net, net_sampled={}, front=True), dict(net, net_sampled={}, voids=True), dict(net, net_sampled={}, fused=False),
               dict(net, net_sampled={}, net_worlds="voids", history=False), dict(net=True, net_sampled={}),
               dict(net, net_sampled={}, net_versus=(1, 1)), dict(net=True, net_sampled={}, net_halving=(1, 2)),
               dict(net=True, net_sampled={}, net_versus=(1, 14), net_halving=(1, 2))):
        with pytest.raises(ValueError):
            P.card_player(**kw)
    for kw, word in ((dict(net=True, net_sampled={}, net_halving=(1, 2)), "net_halving"), (dict(net, net_sampled={}, front=True), "exchange"),
                     (dict(net, net_sampled={}, front=True), "bidding")):
        with pytest.raises(ValueError, match=word):
            P.card_player(**kw)
    w = weights()
    for kw in (dict(worlds=2, net_samples=2), dict(net=w, worlds=2, net_samples=0), dict(net=w, worlds=2, net_temperature=-1.0),
               dict(net=w, worlds=2, net_epsilon=2.0), dict(net=w, worlds=2, net_samples=2, net_seats=1),
               dict(net=w, worlds=2, net_samples=2, net_halving=(1, 1)), dict(net=w, worlds=2, net_samples=2, exchange=2),
               dict(net=w, worlds=2, net_samples=2, net_versus=(1, 14)), dict(net=w, worlds=2, net_samples=2, net_opponent=w),
               dict(net=w, worlds=2, net_versus=(1, 14), net_opponent=w, net_opp_temperature=-2.0)):
        with pytest.raises(ValueError):
            EV.evaluate_playout_vs_bot(None if "net" in kw else 1, 8, 1, **kw)
    snap = weights()
    for tc, more in ((dict(worlds=2, samples=2, temperature=1.0), {}),                                   # requires net=True
                     (dict(net=True, worlds=2, samples=3), {}),                                          # no play-mode key: as before, refused
                     (dict(net=True, worlds=2, samples=0, temperature=1.0), {}), (dict(net=True, worlds=2, temperature=-1.0), {}),
                     (dict(net=True, worlds=2, epsilon=1.5), {}), (dict(net=True, worlds=2, temperature=1.0, net_seats=1), {}),
                     (dict(net=True, temperature=1.0, net_halving=(1, 2)), {}),
                     (dict(net=True, worlds=2, temperature=1.0, versus=(1, 14)), {}),                    # versus without an opponent
                     (dict(net=True, worlds=2, temperature=1.0, versus=(1, 14), opp_temperature=1e7), dict(opponent=snap))):
        with pytest.raises(ValueError):
            SP.SelfPlay(WithHistory(), hidden=256, teacher=tc, **more)


def test_the_doors_issue_the_launch():
    """A sampled player's launch and SelfPlay's teacher on stand-ins: playout_cards_net_sampled with A, then B, the sizes, the
    roles and the modes; a versus teacher that leaves the opponent's mode open takes the env's play mode when it launches; a
    teacher dict without the new keys is the parent's."""
    import torch
    from tarok_amd import playout as P
    from tarok_amd import selfplay as SP

    class Env(Calls):
        n, history, play_mode = 4, True, (0.75, 0.125)
    env = Env()
    p = P.card_player(None, 3, net=True, net_versus=(1, 14), net_worlds="hidden", net_depth=2, net_value_scale=35.0, salt=7,
                      net_sampled=dict(samples=4, temperature=0.5, opp_epsilon=0.25))
    p.prepare(env)
    p.launch(env, ("A", "B"), dict(seats=4), "W", "S", "C")
    assert env.calls == ["playout_net_sampled_scratch(3, 4)",
                         "playout_cards_net_sampled('A', 'B', 3, 4, 1, 14, action_out='C', depth=2, epsilon=0.0, hidden=True, opp_epsilon=0.25, "
                         "opp_temperature=0.5, salt=7, seats=4, sum_out='S', temperature=0.5, value_scale=35.0, voids=False, words='W')"], env.calls

    def teacher_of(tc, **more):
        sp = SP.SelfPlay.__new__(SP.SelfPlay)
        try:
            sp.__init__(WithHistory(), hidden=256, teacher=tc, reward_scale=0.25, **more)
        except (AttributeError, TypeError):                  # (the stand-in is no env: the teacher is read first)
            pass
        return sp
    sp = teacher_of(dict(net=True, worlds=2, samples=3, temperature=1.0, versus=(1, 14), tau=8.0), opponent=weights())
    assert sp._player.launch_kind == "sampled" and sp._player.playouts == 6
    assert sp.teacher == dict(worlds=2, samples=3, tau=8.0, every=1, salt=0, voids=False, hidden=False, net=True, net_seats=15, net_worlds="det",
                              versus=(1, 14), temperature=1.0, epsilon=0.0, opp_temperature=None, opp_epsilon=None)
    old = teacher_of(dict(net=True, worlds=2, tau=8.0, versus=(1, 14)), opponent=weights())
    assert old._player.launch_kind == "versus" and old._player.modes is None and "temperature" not in old.teacher                      # without the keys: as before
    opp = [torch.zeros(1)] * 6
    sp.env, sp.device, sp.fused, sp._w, sp._opp, sp._seats, sp.reward_scale = Env(), torch.device("cpu"), True, weights(), opp, None, 0.25
    sp._alloc(3)
    assert sp.env.calls == ["playout_net_sampled_scratch(2, 3)"]
    del sp.env.calls[:]
    sp._teach(1)
    assert len(sp.env.calls) == 2 and sp.env.calls[1].startswith("playout_targets(int32[4, 12, 4], int64[4], 6, 8.0,")
    assert ", 2, 3, 1, 14, " in sp.env.calls[0] and sp.env.calls[0].startswith("playout_cards_net_sampled([tensor(")
    assert "epsilon=0.0," in sp.env.calls[0] and "opp_epsilon=0.125," in sp.env.calls[0] and "opp_temperature=0.75," in sp.env.calls[0] \
        and " temperature=1.0," in sp.env.calls[0], sp.env.calls[0][-400:]
    # all four seats on the learner's own network: no opponent is read, and B's mode is A's
    solo = teacher_of(dict(net=True, worlds=2, samples=2, temperature=0.5, epsilon=0.25))
    assert solo._player.versus == (15, 0) and solo.teacher["samples"] == 2
    solo.env = Env()
    assert solo.teacher_modes() == (0.5, 0.25, 0.5, 0.25)
