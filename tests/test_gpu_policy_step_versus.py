"""GPU: tarok_policy_step_versus (network A on the seats of a set, network B on the others) and what is built on it —
TarokVecEnv.policy_step(opponent=...), evaluate.evaluate_vs_policy, SelfPlay.snapshot / evaluate(opponent=...) —
checked exactly.

A network's card, log-probability and value for a position are what a separate tarok_policy_mlp launch with its
weights on the same observation words reports (both networks draw with the same spec RNG draw).  So every row of a
versus launch has ONE right answer: the outputs of the launch selected by (set >> seat to move) & 1, and everything the
env half writes follows from that card through the per-slot model on the CPU oracle (tests/oracle_model.py).

Run on the GPU box:  python -m pytest tests/test_gpu_policy_step_versus.py -m gpu -q
"""
import math

import numpy as np
import pytest

from gpu_harness import T  # noqa: F401  (the module fixture)
from policy_step_cases import make_weights, versus

pytestmark = pytest.mark.gpu

STEPS = 64                               # lock-steps per case (games are 48 cards at most)
FIELDS = ("n", "mix", "auto", "reward_ref", "hist", "seats", "logp", "value", "words", "reward", "done", "trick")
# 773 games = four workgroups, the last with 5 games (a partial tile, clamped tail lanes); every slot is modelled.
# seats: a 4-bit set for every game, or "cycle": seats_per_game[i] = i % 16
CASES = [
    (773, "all", 0, 0, 1, 0, "given", "given", "given", "given", "given", "given"),
    (773, "berac", 1, 1, 0, 1, "given", "null", "given", "null", "given", "given"),
    (773, "all", 1, 0, 1, 6, "null", "given", "null", "given", "null", "given"),
    (773, "berac", 0, 1, 0, 15, "given", "given", "null", "given", "given", "null"),
    (773, "all", 1, 1, 0, "cycle", "given", "given", "given", "given", "given", "given"),
    (773, "berac", 0, 0, 1, "cycle", "null", "null", "null", "null", "null", "null"),
]


@pytest.fixture(scope="module")
def S():
    from oracle import tarok_spec
    return tarok_spec


@pytest.fixture(scope="module")
def nets(T):
    """(A, B): two different weight sets."""
    import torch
    A, B = make_weights(T, 0), make_weights(T, 1)
    assert not torch.equal(A[0], B[0])
    return A, B


def run_case(T, S, idx, case, nets):
    import torch
    from guarded import Guarded, assert_guards_intact
    from oracle_model import SlotModel
    from tarok_amd import karte as K
    from output_contract_cases import Outputs, check_against_models, modelled_slots
    from policy_step_cases import bits, seat_sets
    A, B = nets
    c = dict(zip(FIELDS, case))
    n, auto, ref = c["n"], bool(c["auto"]), bool(c["reward_ref"])
    seed, mix = 1700 + idx, (S.MIX_ALL if c["mix"] == "all" else S.MIX_FIXED + 7)
    flags = (K.AUTO_RESET if auto else 0) | (K.REWARD_REF if ref else 0)
    seats, per_game, sets = seat_sets(c["seats"], n)
    env = T.TarokVecEnv(n, seed=seed, mix=mix, history=bool(c["hist"]))
    try:
        p = env._p
        slots = modelled_slots(n)
        assert len(slots) == n                        # every slot is modelled
        models = [(int(i), SlotModel(seed, int(i), mix)) for i in slots]
        env.reset(episode=0)
        for _ in range(idx % 4):                      # lead-in: the launches start mid-trick
            env.step_random(auto_reset=auto)
            for _, m in models:
                m.card(None, auto)
        out = Outputs(1, n, n, slots, dict(action=True, reward=c["reward"] == "given", done=c["done"] == "given", trick=c["trick"] == "given"))
        g_logp = Guarded("logp_out", 1, n, np.uint32, device="cuda") if c["logp"] == "given" else None
        g_value = Guarded("value_out", 1, n, np.uint32, device="cuda") if c["value"] == "given" else None
        g_words = Guarded("feature_words_out", 1, n, np.uint64, inner=(4,), device="cuda") if c["words"] == "given" else None
        extra = [g_logp, g_value, g_words]
        ptr = lambda a: None if a is None else a.ptr
        per_dev = None if per_game is None else torch.from_numpy(per_game).cuda()
        fw = [torch.zeros((n, 4), dtype=torch.int64, device="cuda") for _ in range(2)]
        seen_a = seen_b = differ = differ_on_b = 0
        for t in range(STEPS):
            tag = (idx, case, "step", t)
            if not auto and t == 49:                  # every game is over: a second one from the start
                env.reset(episode=1)
                for _, m in models:
                    m.reset(1)
            out.begin_call()
            for a in extra:
                if a is not None:
                    a.fill()
            with torch.cuda.device(env.device):
                words = env.legal_actions().words
                # each network's card for this very position, from a launch of its own
                ref_out = []
                for k, W in enumerate((A, B)):
                    a_k, lp_k, v_k = env.policy_mlp(W, words, feature_words_out=fw[k])
                    ref_out.append((a_k.cpu().numpy(), lp_k.cpu().numpy(), v_k.cpu().numpy(), fw[k].cpu().numpy().view(np.uint64)))
                w_h = words.cpu().numpy().view(np.uint64)
                versus(env, seats, p(per_dev), A, B, p(words), out.action.ptr, ptr(g_logp), ptr(g_value), ptr(g_words), ptr(out.reward),
                       ptr(out.done), ptr(out.trick), out.obs.ptr, flags)
                torch.cuda.synchronize()
            (a_a, lp_a, v_a, fw_a), (a_b, lp_b, v_b, fw_b) = ref_out
            assert (fw_a == fw_b).all(), (tag, "the feature words do not depend on the weights")
            # ---- every game: card, logp and value of the launch selected by the seat to move of the observation word
            mover = ((w_h >> np.uint64(54)) & np.uint64(3)).astype(np.uint8)
            live = (w_h & np.uint64((1 << 54) - 1)) != 0
            is_a = ((sets >> mover) & 1).astype(bool)
            exp_a = np.where(live, np.where(is_a, a_a, a_b), 255).astype(np.uint8)
            assert (a_a[~live] == 255).all() and (a_b[~live] == 255).all(), tag
            acts, written = out.action.host()
            assert written.all(), (tag, "action_out rows not written")
            bad = np.nonzero(acts[0] != exp_a)[0]
            assert bad.size == 0, (tag, "action_out", int(bad[0]), int(acts[0][bad[0]]), int(exp_a[bad[0]]), len(bad))
            if g_logp is not None:
                got, written = g_logp.host()
                assert written.all(), (tag, "logp_out rows not written")
                exp = np.where(live, np.where(is_a, bits(lp_a), bits(lp_b)), np.uint32(0))
                bad = np.nonzero(got[0] != exp)[0]
                assert bad.size == 0, (tag, "logp_out", int(bad[0]), hex(int(got[0][bad[0]])), hex(int(exp[bad[0]])), len(bad))
            if g_value is not None:
                got, written = g_value.host()
                assert written.all(), (tag, "value_out rows not written")
                exp = np.where(is_a, bits(v_a), bits(v_b))
                bad = np.nonzero(got[0] != exp)[0]
                assert bad.size == 0, (tag, "value_out", int(bad[0]), hex(int(got[0][bad[0]])), hex(int(exp[bad[0]])), len(bad))
            if g_words is not None:
                got, written = g_words.host()
                assert written.all() and (got[0] == fw_a).all(), (tag, "feature_words_out")
            seen_a += int((live & is_a).sum())
            seen_b += int((live & ~is_a).sum())
            differ += int((live & (a_a != a_b)).sum())
            differ_on_b += int((live & ~is_a & (a_a != a_b)).sum())
            # ---- the modelled slots: the card is legal on the oracle, the whole env row follows from it
            for j, (i, m) in enumerate(models):
                legal = m.legal()
                a = int(exp_a[i])
                if legal:
                    assert bool(live[i]) and int(mover[i]) == m.g.seat(), (tag, "observation word", i)
                    assert a < 54 and (legal >> a) & 1, (tag, "tarok_policy_mlp's card is not legal", i, a, legal)
                else:
                    assert not live[i] and a == 255, (tag, "a card where nothing is to be played", i, a)
                out.expect(0, j, m.card(a, auto, ref))
            out.check(tag)
            assert_guards_intact(extra, tag)
            if env.history:
                hist = env.get_history().cpu().numpy()
                for i, m in models:
                    assert hist[:m.played, i].tolist() == m.hist[:m.played], (tag, "history", i)
        check_against_models(env, models, (idx, case, "end"))
        # the case did exercise what it is about
        assert differ > 0                             # the two networks chose different cards somewhere
        if c["seats"] != 0:
            assert seen_a > 0
        if c["seats"] != 15:
            assert seen_b > 0 and differ_on_b > 0     # ... on rows that B moved: always taking A's card cannot pass
    finally:
        env.close()


@pytest.mark.parametrize("idx", range(len(CASES)), ids=lambda i: "%02d-%s" % (i, "-".join(str(v) for v in CASES[i])))
def test_every_row_of_a_versus_launch_against_the_oracle_and_policy_mlp(T, S, nets, idx):
    run_case(T, S, idx, CASES[idx], nets)


@pytest.mark.parametrize("which", ["seats=15 with (A, B) is tarok_policy_step with A", "seats=0 with (A, B) is tarok_policy_step with B",
                                   "any seats with (A, A) is tarok_policy_step with A"])
def test_one_network_tables_reproduce_tarok_policy_step(T, S, nets, which):
    """Twin envs (20,077 games, MIX_ALL, history, TAROK_AUTO_RESET | TAROK_REWARD_REF), 60 lock-steps: every output of
    every launch and the state, counters, history and observation words at the end are bit-equal.  The seat set is
    given as `seats` on one env and as a per-game array on a third ((A, A): the cycle i % 16 and the set 6)."""
    import torch
    from tarok_amd import _native, karte as K
    from policy_step_cases import Twin
    A, B = nets
    n, seed, flags = 20077, 77, K.AUTO_RESET | K.REWARD_REF
    a, b, c = (Twin(T, n, seed, S.MIX_ALL) for _ in range(3))
    if which.startswith("seats=15"):
        plain, pair, val, per = A, (A, B), 15, torch.full((n,), 15, dtype=torch.uint8, device="cuda")
        other = 0                                     # (`seats` beside an array is ignored: any valid value)
    elif which.startswith("seats=0"):
        plain, pair, val, per = B, (A, B), 0, torch.zeros(n, dtype=torch.uint8, device="cuda")
        other = 15
    else:
        plain, pair, val, per = A, (A, A), 6, (torch.arange(n, device="cuda") % 16).to(torch.uint8)
        other = 9
    try:
        for t in range(60):
            for tw in (a, b, c):
                tw.clear()
            for tw, kind in ((a, "plain"), (b, "set"), (c, "array")):
                e, o = tw.env, tw.o
                p = e._p
                words = e.legal_actions().words
                with torch.cuda.device(e.device):
                    if kind == "plain":
                        _native.check(e.L.tarok_policy_step(e._h, *[p(w) for w in plain], p(words), p(o["action"]), p(o["logp"]), p(o["value"]),
                                                            p(o["words"]), p(o["reward"]), p(o["done"]), p(o["trick"]), p(o["obs"]), flags,
                                                            e._stream()))
                    else:
                        versus(e, val if kind == "set" else other, p(per) if kind == "array" else None, pair[0], pair[1], p(words),
                               p(o["action"]), p(o["logp"]), p(o["value"]), p(o["words"]), p(o["reward"]), p(o["done"]), p(o["trick"]),
                               p(o["obs"]), flags)
            torch.cuda.synchronize()
            for k in ("action", "logp", "value", "words", "reward", "done", "trick", "obs"):
                assert torch.equal(a.o[k], b.o[k]), (which, t, k, "seat set")
                assert torch.equal(a.o[k], c.o[k]), (which, t, k, "per-game array")
        ea, eb, ec = a.end_state(), b.end_state(), c.end_state()
        assert ea[1].sum() > n                        # games did finish and were replaced
        for x, y, z in zip(ea, eb, ec):
            assert (x == y).all() and (x == z).all(), which
    finally:
        for tw in (a, b, c):
            tw.env.close()


def test_env_policy_step_with_an_opponent(T, S, nets):
    """TarokVecEnv.policy_step(opponent=A) beside weights=A gives the rows of the plain call whatever the seat set;
    a bad seat set, aliased observation words and a wrong-dtype opponent tensor are refused."""
    import torch
    A, B = nets
    n = 773
    cycle = (torch.arange(n, device="cuda") % 16).to(torch.uint8)
    res = []
    for kw in (dict(), dict(opponent=A), dict(opponent=A, seats=6), dict(opponent=A, seats=0), dict(opponent=A, seats_per_game=cycle)):
        env = T.TarokVecEnv(n, seed=5, mix=S.MIX_ALL)
        try:
            words = [env.reset().words, torch.zeros(n, dtype=torch.int64, device="cuda")]
            act = torch.zeros((8, n), dtype=torch.uint8, device="cuda")
            logp = torch.zeros((8, n), dtype=torch.float32, device="cuda")
            value = torch.zeros((8, n), dtype=torch.float32, device="cuda")
            trick = torch.zeros((8, n), dtype=torch.int16, device="cuda")
            for t in range(8):
                env.policy_step(A, words[t & 1], words[(t + 1) & 1], act[t], logp[t], value[t], tricks=trick[t], **kw)
            res.append((act.cpu(), logp.cpu(), value.cpu(), trick.cpu(), env.state()))
            if kw:
                with pytest.raises(T.TarokNativeError):
                    env.policy_step(A, words[0], words[1], act[0], seats=16, opponent=B)
                with pytest.raises(T.TarokNativeError):
                    env.policy_step(A, words[0], words[0], act[0], seats=3, opponent=B)          # obs == obs_out
                with pytest.raises(ValueError):
                    env.policy_step(A, words[0], words[1], act[0], opponent=B, seats_per_game=torch.zeros(n, dtype=torch.int64, device="cuda"))
                wrong = list(B)
                wrong[2] = wrong[2].float()
                with pytest.raises((AssertionError, ValueError)):
                    env.policy_step(A, words[0], words[1], act[0], opponent=wrong)
                with pytest.raises((AssertionError, ValueError)):
                    env.policy_step(A, words[0], words[1], act[0], opponent=B[:5])
        finally:
            env.close()
    for r in res[1:]:
        for x, y in zip(res[0][:4], r[:4]):
            assert torch.equal(x, y)
        assert (res[0][4] == r[4]).all()
    assert (res[0][3] != 0).any()                     # trick rows were written (cards 4 and 8 complete tricks)
    # ... and with B as the opponent the table does go another way
    env = T.TarokVecEnv(n, seed=5, mix=S.MIX_ALL)
    try:
        words = [env.reset().words, torch.zeros(n, dtype=torch.int64, device="cuda")]
        act = torch.zeros((8, n), dtype=torch.uint8, device="cuda")
        for t in range(8):
            env.policy_step(A, words[t & 1], words[(t + 1) & 1], act[t], seats=6, opponent=B)
        assert not torch.equal(act.cpu(), res[0][0])
    finally:
        env.close()


EVAL = dict(n_games=192, episodes=2, seed=12)


def test_a_network_against_itself_scores_exactly_zero(T, S, nets):
    from tarok_amd import evaluate as EV, karte as K
    A, _ = nets
    r = EV.evaluate_vs_policy(A, [w.clone() for w in A], EVAL["n_games"], EVAL["episodes"], seed=EVAL["seed"])
    assert r["advantage"] == 0.0 and r["stderr"] == 0.0 and r["by_seat"] == [0.0] * 4
    assert r["policy_mean"] == r["bot_mean"] and r["deals"] == EVAL["n_games"] * EVAL["episodes"]
    record = []
    EV._play_passes(A, EVAL["n_games"], EVAL["episodes"], EVAL["seed"], K.MIX_BOT, 0, inspect=record, opponent=A)
    assert len(record) == 5 * EVAL["episodes"]
    for e in range(EVAL["episodes"]):
        passes = [x for x in record if x["episode"] == e]
        for x in passes[1:]:                          # all five passes play the same cards
            assert (x["actions"] == passes[0]["actions"]).all() and (x["scores"] == passes[0]["scores"]).all(), (e, x["seats"])


@pytest.fixture(scope="module")
def evaluation(T, S, nets):
    from tarok_amd import evaluate as EV, karte as K
    A, B = nets
    record = []
    scores = EV._play_passes(A, EVAL["n_games"], EVAL["episodes"], EVAL["seed"], K.MIX_BOT, 0, inspect=record, opponent=B)
    result = EV.evaluate_vs_policy(A, B, EVAL["n_games"], EVAL["episodes"], seed=EVAL["seed"])
    return result, record, scores


def test_evaluate_vs_policy_equals_the_statistic_of_replayed_scores(T, S, nets, evaluation):
    """All five passes of an episode start from the same lanes; every recorded card is legal on the oracle; the recorded
    cards replayed on per-slot oracle models give the recorded scores; duplicate_advantage of those is what
    evaluate_vs_policy returned, twice; pass 0 is a plain tarok_policy_step table of B on a fresh env."""
    import torch
    from oracle_model import SlotModel
    from tarok_amd import karte as K
    from tarok_amd.evaluate import duplicate_advantage, evaluate_vs_policy
    A, B = nets
    result, record, played = evaluation
    n, episodes = EVAL["n_games"], EVAL["episodes"]
    assert [(r["episode"], r["seats"]) for r in record] == [(e, s) for e in range(episodes) for s in (0, 1, 2, 4, 8)]
    for e in range(episodes):
        passes = [r for r in record if r["episode"] == e]
        for r in passes[1:]:
            assert (r["start"] == passes[0]["start"]).all(), (e, r["seats"])
        for i in range(0, n, 7):
            assert (passes[0]["start"][:, i] == SlotModel(EVAL["seed"], i, K.MIX_BOT, episode=e).g.lanes()).all(), (e, i)
    assert (record[0]["start"] != record[5]["start"]).any()
    assert any((record[p]["actions"] != record[0]["actions"]).any() for p in range(1, 5))    # the passes did go different ways
    scores = np.zeros((5, episodes * n, 4), np.int64)
    for r in record:
        e, seats, acts = r["episode"], r["seats"], r["actions"]
        p = (0, 1, 2, 4, 8).index(seats)
        for i in range(n):
            m = SlotModel(EVAL["seed"], i, K.MIX_BOT, episode=e)
            for t in range(48):
                legal, a = m.legal(), int(acts[t, i])
                if legal:
                    assert a < 54 and (legal >> a) & 1, (e, seats, i, t, "card not legal")
                    assert not m.card(a).rejected
                else:
                    assert a == 255, (e, seats, i, t, "a card where nothing is to be played")
            assert m.g.g.phase == 3, (e, seats, i, "game not finished after 48 cards")
            scores[p, e * n + i] = m.sum
            assert list(r["scores"][i]) == m.sum, (e, seats, i)
    assert (scores == played).all()
    assert result == duplicate_advantage(scores)
    assert result["deals"] == n * episodes and all(math.isfinite(result[k]) for k in ("advantage", "stderr", "policy_mean", "bot_mean"))
    assert evaluate_vs_policy(A, B, n, episodes, seed=EVAL["seed"]) == result
    # pass 0 is the baseline's own table: the same deals played by tarok_policy_step with B on a fresh env
    env = T.TarokVecEnv(n, seed=EVAL["seed"], mix=K.MIX_BOT)
    try:
        words = [env.obs_words, torch.empty(n, dtype=torch.int64, device="cuda")]
        acts = torch.empty((48, n), dtype=torch.uint8, device="cuda")
        for e in range(episodes):
            env.reset(episode=e, clear_counters=True)
            for t in range(48):
                env.policy_step(B, words[t & 1], words[(t + 1) & 1], acts[t], auto_reset=False)
            assert (env.counters()[1] == scores[0, e * n:(e + 1) * n]).all(), e
            assert (acts.cpu().numpy() == record[5 * e]["actions"]).all(), e
    finally:
        env.close()


def test_evaluate_vs_bot_is_what_it_was(T, S, nets):
    """Without an opponent the passes are the Bot's, as before: evaluate_vs_bot is the statistic of _play_passes called
    the way its callers always called it."""
    from tarok_amd import evaluate as EV, karte as K
    A, _ = nets
    record = []
    scores = EV._play_passes(A, EVAL["n_games"], EVAL["episodes"], EVAL["seed"], K.MIX_BOT, 0, inspect=record)
    assert EV.evaluate_vs_bot(A, EVAL["n_games"], EVAL["episodes"], seed=EVAL["seed"]) == EV.duplicate_advantage(scores)
    # pass 0 of those is the Bot everywhere: the same deals scored by a plain Bot env
    env = T.TarokVecEnv(EVAL["n_games"], seed=EVAL["seed"], mix=K.MIX_BOT)
    try:
        env.reset(episode=0)
        for _ in range(48):
            env.step_random()
        assert (env.counters()[1] == scores[0, :EVAL["n_games"]]).all()
    finally:
        env.close()


def test_selfplay_snapshot_and_evaluate_against_it(T, S):
    """SelfPlay.evaluate(opponent=snapshot()) is exactly 0 for the current weights; a snapshot survives an update; the
    evaluation changes nothing of the training env or the captured rollout."""
    import torch
    from tarok_amd import selfplay as SP
    res = []
    for with_eval in (False, True):
        env = T.TarokVecEnv(1024, seed=8, mix=S.MIX_ALL)
        sp = SP.SelfPlay(env, hidden=256, seed=0)
        obs = env.legal_actions()
        for _ in range(34):                           # (most games then end inside the updated rollout: it has returns to learn from)
            obs, _, _ = env.step(env.policy_random(obs), auto_reset=True)
        sp.obs_words.copy_(obs.words)
        sp.collect(8)
        old = sp.snapshot()
        kept = [t.clone() for t in old]
        assert len(old) == 6 and all(x.data_ptr() != y.data_ptr() for x, y in zip(old, sp._w))
        if with_eval:
            r = sp.evaluate(n_games=256, episodes=1, opponent=sp.snapshot())
            assert r["advantage"] == 0.0 and r["stderr"] == 0.0 and r["deals"] == 256
        sp.iterate(T=8)
        assert all(torch.equal(x, y) for x, y in zip(old, kept))             # the snapshot is a copy
        assert any(not torch.equal(x, y) for x, y in zip(old, sp.snapshot()))    # ... and the weights did move
        if with_eval:
            r = sp.evaluate(n_games=256, episodes=1, opponent=old)
            assert r["deals"] == 256 and len(r["by_seat"]) == 4
            assert all(math.isfinite(x) for x in [r["advantage"], r["stderr"], r["policy_mean"], r["bot_mean"]] + r["by_seat"])
        b = sp.collect(8)
        torch.cuda.synchronize()
        res.append(({k: v.clone() for k, v in b.items() if k != "reward"}, env.state().copy()))
        del sp
        env.close()
    for k in res[0][0]:
        assert torch.equal(res[0][0][k], res[1][0][k]), k
    assert (res[0][1] == res[1][1]).all()
