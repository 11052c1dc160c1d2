"""GPU: tarok_policy_step_seats (the network on some seats, the Bot on the others) and the duplicate evaluation built
on it (tarok_amd/evaluate.py), checked exactly.

Deals and Bot draws are functions of (seed, game index, episode, cards played); the network's card for a position is
what a separate tarok_policy_mlp launch on the same observation words reports (tarok_policy_step is pinned to that
elsewhere).  So every row of a mixed launch has ONE right answer: the card is the network's where the seat to move is
in the game's seat set and the oracle's Bot card (tests/oracle_model.py) elsewhere, logp is tarok_policy_mlp's bits or
0, and everything the env half writes follows from that card through the per-slot model.

Which reference judges what: the slots that are modelled (every slot up to 773 games, a spread subset of 20,077) have
their whole row, the Bot's card included, from the CPU oracle.  For the games that are not modelled the expected Bot
card is tarok_policy_random's (k_policy, itself pinned to the oracle elsewhere, but the same device function as the
code under test), so there the check is one of agreement between launches; the seats = 0 test against
tarok_step_random covers those games the same way.

Run on the GPU box:  python -m pytest tests/test_gpu_policy_step_seats.py -m gpu -q
"""

import numpy as np
import pytest

from gpu_harness import T  # noqa: F401  (the module fixture)
from policy_step_cases import Twin, bits, seat_sets

pytestmark = pytest.mark.gpu

STEPS = 64                               # lock-steps per case (games are 48 cards at most)
FIELDS = ("n", "mix", "auto", "reward_ref", "hist", "seats", "logp", "value", "words", "reward", "done", "trick")
# sizes, mixes and flags from the case table of tests/test_gpu_output_contract.py; seats: a 4-bit set for every game,
# or "cycle": seats_per_game[i] = i % 16
CASES = [
    (773, "all", 0, 0, 1, 0, "given", "given", "given", "given", "given", "given"),
    (773, "berac", 1, 1, 0, 1, "given", "null", "given", "null", "given", "given"),
    (773, "all", 1, 0, 1, 6, "null", "given", "null", "given", "null", "given"),
    (773, "berac", 0, 1, 0, 15, "given", "given", "null", "given", "given", "null"),
    (773, "all", 1, 1, 0, "cycle", "given", "given", "given", "given", "given", "given"),
    (20077, "all", 1, 1, 1, "cycle", "given", "null", "null", "given", "given", "given"),
    (20077, "berac", 1, 0, 0, 6, "given", "given", "given", "null", "null", "null"),
    (20077, "all", 0, 1, 1, 1, "given", "given", "given", "given", "given", "given"),
    (20077, "berac", 0, 0, 0, "cycle", "null", "null", "null", "given", "given", "given"),
    (20077, "all", 1, 0, 0, 0, "given", "given", "null", "given", "null", "given"),
    (20077, "all", 1, 1, 1, 15, "given", "null", "given", "null", "given", "null"),
]


@pytest.fixture(scope="module")
def S():
    from oracle import tarok_spec
    return tarok_spec


@pytest.fixture(scope="module")
def weights(T):
    """selfplay.PolicyNet(256), fixed seed, in the kernels' fragment order (as tests/test_gpu_output_contract.py builds them)."""
    import torch
    from tarok_amd import selfplay as SP
    torch.manual_seed(0)
    net = SP.PolicyNet(256).cuda()
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(3.0)                  # spread the logits a little
    order = T.TarokVecEnv.mfma_weight_order
    bf = lambda w: order(w.detach().to(torch.bfloat16).contiguous())
    fl = lambda b: b.detach().float().contiguous()
    return [bf(net.fc1.weight), fl(net.fc1.bias), bf(net.fc2.weight), fl(net.fc2.bias), bf(net.head.weight), fl(net.head.bias)]


def run_case(T, S, idx, case, weights):
    import torch
    from guarded import Guarded, assert_guards_intact
    from oracle_model import SlotModel
    from tarok_amd import _native, karte as K
    from output_contract_cases import Outputs, check_against_models, modelled_slots
    c = dict(zip(FIELDS, case))
    n, auto, ref = c["n"], bool(c["auto"]), bool(c["reward_ref"])
    seed, mix = 900 + idx, (S.MIX_ALL if c["mix"] == "all" else S.MIX_FIXED + 7)
    flags = (K.AUTO_RESET if auto else 0) | (K.REWARD_REF if ref else 0)
    seats, per_game, sets = seat_sets(c["seats"], n)
    env = T.TarokVecEnv(n, seed=seed, mix=mix, history=bool(c["hist"]))
    try:
        L, h, p, stream = env.L, env._h, env._p, env._stream
        slots = modelled_slots(n)
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
        fw_mlp = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
        seen_net = seen_bot = 0
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
                # the network's card for this very position, from a launch of its own
                a_mlp, lp_mlp, v_mlp = env.policy_mlp(weights, words, feature_words_out=fw_mlp)
                a_bot = env.policy_random(env.legal_actions())
                w_h = words.cpu().numpy().view(np.uint64)
                a_mlp_h, lp_mlp_h, v_mlp_h, fw_h, a_bot_h = (a_mlp.cpu().numpy(), lp_mlp.cpu().numpy(), v_mlp.cpu().numpy(),
                                                             fw_mlp.cpu().numpy().view(np.uint64), a_bot.cpu().numpy())
                _native.check(L.tarok_policy_step_seats(h, seats, p(per_dev), *[p(w) for w in weights], p(words), out.action.ptr,
                                                        ptr(g_logp), ptr(g_value), ptr(g_words), ptr(out.reward), ptr(out.done),
                                                        ptr(out.trick), out.obs.ptr, flags, stream()))
                torch.cuda.synchronize()
            # ---- the modelled slots: the whole row from the oracle
            for j, (i, m) in enumerate(models):
                legal = m.legal()
                network = legal != 0 and (int(sets[i]) >> m.g.seat()) & 1
                if network:
                    a = int(a_mlp_h[i])
                    assert a < 54 and (legal >> a) & 1, (tag, "tarok_policy_mlp's card is not legal", i, a, legal)
                    row = m.card(a, auto, ref)
                    seen_net += 1
                else:
                    row = m.card(None, auto, ref)     # the oracle's Bot card (NO_CARD where no game is in play)
                    seen_bot += legal != 0
                out.expect(0, j, row)
            out.check(tag)
            assert_guards_intact(extra, tag)
            # ---- every game: card and logp by the seat to move of the observation word, value and features as tarok_policy_mlp's
            mover = ((w_h >> np.uint64(54)) & np.uint64(3)).astype(np.uint8)
            live = (w_h & np.uint64((1 << 54) - 1)) != 0
            net = ((sets >> mover) & 1).astype(bool)
            acts, written = out.action.host()
            assert written.all(), (tag, "action_out rows not written")
            exp_a = np.where(live, np.where(net, a_mlp_h, a_bot_h), 255)
            bad = np.nonzero(acts[0] != exp_a)[0]
            assert bad.size == 0, (tag, "action_out", int(bad[0]), int(acts[0][bad[0]]), int(exp_a[bad[0]]), len(bad))
            if g_logp is not None:
                got, written = g_logp.host()
                assert written.all(), (tag, "logp_out rows not written")
                exp = np.where(net & live, bits(lp_mlp_h), np.uint32(0))
                bad = np.nonzero(got[0] != exp)[0]
                assert bad.size == 0, (tag, "logp_out", int(bad[0]), hex(int(got[0][bad[0]])), hex(int(exp[bad[0]])), len(bad))
            if g_value is not None:
                got, written = g_value.host()
                assert written.all() and (got[0] == bits(v_mlp_h)).all(), (tag, "value_out")
            if g_words is not None:
                got, written = g_words.host()
                assert written.all() and (got[0] == fw_h).all(), (tag, "feature_words_out")
            if env.history:
                hist = env.get_history().cpu().numpy()
                for i, m in models:
                    assert hist[:m.played, i].tolist() == m.hist[:m.played], (tag, "history", i)
        check_against_models(env, models, (idx, case, "end"))
        # the case did exercise what it is about
        if c["seats"] != 0:
            assert seen_net > 0
        if c["seats"] != 15:
            assert seen_bot > 0
    finally:
        env.close()


@pytest.mark.parametrize("idx", range(len(CASES)), ids=lambda i: "%02d-%s" % (i, "-".join(str(v) for v in CASES[i])))
def test_every_row_of_a_mixed_launch_against_the_oracle(T, S, weights, idx):
    run_case(T, S, idx, CASES[idx], weights)


@pytest.mark.parametrize("which", ["seats=15 is tarok_policy_step", "seats=0 is tarok_step_random"])
def test_all_network_and_all_bot_tables_reproduce_the_existing_launches(T, S, weights, which):
    """Twin envs (20,077 games, MIX_ALL, history, TAROK_AUTO_RESET | TAROK_REWARD_REF), 60 lock-steps: every output of
    every launch and the state, counters, history and observation words at the end are bit-equal.  seats = 0 is also
    given as a per-game array of zeros, seats = 15 as an array of 15s, on a third env."""
    import torch
    from tarok_amd import _native, karte as K
    n, seed, flags = 20077, 77, K.AUTO_RESET | K.REWARD_REF
    all_net = which.startswith("seats=15")
    val = 15 if all_net else 0
    a, b, c = (Twin(T, n, seed, S.MIX_ALL) for _ in range(3))
    per = torch.full((n,), val, dtype=torch.uint8, device="cuda")
    try:
        W = [a.env._p(w) for w in weights]
        compare = ("action", "logp", "value", "words", "reward", "done", "trick", "obs") if all_net else ("action", "reward", "done", "trick", "obs")
        for t in range(60):
            for tw in (a, b, c):
                tw.clear()
            for tw, kind in ((a, "old"), (b, "set"), (c, "array")):
                e, o = tw.env, tw.o
                p = e._p
                words = e.legal_actions().words
                with torch.cuda.device(e.device):
                    if kind == "old" and all_net:
                        _native.check(e.L.tarok_policy_step(e._h, *W, p(words), p(o["action"]), p(o["logp"]), p(o["value"]), p(o["words"]),
                                                            p(o["reward"]), p(o["done"]), p(o["trick"]), p(o["obs"]), flags, e._stream()))
                    elif kind == "old":
                        _native.check(e.L.tarok_step_random(e._h, p(o["action"]), p(o["reward"]), p(o["done"]), p(o["trick"]), p(o["obs"]),
                                                            flags, e._stream()))
                    else:
                        _native.check(e.L.tarok_policy_step_seats(e._h, val if kind == "set" else 15 - val, p(per) if kind == "array" else None,
                                                                  *W, p(words), p(o["action"]), p(o["logp"]), p(o["value"]), p(o["words"]),
                                                                  p(o["reward"]), p(o["done"]), p(o["trick"]), p(o["obs"]), flags, e._stream()))
            torch.cuda.synchronize()
            for k in compare:
                assert torch.equal(a.o[k], b.o[k]), (which, t, k, "seat set")
                assert torch.equal(a.o[k], c.o[k]), (which, t, k, "per-game array")
            if not all_net:                           # no row is the network's
                for tw in (b, c):
                    assert (tw.o["logp"] == 0).all().item(), (which, t, "logp_out")
        ea, eb, ec = a.end_state(), b.end_state(), c.end_state()
        assert ea[1].sum() > n                        # games did finish and were replaced
        for x, y, z in zip(ea, eb, ec):
            assert (x == y).all() and (x == z).all(), which
    finally:
        for tw in (a, b, c):
            tw.env.close()


def test_env_policy_step_default_is_the_plain_launch_and_seats_select_the_mixed_one(T, S, weights):
    """TarokVecEnv.policy_step: seats=None is tarok_policy_step; seats=15 and an array of 15s give the same rows; a bad
    seat set or array is refused."""
    import torch
    n = 773
    res = []
    for kw in (dict(), dict(seats=15), dict(seats_per_game=torch.full((n,), 15, dtype=torch.uint8, device="cuda"))):
        env = T.TarokVecEnv(n, seed=5, mix=S.MIX_ALL)
        try:
            words = [env.reset().words, torch.zeros(n, dtype=torch.int64, device="cuda")]
            act = torch.zeros((8, n), dtype=torch.uint8, device="cuda")
            logp = torch.zeros((8, n), dtype=torch.float32, device="cuda")
            trick = torch.zeros((8, n), dtype=torch.int16, device="cuda")
            for t in range(8):
                env.policy_step(weights, words[t & 1], words[(t + 1) & 1], act[t], logp[t], tricks=trick[t], **kw)
            res.append((act.cpu(), logp.cpu(), trick.cpu(), env.state()))
            if kw:
                with pytest.raises(T.TarokNativeError):
                    env.policy_step(weights, words[0], words[1], act[0], seats=16)
                with pytest.raises(T.TarokNativeError):
                    env.policy_step(weights, words[0], words[0], act[0], seats=3)          # obs == obs_out
                with pytest.raises(ValueError):
                    env.policy_step(weights, words[0], words[1], act[0], seats_per_game=torch.zeros(n, dtype=torch.int64, device="cuda"))
        finally:
            env.close()
    for r in res[1:]:
        for x, y in zip(res[0][:3], r[:3]):
            assert torch.equal(x, y)
        assert (res[0][3] == r[3]).all()
    assert (res[0][2] != 0).any()                     # trick rows were written (cards 4 and 8 complete tricks)


EVAL = dict(n_games=192, episodes=2, seed=12)


@pytest.fixture(scope="module")
def evaluation(T, S, weights):
    from tarok_amd import evaluate as EV, karte as K
    record = []
    scores = EV._play_passes(weights, EVAL["n_games"], EVAL["episodes"], EVAL["seed"], K.MIX_BOT, 0, inspect=record)
    result = EV.evaluate_vs_bot(weights, EVAL["n_games"], EVAL["episodes"], seed=EVAL["seed"])
    assert result == EV.duplicate_advantage(scores)       # the inspected passes are the ones evaluate_vs_bot plays
    return result, record


def test_duplicate_deals_start_identically_in_all_five_passes(T, S, evaluation):
    """After reset(episode=e) the canonical lanes of the env evaluate_vs_bot's passes are played on are the same in the five passes of an
    episode (the passes before it played different cards on it), they are the oracle's deal, and episodes differ."""
    from oracle_model import SlotModel
    from tarok_amd import karte as K
    _, record = evaluation
    assert [(r["episode"], r["seats"]) for r in record] == [(e, s) for e in range(EVAL["episodes"]) for s in (0, 1, 2, 4, 8)]
    for e in range(EVAL["episodes"]):
        passes = [r for r in record if r["episode"] == e]
        for r in passes[1:]:
            assert (r["start"] == passes[0]["start"]).all(), (e, r["seats"])
        for i in range(0, EVAL["n_games"], 7):
            assert (passes[0]["start"][:, i] == SlotModel(EVAL["seed"], i, K.MIX_BOT, episode=e).g.lanes()).all(), (e, i)
    assert (record[0]["start"] != record[5]["start"]).any()
    # the passes did go different ways
    assert any((record[p]["actions"] != record[0]["actions"]).any() for p in range(1, 5))


def test_evaluate_vs_bot_equals_the_statistic_of_replayed_scores(T, S, weights, evaluation):
    """Every pass replayed on per-slot oracle models — the network's cards from the recorded action rows (each one
    legal, and only on the network's seat), the Bot's from the oracle (and equal to the recorded ones) — gives the
    scores; duplicate_advantage of those is what evaluate_vs_bot returned.  A second call returns the same numbers."""
    from oracle_model import SlotModel
    from tarok_amd import karte as K
    from tarok_amd.evaluate import duplicate_advantage, evaluate_vs_bot
    result, record = evaluation
    n, episodes = EVAL["n_games"], EVAL["episodes"]
    scores = np.zeros((5, episodes * n, 4), np.int64)
    network_cards = 0
    for r in record:
        e, seats, acts = r["episode"], r["seats"], r["actions"]
        p = (0, 1, 2, 4, 8).index(seats)
        for i in range(n):
            m = SlotModel(EVAL["seed"], i, K.MIX_BOT, episode=e)
            for t in range(48):
                legal, a = m.legal(), int(acts[t, i])
                if legal and (seats >> m.g.seat()) & 1:
                    assert a < 54 and (legal >> a) & 1, (e, seats, i, t, "network card not legal")
                    row = m.card(a)
                    network_cards += 1
                else:
                    row = m.card(None)
                    assert row.action == a, (e, seats, i, t, "Bot card")
                assert not row.rejected or not legal
            assert m.g.g.phase == 3, (e, seats, i, "game not finished after 48 cards")
            scores[p, e * n + i] = m.sum
            assert list(r["scores"][i]) == m.sum, (e, seats, i)
    assert network_cards > 0
    assert result == duplicate_advantage(scores)
    assert result["deals"] == n * episodes
    again = evaluate_vs_bot(weights, n, episodes, seed=EVAL["seed"])
    assert again == result
    # pass 0 is the Bot's own table: the same deals scored by a plain Bot env
    env = T.TarokVecEnv(n, seed=EVAL["seed"], mix=K.MIX_BOT)
    try:
        for e in range(episodes):
            env.reset(episode=e)
            for _ in range(48):
                env.step_random()
            assert (env.counters()[1] == scores[0, e * n:(e + 1) * n]).all(), e
    finally:
        env.close()


def test_selfplay_evaluate_leaves_training_alone(T, S):
    """SelfPlay.evaluate returns evaluate_vs_bot's figures for the current weights and changes nothing of the training
    env or the captured rollout: the next collect() is what it would have been without the evaluation."""
    import torch
    from tarok_amd import selfplay as SP
    from tarok_amd.evaluate import evaluate_vs_bot
    res = []
    for with_eval in (False, True):
        env = T.TarokVecEnv(1024, seed=8, mix=S.MIX_ALL)
        sp = SP.SelfPlay(env, hidden=256, seed=0)
        sp.collect(8)
        if with_eval:
            r = sp.evaluate(n_games=256, episodes=1)
            assert r == evaluate_vs_bot(sp._w, 256, 1)
            assert r["deals"] == 256 and len(r["by_seat"]) == 4
        b = sp.collect(8)
        torch.cuda.synchronize()
        res.append(({k: v.clone() for k, v in b.items() if k != "reward"}, env.state().copy()))
        del sp
        env.close()
    for k in res[0][0]:
        assert torch.equal(res[0][0][k], res[1][0][k]), k
    assert (res[0][1] == res[1][1]).all()
