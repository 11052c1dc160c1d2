"""GPU: tarok_policy_step_pool (the learner on the seats of a set, a POOL of frozen networks on the others, one network
per step group of 256 slots) checked exactly.

A network's card, log-probability and value for a position are what a separate tarok_policy_mlp launch with its weights
on the same observation words reports.  So every row of a pool launch has ONE right answer: the learner's launch where
the mover's seat is in the game's set or the game's step group is a self-play group (group_net[g] >= pool_size), else
the launch of pool entry group_net[g] (g % pool_size without a table), and everything the env half writes follows from
that card through the per-slot model on the CPU oracle (tests/oracle_model.py).

Run on the GPU box:  python -m pytest tests/test_gpu_policy_step_pool.py -m gpu -q
"""

import numpy as np
import pytest

from gpu_harness import T  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

STEPS = 64                               # lock-steps per case (games are 48 cards at most)
N = 773                                  # four step groups, the last with 5 games (a partial tile, clamped tail lanes)
KP = 3                                   # networks in the pool
FIELDS = ("mix", "auto", "reward_ref", "hist", "seats", "group_net", "logp", "value", "words", "reward", "done", "trick")
# seats: a 4-bit set for every game, or "cycle": seats_per_game[i] = i % 16.  group_net: the table, or None (g % 3); an
# entry >= 3 is the learner itself.  Pairs of settings are covered, not the cross product (as in the versus test).
CASES = [
    ("all", 0, 0, 1, 6, (2, 0, 3, 1), "given", "given", "given", "given", "given", "given"),
    ("berac", 1, 1, 0, "cycle", None, "given", "null", "given", "null", "given", "given"),
    ("all", 1, 0, 1, 1, (200, 1, 1, 0), "null", "given", "null", "given", "null", "given"),
    ("berac", 0, 1, 0, "cycle", (2, 0, 3, 1), "given", "given", "null", "given", "given", "null"),
    ("all", 1, 1, 0, 9, None, "given", "given", "given", "given", "given", "given"),
    ("berac", 0, 0, 1, "cycle", (200, 1, 1, 0), "null", "null", "null", "null", "null", "null"),
]


@pytest.fixture(scope="module")
def S():
    from oracle import tarok_spec
    return tarok_spec


@pytest.fixture(scope="module")
def nets(T):
    """(the learner's weight set, [three pool weight sets], a fifth set): five different networks."""
    import torch
    from policy_step_cases import make_weights
    sets = [make_weights(T, s) for s in range(5)]
    for a in range(5):
        for b in range(a):
            assert not torch.equal(sets[a][0], sets[b][0])
    return sets[0], sets[1:4], sets[4]


def pool_step(env, seats, per_game, A, k, pool, group_net, obs, action, logp, value, words, reward, done, trick, obs_out, flags):
    """One tarok_policy_step_pool launch through the C ABI (every argument a ctypes pointer or None); returns the code."""
    p = env._p
    return env.L.tarok_policy_step_pool(env._h, seats, per_game, *[p(w) for w in A], k, *[(t if t is None else p(t)) for t in pool],
                                        group_net, obs, action, logp, value, words, reward, done, trick, obs_out, flags, env._stream())


def group_index(n, k, table):
    """The pool index of every game [n] (k = the learner itself) under a group_net table or None."""
    g = np.arange(n) // 256
    idx = g % k if table is None else np.asarray(table, np.int64)[g]
    return np.minimum(idx, k)


def run_case(T, S, idx, case, nets):
    import torch
    from guarded import Guarded, assert_guards_intact
    from oracle_model import SlotModel
    from tarok_amd import _native, karte as K
    from output_contract_cases import Outputs, check_against_models, modelled_slots
    from policy_step_cases import bits, seat_sets
    A, P, _ = nets
    c = dict(zip(FIELDS, case))
    n, auto, ref = N, bool(c["auto"]), bool(c["reward_ref"])
    seed, mix = 2300 + idx, (S.MIX_ALL if c["mix"] == "all" else S.MIX_FIXED + 7)
    flags = (K.AUTO_RESET if auto else 0) | (K.REWARD_REF if ref else 0)
    seats, per_game, sets = seat_sets(c["seats"], n)
    net_of = group_index(n, KP, c["group_net"])
    env = T.TarokVecEnv(n, seed=seed, mix=mix, history=bool(c["hist"]))
    try:
        p = env._p
        pool = T.TarokVecEnv.stack_pool(P)
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
        gn_dev = None if c["group_net"] is None else torch.tensor(c["group_net"], dtype=torch.uint8, device="cuda")
        fw = [torch.zeros((n, 4), dtype=torch.int64, device="cuda") for _ in range(1 + KP)]
        differ_on = np.zeros(KP, np.int64)            # rows pool entry k moved with a card that is not the learner's
        seen_learner = 0
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
                # each network's card for this very position, from a launch of its own: [0] the learner, [1 + k] entry k
                ref_a, ref_lp, ref_v = [], [], []
                for k, W in enumerate([A] + list(P)):
                    a_k, lp_k, v_k = env.policy_mlp(W, words, feature_words_out=fw[k])
                    ref_a.append(a_k.cpu().numpy()); ref_lp.append(bits(lp_k.cpu().numpy())); ref_v.append(bits(v_k.cpu().numpy()))
                fw_h = [f.cpu().numpy().view(np.uint64) for f in fw]
                w_h = words.cpu().numpy().view(np.uint64)
                _native.check(pool_step(env, seats, p(per_dev), A, KP, pool, p(gn_dev), p(words), out.action.ptr, ptr(g_logp), ptr(g_value),
                                        ptr(g_words), ptr(out.reward), ptr(out.done), ptr(out.trick), out.obs.ptr, flags))
                torch.cuda.synchronize()
            for f in fw_h[1:]:
                assert (f == fw_h[0]).all(), (tag, "the feature words do not depend on the weights")
            ref_a, ref_lp, ref_v = np.stack(ref_a), np.stack(ref_lp), np.stack(ref_v)
            # ---- every game: card, logp and value of the launch of its mover's network
            mover = ((w_h >> np.uint64(54)) & np.uint64(3)).astype(np.uint8)
            live = (w_h & np.uint64((1 << 54) - 1)) != 0
            is_a = ((sets >> mover) & 1).astype(bool) | (net_of >= KP)
            which = np.where(is_a, 0, 1 + np.minimum(net_of, KP - 1))
            rows = np.arange(n)
            exp_a = np.where(live, ref_a[which, rows], 255).astype(np.uint8)
            assert (ref_a[:, ~live] == 255).all(), tag
            acts, written = out.action.host()
            assert written.all(), (tag, "action_out rows not written")
            bad = np.nonzero(acts[0] != exp_a)[0]
            assert bad.size == 0, (tag, "action_out", int(bad[0]), int(acts[0][bad[0]]), int(exp_a[bad[0]]), len(bad))
            if g_logp is not None:
                got, written = g_logp.host()
                assert written.all(), (tag, "logp_out rows not written")
                exp = np.where(live, ref_lp[which, rows], np.uint32(0))
                bad = np.nonzero(got[0] != exp)[0]
                assert bad.size == 0, (tag, "logp_out", int(bad[0]), hex(int(got[0][bad[0]])), hex(int(exp[bad[0]])), len(bad))
            if g_value is not None:
                got, written = g_value.host()
                assert written.all(), (tag, "value_out rows not written")
                exp = ref_v[which, rows]
                bad = np.nonzero(got[0] != exp)[0]
                assert bad.size == 0, (tag, "value_out", int(bad[0]), hex(int(got[0][bad[0]])), hex(int(exp[bad[0]])), len(bad))
            if g_words is not None:
                got, written = g_words.host()
                assert written.all() and (got[0] == fw_h[0]).all(), (tag, "feature_words_out")
            seen_learner += int((live & is_a).sum())
            for k in range(KP):
                differ_on[k] += int((live & (which == 1 + k) & (ref_a[1 + k] != ref_a[0])).sum())
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
        # the case did exercise what it is about: rows moved by at least two different pool entries whose cards differ from
        # the learner's (always taking the learner's card, or one entry's for every group, cannot pass), and the learner's
        assert int((differ_on > 0).sum()) >= 2, differ_on
        assert seen_learner > 0
    finally:
        env.close()


@pytest.mark.parametrize("idx", range(len(CASES)), ids=lambda i: "%02d-%s" % (i, "-".join(str(v).replace(" ", "") for v in CASES[i])))
def test_every_row_of_a_pool_launch_against_the_oracle_and_policy_mlp(T, S, nets, idx):
    run_case(T, S, idx, CASES[idx], nets)


def twin_run(T, S, n, steps, launches, play_mode=None, seed=77):
    """One Twin env per launch function, `steps` lock-steps each; every output of every launch and the end state must be
    byte-equal to the first's."""
    import torch
    from policy_step_cases import Twin
    twins = [Twin(T, n, seed, S.MIX_ALL) for _ in launches]
    try:
        if play_mode is not None:
            for tw in twins:
                tw.env.set_play_mode(*play_mode)
        for t in range(steps):
            for tw, launch in zip(twins, launches):
                tw.clear()
                e, o = tw.env, tw.o
                words = e.legal_actions().words
                with torch.cuda.device(e.device):
                    launch(e, o, words)
            torch.cuda.synchronize()
            for j, tw in enumerate(twins[1:]):
                for k in ("action", "logp", "value", "words", "reward", "done", "trick", "obs"):
                    assert torch.equal(twins[0].o[k], tw.o[k]), (t, k, "launch", 1 + j)
        ends = [tw.end_state() for tw in twins]
        assert ends[0][1].sum() > n                   # games did finish and were replaced
        for j, end in enumerate(ends[1:]):
            for x, y in zip(ends[0], end):
                assert (x == y).all(), ("end state", 1 + j)
    finally:
        for tw in twins:
            tw.env.close()


def launchers(T, flags):
    """Launch functions (env, outputs, words) of the three kinds, bound to their weights."""
    from tarok_amd import _native
    from policy_step_cases import versus

    def outs(e, o):
        p = e._p
        return [p(o["action"]), p(o["logp"]), p(o["value"]), p(o["words"]), p(o["reward"]), p(o["done"]), p(o["trick"]), p(o["obs"]), flags]

    def plain(W):
        return lambda e, o, words: _native.check(e.L.tarok_policy_step(e._h, *[e._p(w) for w in W], e._p(words), *outs(e, o), e._stream()))

    def vs(seats, per, A, B):
        return lambda e, o, words: versus(e, seats, e._p(per), A, B, e._p(words), *outs(e, o))

    def pool(seats, per, A, sets, table):
        stacked = T.TarokVecEnv.stack_pool(sets)
        return lambda e, o, words: _native.check(pool_step(e, seats, e._p(per), A, len(sets), stacked, e._p(table), e._p(words), *outs(e, o)))
    return plain, vs, pool


@pytest.mark.parametrize("which", ["pool_size=1, NULL group_net is the versus launch", "seats=15 is tarok_policy_step",
                                   "every group self is tarok_policy_step", "three copies of B is the versus launch with B"])
def test_pool_launches_reduce_to_the_existing_launches(T, S, nets, which):
    """Twin envs (1,797 games = eight step groups, the last partial; MIX_ALL, history, TAROK_AUTO_RESET |
    TAROK_REWARD_REF), 60 lock-steps: all outputs of every launch and the state, counters, history and observation words
    at the end are byte-equal."""
    import torch
    from tarok_amd import karte as K
    A, P, _ = nets
    B = P[0]
    n = 1797
    plain, vs, pool = launchers(T, K.AUTO_RESET | K.REWARD_REF)
    cycle = (torch.arange(n, device="cuda") % 16).to(torch.uint8)
    u8 = lambda v: torch.tensor(v, dtype=torch.uint8, device="cuda")
    if which.startswith("pool_size=1"):
        launches = [vs(9, cycle, A, B), pool(6, cycle, A, [B], None), pool(6, cycle, A, [B], u8([0] * 8))]
    elif which.startswith("seats=15"):
        launches = [plain(A), pool(15, None, A, P, None), pool(0, torch.full((n,), 15, dtype=torch.uint8, device="cuda"), A, P, u8([2, 1, 0, 2, 1, 0, 2, 1]))]
    elif which.startswith("every group self"):
        launches = [plain(A), pool(6, None, A, P, u8([3, 64, 200, 255, 3, 4, 5, 6])), pool(0, cycle, A, P[:1], u8([1] * 8))]
    else:
        launches = [vs(6, None, A, B), pool(6, None, A, [B, B, B], None), pool(6, None, A, [[w.clone() for w in B] for _ in range(3)], u8([2, 2, 1, 0, 1, 2, 0, 0]))]
    twin_run(T, S, n, 60, launches)


@pytest.mark.parametrize("mode", [(0.0, 0.0), (0.5, 0.25)], ids=["greedy", "T0.5-eps0.25"])
def test_pool_launch_under_a_play_mode_is_the_versus_mode_kernel(T, S, nets, mode):
    """A pool of three copies of B under a play mode: k_policy_step_pool_mode's outputs and end state are
    k_policy_step_versus_mode's with B, to the byte (twin envs, 1,797 games, 60 lock-steps)."""
    import torch
    from tarok_amd import karte as K
    A, P, _ = nets
    B = P[1]
    n = 1797
    _, vs, pool = launchers(T, K.AUTO_RESET | K.REWARD_REF)
    cycle = (torch.arange(n, device="cuda") % 16).to(torch.uint8)
    twin_run(T, S, n, 60, [vs(9, cycle, A, B), pool(9, cycle, A, [B, B, B], None)], play_mode=mode)


def test_bad_arguments_are_refused(T, S, nets):
    import torch
    from tarok_amd import karte as K
    A, P, _ = nets
    n = 300
    env = T.TarokVecEnv(n, seed=3, mix=S.MIX_ALL)
    try:
        p = env._p
        pool = list(T.TarokVecEnv.stack_pool(P))
        words = env.reset().words
        obs_out = torch.zeros(n, dtype=torch.int64, device="cuda")
        act = torch.zeros(n, dtype=torch.uint8, device="cuda")
        before = env.state().copy()

        def call(seats=6, k=KP, pool=pool, obs=words, out=obs_out):
            return pool_step(env, seats, None, A, k, pool, None, p(obs), p(act), None, None, None, None, None, None, p(out), K.AUTO_RESET)
        for kw in (dict(k=0), dict(k=65), dict(k=-1), dict(seats=16), dict(seats=-1), dict(out=words)):
            assert call(**kw) == -1, kw
        for j in range(6):
            holed = list(pool)
            holed[j] = None
            assert call(pool=holed) == -1, j
        torch.cuda.synchronize()
        assert (env.state() == before).all()          # nothing was launched
        assert call() == 0
        # the Python surface: one of opponent / opponent_pool; shapes and dtypes with a leading K
        with pytest.raises(ValueError):
            env.policy_step(A, words, obs_out, act, opponent=P[0], opponent_pool=pool)
        with pytest.raises(ValueError):
            env.policy_step(A, words, obs_out, act, opponent_pool=pool[:5])
        with pytest.raises(ValueError):
            env.policy_step(A, words, obs_out, act, opponent_pool=pool, group_net=torch.zeros(3, dtype=torch.uint8, device="cuda"))
        with pytest.raises(ValueError):
            env.policy_step(A, words, obs_out, act, group_net=torch.zeros(2, dtype=torch.uint8, device="cuda"))
        with pytest.raises(T.TarokNativeError):
            env.policy_step(A, obs_out, obs_out, act, opponent_pool=pool)
    finally:
        env.close()


def test_a_captured_graph_plays_an_entry_swapped_in_place(T, S, nets):
    """Eight pool launches captured with torch.cuda.graph (773 games; seats 0, so every row is its group's pool entry's;
    group_net NULL: groups 0..3 on entries 0, 1, 2, 0).  Replay 0 plays the pool as captured.  Then entry 1 is overwritten
    in place with a fifth network D, and from that replay on the rows of group 1 are D's tarok_policy_mlp rows on the very
    positions (taken on an eager twin that swapped too and is byte-equal to the graph env throughout), while the other
    groups' rows are those of an eager twin that kept the old pool."""
    import torch
    A, P, D = nets
    n, Tn = N, 8
    envs = [T.TarokVecEnv(n, seed=41, mix=S.MIX_ALL) for _ in range(3)]         # 0: the graph, 1: eager, old pool, 2: eager, swaps
    try:
        z = lambda dt, *shape: torch.zeros(shape, dtype=dt, device="cuda")
        bufs = [dict(words=z(torch.int64, Tn + 1, n), act=z(torch.uint8, Tn, n), logp=z(torch.float32, Tn, n), val=z(torch.float32, Tn, n))
                for _ in envs]
        pools = [T.TarokVecEnv.stack_pool(P) for _ in envs]
        mlp = []                                      # D's rows on env 2's positions, per lock-step of the last body(2)

        def body(j, with_mlp=False):
            e, b = envs[j], bufs[j]
            b["words"][0].copy_(b["words"][Tn])
            for t in range(Tn):
                if with_mlp:
                    mlp.append(e.policy_mlp(D, b["words"][t]))
                e.policy_step(A, b["words"][t], b["words"][t + 1], b["act"][t], b["logp"][t], b["val"][t], seats=0, opponent_pool=pools[j])

        for j, e in enumerate(envs):
            bufs[j]["words"][Tn].copy_(e.reset().words)
        side = torch.cuda.Stream()                    # the graph env warms up on a side stream, the twins play the same launches
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            body(0)
        torch.cuda.current_stream().wait_stream(side)
        body(1)
        body(2)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            body(0)
        group = torch.arange(n, device="cuda") // 256
        on1 = group == 1
        for rnd in range(3):
            if rnd == 1:                              # entry 1 := D, in place, where the captured graph reads it
                for j in (0, 2):
                    for dst, src in zip(pools[j], D):
                        dst[1].copy_(src)
            g.replay()
            body(1)
            del mlp[:]
            body(2, with_mlp=True)
            torch.cuda.synchronize()
            for k in ("words", "act", "logp", "val"):
                assert torch.equal(bufs[0][k], bufs[2][k]), (rnd, k, "the replay against the eager launches on the same pool")
                keep = ~on1 if rnd else group >= 0
                assert torch.equal(bufs[0][k][:, keep], bufs[1][k][:, keep]), (rnd, k, "groups whose entry was not touched")
            if rnd:
                assert not torch.equal(bufs[0]["act"][:, on1], bufs[1]["act"][:, on1]), (rnd, "group 1 plays on as before the swap")
                for t, (a, lp, v) in enumerate(mlp):
                    assert torch.equal(bufs[0]["act"][t][on1], a[on1]), (rnd, t, "card")
                    assert torch.equal(bufs[0]["logp"][t][on1].view(torch.int32), lp[on1].view(torch.int32)), (rnd, t, "logp")
                    assert torch.equal(bufs[0]["val"][t][on1].view(torch.int32), v[on1].view(torch.int32)), (rnd, t, "value")
                assert int((bufs[0]["act"][:, on1] != 255).sum()) > 0
    finally:
        for e in envs:
            e.close()
