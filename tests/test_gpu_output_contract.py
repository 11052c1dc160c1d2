"""GPU: the OUTPUT ROWS of every step launch kind against the per-slot oracle model, inside guard bands.

A learner does not read the env state, it reads what the step launches write: action_out, reward_out, done_out,
trick_out, obs_out, the history lane (and seat_out of tarok_legal_actions).  Every case of CASES below calls the C
ABI directly (env.L) with output arrays that sit between guard bands (tests/guarded.py), on an env whose slots are
replayed card by card on the CPU oracle (tests/oracle_model.py), and after every launch requires that

  * every guard byte and every padding column [N, stride) still holds the sentinel,
  * reward_out rows of games that did not finish in that launch still hold the sentinel (include/tarok_env.h:
    "written ONLY for games that finish in this step"),
  * every row the header says is written equals the model's, bit for bit,
  * the history rows p < cards played equal the model's (the rest is declared stale),
and after the last launch that canonical state, episode numbers, score sums and observation words equal the model's.

CASES is a literal table, not a cross product: tests/test_oracle_model.py checks from it that every pair of values
of two different axes that `allowed` admits occurs in at least one case.

Not covered here: the numerical side of the learned policy (tarok_policy_step's card only has to be legal; logp and
value are not judged), and slots of the 20,077-game cases that are not modelled (guards only).  Every next-game line
consumed here is one deal_into_buffer wrote: the same rows on lines that tarok_front_lines decided again, and the
tarok_policy_step_seats / _versus / _pool launches, are in tests/test_gpu_front_rows.py.

Run on the GPU box:  python -m pytest tests/test_gpu_output_contract.py -m gpu -q
"""

import numpy as np
import pytest

from gpu_harness import T  # noqa: F401  (the module fixture)
from output_contract_cases import CASES, FIELDS, Outputs, _explicit_cards, allowed, check_against_models, modelled_slots

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def S():
    from oracle import tarok_spec
    return tarok_spec


@pytest.fixture(scope="module")
def E():
    from oracle import encoder_spec
    return encoder_spec


@pytest.fixture(scope="module")
def weights(T):
    """selfplay.PolicyNet(256), fixed seed, in the kernels' fragment order."""
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
    from tarok_amd import _native, karte as K
    from oracle_model import SlotModel
    c = dict(zip(FIELDS, case))
    assert allowed(case), case
    kind, n = c["kind"], c["n"]
    part = kind.split(":")
    auto, ref = bool(c["auto"]), bool(c["reward_ref"])
    seed, mix = 500 + idx, (S.MIX_ALL if c["mix"] == "all" else S.MIX_FIXED + 7)
    flags = (K.AUTO_RESET if auto else 0) | (K.REWARD_REF if ref else 0)
    cards = int(part[1]) if part[0] in ("krog", "run") else 1
    rows = max(cards, 1)
    stride = n + 192 if c["stride"] == "N+192" else n
    # tarok_run_random: lock-steps per call (three one-card launches, two 4-card launches, one of 128 cards: the later
    # launches of a call overwrite the rows of the earlier ones)
    run_steps = {0: 3, 1: 3, 4: 8, 128: 128}.get(cards, 0)
    launches = run_steps // rows if part[0] == "run" else 1
    rnd = np.random.RandomState(1000 + idx)
    env = T.TarokVecEnv(n, seed=seed, mix=mix, history=bool(c["hist"]), lazy_refill=None if c["lazy"] == "default" else 0)
    try:
        L, h, p, stream = env.L, env._h, env._p, env._stream
        slots = modelled_slots(n)
        models = [(int(i), SlotModel(seed, int(i), mix)) for i in slots]
        env.reset(episode=0)
        for _ in range(idx % 4):                      # lead-in: the launches start mid-trick
            env.step_random(auto_reset=auto)
            for _, m in models:
                m.card(None, auto)
        out = Outputs(rows, n, stride, slots, {k: c[k] == "given" for k in ("action", "reward", "done", "trick")})
        ptr = lambda a: None if a is None else a.ptr
        if kind == "policy_step":
            logp = torch.zeros(n, dtype=torch.float32, device="cuda")
            value = torch.zeros(n, dtype=torch.float32, device="cuda")
        for call in range(3):
            tag = (idx, case, "call", call)
            out.begin_call()
            given_cards = None
            with torch.cuda.device(env.device):
                if kind == "policy_random+step":
                    words = env.legal_actions().words
                    _native.check(L.tarok_policy_random(h, p(words), out.action.ptr, stream()))
                    _native.check(L.tarok_step(h, out.action.ptr, ptr(out.reward), ptr(out.done), ptr(out.trick), out.obs.ptr, flags, stream()))
                elif kind == "step":
                    base = env.policy_random(env.legal_actions()).cpu().numpy()
                    given_cards = _explicit_cards(rnd, models, base)
                    a_dev = torch.from_numpy(given_cards).cuda()
                    _native.check(L.tarok_step(h, p(a_dev), ptr(out.reward), ptr(out.done), ptr(out.trick), out.obs.ptr, flags, stream()))
                elif kind == "step_random":
                    _native.check(L.tarok_step_random(h, ptr(out.action), ptr(out.reward), ptr(out.done), ptr(out.trick), out.obs.ptr, flags,
                                                      stream()))
                elif part[0] == "krog":
                    _native.check(L.tarok_krog_random(h, cards, stride, ptr(out.action), ptr(out.reward), ptr(out.done), ptr(out.trick),
                                                      out.obs.ptr, flags, stream()))
                elif part[0] == "run":
                    if cards == 0:                    # the policy kernel of every step reads obs_out: it starts as the current observation
                        _native.check(L.tarok_legal_actions(h, out.obs.ptr, None, stream()))
                    _native.check(L.tarok_run_random(h, run_steps, cards, run_steps if part[2] == "graph" else 0, 0, ptr(out.action),
                                                     ptr(out.reward), ptr(out.done), out.obs.ptr, flags, stream()))
                else:
                    words = env.legal_actions().words
                    _native.check(L.tarok_policy_step(h, *[p(w) for w in weights], p(words), out.action.ptr, p(logp), p(value), None,
                                                      ptr(out.reward), ptr(out.done), ptr(out.trick), out.obs.ptr, flags, stream()))
                torch.cuda.synchronize()
            if kind == "policy_step":                 # the model takes the card the kernel reports: it must be a legal one
                acts, _ = out.action.host()
                for j, (i, m) in enumerate(models):
                    a, legal = int(acts[0, i]), m.legal()
                    assert (a == 255) if not legal else (a < 54 and (legal >> a) & 1), (tag, "card not in the legal mask", i, a, legal)
                    out.expect(0, j, m.card(a, auto, ref))
            else:
                for _ in range(launches):
                    for r in range(rows):
                        for j, (i, m) in enumerate(models):
                            out.expect(r, j, m.card(None if given_cards is None else int(given_cards[i]), auto, ref))
            # (tarok_step's card array is an input; cards_per_launch = 1 leaves `action` alone: nothing to compare there)
            out.check(tag, judge_action=kind not in ("step", "run:1:eager", "run:1:graph"))
            if env.history:
                hist = env.get_history().cpu().numpy()
                for i, m in models:
                    assert hist[:m.played, i].tolist() == m.hist[:m.played], (tag, "history", i)
        check_against_models(env, models, (idx, case, "end"))
    finally:
        env.close()


@pytest.mark.parametrize("idx", range(len(CASES)), ids=lambda i: "%03d-%s" % (i, "-".join(str(v) for v in CASES[i])))
def test_output_rows_of_every_launch_kind(T, S, weights, idx):
    run_case(T, S, idx, CASES[idx], weights)


def test_full_size_long_launch_rows_with_stride_history_and_reward_ref(T, O, S):
    """65,536 games, MIX_ALL, tarok_krog_random(128) with stride = N + 192 on a history env, TAROK_AUTO_RESET |
    TAROK_REWARD_REF, trick_out given, action_out NULL: two launches after a lead-in launch, 1 slot in 64 replayed
    on the model, all guards checked."""
    import torch
    from tarok_amd import _native, karte as K
    from oracle_model import SlotModel
    n, seed, cards = 65536, 3, 128
    stride = n + 192
    env = T.TarokVecEnv(n, seed=seed, mix=S.MIX_ALL, history=True)
    try:
        env.reset()
        slots = np.arange(0, n, 64)
        models = [(int(i), SlotModel(seed, int(i), S.MIX_ALL)) for i in slots]
        env.run_random(cards, cards_per_launch=cards, graph_chunk=0, auto_reset=True)     # lead-in: slots mid-run, lines consumed
        for _ in range(cards):
            for _, m in models:
                m.card(None, True)
        check_against_models(env, models, "lead-in")
        out = Outputs(cards, n, stride, slots, dict(action=False, reward=True, done=True, trick=True))
        for launch in range(2):
            out.begin_call()
            with torch.cuda.device(env.device):
                _native.check(env.L.tarok_krog_random(env._h, cards, stride, None, out.reward.ptr, out.done.ptr, out.trick.ptr, out.obs.ptr,
                                                      K.AUTO_RESET | K.REWARD_REF, env._stream()))
                torch.cuda.synchronize()
            for r in range(cards):
                for j, (i, m) in enumerate(models):
                    out.expect(r, j, m.card(None, True, True))
            out.check(("full size", launch))
            assert out.e_finished.any(axis=0).all()           # every modelled slot finished a game in the launch
        check_against_models(env, models, "end")
    finally:
        env.close()


def test_legal_actions_seat_out(T, O, S):
    """tarok_legal_actions with seat_out given: bits [55:54] of the observation word and the model's seat to move, on
    positions of every contract at several depths of the game, guards intact."""
    import torch
    from guarded import Guarded, assert_guards_intact
    from tarok_amd import _native
    from oracle_model import SlotModel
    n, seed = 773, 61
    env = T.TarokVecEnv(n, seed=seed, mix=S.MIX_ALL)
    try:
        env.reset()
        models = [(i, SlotModel(seed, i, S.MIX_ALL)) for i in range(n)]
        obs, seat = Guarded("obs_out", 1, n, np.uint64, device="cuda"), Guarded("seat_out", 1, n, np.int8, device="cuda")
        seen = set()
        for cards in (0, 1, 2, 3, 7, 18, 16):
            for _ in range(cards):
                env.step_random(auto_reset=True)
                for _, m in models:
                    m.card(None, True)
            obs.fill(); seat.fill()
            with torch.cuda.device(env.device):
                _native.check(env.L.tarok_legal_actions(env._h, obs.ptr, seat.ptr, env._stream()))
                torch.cuda.synchronize()
            assert_guards_intact([obs, seat], cards)
            (w, ww), (s, sw) = obs.host(), seat.host()
            assert ww.all() and sw.all()
            assert (s[0].astype(np.int64) == ((w[0] >> np.uint64(54)) & np.uint64(3)).astype(np.int64)).all(), cards
            for i, m in models:
                assert int(s[0, i]) == m.g.seat() and int(w[0, i]) == m.g.obs_word(False), (cards, i)
                seen.add(int(m.g.g.contract))
        assert seen == set(range(10))
    finally:
        env.close()


def test_policy_mlp_optional_outputs_do_not_change_the_rest(T, S, weights):
    """tarok_policy_mlp at a ragged N: action_out is bit-identical for every combination of logp_out, value_out,
    features_out and feature_words_out given or NULL, the outputs that are given are bit-identical to the all-given
    run's, and nothing is written outside any of them."""
    import itertools
    import torch
    from guarded import Guarded, assert_guards_intact
    from tarok_amd import _native
    n = 1000 + 37
    env = T.TarokVecEnv(n, seed=23, mix=S.MIX_ALL)
    try:
        obs = env.reset()
        for t in range(9):
            obs, _, _ = env.step(env.policy_random(obs), auto_reset=(t < 4))           # the last trick's finished games stay: no card to play
        words = obs.words.clone()
        spec = dict(action=(np.uint8, ()), logp=(np.uint32, ()), value=(np.uint32, ()), features=(np.uint16, (256,)), words=(np.uint64, (4,)))
        first = None
        for combo in itertools.product((True, False), repeat=4):
            on = dict(zip(("logp", "value", "features", "words"), combo), action=True)
            g = {k: Guarded(k, 1, n, dt, inner=inner, device="cuda") if on[k] else None for k, (dt, inner) in spec.items()}
            ptr = lambda a: None if a is None else a.ptr
            with torch.cuda.device(env.device):
                _native.check(env.L.tarok_policy_mlp(env._h, *[env._p(w) for w in weights], env._p(words), g["action"].ptr, ptr(g["logp"]),
                                                     ptr(g["value"]), ptr(g["features"]), ptr(g["words"]), env._stream()))
                torch.cuda.synchronize()
            assert_guards_intact(g.values(), combo)
            got = {}
            for k, a in g.items():
                if a is not None:
                    got[k], written = a.host()
                    assert written.all(), (combo, k)
            if first is None:
                first = got
                assert (first["action"] != 255).any() and (first["action"] == 255).any()
            for k, v in got.items():
                assert (v == first[k]).all(), (combo, k)
    finally:
        env.close()


def test_rollout_random_traces_are_optional(T, S):
    """tarok_rollout_random at a ragged N: scores and nsteps are identical with the three trace arrays NULL and given;
    the [48, N] traces and the two result arrays keep their guards."""
    import torch
    from guarded import Guarded, assert_guards_intact
    from tarok_amd import _native
    n = 257
    env = T.TarokVecEnv(n, seed=21, mix=S.MIX_ALL)
    try:
        res = []
        for trace in (False, True):
            scores, nsteps = Guarded("scores_out", 1, n, np.int16, inner=(4,), device="cuda"), Guarded("nsteps_out", 1, n, np.int16, device="cuda")
            tr = [Guarded("seats_out", 48, n, np.int8, device="cuda"), Guarded("masks_out", 48, n, np.uint64, device="cuda"),
                  Guarded("actions_out", 48, n, np.uint8, device="cuda")] if trace else [None] * 3
            with torch.cuda.device(env.device):
                _native.check(env.L.tarok_rollout_random(env._h, 1, scores.ptr, nsteps.ptr, *[None if a is None else a.ptr for a in tr],
                                                         env._stream()))
                torch.cuda.synchronize()
            assert_guards_intact([scores, nsteps] + tr, trace)
            (sc, sw), (ns, nw) = scores.host(), nsteps.host()
            assert sw.all() and nw.all()
            res.append((sc, ns))
            if trace:                                 # rows beyond a game's end are padded with -1 / 0 / 255: every element is written
                seats, masks, acts = [a.host()[0] for a in tr]
                live = np.arange(48)[:, None] < ns[0][None, :]
                assert (seats[~live] == -1).all() and (masks[~live] == 0).all() and (acts[~live] == 255).all()
                assert (seats[live] >= 0).all() and (masks[live] != 0).all() and (acts[live] < 54).all()
        assert (res[0][0] == res[1][0]).all() and (res[0][1] == res[1][1]).all()
    finally:
        env.close()
