"""TEST INFRASTRUCTURE — the output contract of the step launch kinds (tests/test_gpu_output_contract.py): the axes and cases,
which rows a case may leave unwritten, the guarded Outputs of one launch and their comparison with the per-slot models.
Device-free where the caller asks for it: tests/test_oracle_model.py runs the checker on the CPU."""

import numpy as np


KROG_CARDS = (1, 2, 3, 4, 5, 7, 48, 128, 192)
RUN_CARDS = (0, 1, 4, 128)
AXES = dict(
    kind=["policy_random+step", "step", "step_random"] + ["krog:%d" % c for c in KROG_CARDS] +
         ["run:%d:%s" % (c, m) for c in RUN_CARDS for m in ("eager", "graph")] + ["policy_step"],
    hist=[0, 1],                         # env created with TAROK_HISTORY
    auto=[0, 1],                         # TAROK_AUTO_RESET
    reward_ref=[0, 1],                   # TAROK_REWARD_REF
    lazy=["default", 0],                 # TAROK_OPT_LAZY_REFILL
    action=["given", "null"],            # action_out
    reward=["given", "null"],            # reward_out
    done=["given", "null"],              # done_out
    trick=["given", "null"],             # trick_out
    stride=["N", "N+192"],
    n=[1, 63, 257, 773, 20077],
    mix=["all", "berac"],                # TAROK_MIX_ALL / TAROK_MIX_FIXED + 7: several games per slot and launch
)
FIELDS = tuple(AXES)


def allowed(case):
    """Which combinations the API admits, from include/tarok_env.h."""
    c = dict(zip(FIELDS, case))
    kind = c["kind"]
    if c["stride"] != "N" and not kind.startswith("krog:"):
        return False                     # `stride` is an argument of tarok_krog_random alone
    if kind.startswith("run:") and c["trick"] != "null":
        return False                     # tarok_run_random takes no trick_out
    if kind in ("policy_random+step", "step", "policy_step", "run:0:eager", "run:0:graph") and c["action"] != "given":
        return False                     # the card array is an input (tarok_step), the policy's required output
                                         # (tarok_policy_random, tarok_policy_step) or required scratch (cards_per_launch = 0)
    return True


# (kind, hist, auto, reward_ref, lazy, action, reward, done, trick, stride, n, mix)
CASES = [
    ('policy_random+step', 1, 0, 0, 'default', 'given', 'null', 'given', 'given', 'N', 1, 'all'),
    ('policy_random+step', 1, 0, 0, 0, 'given', 'given', 'given', 'given', 'N', 63, 'all'),
    ('policy_random+step', 0, 1, 1, 0, 'given', 'given', 'null', 'null', 'N', 257, 'berac'),
    ('policy_random+step', 0, 0, 0, 'default', 'given', 'null', 'null', 'given', 'N', 773, 'berac'),
    ('policy_random+step', 0, 0, 0, 'default', 'given', 'given', 'null', 'given', 'N', 20077, 'all'),
    ('step', 1, 1, 1, 'default', 'given', 'given', 'null', 'given', 'N', 1, 'berac'),
    ('step', 1, 1, 1, 0, 'given', 'null', 'given', 'null', 'N', 63, 'berac'),
    ('step', 0, 1, 0, 'default', 'given', 'null', 'given', 'given', 'N', 257, 'all'),
    ('step', 0, 0, 0, 'default', 'given', 'null', 'given', 'null', 'N', 773, 'all'),
    ('step', 0, 0, 0, 0, 'given', 'given', 'null', 'given', 'N', 20077, 'all'),
    ('step_random', 0, 1, 1, 0, 'null', 'null', 'given', 'given', 'N', 1, 'berac'),
    ('step_random', 0, 0, 1, 'default', 'null', 'given', 'null', 'null', 'N', 63, 'all'),
    ('step_random', 1, 0, 0, 'default', 'given', 'null', 'given', 'given', 'N', 257, 'all'),
    ('step_random', 1, 0, 0, 'default', 'given', 'given', 'null', 'null', 'N', 773, 'all'),
    ('step_random', 0, 0, 1, 0, 'null', 'null', 'given', 'given', 'N', 20077, 'all'),
    ('krog:1', 0, 0, 1, 'default', 'given', 'null', 'given', 'null', 'N+192', 1, 'all'),
    ('krog:1', 1, 0, 0, 'default', 'given', 'given', 'null', 'null', 'N+192', 63, 'berac'),
    ('krog:1', 1, 0, 1, 0, 'null', 'given', 'given', 'given', 'N', 257, 'all'),
    ('krog:1', 0, 1, 1, 0, 'null', 'null', 'given', 'given', 'N', 773, 'all'),
    ('krog:1', 1, 0, 0, 0, 'given', 'given', 'given', 'given', 'N', 20077, 'all'),
    ('krog:2', 1, 0, 0, 'default', 'given', 'given', 'given', 'given', 'N+192', 1, 'berac'),
    ('krog:2', 0, 1, 1, 0, 'null', 'null', 'null', 'null', 'N', 63, 'all'),
    ('krog:2', 0, 0, 1, 'default', 'null', 'given', 'null', 'given', 'N+192', 257, 'berac'),
    ('krog:2', 1, 0, 1, 0, 'null', 'null', 'null', 'null', 'N', 773, 'all'),
    ('krog:2', 1, 0, 1, 'default', 'given', 'given', 'null', 'given', 'N+192', 20077, 'berac'),
    ('krog:3', 0, 1, 0, 'default', 'given', 'null', 'null', 'null', 'N', 1, 'all'),
    ('krog:3', 0, 1, 0, 'default', 'given', 'given', 'null', 'null', 'N', 63, 'berac'),
    ('krog:3', 1, 0, 1, 0, 'null', 'given', 'given', 'given', 'N+192', 257, 'berac'),
    ('krog:3', 1, 0, 0, 'default', 'given', 'given', 'given', 'null', 'N', 773, 'all'),
    ('krog:3', 1, 0, 0, 'default', 'null', 'null', 'given', 'given', 'N', 20077, 'berac'),
    ('krog:4', 0, 1, 0, 'default', 'given', 'null', 'null', 'null', 'N', 1, 'berac'),
    ('krog:4', 0, 1, 1, 'default', 'null', 'null', 'given', 'null', 'N', 63, 'berac'),
    ('krog:4', 0, 1, 0, 'default', 'null', 'given', 'null', 'given', 'N+192', 257, 'berac'),
    ('krog:4', 1, 0, 1, 0, 'null', 'given', 'given', 'given', 'N+192', 773, 'all'),
    ('krog:4', 0, 1, 0, 0, 'null', 'null', 'null', 'null', 'N', 20077, 'all'),
    ('krog:5', 1, 0, 1, 'default', 'null', 'given', 'null', 'null', 'N', 1, 'berac'),
    ('krog:5', 1, 1, 0, 'default', 'null', 'null', 'given', 'given', 'N', 63, 'all'),
    ('krog:5', 1, 0, 0, 'default', 'null', 'null', 'given', 'null', 'N+192', 257, 'all'),
    ('krog:5', 0, 0, 0, 0, 'given', 'given', 'null', 'given', 'N', 773, 'all'),
    ('krog:5', 1, 1, 1, 'default', 'null', 'null', 'given', 'null', 'N+192', 20077, 'all'),
    ('krog:7', 0, 1, 0, 0, 'given', 'given', 'null', 'null', 'N+192', 1, 'berac'),
    ('krog:7', 1, 0, 0, 0, 'null', 'null', 'null', 'null', 'N', 63, 'berac'),
    ('krog:7', 0, 0, 1, 'default', 'null', 'given', 'given', 'given', 'N+192', 257, 'all'),
    ('krog:7', 0, 0, 1, 'default', 'null', 'given', 'null', 'given', 'N+192', 773, 'berac'),
    ('krog:7', 1, 0, 1, 'default', 'null', 'null', 'given', 'given', 'N', 20077, 'all'),
    ('krog:48', 0, 0, 0, 0, 'null', 'null', 'null', 'null', 'N', 1, 'berac'),
    ('krog:48', 1, 1, 1, 'default', 'given', 'given', 'given', 'given', 'N+192', 63, 'all'),
    ('krog:48', 1, 1, 0, 'default', 'given', 'null', 'given', 'given', 'N', 257, 'all'),
    ('krog:48', 0, 0, 0, 'default', 'given', 'given', 'null', 'null', 'N', 773, 'all'),
    ('krog:48', 1, 1, 1, 'default', 'given', 'given', 'given', 'given', 'N+192', 20077, 'berac'),
    ('krog:128', 0, 1, 0, 0, 'given', 'null', 'given', 'given', 'N+192', 1, 'all'),
    ('krog:128', 1, 0, 1, 'default', 'null', 'given', 'null', 'null', 'N', 63, 'berac'),
    ('krog:128', 0, 1, 0, 0, 'null', 'null', 'null', 'given', 'N', 257, 'all'),
    ('krog:128', 0, 0, 1, 0, 'given', 'null', 'given', 'null', 'N', 773, 'all'),
    ('krog:128', 0, 0, 1, 'default', 'given', 'given', 'null', 'given', 'N+192', 20077, 'all'),
    ('krog:192', 0, 0, 1, 'default', 'given', 'given', 'given', 'given', 'N', 1, 'all'),
    ('krog:192', 1, 1, 0, 'default', 'given', 'null', 'given', 'null', 'N', 63, 'berac'),
    ('krog:192', 1, 1, 0, 0, 'null', 'given', 'null', 'null', 'N+192', 257, 'berac'),
    ('krog:192', 1, 1, 0, 0, 'given', 'given', 'given', 'given', 'N', 773, 'all'),
    ('krog:192', 1, 0, 1, 0, 'null', 'null', 'null', 'null', 'N+192', 20077, 'all'),
    ('run:0:eager', 0, 1, 1, 'default', 'given', 'null', 'null', 'null', 'N', 1, 'all'),
    ('run:0:eager', 0, 0, 0, 0, 'given', 'given', 'null', 'null', 'N', 63, 'all'),
    ('run:0:eager', 1, 1, 0, 0, 'given', 'null', 'given', 'null', 'N', 257, 'berac'),
    ('run:0:eager', 0, 0, 1, 'default', 'given', 'given', 'null', 'null', 'N', 773, 'all'),
    ('run:0:eager', 0, 1, 1, 0, 'given', 'given', 'given', 'null', 'N', 20077, 'all'),
    ('run:0:graph', 1, 1, 0, 0, 'given', 'given', 'null', 'null', 'N', 1, 'all'),
    ('run:0:graph', 0, 1, 1, 0, 'given', 'given', 'given', 'null', 'N', 63, 'all'),
    ('run:0:graph', 1, 1, 1, 0, 'given', 'null', 'null', 'null', 'N', 257, 'berac'),
    ('run:0:graph', 0, 0, 1, 0, 'given', 'given', 'given', 'null', 'N', 773, 'all'),
    ('run:0:graph', 0, 0, 1, 'default', 'given', 'null', 'given', 'null', 'N', 20077, 'berac'),
    ('run:1:eager', 0, 1, 1, 0, 'given', 'given', 'given', 'null', 'N', 1, 'all'),
    ('run:1:eager', 1, 0, 0, 'default', 'null', 'null', 'null', 'null', 'N', 63, 'all'),
    ('run:1:eager', 0, 1, 0, 'default', 'null', 'given', 'null', 'null', 'N', 257, 'berac'),
    ('run:1:eager', 0, 0, 0, 0, 'null', 'null', 'null', 'null', 'N', 773, 'berac'),
    ('run:1:eager', 0, 1, 0, 'default', 'null', 'given', 'given', 'null', 'N', 20077, 'berac'),
    ('run:1:graph', 1, 1, 1, 'default', 'given', 'null', 'null', 'null', 'N', 1, 'all'),
    ('run:1:graph', 1, 0, 1, 0, 'given', 'given', 'given', 'null', 'N', 63, 'all'),
    ('run:1:graph', 1, 0, 0, 0, 'null', 'given', 'null', 'null', 'N', 257, 'all'),
    ('run:1:graph', 0, 1, 0, 'default', 'null', 'null', 'null', 'null', 'N', 773, 'berac'),
    ('run:1:graph', 1, 0, 1, 0, 'given', 'given', 'null', 'null', 'N', 20077, 'all'),
    ('run:4:eager', 1, 0, 0, 0, 'null', 'given', 'null', 'null', 'N', 1, 'berac'),
    ('run:4:eager', 1, 0, 1, 'default', 'given', 'null', 'null', 'null', 'N', 63, 'berac'),
    ('run:4:eager', 0, 0, 0, 'default', 'null', 'given', 'given', 'null', 'N', 257, 'berac'),
    ('run:4:eager', 0, 1, 1, 'default', 'given', 'null', 'given', 'null', 'N', 773, 'all'),
    ('run:4:eager', 1, 0, 1, 'default', 'null', 'null', 'given', 'null', 'N', 20077, 'berac'),
    ('run:4:graph', 1, 1, 1, 'default', 'given', 'null', 'null', 'null', 'N', 1, 'all'),
    ('run:4:graph', 0, 0, 0, 0, 'null', 'null', 'null', 'null', 'N', 63, 'berac'),
    ('run:4:graph', 0, 0, 0, 0, 'null', 'given', 'given', 'null', 'N', 257, 'berac'),
    ('run:4:graph', 1, 1, 1, 0, 'null', 'given', 'null', 'null', 'N', 773, 'all'),
    ('run:4:graph', 1, 1, 0, 'default', 'null', 'given', 'null', 'null', 'N', 20077, 'all'),
    ('run:128:eager', 1, 1, 0, 'default', 'null', 'null', 'null', 'null', 'N', 1, 'all'),
    ('run:128:eager', 0, 0, 1, 0, 'given', 'given', 'given', 'null', 'N', 63, 'berac'),
    ('run:128:eager', 1, 0, 0, 'default', 'given', 'null', 'given', 'null', 'N', 257, 'berac'),
    ('run:128:eager', 0, 1, 0, 'default', 'given', 'null', 'given', 'null', 'N', 773, 'all'),
    ('run:128:eager', 0, 0, 1, 0, 'given', 'given', 'null', 'null', 'N', 20077, 'all'),
    ('run:128:graph', 1, 1, 1, 0, 'null', 'given', 'given', 'null', 'N', 1, 'berac'),
    ('run:128:graph', 0, 0, 1, 0, 'null', 'given', 'null', 'null', 'N', 63, 'all'),
    ('run:128:graph', 0, 0, 0, 'default', 'given', 'null', 'null', 'null', 'N', 257, 'all'),
    ('run:128:graph', 0, 1, 1, 0, 'null', 'null', 'given', 'null', 'N', 773, 'berac'),
    ('run:128:graph', 0, 0, 1, 0, 'given', 'given', 'given', 'null', 'N', 20077, 'berac'),
    ('policy_step', 0, 1, 1, 0, 'given', 'null', 'null', 'given', 'N', 1, 'all'),
    ('policy_step', 0, 0, 1, 'default', 'given', 'given', 'null', 'given', 'N', 63, 'all'),
    ('policy_step', 0, 1, 0, 'default', 'given', 'null', 'null', 'null', 'N', 257, 'all'),
    ('policy_step', 1, 0, 1, 0, 'given', 'given', 'given', 'given', 'N', 773, 'berac'),
    ('policy_step', 1, 0, 0, 'default', 'given', 'null', 'given', 'given', 'N', 20077, 'berac'),
]
FULL_SLOTS = 773                         # batches up to this size are modelled slot by slot


def modelled_slots(n):
    if n <= FULL_SLOTS:
        return np.arange(n)
    return np.unique(np.concatenate([np.arange(0, n, 29), np.arange(64), np.arange(n - 64, n)]))


def _first_bad(got, exp, slots):
    bad = np.argwhere(got != exp)
    if bad.size == 0:
        return None
    b = tuple(int(x) for x in bad[0])
    return dict(row=b[0], slot=int(slots[b[1]]), got=got[b].tolist(), expected=exp[b].tolist(), wrong=len(bad))


class Outputs:
    """The guarded output arrays of one case and the model's expectation for the modelled slots."""

    def __init__(self, rows, n, stride, slots, given):
        from guarded import Guarded
        mk = lambda name, dt, inner=(): Guarded(name, rows, n, dt, inner=inner, stride=stride, device="cuda")
        self.rows, self.n, self.slots = rows, n, slots
        self.obs = mk("obs_out", np.uint64)
        self.action = mk("action_out", np.uint8) if given["action"] else None
        self.reward = mk("reward_out", np.int16, (4,)) if given["reward"] else None
        self.done = mk("done_out", np.uint8) if given["done"] else None
        self.trick = mk("trick_out", np.uint16) if given["trick"] else None

    def arrays(self):
        return [self.obs, self.action, self.reward, self.done, self.trick]

    def begin_call(self):
        for a in self.arrays():
            if a is not None:
                a.fill()
        m = len(self.slots)
        self.e_obs = np.zeros((self.rows, m), np.uint64)
        self.e_action = np.zeros((self.rows, m), np.uint8)
        self.e_done = np.zeros((self.rows, m), np.uint8)
        self.e_trick = np.zeros((self.rows, m), np.uint16)
        self.e_reward = np.zeros((self.rows, m, 4), np.int16)
        self.e_finished = np.zeros((self.rows, m), bool)      # a reward row was written during this call

    def expect(self, c, j, row):
        """Row c of modelled slot number j is overwritten by `row` (a later launch of the same call overwrites an earlier
        one's; a reward row only where the game finished)."""
        self.e_obs[c, j], self.e_action[c, j], self.e_done[c, j], self.e_trick[c, j] = row.obs, row.action, row.done, row.trick
        if row.done:
            self.e_reward[c, j] = row.reward
            self.e_finished[c, j] = True

    def check(self, tag, judge_action=True):
        from guarded import assert_guards_intact
        assert_guards_intact(self.arrays(), tag)
        s = self.slots
        pairs = [("obs_out", self.obs, self.e_obs), ("done_out", self.done, self.e_done), ("trick_out", self.trick, self.e_trick)]
        if judge_action:
            pairs.append(("action_out", self.action, self.e_action))
        for name, arr, exp in pairs:
            if arr is None:
                continue
            vals, written = arr.host()
            assert written[:, s].all(), (tag, name, "rows not written", _first_bad(written[:, s], np.ones_like(written[:, s]), s))
            bad = _first_bad(vals[:, s], exp, s)
            assert bad is None, (tag, name, bad)
        if self.reward is not None:
            vals, written = self.reward.host()
            bad = _first_bad(written[:, s], self.e_finished, s)
            assert bad is None, (tag, "reward_out written exactly where the game finished", bad)
            f = self.e_finished
            bad = _first_bad(vals[:, s][f][None], self.e_reward[f][None], np.argwhere(f)[:, 1] if f.any() else s)
            assert bad is None, (tag, "reward_out", bad)


def _explicit_cards(rnd, models, base):
    """tarok_step's cards: the legal / illegal / garbage mix of test_random_api_sequences_against_an_oracle_model for the
    modelled slots, `base` (the Bot policy's card) for the others."""
    acts = base.copy()
    for i, m in models:
        legal = m.legal()
        u = rnd.rand()
        if legal and u < 0.85:
            ids = [c for c in range(54) if (legal >> c) & 1]
            acts[i] = ids[rnd.randint(len(ids))]
        elif u < 0.95:
            acts[i] = rnd.randint(0, 54)              # often illegal
        else:
            acts[i] = rnd.randint(54, 256)            # garbage
    return acts


def check_against_models(env, models, tag):
    """Canonical state, episode numbers, score sums, observation words and (history env) the history rows of the cards
    played, for the modelled slots."""
    st = env.state()
    ep, ss = env.counters()
    words = env.legal_actions().words.cpu().numpy().view(np.uint64)
    hist = env.get_history().cpu().numpy() if env.history else None
    for i, m in models:
        assert (st[:, i] == m.g.lanes()).all(), (tag, "state", i)
        assert ep[i] == m.ep and list(ss[i]) == m.sum, (tag, "counters", i)
        assert int(words[i]) == m.g.obs_word(False), (tag, "observation word", i)
        if hist is not None:
            assert hist[:m.played, i].tolist() == m.hist[:m.played], (tag, "history", i)
