"""GPU: the OUTPUT ROWS of every step launch kind on games that began on a FRONTED next-game line.

tests/test_gpu_front_lines.py pins the words tarok_front_lines writes into the lines; tests/test_gpu_output_contract.py
pins every output row of every launch kind, but only on lines deal_into_buffer wrote.  Here the two meet: an env of
n = 300 (two step groups, the second partial), K.MIX_BOT, auto-reset, reset(0) + prefetch(), then ONE front_lines call
with both heads, contracts = 0x3FF and per-slot seat sets (the empty set and partial sets among them), so that the
fourteen lines of a slot are a mix of head-decided and Bot-decided games, all marked.  Then 144 lock-steps (the next
multiple of the launch length where it does not divide 144) of one launch kind, and after EVERY launch what
test_gpu_output_contract.py requires: guard bands and padding columns intact, reward rows of unfinished games
untouched, action / done / reward / trick / obs rows equal to the model bit for bit, history rows below the number of
cards played; after the last launch state(), counters() and the observation words.

The model is tests/oracle_model.SlotModel with its game_of hook.  The START of the game of (slot, episode) is
Game.from_lanes of the TWIN CHAIN's lanes at that episode (bid_values -> bid_round -> reset(defer_exchange) ->
exchange_values -> exchange -> state(): each link pinned elsewhere, neither front_lines nor a step kernel in it); one
case takes it from tests/front_lines_model.front_game on integer weights instead (pure CPU).  Everything after the start
is the oracle.  A game whose episode lies beyond the call's fourteen lines (a slot that ran through many short Berac
games) started on a line dealt after the call: unmarked, the Bot's — the synthetic game.

For the network kinds the card is not predicted: the written action is fed to the model as an explicit card and must be
legal (tarok_policy_step_seats: on a Bot seat it must be the Bot's card under the line's key); every other row is exact.

The module fixture asserts, from the twin chain and front_lines_model.bot_line alone and before any step kernel runs,
that the lines every run consumes (episodes 1 and 2 of every slot: 144 lock-steps end at least two games) hold a Klop, a
Berac or open Berac, an exchange that differs from the Bot's, a Solo-without or higher, and differ from the Bot's line
of the same key in a quarter of the cases or more; every case repeats this over the lines it did consume.

tarok_run_random with 128 cards a launch takes multiples of 128: its graph chunk is 128, which does not divide 144.

Run on the GPU box:  python -m pytest tests/test_gpu_front_rows.py -m gpu -q
"""
import numpy as np
import pytest

from gpu_harness import T  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

STEPS = 144
HEAD_GAIN, HEAD_SCALE = 4.0, 70.0
RUN_STEPS = {0: 3, 1: 3, 4: 8, 128: 128}     # lock-steps per tarok_run_random call (= the graph chunk when replayed)

# kind -> options (hist: TAROK_HISTORY env, ref: TAROK_REWARD_REF, pad: stride = n + pad, lazy: TAROK_OPT_LAZY_REFILL,
# one: a one-slot env, mode: (temperature, epsilon))
CASES = [
    ("policy_random+step", {}),
    ("step", {}),
    ("step_random", {}),
    ("krog:2", dict(hist=True)),
    ("krog:4", {}),
    ("krog:7", dict(pad=192)),
    ("krog:48", dict(ref=True)),
    ("krog:128", {}),
    ("krog:128", dict(lazy=0)),
    ("krog:4", dict(one=True)),
] + [("run:%d:%s" % (c, m), {}) for c in (0, 1, 4, 128) for m in ("eager", "graph")] + [
    ("policy_step", {}),
    ("policy_step_seats", {}),
    ("policy_step_versus", {}),
    ("policy_step_pool", {}),
    ("policy_step_versus", dict(mode=(0.5, 0.25))),
]


def case_id(case):
    return case[0] + "".join("-%s=%s" % kv for kv in sorted(case[1].items()))


@pytest.fixture(scope="module")
def world(T):
    """The front_lines call of every case and what its lines must hold: twin[e] / bot[e] are the lanes [10, N] of the
    twin chain's and of the Bot's game of episode e = 1..14; differ[e], family[e] and xdiff[e] say per slot whether the
    two differ, the contract, and whether the exchange differs from the Bot's exchange of the same contract."""
    import front_lines_model as FM
    import front_lines_cases as FL
    from oracle import oracle as O
    from oracle import tarok_spec as S
    n = FL.N
    sets = FL.sets_tensor(n)
    assert (sets == 0).any() and (sets == 15).any() and ((sets != 0) & (sets != 15)).any()
    kw = dict(bid=FL.random_weights(11, HEAD_GAIN), exchange=FL.random_weights(12, HEAD_GAIN), scale=HEAD_SCALE, contracts=0x3FF,
              seats_per_game=sets)
    w = dict(kw=kw, sets=sets, twin={}, bot={}, differ={}, contract={}, xdiff={}, keys={})
    for e in range(1, FL.AHEAD + 1):
        twin, keys = FL.twin_chain(T, e, kw)
        bot = np.stack([FM.bot_line(FL.SEED, FL.OFFSET + j, e, S.MIX_BOT).lanes() for j in range(n)], axis=1)
        contract = ((twin[9] >> np.uint64(33)) & np.uint64(15)).astype(np.int64)
        xdiff = np.zeros(n, bool)
        for j in np.nonzero(np.array(S.N_DISCARD)[contract] > 0)[0]:     # the same contract with the Bot's exchange
            m = int(twin[9, j])
            king = (m >> 39) & 7
            g = O.Game(S.deal(int(keys[j])), int(contract[j]), (m >> 37) & 3, -1 if king == 7 else king)
            FM.bot_exchange(g, int(keys[j]))
            xdiff[j] = (g.lanes() != twin[:, j]).any()
        w["twin"][e], w["bot"][e], w["keys"][e] = twin, bot, keys
        w["differ"][e], w["contract"][e], w["xdiff"][e] = (twin != bot).any(axis=0), contract, xdiff
    w["game_of"] = game_of(w)
    assert_not_vacuous(w, [(j, e) for j in range(n) for e in (1, 2)], "the lines every run consumes")
    return w


def game_of(w):
    """SlotModel's hook: the twin chain's game for the fourteen lines of the call, the synthetic one elsewhere."""
    import front_lines_cases as FL
    from oracle import oracle as O

    def hook(index, ep):
        if not 1 <= ep <= FL.AHEAD:
            return None
        j = index - FL.OFFSET
        return O.Game.from_lanes(w["twin"][ep][:, j]), int(w["keys"][ep][j])
    return hook


def assert_not_vacuous(w, consumed, tag):
    """consumed: [(slot, episode)] with episode within the call's lines."""
    from oracle import tarok_spec as S
    c = np.array([w["contract"][e][j] for j, e in consumed])
    d = np.array([w["differ"][e][j] for j, e in consumed])
    x = np.array([w["xdiff"][e][j] for j, e in consumed])
    print(tag, "lines", len(consumed), "contracts", np.bincount(c, minlength=10).tolist(), "differ from the Bot's", int(d.sum()),
          "exchange differs", int(x.sum()))
    assert (c == S.KLOP).any(), (tag, "no Klop")
    assert np.isin(c, (S.BERAC, S.ODPRTI_BERAC)).any(), (tag, "no Berac")
    assert x.any(), (tag, "no exchange that differs from the Bot's")
    assert (c >= S.SOLO_BREZ).any(), (tag, "no Solo-without or higher")
    assert 4 * int(d.sum()) >= len(consumed), (tag, "fewer than a quarter of the lines differ from the Bot's", int(d.sum()), len(consumed))


class Run:
    """One env behind one launch kind, its guarded outputs and its models; play() is a stretch of lock-steps."""

    def __init__(self, T, kind, opt, n, offset, sets, hook, slots=None):
        import torch
        import front_lines_cases as FL
        import output_contract_cases as G
        from oracle_model import SlotModel
        from tarok_amd import karte as K
        self.G, self.kind, self.part, self.n, self.sets = G, kind, kind.split(":"), n, sets
        self.ref = bool(opt.get("ref"))
        self.flags = K.AUTO_RESET | (K.REWARD_REF if self.ref else 0)
        self.cards = int(self.part[1]) if self.part[0] in ("krog", "run") else 1
        self.rows = max(self.cards, 1)
        self.stride = n + opt.get("pad", 0)
        self.env = T.TarokVecEnv(n, seed=FL.SEED, mix=K.MIX_BOT, game_offset=offset, history=bool(opt.get("hist")),
                                 lazy_refill=opt.get("lazy"))
        self.env.reset(episode=0)
        self.env.prefetch()
        if "mode" in opt:
            self.env.set_play_mode(*opt["mode"])
        self.slots = np.arange(n) if slots is None else np.asarray(slots)
        self.models = [(int(j), SlotModel(FL.SEED, offset + int(j), K.MIX_BOT, game_of=hook)) for j in self.slots]
        self.out = G.Outputs(self.rows, n, self.stride, self.slots, dict(action=True, reward=True, done=True, trick=self.part[0] != "run"))
        self.rnd = np.random.RandomState(77)
        self.sets_host = sets.cpu().numpy()
        self.launch = 0
        if kind.startswith("policy_step"):
            self.logp = torch.zeros(n, dtype=torch.float32, device="cuda")
            self.value = torch.zeros(n, dtype=torch.float32, device="cuda")
            self.net = FL.random_weights(13)
            self.other = FL.random_weights(14)
            self.pool = T.TarokVecEnv.stack_pool([FL.random_weights(s) for s in (14, 15, 16)])

    def close(self):
        self.env.close()

    def play(self, steps):
        """At least `steps` lock-steps in whole launches (tarok_run_random: whole calls); every launch checked."""
        import torch
        from oracle import oracle as O
        from tarok_amd import _native
        env, out, kind, part, G = self.env, self.out, self.kind, self.part, self.G
        L, h, p, stream = env.L, env._h, env._p, env._stream
        ptr = lambda a: None if a is None else a.ptr
        per_call = RUN_STEPS[self.cards] if part[0] == "run" else self.rows
        auto, ref = True, self.ref
        for _ in range(-(-steps // per_call)):
            tag = (kind, "launch", self.launch)
            self.launch += 1
            out.begin_call()
            given = None
            env_out = (ptr(out.reward), ptr(out.done), ptr(out.trick), out.obs.ptr, self.flags, stream())
            with torch.cuda.device(env.device):
                if kind == "policy_random+step":
                    _native.check(L.tarok_policy_random(h, p(env.legal_actions().words), out.action.ptr, stream()))
                    _native.check(L.tarok_step(h, out.action.ptr, *env_out))
                elif kind == "step":
                    base = env.policy_random(env.legal_actions()).cpu().numpy()
                    given = G._explicit_cards(self.rnd, self.models, base)
                    a_dev = torch.from_numpy(given).cuda()
                    _native.check(L.tarok_step(h, p(a_dev), *env_out))
                elif kind == "step_random":
                    _native.check(L.tarok_step_random(h, out.action.ptr, *env_out))
                elif part[0] == "krog":
                    _native.check(L.tarok_krog_random(h, self.cards, self.stride, out.action.ptr, *env_out))
                elif part[0] == "run":
                    if self.cards == 0:               # the policy kernel of every step reads obs_out: it starts as the current observation
                        _native.check(L.tarok_legal_actions(h, out.obs.ptr, None, stream()))
                    _native.check(L.tarok_run_random(h, per_call, self.cards, per_call if part[2] == "graph" else 0, 0, out.action.ptr,
                                                     ptr(out.reward), ptr(out.done), out.obs.ptr, self.flags, stream()))
                else:
                    words = env.legal_actions().words
                    head = [out.action.ptr, p(self.logp), p(self.value), None]
                    net, sets = [p(t) for t in self.net], (15, p(self.sets))
                    if kind == "policy_step":
                        _native.check(L.tarok_policy_step(h, *net, p(words), *head, *env_out))
                    elif kind == "policy_step_seats":
                        _native.check(L.tarok_policy_step_seats(h, *sets, *net, p(words), *head, *env_out))
                    elif kind == "policy_step_versus":
                        _native.check(L.tarok_policy_step_versus(h, *sets, *net, *[p(t) for t in self.other], p(words), *head, *env_out))
                    else:
                        _native.check(L.tarok_policy_step_pool(h, *sets, *net, 3, *[p(t) for t in self.pool], None, p(words), *head, *env_out))
                torch.cuda.synchronize()
            if kind.startswith("policy_step"):        # the model takes the card the kernel reports: it must be a legal one
                acts, _ = out.action.host()
                for k, (j, m) in enumerate(self.models):
                    a, legal = int(acts[0, j]), m.legal()
                    assert (a == 255) if not legal else (a < 54 and (legal >> a) & 1), (tag, "card not in the legal mask", j, a, legal)
                    if kind == "policy_step_seats" and legal and not (int(self.sets_host[j]) >> m.g.seat()) & 1:
                        pos = m.g.g.trick_no * 4 + m.g.g.n_in_trick
                        assert a == int(O.lib().to_policy_action(m.key, pos, legal)), (tag, "a Bot seat's card under the line's key", j)
                    out.expect(0, k, m.card(a, auto, ref))
            else:
                for _ in range(per_call // self.rows):
                    for r in range(self.rows):
                        for k, (j, m) in enumerate(self.models):
                            out.expect(r, k, m.card(None if given is None else int(given[j]), auto, ref))
            # (tarok_step's card array is an input; cards_per_launch = 1 leaves `action` alone: nothing to compare there)
            out.check(tag, judge_action=kind not in ("step", "run:1:eager", "run:1:graph"))
            if env.history:
                hist = env.get_history().cpu().numpy()
                for j, m in self.models:
                    assert hist[:m.played, j].tolist() == m.hist[:m.played], (tag, "history", j)

    def check_end(self, tag):
        self.G.check_against_models(self.env, self.models, tag)


def front_once(env, kw):
    import front_lines_cases as FL
    count, _ = FL.front(env, **kw)
    assert count == FL.AHEAD * env.n
    _, _, nep, mark = FL.split(env.get_lines())
    assert FL.valid_lines(env, nep).all() and (mark == nep).all(), "fourteen valid lines a slot, all marked"


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_rows_on_fronted_lines(T, world, case):
    import front_lines_cases as FL
    kind, opt = case
    n, offset, sets, base = FL.N, FL.OFFSET, world["sets"], 0
    if opt.get("one"):                   # one slot: the first whose set is 15 and whose first three lines all differ from the Bot's
        base = next(j for j in range(FL.N) if int(sets[j]) == 15 and all(world["differ"][e][j] for e in (1, 2, 3)))
        n, offset, sets = 1, FL.OFFSET + base, sets[base:base + 1].clone()
    run = Run(T, kind, opt, n, offset, sets, world["game_of"])
    try:
        front_once(run.env, dict(world["kw"], seats_per_game=sets))
        run.play(STEPS)
        run.check_end((case_id(case), "end"))
        eps = np.array([m.ep for _, m in run.models])
        assert (eps >= 2).all(), "every slot's episode counter advanced by at least 2"
        consumed = [(base + j, e) for j, m in run.models for e in range(1, min(m.ep, FL.AHEAD) + 1)]
        if opt.get("one"):
            assert all(world["differ"][e][j] for j, e in consumed[:2])
        else:
            assert_not_vacuous(world, consumed, case_id(case))
    finally:
        run.close()


def test_rows_on_integer_weight_lines_against_the_cpu_model(T):
    """krog:4 on the lines of a call with the integer weight sets of tests/policy_exact_ref.py (sums exact in
    float32 in any order): the start of every game is tests/front_lines_model.front_game, no GPU in the reference at all.
    Every third slot is modelled; the others keep their guards."""
    import front_lines_model as FM
    import front_lines_cases as FL
    import policy_exact_ref as PE
    from oracle import tarok_spec as S
    Wb, Wx = PE.weights_p(*PE.P_PARAMS[1]), PE.weights_p(*PE.P_PARAMS[8])
    sets = FL.sets_tensor(FL.N)
    seats = sets.cpu().numpy()
    bid = dict(W=Wb, scale=64.0, playouts=1, margin=1, contracts=0x3FF, pass_value=False)
    started = {}

    def hook(index, ep):
        if not 1 <= ep <= FL.AHEAD:
            return None
        front = lambda: FM.front_game(FL.SEED, index, ep, int(seats[index - FL.OFFSET]), S.MIX_BOT, bid=bid, exchange=Wx)
        started[(index - FL.OFFSET, ep)] = front().lanes()
        return front(), S.game_key(FL.SEED, index, ep)
    run = Run(T, "krog:4", {}, FL.N, FL.OFFSET, sets, hook, slots=np.arange(0, FL.N, 3))
    try:
        front_once(run.env, dict(bid=PE.kernel_weights(T, Wb), exchange=PE.kernel_weights(T, Wx), scale=64.0, contracts=0x3FF, margin=1,
                                 seats_per_game=sets))
        run.play(STEPS)
        run.check_end("end")
        assert all(m.ep >= 2 for _, m in run.models), "every slot's episode counter advanced by at least 2"
        differ = [(lanes != FM.bot_line(FL.SEED, FL.OFFSET + j, e, S.MIX_BOT).lanes()).any() for (j, e), lanes in started.items()]
        contracts = {int((int(lanes[9]) >> 33) & 15) for lanes in started.values()}
        print("integer weights: games started", len(started), "differ from the Bot's", int(np.sum(differ)), "contracts", sorted(contracts))
        assert 4 * int(np.sum(differ)) >= len(differ) and len(contracts) >= 3
    finally:
        run.close()


def test_rows_with_a_second_call_between_refills(T, world):
    """64 lock-steps of krog:4, prefetch(), a second front_lines call — with OTHER head weights, so that a line of the first
    call that the second decided again would show —, 80 more.  The lines dealt again since the first call are taken by the
    second and hold its chain's games; the first call's keep theirs.  The marks are read before each stretch: a game of
    (slot, episode) starts as the twin chain's of the call that marked its line, and as the Bot's if no call did (a line
    still on a refill list at the second call, or dealt after it).  With 80 lock-steps left a slot rarely gets past its
    fourteenth game: what the rows see of the second call is mostly that it left the lines ahead of the slots alone."""
    import front_lines_cases as FL
    from oracle import oracle as O
    from oracle import tarok_spec as S
    calls = [world["kw"], dict(world["kw"], bid=FL.random_weights(21, HEAD_GAIN), exchange=FL.random_weights(22, HEAD_GAIN))]
    chains, fronted = {(0, e): lanes for e, lanes in world["twin"].items()}, {}

    def hook(index, ep):
        j = index - FL.OFFSET
        if (j, ep) not in fronted:
            return None
        k = fronted[(j, ep)]
        if (k, ep) not in chains:
            chains[(k, ep)] = FL.twin_chain(T, ep, calls[k])[0]
        return O.Game.from_lanes(chains[(k, ep)][:, j]), S.game_key(FL.SEED, index, ep)

    def read_marks(env, call):
        """(valid, valid and unmarked, valid and marked by this call) [n, 14]; `fronted` learns the lines this call marked."""
        _, _, nep, mark = FL.split(env.get_lines())
        valid = FL.valid_lines(env, nep)
        new = np.zeros_like(valid)
        for j, b in zip(*np.nonzero(valid & (mark == nep))):
            new[j, b] = fronted.setdefault((int(j), int(nep[j, b])), call) == call
        return valid, valid & (mark != nep), new
    run = Run(T, "krog:4", {}, FL.N, FL.OFFSET, world["sets"], hook)
    try:
        env = run.env
        front_once(env, calls[0])
        valid, unmarked, new = read_marks(env, 0)
        assert new.all() and len(fronted) == FL.AHEAD * FL.N
        run.play(64)
        env.prefetch()
        valid, unmarked, new = read_marks(env, 0)
        ended = int(env.counters()[0].sum())
        # one line dealt again, unmarked, for every game that ended — but for those still on a refill list (stale tag):
        # the next launch deals them, unmarked, and the model plays the Bot's game there
        assert 0 < unmarked.sum() <= ended and int(valid.sum()) == FL.AHEAD * FL.N - (ended - int(unmarked.sum()))
        count, _ = FL.front(env, **calls[1])
        assert count == int(unmarked.sum()), "the second call takes exactly the valid lines dealt again"
        valid, still, second = read_marks(env, 1)
        assert not still.any() and (second == unmarked).all()
        FL.assert_lines_are_twins(T, env, second, calls[1])
        FL.assert_lines_are_twins(T, env, valid & ~second, calls[0])
        mid = {j: m.ep for j, m in run.models}
        run.play(80)
        run.check_end("end")
        assert all(m.ep >= 2 for _, m in run.models), "every slot's episode counter advanced by at least 2"
        assert any(m.ep > mid[j] for j, m in run.models)
        print("second call: slots that started a game of its lines", sum(1 for j, m in run.models if fronted.get((j, m.ep)) == 1),
              "highest episode", max(m.ep for _, m in run.models))
        assert_not_vacuous(world, [(j, e) for j, m in run.models for e in range(1, min(m.ep, FL.AHEAD) + 1)], "two calls")
    finally:
        run.close()
