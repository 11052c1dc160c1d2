"""GPU: the 256 observation features, bit for bit against the oracle-side statement (tests/observe_model.py).

The encoder exists as two instruction streams — k_observe (tarok_observe) and policy_feature_words() (the fused policy
launches: features_out and feature_words_out of tarok_policy_mlp, feature_words_out of tarok_policy_step) — and every
network of the project reads it.  Here every row of every launch is compared with the statement on the CPU oracle's own
game of that slot (tests/oracle_model.py follows the slots; nothing is decoded from the device's state): whole games card
by card with auto-reset, the 2,880 games recorded from the reference, games waiting for the exchange and finished games,
positions reached by multi-card launches and by set_state(), ragged sizes, and tarok_expand_features.  All comparisons
are of bits: no tolerance anywhere, no row sampled.  Every output sits between guard bands (tests/guarded.py).

tests/test_observe_model_cpu.py pins the statement itself to the reference's recording and counts what the positions
used here cover (tests/observe_cases.py).

Run on the GPU box:  python -m pytest tests/test_gpu_observe_features.py -m gpu -q
"""
import os

import numpy as np
import pytest

import observe_cases as OC
import observe_model as OM
from guarded import Guarded, assert_guards_intact
from gpu_harness import T  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

MODEL = OM.Statement()


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def S():
    from oracle import tarok_spec
    return tarok_spec


@pytest.fixture(scope="module")
def KW(T):
    """An integer weight set of tests/policy_exact_ref.py in the kernels' layout (the weights do not matter here)."""
    from policy_exact_ref import kernel_weights, weights_r
    return kernel_weights(T, weights_r())


@pytest.fixture(scope="module")
def traces(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "traces_v1.npz")))


def view(G, torch_dtype, shape):
    """The payload of a guarded array as a device tensor a wrapper of tarok_amd.env takes for an output."""
    return G.payload().view(torch_dtype).view(*shape)


def all_written(G, tag):
    vals, written = G.host()
    assert written.all(), ("rows not written", G.name, tag, np.argwhere(~written)[:8].tolist())
    return vals[0]


def assert_rows(got, want_words, tag):
    """got [n, 256] 0 / 1 against the statement's words of every row."""
    want = OM.expand(want_words)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, (tag, "%d rows differ" % len(bad), [(int(i), np.nonzero(got[i] != want[i])[0].tolist()) for i in bad[:6]])


class Launches:
    """The three feature outputs of one env between guard bands: tarok_observe's rows, and features_out and
    feature_words_out of tarok_policy_mlp (with its action, logp and value rows)."""

    def __init__(self, env, kw):
        import torch
        self.torch, self.env, self.kw, n = torch, env, kw, env.n
        dev = env.device
        self.obs = Guarded("tarok_observe", 1, n, np.uint16, inner=(256,), device=dev)
        self.feat = Guarded("features_out", 1, n, np.uint16, inner=(256,), device=dev)
        self.fw = Guarded("feature_words_out", 1, n, np.uint64, inner=(4,), device=dev)
        self.act = Guarded("action_out", 1, n, np.uint8, device=dev)
        self.logp = Guarded("logp_out", 1, n, np.float32, device=dev)
        self.val = Guarded("value_out", 1, n, np.float32, device=dev)
        self.all = [self.obs, self.feat, self.fw, self.act, self.logp, self.val]

    def observe(self, tag):
        """tarok_observe -> [n, 256] 0 / 1 (every row written, guards intact, only the two bf16 patterns)."""
        self.obs.fill()
        self.env.observe(out=view(self.obs, self.torch.bfloat16, (self.env.n, 256)))
        assert_guards_intact([self.obs], tag)
        return OM.from_bf16(all_written(self.obs, tag))

    def mlp(self, words, tag, feat=True, fw=True):
        """tarok_policy_mlp -> (features_out as [n, 256] 0 / 1 or None, feature_words_out as [n, 4] uint64 or None)."""
        t, n = self.torch, self.env.n
        for g in self.all[1:]:
            g.fill()
        self.env.policy_mlp(self.kw, words, action_out=view(self.act, t.uint8, (n,)), logp_out=view(self.logp, t.float32, (n,)),
                            value_out=view(self.val, t.float32, (n,)),
                            features_out=view(self.feat, t.bfloat16, (n, 256)) if feat else None,
                            feature_words_out=view(self.fw, t.int64, (n, 4)) if fw else None)
        assert_guards_intact(self.all[1:], tag)
        for g in (self.act, self.logp, self.val):
            all_written(g, tag)
        for g, used in ((self.feat, feat), (self.fw, fw)):
            if not used:
                assert not g.host()[1].any(), ("an output that was not given was written", g.name, tag)
        return (OM.from_bf16(all_written(self.feat, tag)) if feat else None, all_written(self.fw, tag).copy() if fw else None)

    def check(self, words, want_words, tag):
        """All three outputs on the env's current position against the statement's words."""
        want = OM.words_array(want_words)
        assert_rows(self.observe(tag), want, (tag, "tarok_observe"))
        feat, fw = self.mlp(words, tag)
        assert_rows(feat, want, (tag, "features_out"))
        bad = np.nonzero((fw != want).any(axis=1))[0]
        assert len(bad) == 0, (tag, "feature_words_out", [(int(i), [hex(int(x)) for x in fw[i]], [hex(int(x)) for x in want[i]]) for i in bad[:6]])

    def no_error(self, tag):
        assert not self.env.legal_actions().error.any().item(), ("a launch flagged an error", tag)


def model_words(slots):
    return [MODEL.words(s.g) for s in slots]


# ---- a. whole games, every card
@pytest.mark.parametrize("name,mix,n,seed", OC.WHOLE, ids=[w[0] for w in OC.WHOLE])
def test_whole_games_every_card(T, KW, name, mix, n, seed):
    """STEPS lock-steps of tarok_step_random with auto-reset; before every step tarok_observe's rows and tarok_policy_mlp's
    features_out and feature_words_out equal the statement on every slot's own oracle game."""
    env = T.TarokVecEnv(n, seed=seed, mix=mix)
    obs = env.reset()
    slots = OC.slots_of(seed, mix, n)
    L = Launches(env, KW)
    for t in range(OC.STEPS):
        L.check(obs.words, model_words(slots), (name, t))
        obs, _, _ = env.step_random(auto_reset=True)
        OC.play(slots, auto=True)
    L.no_error(name)
    assert any(s.ep > 0 for s in slots)                 # renewed games (what the positions cover: tests/test_observe_model_cpu.py)
    env.close()


def test_policy_step_twin_writes_the_observation_before_the_step(T, KW):
    """An env driven by tarok_policy_step (the network's own cards, auto-reset): feature_words_out of every launch is the
    statement on the position BEFORE the card, on the slot's oracle game replayed with the cards the launch played."""
    import torch
    name, mix, n, seed = OC.WHOLE[0]
    env = T.TarokVecEnv(n, seed=seed, mix=mix)
    slots = OC.slots_of(seed, mix, n)
    words = [Guarded("obs_out %d" % k, 1, n, np.int64, device=env.device) for k in (0, 1)]
    fw = Guarded("feature_words_out", 1, n, np.uint64, inner=(4,), device=env.device)
    act = Guarded("action_out", 1, n, np.uint8, device=env.device)
    view(words[0], torch.int64, (n,)).copy_(env.reset().words)
    last_trick_renewed = 0
    for t in range(OC.STEPS):
        want = OM.words_array(model_words(slots))
        src, dst = words[t & 1], words[(t + 1) & 1]
        for g in (dst, fw, act):
            g.fill()
        env.policy_step(KW, view(src, torch.int64, (n,)), view(dst, torch.int64, (n,)), view(act, torch.uint8, (n,)),
                        feature_words_out=view(fw, torch.int64, (n, 4)), auto_reset=True)
        assert_guards_intact([dst, fw, act], t)
        got, cards = all_written(fw, t), all_written(act, t)
        all_written(dst, t)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert len(bad) == 0, (t, [(int(i), [hex(int(x)) for x in got[i]], [hex(int(x)) for x in want[i]]) for i in bad[:6]])
        for s, c in zip(slots, cards):
            last = s.g.g.trick_no == 11 and s.g.g.n_in_trick == 3
            row = s.card(int(c), auto=True)
            assert not row.rejected, (t, s.i, int(c))
            last_trick_renewed += 1 if last and s.g.g.trick_no == 0 else 0
    assert last_trick_renewed > 0                       # rows whose game was renewed inside the launch that wrote them
    assert not env.legal_actions().error.any().item()
    env.close()


# ---- b. the games recorded from the reference, on the device
def test_reference_traces_every_step(T, O, S, KW, traces):
    """The 2,880 recorded games with their explicit deals, exchanges and cards: at every step tarok_observe and
    tarok_policy_mlp's feature outputs equal the statement on the oracle's replay — whose legal region is the
    reference's recorded mask (tests/test_observe_model_cpu.py).  Games that finished earlier are non-live rows."""
    tr = traces
    n = len(tr["contract"])
    assert n == 2880
    env = T.TarokVecEnv(n, seed=0, mix=T.karte.MIX_ALL)
    king = np.where(tr["king"] < 0, 0, tr["king"]).astype(np.int8)
    choice = np.where(tr["choice"] < 0, 0, tr["choice"]).astype(np.int8)
    obs = env.reset(deals=tr["deals"], contract=tr["contract"], declarer=tr["declarer"], king_suit=king, talon_choice=choice,
                    discards=tr["discards"])
    games = []
    for i in range(n):
        g = O.Game(tr["deals"][i], tr["contract"][i], tr["declarer"][i], tr["king"][i])
        if g.g.phase == OM.PHASE_EXCHANGE:
            assert g.exchange(tr["choice"][i], tr["discards"][i][: S.N_DISCARD[int(tr["contract"][i])]]) == 0
        games.append(g)
    L = Launches(env, KW)
    for t in range(49):
        want = [MODEL.words(g) for g in games]
        live = tr["nsteps"] > t
        legal = np.array([w[1] & OM.DECK for w in want], dtype=np.uint64)
        assert (legal == np.where(live, tr["masks"][:, min(t, 47)].astype(np.uint64), np.uint64(0))).all(), t
        L.check(obs.words, want, ("traces", t))
        assert not obs.error.any().item(), t
        if t == 48:
            break
        obs, _, _ = env.step(tr["actions"][:, t])
        for i in np.nonzero(live)[0]:
            assert games[i].step(tr["actions"][i, t]) >= 0
    assert all(g.done for g in games)
    env.close()


# ---- c. games that are not in play
@pytest.mark.parametrize("n,seed", OC.PHASES)
def test_waiting_and_finished_games(T, KW, n, seed):
    """reset(defer_exchange=True): the rows of waiting games (beside games in play) before the exchange, every row after
    it; then the env stepped WITHOUT auto-reset until every game is finished and once more.  Non-live rows are the
    statement's: no legal card, the live bit 0, the other regions the oracle's state.  No launch flags an error."""
    mix = OC.PHASE_MIX
    env = T.TarokVecEnv(n, seed=seed, mix=mix)
    L = Launches(env, KW)
    obs = env.reset(defer_exchange=True)
    waiting = [OC.waiting_game(seed, i, 0, mix) for i in range(n)]
    assert any(g.g.phase == OM.PHASE_EXCHANGE for g in waiting) and any(g.g.phase == OM.PHASE_PLAY for g in waiting)
    L.check(obs.words, [MODEL.words(g) for g in waiting], (n, "waiting"))
    L.no_error((n, "waiting"))
    obs = env.exchange()
    slots = OC.slots_of(seed, mix, n)
    L.check(obs.words, model_words(slots), (n, "exchanged"))
    for t in range(OC.FINISH_STEPS + 1):
        obs, _, _ = env.step_random(auto_reset=False)
        OC.play(slots, auto=False)
        L.check(obs.words, model_words(slots), (n, "to the finish", t))
        if t == OC.FINISH_STEPS - 1:
            assert all(s.g.done for s in slots)
    L.no_error((n, "finished"))
    env.close()


# ---- d. positions reached by multi-card launches, and restored ones
def test_after_multi_card_launches_and_set_state(T, S, KW):
    """tarok_krog_random with 4 and 2 cards, one tarok_run_random chunk of 128 cards in one launch (auto-reset): the
    state those kernels leave is observed as the statement says.  Then a position with 3 cards on the table, captured
    from one env and restored into another with set_state()."""
    n, seed, mix = 257, 38, OC.PHASE_MIX
    env = T.TarokVecEnv(n, seed=seed, mix=mix)
    env.reset()
    slots = OC.slots_of(seed, mix, n)
    L = Launches(env, KW)
    for what, cards in (("krog 4", 4), ("krog 2", 2), ("run 128", 128)):
        if what == "run 128":
            env.run_random(128, cards_per_launch=128, auto_reset=True)
        else:
            env.krog_random(cards, auto_reset=True)
        for _ in range(cards):
            OC.play(slots, auto=True)
        L.check(env.obs_words, model_words(slots), what)
    L.no_error("multi-card")
    env.close()

    src = T.TarokVecEnv(n, seed=seed + 1, mix=mix)
    src.reset()
    slots = OC.slots_of(seed + 1, mix, n)
    for _ in range(7):
        src.step_random(auto_reset=False)
        OC.play(slots, auto=False)
    assert all(s.g.done or (s.g.g.n_in_trick == 3 and s.g.g.trick_no == 1) for s in slots)     # (a Berac can end at its first trick)
    assert sum(1 for s in slots if s.g.g.n_in_trick == 3) > n // 2
    lanes = src.state()
    assert (lanes == np.stack([s.g.lanes() for s in slots], axis=1)).all()
    src.close()
    dst = T.TarokVecEnv(n, seed=seed + 2, mix=S.MIX_FIXED + S.KLOP)
    dst.reset()
    obs = dst.set_state(lanes)
    L = Launches(dst, KW)
    L.check(obs.words, model_words(slots), "set_state")
    L.no_error("set_state")
    dst.close()


# ---- e. ragged sizes
@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_ragged_sizes_and_null_outputs(T, KW, n):
    """Sizes around the wave and the workgroup: every row written, none beyond; tarok_policy_mlp with one of its two
    feature outputs NULL writes the other's bytes unchanged."""
    seed, mix = 40 + n, OC.PHASE_MIX
    env = T.TarokVecEnv(n, seed=seed, mix=mix)
    obs = env.reset()
    slots = OC.slots_of(seed, mix, n)
    for _ in range(5):
        obs, _, _ = env.step_random(auto_reset=True)
        OC.play(slots, auto=True)
    L = Launches(env, KW)
    want = model_words(slots)
    L.check(obs.words, want, n)
    feat, fw = L.mlp(obs.words, (n, "both"))
    raw_feat, raw_fw = L.feat.host()[0].copy(), L.fw.host()[0].copy()
    only_fw = L.mlp(obs.words, (n, "features_out NULL"), feat=False)[1]
    assert (L.fw.host()[0] == raw_fw).all() and (only_fw == OM.words_array(want)).all()
    only_feat = L.mlp(obs.words, (n, "feature_words_out NULL"), fw=False)[0]
    assert (L.feat.host()[0] == raw_feat).all() and (only_feat == feat).all()
    L.mlp(obs.words, (n, "both NULL"), feat=False, fw=False)
    L.no_error(n)
    env.close()


# ---- f. tarok_expand_features
EXPAND_M = 773


@pytest.fixture(scope="module")
def real_words():
    """[773, 4] uint64: the statement's words of 773 mixed games, nine cards in."""
    name, mix, n, seed = OC.WHOLE[0]
    slots = OC.slots_of(seed, mix, EXPAND_M)
    for _ in range(9):
        OC.play(slots, auto=True)
    return OM.words_array(model_words(slots))


def index_of(kind, b):
    m = EXPAND_M
    return {"null": None, "identity": np.arange(b), "reversed": m - 1 - np.arange(b), "duplicates": (np.arange(b) // 3 * 131) % m,
            "last row": np.full(b, m - 1)}[kind]


@pytest.mark.parametrize("kind", ["null", "identity", "reversed", "duplicates", "last row"])
def test_expand_features_gathers_and_expands(T, real_words, kind):
    """tarok_expand_features into a guarded [n_samples, 256] output: the rows are expand() of the rows the index names
    (rows 0 .. n_samples - 1 without one), and no byte outside them is touched."""
    import torch
    from tarok_amd import _native
    env = T.TarokVecEnv(1, seed=1)
    fw = torch.from_numpy(real_words.view(np.int64)).to(env.device)
    for b in (1, 255, 257, 773):
        idx = index_of(kind, b)
        rows = np.arange(b) if idx is None else idx
        assert len(rows) == b and rows.min() >= 0 and rows.max() < EXPAND_M
        if kind == "duplicates" and b > 3:
            assert len(set(rows.tolist())) < b
        out = Guarded("tarok_expand_features", 1, b, np.uint16, inner=(256,), device=env.device)
        dev_idx = None if idx is None else torch.from_numpy(idx.astype(np.int64)).to(env.device)
        with torch.cuda.device(env.device):
            _native.check(env.L.tarok_expand_features(env._h, b, env._p(fw), env._p(dev_idx), out.ptr, env._stream()))
        assert_guards_intact([out], (kind, b))
        assert_rows(OM.from_bf16(all_written(out, (kind, b))), real_words[rows], (kind, b))
    env.close()
