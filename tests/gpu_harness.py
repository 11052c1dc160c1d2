"""TEST INFRASTRUCTURE — what the GPU test modules share: the `T` fixture that builds and loads the library, make_env,
and the guarded launch-and-read plumbing of the playout launches (card playouts, the bidding pair, the exchange).

A plain module, not a conftest: a test module takes what it needs by name (`from gpu_harness import T  # noqa: F401`).
pytest does not rewrite the assertions of a module that is no test module, so every assert here carries its message.
The readers and the comparison are tested on the CPU (tests/test_oracle_model.py).
"""
import os

import numpy as np
import pytest

from guarded import SENTINEL_BYTE, Guarded, assert_guards_intact

SENTINEL_I32 = np.array([0xA5A5A5A5], np.uint32).view(np.int32)[0]
U = np.uint64


@pytest.fixture(scope="module")
def T():
    """The package, built, with the library loaded: _native.lib() sets argtypes on every name of _native.SYMBOLS, so a
    library that lacks one fails here."""
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import tarok_amd
    from tarok_amd import _native
    tarok_amd.build()
    assert os.path.exists(_native.LIB_PATH), "libtarokenv.so missing: the HIP path is the product, no fallback"
    assert _native.lib() is not None, "libtarokenv.so did not load"
    return tarok_amd


@pytest.fixture(scope="module")
def nets(T):
    """The exactly summable weight sets of tests/policy_exact_ref.py — R and one P — as (float64 set, kernel set)."""
    import policy_exact_ref as PE
    WR, WP = PE.weights_r(), PE.weights_p(*PE.P_PARAMS[2])
    return dict(R=(WR, PE.kernel_weights(T, WR)), P=(WP, PE.kernel_weights(T, WP)))


def make_env(T, n, mix, cards=0, history=False, *, seed, offset, episode, **reset):
    """An env of n games (gidx = offset + g) reset to `episode` after `cards` Bot cards without auto-reset.  Every family
    of tests passes its own seed, offset and episode: its expected values hang on them."""
    env = T.TarokVecEnv(n, seed=seed, mix=mix, game_offset=offset, history=history)
    env.reset(episode=episode, **reset)
    for _ in range(cards):
        env.step_random(auto_reset=False)
    return env


def make_bid_env(T, n, seed, offset, **kw):
    """An env of n games that has NOT been reset: bidding comes first."""
    from oracle import tarok_spec as S
    return T.TarokVecEnv(n, seed=seed, mix=S.MIX_BOT, game_offset=offset, **kw)


def perms_of(n, *, seed, offset, episode):
    """The deals of games offset .. offset + n - 1 at `episode`."""
    from oracle import tarok_spec as S
    return [S.deal(S.game_key(seed, offset + g, episode)) for g in range(n)]


def dev_u8(a):
    """A host array of bytes (the per-game seat sets, a deals array) on the device; None stays None."""
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.uint8)).cuda()


def games_of(env, per_game=None, *, offset):
    lanes = env.state()
    ep, _ = env.counters()
    return [(lanes[:, g].copy(), int(ep[g]), offset + g, None if per_game is None else int(per_game[g]) & 15) for g in range(env.n)]


def random_net(T, seed):
    import torch
    g = torch.Generator(); g.manual_seed(seed)
    order = T.TarokVecEnv.mfma_weight_order
    r = lambda *s: torch.randn(*s, generator=g)
    return [order((r(256, 256) / 6).cuda()), (r(256) / 4).cuda(), order((r(256, 256) / 12).cuda()), (r(256) / 4).cuda(),
            order((r(64, 256) / 12).cuda()), (r(64) / 4).cuda()]


# ---- one guarded launch: outputs (and the scratch) between guard bands, the env compared before and after
def _ptr(a):
    return None if a is None else a.ptr


def _scratch(env, scratch):
    """scratch = (the size entry, its arguments after the handle, the size it must return): (guarded bytes, size)."""
    entry, args, want = scratch
    size = int(getattr(env.L, entry)(env._h, *args))
    assert size == want, ("%s returned %d, expected %d" % (entry, size, want))
    return Guarded("scratch", 1, size, np.uint8, device="cuda"), size


def _snapshot(env):
    """The env's lanes, counters and (where it keeps one) history, on the host."""
    return env.state().copy(), env.counters(), env.get_history().cpu().numpy().copy() if env.history else None


def _assert_env_untouched(before, after, tag):
    assert (before[0] == after[0]).all(), ("the env was written", tag)
    assert all((a == b).all() for a, b in zip(before[1], after[1])), ("the env's counters were written", tag)
    assert before[2] is None or (before[2] == after[2]).all(), ("the env's history was written", tag)


def _launch(env, entry, args, outs, scratch, check_env_untouched, tag, scratch_out=None):
    """getattr(env.L, entry)(handle, *args, [scratch, size,] *outs, stream), checked and synchronized; then the guards of
    the scratch and of every output.  A tensor among args goes as its pointer, None as NULL."""
    import torch
    from tarok_amd import _native
    with torch.cuda.device(env.device):
        g_scr, tail = None, []
        if scratch is not None:
            g_scr, size = _scratch(env, scratch)
            tail = [g_scr.ptr, size]
        before = _snapshot(env) if check_env_untouched else None
        args = [env._p(a) if a is None or isinstance(a, torch.Tensor) else a for a in args]
        _native.check(getattr(env.L, entry)(env._h, *args, *tail, *[_ptr(o) for o in outs], env._stream()))
        torch.cuda.synchronize()
    assert_guards_intact([g_scr] + list(outs), (entry, env.n) + tuple(tag))
    if check_env_untouched:
        _assert_env_untouched(before, _snapshot(env), (entry,) + tuple(tag))
    if scratch_out is not None:
        scratch_out.append(g_scr.host()[0][0].copy())


def read_words(g):
    """[n, *inner] i32 of a guarded output of one row; fails on a word that was not written."""
    vals = g.host()[0][0]
    assert (vals != SENTINEL_I32).all(), "a word of %s was not written" % g.name
    return vals


def read_bytes(g):
    """[n, *inner] of a guarded one-byte output of one row; fails on a byte that was not written."""
    vals = g.host()[0][0]
    assert (vals.view(np.uint8) != SENTINEL_BYTE).all(), "a byte of %s was not written" % g.name
    return vals


# ---- the card playouts: (sum_out [n,12,4] i32, action_out [n] u8)
def card_outputs(n, want, device="cuda"):
    g_sum = Guarded("sum_out", 1, n, np.int32, inner=(12, 4), device=device) if "sum" in want else None
    g_act = Guarded("action_out", 1, n, np.uint8, device=device) if "action" in want else None
    return g_sum, g_act


def read_cards(g_sum, g_act):
    """(sum [n,12,4] i32 or None, action [n] u8 or None) of the outputs that were asked for."""
    return None if g_sum is None else read_words(g_sum), None if g_act is None else read_bytes(g_act)


def launch_cards(env, entry, args, want=("sum", "action"), scratch=None, check_env_untouched=False, tag=()):
    """One launch of a card-playout entry into guarded outputs: (sum [n,12,4] i32 or None, action [n] u8 or None).  args:
    what the entry takes between the handle and its scratch / outputs."""
    outs = card_outputs(env.n, want)
    _launch(env, entry, args, outs, scratch, check_env_untouched, tag)
    return read_cards(*outs)


def launch_det(env, worlds, samples, salt=0, seats=15, per_game=None, want=("sum", "action")):
    """tarok_playout_cards_det (worlds=None: the open-hand tarok_playout_cards) into guarded outputs."""
    head = ("tarok_playout_cards", []) if worlds is None else ("tarok_playout_cards_det", [int(worlds)])
    return launch_cards(env, head[0], head[1] + [int(samples), int(salt), int(seats), dev_u8(per_game)], want, tag=(worlds, samples, seats))


WORD = dict(voids=(np.uint32, np.int32), hidden=(np.uint64, np.int64))       # the worlds' word per game: (its type, torch's)


def words_of(kind, env, words=None):
    """The launch's word tensor: the env's own (shown_voids / played_cards), or a host array of the caller's."""
    import torch
    if words is None:
        return env.shown_voids() if kind == "voids" else env.played_cards()
    u, i = WORD[kind]
    return torch.from_numpy(np.asarray(words, u).view(i).copy()).cuda()


def host_words(kind, env):
    return words_of(kind, env).cpu().numpy().view(WORD[kind][0])


def model_words(kind, env):
    """The env's words rebuilt on the oracle from its state and history."""
    import playout_hidden_model as HM
    import playout_voids_model as VM
    lanes, hist = env.state(), env.get_history().cpu().numpy()
    f = VM.voids_of_lanes if kind == "voids" else HM.played_of_lanes
    return np.array([f(lanes[:, g], hist[:, g]) for g in range(env.n)], WORD[kind][0])


def launch_worlds(kind, env, worlds, samples, words=None, salt=0, seats=15, per_game=None, want=("sum", "action")):
    """tarok_playout_cards_voids / _hidden into guarded outputs.  words: [n] host array; None: the env's own."""
    return launch_cards(env, "tarok_playout_cards_" + kind,
                        [int(worlds), int(samples), int(salt), int(seats), dev_u8(per_game), words_of(kind, env, words)], want,
                        tag=(worlds, samples, seats))


def launch_net(kind, env, kw, worlds, net_seats, words=None, salt=0, seats=15, per_game=None, want=("sum", "action"), value=None):
    """The net-played card playouts of the kind (det, voids, hidden) into guarded outputs over a guarded scratch, the env
    compared before and after.  value = (depth, value_scale): tarok_playout_cards_net_value."""
    w = [] if kind == "det" else [words_of(kind, env, words)]
    head = [int(worlds), int(salt), int(seats), dev_u8(per_game)]
    if value is None:
        entry, args = "tarok_playout_cards_net" + ("" if kind == "det" else "_" + kind), head + w + [int(net_seats)]
    else:
        import playout_net_value_model as VM
        entry = "tarok_playout_cards_net_value"
        args = head + [VM.KINDS.index(kind), w[0] if w else None, int(net_seats), int(value[0]), float(value[1])]
    return launch_cards(env, entry, args + list(kw), want, scratch=("tarok_playout_net_scratch", (int(worlds),), env.n * 12 * worlds * 48),
                        check_env_untouched=True, tag=(kind, worlds, net_seats, seats) + (() if value is None else (value[0],)))


def assert_cards_equal(got_sum, want_sum, got_act, want_act, tag):
    bad = np.nonzero((got_sum != want_sum).any(axis=(1, 2)))[0]
    assert bad.size == 0, (tag, "sums differ", bad[:8], got_sum[bad[0]].tolist(), want_sum[bad[0]].tolist())
    bad = np.nonzero(got_act != want_act)[0]
    assert bad.size == 0, (tag, "cards differ", bad[:8], got_act[bad[:8]], want_act[bad[:8]])


# ---- the bidding pair: sum_out [n,4,20] i32; (contract, declarer, king) [n,3] i8
def launch_bids(env, worlds, samples, contracts, deals=None, salt=0, seats=15, per_game=None, *, episode, entry):
    """One launch of `entry` (tarok_playout_bids, tarok_playout_bids_pass) into a guarded sum_out: [n, 4, 20] i32."""
    g_sum = Guarded("sum_out", 1, env.n, np.int32, inner=(4, 20), device="cuda")
    assert g_sum.ptr.value % 16 == 0, "sum_out is not 16-byte aligned"
    _launch(env, entry, [int(episode), dev_u8(deals), int(worlds), int(samples), int(contracts), int(salt), int(seats), dev_u8(per_game)],
            [g_sum], None, False, (worlds, samples, contracts, seats))
    return read_words(g_sum)


def launch_bids_net(env, kw, worlds, net_seats, contracts, deals, salt, seats, per_game, episode, scratch_out=None):
    """One tarok_playout_bids_net into a guarded sum_out [n, 4, 20] i32 over a guarded scratch, the env compared before and
    after.  scratch_out: a list that receives the scratch's bytes after the launch."""
    g_sum = Guarded("sum_out", 1, env.n, np.int32, inner=(4, 20), device="cuda")
    _launch(env, "tarok_playout_bids_net",
            [int(episode), dev_u8(deals), int(worlds), int(contracts), int(salt), int(seats), dev_u8(per_game), int(net_seats)] + list(kw),
            [g_sum], ("tarok_playout_bids_net_scratch", (int(worlds),), env.n * 80 * worlds * 48 + env.n * 40), True,
            (worlds, contracts, net_seats, seats), scratch_out)
    return read_words(g_sum)


def launch_round(env, sums, playouts, threshold, contracts, seats=15, per_game=None, *, episode, entry):
    """One launch of `entry` (tarok_bid_round, tarok_bid_round_pass; threshold: the pass round's margin) into three guarded
    outputs: [n, 3] i8 (contract, declarer, king)."""
    import torch
    outs = [Guarded(name, 1, env.n, np.int8, device="cuda") for name in ("contract_out", "declarer_out", "king_out")]
    s = None if sums is None else torch.from_numpy(np.ascontiguousarray(sums, np.int32)).cuda()
    _launch(env, entry, [int(episode), s, int(playouts), int(threshold), int(contracts), int(seats), dev_u8(per_game)], outs, None, False,
            (playouts, threshold, contracts, seats))
    return np.stack([read_bytes(o) for o in outs], axis=1)


# ---- the exchange: (sum_out [n, 6 * sets, 4] i32, choice_out [n] i8, discards_out [n,3] u8)
def launch_exchange(env, entry, args, sets, want=("sum", "choice", "discards"), scratch=None, check_env_untouched=False, tag=(),
                    scratch_out=None):
    """One launch of an exchange-playout entry into guarded outputs, None where not asked.  scratch_out: a list that
    receives the scratch's bytes after the launch."""
    n = env.n
    g_sum = Guarded("sum_out", 1, n, np.int32, inner=(6 * sets, 4), device="cuda") if "sum" in want else None
    g_ch = Guarded("choice_out", 1, n, np.int8, device="cuda") if "choice" in want else None
    g_di = Guarded("discards_out", 1, n, np.uint8, inner=(3,), device="cuda") if "discards" in want else None
    assert g_sum is None or g_sum.ptr.value % 16 == 0, "sum_out is not 16-byte aligned"
    _launch(env, entry, args, [g_sum, g_ch, g_di], scratch, check_env_untouched, tag, scratch_out)
    return (None if g_sum is None else read_words(g_sum), None if g_ch is None else read_bytes(g_ch),
            None if g_di is None else read_bytes(g_di))


def replay_on_a_twin(T, kw, hs, *, seed):
    """The final scores [m, 4] of the oracle Games `hs` (at 0 cards played) put into a twin env through the canonical lanes
    and played to their ends by the greedy tarok_policy_step on every seat."""
    import torch
    from oracle import tarok_spec as S
    m = len(hs)
    twin = T.TarokVecEnv(m, seed=seed, mix=S.MIX_ALL)
    try:
        twin.reset()
        twin.set_state(np.stack([h.lanes() for h in hs], axis=1))
        twin.set_play_mode(0.0, 0.0)
        words = [twin.legal_actions().words.clone(), torch.zeros(m, dtype=torch.int64, device="cuda")]
        act = torch.zeros(m, dtype=torch.uint8, device="cuda")
        rew, dn = torch.zeros((m, 4), dtype=torch.int16, device="cuda"), torch.zeros(m, dtype=torch.uint8, device="cuda")
        final, finished = np.zeros((m, 4), np.int64), np.zeros(m, bool)
        for t in range(48):
            if finished.all():
                break
            twin.policy_step(kw, words[t & 1], words[(t + 1) & 1], act, reward_out=rew, done_out=dn, auto_reset=False)
            d = dn.cpu().numpy().astype(bool) & ~finished
            final[d] = rew.cpu().numpy()[d]
            finished |= d
        assert finished.all(), "a twin game did not end within 48 cards"
    finally:
        twin.close()
    return final


def item_arrays(scratch, items):
    """(keys [items] u64, results [items, 4] i16 and as u64) of a launch's scratch bytes."""
    keys = scratch[items * 32:items * 40].view(np.uint64)
    res = scratch[items * 40:items * 48]
    return keys, res.view(np.int16).reshape(items, 4), res.view(np.uint64)


def launch_exchange_bot(env, worlds, samples, sets, salt=0, seats=15, per_game=None, want=("sum", "choice", "discards")):
    """tarok_playout_exchange into guarded outputs."""
    return launch_exchange(env, "tarok_playout_exchange", [int(worlds), int(samples), int(sets), int(salt), int(seats), dev_u8(per_game)],
                           sets, want, tag=(worlds, samples, sets, seats))
