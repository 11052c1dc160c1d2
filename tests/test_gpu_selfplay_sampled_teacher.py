"""GPU: SelfPlay(opponent=snapshot, teacher=dict(net=True, worlds=2, samples=2, temperature=1.0, versus=(1, 14))) — the
teacher's playouts seat the learner's live weights and the frozen opponent as they play at the table
(tarok_playout_cards_net_sampled) inside the captured rollout.  512 games, T = 4: the recorded rows equal an eager launch of
the entry with the same arguments on a twin env, captured equals eager, B's mode — left open — is the env's play mode at
capture, and a teacher dict without the new keys records the parent's bytes.

Run on the GPU box:  python -m pytest tests/test_gpu_selfplay_sampled_teacher.py -m gpu -q
"""
import pytest

from gpu_harness import T  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu
N, STEPS = 512, 4
TEACHER = dict(net=True, worlds=2, samples=2, temperature=1.0, versus=(1, 14), tau=8, salt=11)


def snapshot_of(T, seed):
    """Six tensors of a freshly initialised policy at `seed`: a frozen opponent that differs from the learner (seed 0)."""
    from tarok_amd import selfplay as SP
    env = T.TarokVecEnv(256, seed=1, mix=T.karte.MIX_BOT)
    try:
        return SP.SelfPlay(env, hidden=256, seed=seed, use_graph=False).snapshot()
    finally:
        env.close()


def make(T, snap, use_graph, teacher=TEACHER, mode=None):
    from tarok_amd import selfplay as SP
    env = T.TarokVecEnv(N, seed=6, mix=T.karte.MIX_BOT)
    if mode is not None:
        env.set_play_mode(*mode)
    return env, SP.SelfPlay(env, hidden=256, seed=0, fused_learner=True, opponent=snap, teacher=teacher, distill_coef=0.5, use_graph=use_graph)


def bits(t):
    import torch
    return t.view(torch.int16)


def rows_of(twin, c, buf, launch):
    """The teacher rows of every lock-step of `buf` from launch(twin) -> sums on a twin env that mirrors the rollout."""
    out = []
    for t in range(STEPS):
        out.append(twin.playout_targets(launch(twin), buf["words"][t], c._player.playouts, 8.0, seats_per_game=c._seats).clone())
        twin.step(buf["act"][t], auto_reset=True)
    return out


@pytest.mark.parametrize("mode", [None, (0.5, 0.25)])
def test_the_recorded_rows_are_the_eager_launch_and_captured_equals_eager(T, mode):
    """mode: the env's play mode when the rollout is captured (None: a new env's (1, 0)); the teacher leaves B's mode open, so B
    plays that mode inside the playouts — and the rows differ from those of B at another mode and from the greedy launch's."""
    import torch
    snap = snapshot_of(T, 3)
    ea, a = make(T, snap, True, mode=mode)
    eb, b = make(T, snap, False, mode=mode)
    assert a._player.launch_kind == "sampled" and a._player.playouts == 4
    with torch.no_grad():
        b._alloc(STEPS)
        b._collect_body(2)                               # (SelfPlay.collect warms up with two lock-steps before it captures)
    bufa, bufb = a.collect(STEPS), b.collect(STEPS)
    torch.cuda.synchronize()
    assert ea.play_mode == ((1.0, 0.0) if mode is None else mode)
    for k in ("words", "act", "done", "reward"):
        assert torch.equal(bufa[k], bufb[k]), k
    assert torch.equal(bits(bufa["teach"]), bits(bufb["teach"]))
    assert bits(bufa["teach"]).ne(0).any().item()
    # the rows against an eager launch of the entry: an eager learner from the reset, its env mirrored by a twin
    eb.close()
    eb, b = make(T, snap, False, mode=mode)
    bufb = b.collect(STEPS)
    twin = T.TarokVecEnv(N, seed=6, mix=T.karte.MIX_BOT)
    twin.reset()
    if mode is not None:
        twin.set_play_mode(*mode)                        # (the twin's steps replay recorded cards: its mode plays no part in them)
    torch.cuda.synchronize()
    bt, be = (1.0, 0.0) if mode is None else mode
    want = rows_of(twin, b, bufb, lambda env: env.playout_cards_net_sampled(b._w, b._opp, 2, 2, 1, 14, temperature=1.0, epsilon=0.0,
                                                                            opp_temperature=bt, opp_epsilon=be, salt=11,
                                                                            seats_per_game=b._seats)[0])
    for t in range(STEPS):
        assert torch.equal(bits(bufb["teach"][t]), bits(want[t])), t
    twin.reset()
    other = rows_of(twin, b, bufb, lambda env: env.playout_cards_net_sampled(b._w, b._opp, 2, 2, 1, 14, temperature=1.0, epsilon=0.0,
                                                                             opp_temperature=2.0, opp_epsilon=0.0, salt=11,
                                                                             seats_per_game=b._seats)[0])
    assert any(not torch.equal(bits(x), bits(y)) for x, y in zip(want, other)), "B's mode does not reach the rows"
    for e in (ea, eb, twin):
        e.close()


def test_a_teacher_without_the_new_keys_records_the_existing_launch(T):
    """teacher=dict(net=True, worlds=2, versus=(1, 14)) — no temperature, no samples: the greedy versus launch's rows, as before."""
    import torch
    snap = snapshot_of(T, 3)
    ec, c = make(T, snap, False, dict(net=True, worlds=2, versus=(1, 14), tau=8, salt=11))
    assert "temperature" not in c.teacher and c._player.launch_kind == "versus" and c._player.modes is None
    buf = c.collect(STEPS)
    twin = T.TarokVecEnv(N, seed=6, mix=T.karte.MIX_BOT)
    twin.reset()
    torch.cuda.synchronize()
    want = rows_of(twin, c, buf, lambda env: env.playout_cards_net_versus(c._w, c._opp, 2, 1, 14, salt=11, seats_per_game=c._seats)[0])
    for t in range(STEPS):
        assert torch.equal(bits(buf["teach"][t]), bits(want[t])), t
    ec.close(); twin.close()
