"""GPU: SelfPlay(opponent=snapshot, teacher=dict(net=True, worlds=2, versus=(1, 14))) — the teacher's playouts seat the
learner's live rollout weights on the mover and the frozen opponent's tensors on the three other seats
(tarok_playout_cards_net_versus) inside the captured rollout.  512 games, T = 4: the recorded rows against a replayed eager
launch on a twin env, captured against eager, set_opponent() picked up by the next replay without a new capture, and a
teacher without `versus` recording what the existing launch gives.

Run on the GPU box:  python -m pytest tests/test_gpu_selfplay_versus_teacher.py -m gpu -q
"""
import pytest

from gpu_harness import T  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu
N, STEPS = 512, 4
TEACHER = dict(net=True, worlds=2, versus=(1, 14), tau=8, salt=11)


def snapshot_of(T, seed):
    """Six tensors of a freshly initialised policy at `seed`: a frozen opponent that differs from the learner (seed 0)."""
    from tarok_amd import selfplay as SP
    env = T.TarokVecEnv(256, seed=1, mix=T.karte.MIX_BOT)
    try:
        return SP.SelfPlay(env, hidden=256, seed=seed, use_graph=False).snapshot()
    finally:
        env.close()


def make(T, snap, use_graph, teacher=TEACHER):
    from tarok_amd import selfplay as SP
    env = T.TarokVecEnv(N, seed=6, mix=T.karte.MIX_BOT)
    return env, SP.SelfPlay(env, hidden=256, seed=0, fused_learner=True, opponent=snap, teacher=teacher, distill_coef=0.5, use_graph=use_graph)


def bits(t):
    import torch
    return t.view(torch.int16)


def test_the_recorded_rows_are_the_eager_launch_and_captured_equals_eager(T):
    import torch
    snap = snapshot_of(T, 3)
    ea, a = make(T, snap, True)
    eb, b = make(T, snap, False)
    with torch.no_grad():
        b._alloc(STEPS)
        b._collect_body(2)                               # (SelfPlay.collect warms up with two lock-steps before it captures)
    bufa, bufb = a.collect(STEPS), b.collect(STEPS)
    torch.cuda.synchronize()
    for k in ("obs", "words", "act", "logp", "val", "done", "reward"):
        assert torch.equal(bufa[k], bufb[k]), k
    assert torch.equal(bits(bufa["teach"]), bits(bufb["teach"]))
    assert bits(bufa["teach"]).ne(0).any().item()
    # the rows against a replayed eager launch: an eager learner from the reset, its env mirrored by a twin
    ec, c = make(T, snap, False)
    buf = c.collect(STEPS)
    twin = T.TarokVecEnv(N, seed=6, mix=T.karte.MIX_BOT)
    twin.reset()
    torch.cuda.synchronize()
    differ_a = differ_b = 0
    for t in range(STEPS):
        sums, _ = twin.playout_cards_net_versus(c._w, c._opp, 2, 1, 14, salt=11, seats_per_game=c._seats)
        want = twin.playout_targets(sums, buf["words"][t], 2, 8.0, seats_per_game=c._seats)
        assert torch.equal(bits(buf["teach"][t]), bits(want)), t
        for w, name in ((c._w, "a"), (c._opp, "b")):     # ... and they are neither network's own single-network rows
            single = twin.playout_targets(twin.playout_cards_net(w, 2, salt=11, seats_per_game=c._seats)[0], buf["words"][t], 2, 8.0,
                                          seats_per_game=c._seats)
            d = int(bits(buf["teach"][t]).ne(bits(single)).any(-1).sum())
            differ_a, differ_b = differ_a + (d if name == "a" else 0), differ_b + (d if name == "b" else 0)
        twin.step(buf["act"][t], auto_reset=True)
    assert differ_a > 0 and differ_b > 0
    # set_opponent(): written in place, so the captured graph's next replay plays and searches against the new opponent
    other = snapshot_of(T, 4)
    a.set_opponent(other)
    torch.cuda.synchronize()
    graph = a._graph
    new_sums, _ = ea.playout_cards_net_versus(a._w, a._opp, 2, 1, 14, salt=11, seats_per_game=a._seats)
    old_sums, _ = ea.playout_cards_net_versus(a._w, list(snap), 2, 1, 14, salt=11, seats_per_game=a._seats)
    want_new = ea.playout_targets(new_sums, a.obs_words, 2, 8.0, seats_per_game=a._seats).clone()
    want_old = ea.playout_targets(old_sums, a.obs_words, 2, 8.0, seats_per_game=a._seats).clone()
    assert not torch.equal(bits(want_new), bits(want_old))
    bufa = a.collect(STEPS)
    torch.cuda.synchronize()
    assert a._graph is graph and graph is not None, "set_opponent() must not force a new capture"
    assert torch.equal(bits(bufa["teach"][0]), bits(want_new))
    for e in (ea, eb, ec, twin):
        e.close()


def test_a_teacher_without_versus_records_the_existing_launch(T):
    """teacher=dict(net=True, worlds=2) beside opponent=: the rows of tarok_playout_cards_net on the live weights, as before."""
    import torch
    snap = snapshot_of(T, 3)
    plain = dict(net=True, worlds=2, tau=8, salt=11)
    ec, c = make(T, snap, False, plain)
    assert "versus" not in c.teacher and c._player.versus is None and c._player.launch_kind == "net"
    buf = c.collect(STEPS)
    twin = T.TarokVecEnv(N, seed=6, mix=T.karte.MIX_BOT)
    twin.reset()
    torch.cuda.synchronize()
    for t in range(STEPS):
        sums, _ = twin.playout_cards_net(c._w, 2, salt=11, seats_per_game=c._seats)
        want = twin.playout_targets(sums, buf["words"][t], 2, 8.0, seats_per_game=c._seats)
        assert torch.equal(bits(buf["teach"][t]), bits(want)), t
        twin.step(buf["act"][t], auto_reset=True)
    ec.close(); twin.close()
