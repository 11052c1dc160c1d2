"""GPU: SelfPlay(teacher=dict(..., voids=True)) — the void-aware playout teacher recorded inside the captured rollout.

Run on the GPU box:  python -m pytest tests/test_gpu_distill_voids.py -m gpu -q
"""
import pytest

from gpu_harness import T  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu
N, STEPS = 512, 8
TEACHER = dict(worlds=2, samples=1, tau=8, voids=True)


def make(T, teacher=None, history=True, seed=6, **kw):
    from tarok_amd import selfplay as SP
    env = T.TarokVecEnv(N, seed=seed, mix=T.karte.MIX_ALL, history=history)
    return env, SP.SelfPlay(env, hidden=256, seed=0, fused_learner=True, teacher=teacher, distill_coef=0.0, **kw)


def test_recorded_rows_are_the_targets_of_a_replayed_launch(T):
    """Eager rollout from the reset: buf["teach"][t] equals playout_targets of a separate shown_voids +
    playout_cards_voids launch on a twin env stepped with the recorded actions.  Voids appear from the second card on, so
    from there the rows differ from a teacher without voids somewhere."""
    import torch
    tc = dict(TEACHER, salt=11)
    ea, a = make(T, tc, use_graph=False)
    buf = a.collect(STEPS)
    twin = T.TarokVecEnv(N, seed=6, mix=T.karte.MIX_ALL, history=True)
    twin.reset()
    torch.cuda.synchronize()
    differ = 0
    for t in range(STEPS):
        words = twin.shown_voids()
        sums, _ = twin.playout_cards_voids(2, 1, salt=11, voids=words)
        want = twin.playout_targets(sums, buf["words"][t], 2, 8.0)
        assert torch.equal(buf["teach"][t].view(torch.int16), want.view(torch.int16)), t
        plain = twin.playout_targets(twin.playout_cards_det(2, 1, salt=11)[0], buf["words"][t], 2, 8.0)
        differ += int(buf["teach"][t].view(torch.int16).ne(plain.view(torch.int16)).any(-1).sum())
        if t < 2:
            assert not words.any()
        twin.step(buf["act"][t], auto_reset=True)
    assert differ > 0
    ea.close(); twin.close()


def test_graph_replay_and_eager_record_the_same_bytes(T):
    import torch
    ea, a = make(T, TEACHER, use_graph=True)
    eb, b = make(T, TEACHER, use_graph=False)
    with torch.no_grad():
        b._alloc(STEPS)
        b._collect_body(2)                               # (SelfPlay.collect warms up with two lock-steps before it captures)
    for rnd in range(2):
        bufa, bufb = a.collect(STEPS), b.collect(STEPS)
        torch.cuda.synchronize()
        for k in ("obs", "words", "act", "logp", "val", "done", "reward"):
            assert torch.equal(bufa[k], bufb[k]), (rnd, k)
        assert torch.equal(bufa["teach"].view(torch.int16), bufb["teach"].view(torch.int16)), rnd
        assert bufa["teach"].view(torch.int16).ne(0).any(-1).all()
    ea.close(); eb.close()


def test_a_teacher_without_voids_is_unchanged_and_voids_need_the_history(T):
    """teacher=dict(worlds=2, samples=1) on a history env and on a plain one: the same rows (the determinized launch's);
    voids=True without the history, or without worlds, is refused."""
    import torch
    plain = dict(worlds=2, samples=1, tau=8)
    ea, a = make(T, plain, history=True, use_graph=False)
    eb, b = make(T, plain, history=False, use_graph=False)
    bufa, bufb = a.collect(STEPS), b.collect(STEPS)
    assert torch.equal(bufa["teach"].view(torch.int16), bufb["teach"].view(torch.int16))
    twin = T.TarokVecEnv(N, seed=6, mix=T.karte.MIX_ALL)
    twin.reset()
    for t in range(STEPS):
        want = twin.playout_targets(twin.playout_cards_det(2, 1)[0], bufa["words"][t], 2, 8.0)
        assert torch.equal(bufa["teach"][t].view(torch.int16), want.view(torch.int16)), t
        twin.step(bufa["act"][t], auto_reset=True)
    with pytest.raises(ValueError):
        make(T, TEACHER, history=False)
    with pytest.raises(ValueError):
        make(T, dict(samples=2, voids=True))
    ea.close(); eb.close(); twin.close()
