"""TEST INFRASTRUCTURE — what the policy-step tests share (tests/test_gpu_policy_step_seats.py, _versus.py, _pool.py and the
evaluation tests): per-game seat sets, the Twin env pair, random bf16 weight sets and the versus weight pair."""
import numpy as np


def seat_sets(spec, n):
    """(the `seats` argument, the seats_per_game host array or None, the set of every game [n])."""
    if spec == "cycle":
        per = (np.arange(n) % 16).astype(np.uint8)
        return 9, per, per               # (`seats` is ignored when the array is given: any valid value)
    return int(spec), None, np.full(n, int(spec), np.uint8)


def bits(x):
    """f32 array -> its bit patterns."""
    return np.ascontiguousarray(x).view(np.uint32)


class Twin:
    """An env and one set of plain output tensors; `launch` is called with them."""

    def __init__(self, T, n, seed, mix):
        import torch
        self.env = T.TarokVecEnv(n, seed=seed, mix=mix, history=True)
        self.env.reset(episode=0)
        z = lambda dt, *shape: torch.zeros(shape or (n,), dtype=dt, device="cuda")
        self.o = dict(action=z(torch.uint8), logp=z(torch.float32), value=z(torch.float32), words=z(torch.int64, n, 4),
                      reward=z(torch.int16, n, 4), done=z(torch.uint8), trick=z(torch.int16), obs=z(torch.int64))

    def clear(self):
        for k, v in self.o.items():
            v.fill_(77)                               # (reward rows are written only where a game finished)

    def end_state(self):
        ep, ss = self.env.counters()
        return self.env.state(), ep, ss, self.env.get_history().cpu().numpy(), self.env.legal_actions().words.cpu().numpy()


def make_weights(T, seed):
    """selfplay.PolicyNet(256) of a torch seed, parameters x 3, in the kernels' fragment order."""
    import torch
    from tarok_amd import selfplay as SP
    torch.manual_seed(seed)
    net = SP.PolicyNet(256).cuda()
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(3.0)                  # spread the logits a little
    order = T.TarokVecEnv.mfma_weight_order
    bf = lambda w: order(w.detach().to(torch.bfloat16).contiguous())
    fl = lambda b: b.detach().float().contiguous()
    return [bf(net.fc1.weight), fl(net.fc1.bias), bf(net.fc2.weight), fl(net.fc2.bias), bf(net.head.weight), fl(net.head.bias)]


def versus(env, seats, per_game, A, B, obs, action, logp, value, words, reward, done, trick, obs_out, flags):
    """One tarok_policy_step_versus launch through the C ABI (every argument a ctypes pointer or None)."""
    from tarok_amd import _native
    p = env._p
    _native.check(env.L.tarok_policy_step_versus(env._h, seats, per_game, *[p(w) for w in A], *[p(w) for w in B], obs, action, logp, value,
                                                 words, reward, done, trick, obs_out, flags, env._stream()))
