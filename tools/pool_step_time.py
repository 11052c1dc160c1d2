"""Times 48 graph-replayed tarok_policy_step_pool launches at 65,536 games with HIP events, beside
tarok_policy_step_versus and tarok_policy_step_seats in the same process (profiles/pool_step_times.txt).

usage: python tools/pool_step_time.py OUT [KIND ...]
  OUT    the lines are appended to this file
  KIND   "pool:<K>" (K different weight sets, group g on entry g % K, seats = 1), "pool:<K>:self" (the same with every
         fourth group plain self-play), "versus" (tarok_policy_step_versus, seats = 1) or "seats" (policy_step_seats = 1);
         default: seats versus pool:1 pool:4 pool:16
The weight sets are PolicyNet(256) of torch seeds 0, 1, 2, ..., parameters x 3; the learner is seed 0, pool entry k seed
1 + k (the versus launch's second network is seed 1 = pool entry 0)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tarok_amd
from tarok_amd import karte as K, selfplay as SP
from tarok_amd.env import TarokVecEnv

out_path = sys.argv[1]
kinds = sys.argv[2:] or ["seats", "versus", "pool:1", "pool:4", "pool:16"]
N, T, REPEATS, INNER = 65536, 48, 5, 20
tarok_amd.build()


def scaled(seed):
    torch.manual_seed(seed)
    m = SP.PolicyNet(256).cuda()
    with torch.no_grad():
        for q in m.parameters():
            q.mul_(3.0)
    order = TarokVecEnv.mfma_weight_order
    bf = lambda w: order(w.detach().to(torch.bfloat16).contiguous())
    fl = lambda b: b.detach().float().contiguous()
    return [bf(m.fc1.weight), fl(m.fc1.bias), bf(m.fc2.weight), fl(m.fc2.bias), bf(m.head.weight), fl(m.head.bias)]


A = scaled(0)
lines = []
for kind in kinds:
    env = TarokVecEnv(N, seed=0, mix=K.MIX_ALL)
    dev = env.device
    kw = dict(seats=1)
    if kind.startswith("pool:"):
        k = int(kind.split(":")[1])
        kw["opponent_pool"] = TarokVecEnv.stack_pool([scaled(1 + j) for j in range(k)])
        if kind.endswith(":self"):
            kw["group_net"] = torch.tensor(SP.SelfPlay.pool_group_net(N // 256, k, 0.25), dtype=torch.uint8, device=dev)
    elif kind == "versus":
        kw["opponent"] = scaled(1)
    words = torch.zeros((2, N), dtype=torch.int64, device=dev)       # the observation words go back and forth
    act = torch.zeros((T, N), dtype=torch.uint8, device=dev)
    logp = torch.zeros((T, N), dtype=torch.float32, device=dev)
    val = torch.zeros((T, N), dtype=torch.float32, device=dev)
    fw = torch.zeros((T, N, 4), dtype=torch.int64, device=dev)
    rew = torch.zeros((T, N, 4), dtype=torch.int16, device=dev)
    done = torch.zeros((T, N), dtype=torch.uint8, device=dev)

    def body():
        for t in range(T):
            env.policy_step(A, words[t % 2], words[(t + 1) % 2], act[t], logp[t], val[t], feature_words_out=fw[t], reward_out=rew[t],
                            done_out=done[t], **kw)

    words[0].copy_(env.reset().words)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        body()
    for _ in range(5):
        g.replay()
    torch.cuda.synchronize()
    one, many = [], []
    for r in range(REPEATS):
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record(); g.replay(); e1.record()
        for _ in range(INNER):
            g.replay()
        e2.record()
        torch.cuda.synchronize()
        one.append(e0.elapsed_time(e1) * 1e3)
        many.append(e1.elapsed_time(e2) * 1e3 / INNER)
    name = {"seats": "policy_step_seats=1", "versus": "policy_step_versus=1"}.get(kind, "policy_step_" + kind.replace(":", "=", 1))
    lines.append("%-26s one replay of 48 launches, us: %s | mean of %d back-to-back replays, us: %s" % (
        name, " ".join("%.1f" % x for x in one), INNER, " ".join("%.1f" % x for x in many)))
    del g
    env.close()
with open(out_path, "a") as f:
    for ln in lines:
        print(ln)
        f.write(ln + "\n")
