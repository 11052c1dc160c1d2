"""Times 48 graph-replayed policy-step launches at 65,536 games with HIP events (profiles/eval_step_times.txt).

usage: python tools/eval_step_times.py [--evaluate] LIB LABEL OUT [KIND ...]
  --evaluate  also time one evaluate_vs_bot run of untrained weights (this checkout's library)
  LIB    a libtarokenv.so (this checkout's, or one built from another commit: bound here directly, so a library
         without tarok_policy_step_seats can be timed too)
  LABEL  goes in front of every line
  OUT    the lines are appended to this file
  KIND   "plain" (tarok_policy_step), a seat set 0..15 (tarok_policy_step_seats) or "versus:<set>"
         (tarok_policy_step_versus: two different weight sets, PolicyNet(256) of torch seeds 0 and 1, parameters x 3)
         or "mode:<temperature>:<epsilon>" (tarok_policy_step after tarok_set_play_mode: profiles/play_mode_step_times.txt;
         the graph is captured with the mode set, so it replays the mode's kernel)"""
import ctypes as C
import os
import sys
import time

import torch

args = [a for a in sys.argv[1:] if a != "--evaluate"]
evaluate = "--evaluate" in sys.argv[1:]
lib_path, label, out_path, kinds = args[0], args[1], args[2], args[3:]
N, T, REPEATS, INNER = 65536, 48, 5, 20
L = C.CDLL(lib_path)
vp, i32, i64, u64, u32 = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_uint32
L.tarok_create.restype = i32; L.tarok_create.argtypes = [C.POINTER(vp), i32, i64, u64, u64, i32, i32]
L.tarok_destroy.restype = None; L.tarok_destroy.argtypes = [vp]
L.tarok_reset.restype = i32; L.tarok_reset.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp, i32, vp]
L.tarok_legal_actions.restype = i32; L.tarok_legal_actions.argtypes = [vp, vp, vp, vp]
L.tarok_policy_step.restype = i32; L.tarok_policy_step.argtypes = [vp] * 16 + [i32, vp]
if hasattr(L, "tarok_policy_step_seats"):
    L.tarok_policy_step_seats.restype = i32; L.tarok_policy_step_seats.argtypes = [vp, i32, vp] + [vp] * 15 + [i32, vp]
if hasattr(L, "tarok_policy_step_versus"):
    L.tarok_policy_step_versus.restype = i32; L.tarok_policy_step_versus.argtypes = [vp, i32, vp] + [vp] * 21 + [i32, vp]

if hasattr(L, "tarok_set_play_mode"):
    L.tarok_set_play_mode.restype = i32; L.tarok_set_play_mode.argtypes = [vp, C.c_float, C.c_float]

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tarok_amd import karte as K, selfplay as SP
from tarok_amd.env import TarokVecEnv
torch.manual_seed(0)
net = SP.PolicyNet(256).cuda()
order = TarokVecEnv.mfma_weight_order
bf = lambda w: order(w.detach().to(torch.bfloat16).contiguous())
fl = lambda b: b.detach().float().contiguous()
pack = lambda net: [bf(net.fc1.weight), fl(net.fc1.bias), bf(net.fc2.weight), fl(net.fc2.bias), bf(net.head.weight), fl(net.head.bias)]
W = pack(net)


def scaled(seed):
    torch.manual_seed(seed)
    m = SP.PolicyNet(256).cuda()
    with torch.no_grad():
        for q in m.parameters():
            q.mul_(3.0)
    return pack(m)


VS = [scaled(0), scaled(1)] if any(k.startswith("versus:") for k in kinds) else None
p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
dev = torch.device("cuda", 0)
lines = []
for kind in kinds:
    h = vp()
    assert L.tarok_create(C.byref(h), 0, N, 0, 0, 0, 0) == 0
    if kind.startswith("mode:"):
        assert L.tarok_set_play_mode(h, float(kind.split(":")[1]), float(kind.split(":")[2])) == 0
    words = torch.zeros((2, N), dtype=torch.int64, device=dev)       # the observation words go back and forth
    act = torch.zeros((T, N), dtype=torch.uint8, device=dev)
    logp = torch.zeros((T, N), dtype=torch.float32, device=dev)
    val = torch.zeros((T, N), dtype=torch.float32, device=dev)
    fw = torch.zeros((T, N, 4), dtype=torch.int64, device=dev)
    rew = torch.zeros((T, N, 4), dtype=torch.int16, device=dev)
    done = torch.zeros((T, N), dtype=torch.uint8, device=dev)

    def body(stream):
        s = C.c_void_p(stream.cuda_stream)
        for t in range(T):
            a = ([p(x) for x in VS[0] + VS[1]] if kind.startswith("versus:") else [p(x) for x in W]) + [p(words[t % 2]), p(act[t]), p(logp[t]), p(val[t]), p(fw[t]), p(rew[t]), p(done[t]), None, p(words[(t + 1) % 2]), K.AUTO_RESET, s]
            if kind == "plain" or kind.startswith("mode:"):
                rc = L.tarok_policy_step(h, *a)
            elif kind.startswith("versus:"):
                rc = L.tarok_policy_step_versus(h, int(kind[7:]), None, *a)
            else:
                rc = L.tarok_policy_step_seats(h, int(kind), None, *a)
            assert rc == 0, rc

    cur = torch.cuda.current_stream(dev)
    assert L.tarok_reset(h, 0, None, None, None, None, None, None, K.CLEAR_COUNTERS, C.c_void_p(cur.cuda_stream)) == 0
    assert L.tarok_legal_actions(h, p(words[0]), None, C.c_void_p(cur.cuda_stream)) == 0
    side = torch.cuda.Stream(dev)
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        body(side)
    cur.wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        body(torch.cuda.current_stream(dev))
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
    lines.append("%-8s %-22s one replay of 48 launches, us: %s | mean of %d back-to-back replays, us: %s" % (
        label, "tarok_policy_step" if kind == "plain" else "policy_step (%s, %s)" % tuple(kind.split(":")[1:]) if kind.startswith("mode:") else "policy_step_versus=%s" % kind[7:] if kind.startswith("versus:") else "policy_step_seats=%s" % kind,
        " ".join("%.1f" % x for x in one), INNER, " ".join("%.1f" % x for x in many)))
    L.tarok_destroy(h)
    del g
if evaluate:
    from tarok_amd.evaluate import evaluate_vs_bot
    evaluate_vs_bot(W, 256, 1)                        # library / allocator warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = evaluate_vs_bot(W, 4096, 4)
    dt = time.perf_counter() - t0
    lines.append("%-8s evaluate_vs_bot(untrained PolicyNet seed 0, n_games=4096, episodes=4, seed=0, MIX_BOT): wall %.3f s, advantage %+.4f, stderr %.4f, "
                 "policy_mean %.4f, bot_mean %.4f, by_seat %s, deals %d" % (label, dt, r["advantage"], r["stderr"], r["policy_mean"], r["bot_mean"],
                                                                             " ".join("%+.3f" % x for x in r["by_seat"]), r["deals"]))
with open(out_path, "a") as f:
    for ln in lines:
        print(ln)
        f.write(ln + "\n")
