"""Times the fused chain with and without the distillation term, tarok_playout_targets and a rollout with and without the
playout teacher (profiles/distill_times.txt).  One session; every figure is the median of 9 launches between device events,
and the plain chain's median is repeated to show its own spread.

usage: python tools/distill_time.py OUT [--parent REV | --parent-lib LIB]
  OUT           the lines are appended to this file
  --parent REV  build the library of that commit into a scratch directory (git archive + the package's compile flags) and
                time its tarok_learn_chain in a process of its own (default: HEAD^)
  --parent-lib  a library already built from the parent commit

The minibatch is the bench's: 393,216 samples of a rollout of 65,536 games (tests/test_gpu_learner.py,
test_learn_chain_and_dw_at_the_bench_minibatch).  The one condition: this build's plain tarok_learn_chain stays inside the
spread of the parent's own repeated medians."""
import ctypes
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, T, B, LAUNCHES, REPEATS = 65536, 48, 393216, 9, 7


def event_median(torch, fn, launches=LAUNCHES):
    times = []
    for _ in range(launches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1000.0)
    return statistics.median(times)


def chain_session(lib_path, label, out, distill):
    """The chain of one library on a rollout of this session; distill: also time the launches only this build has."""
    import torch
    from tarok_amd import _native
    if lib_path:
        class Tolerant(ctypes.CDLL):                          # (a parent library lacks the new entry points: never called here)
            def __getattr__(self, name):
                try:
                    return super().__getattr__(name)
                except AttributeError:
                    if not name.startswith("tarok_"):
                        raise
                    import types
                    return types.SimpleNamespace(restype=None, argtypes=None)
        _native.LIB_PATH = lib_path
        ctypes.CDLL = Tolerant
    import tarok_amd
    from tarok_amd import karte as K, selfplay as SP
    env = tarok_amd.TarokVecEnv(N, seed=3, mix=K.MIX_ALL)
    sp = SP.SelfPlay(env, hidden=256, seed=0, fused_learner=True)
    buf = sp.collect(T)
    M = T * N
    lb = sp._learn_bufs(M, B)
    env.learn_returns_seats(T, buf["done"], buf["reward"], buf["words"][:T], buf["logp"], buf["val"], buf["act"], sp.reward_scale,
                            lb["rec"], lb["stats"], lb["scratch"])
    words = buf["obs"].view(M, 4)
    idx = sp._epoch_permutation(M)[:B].contiguous()
    bias = (sp._w[1], sp._w[3], sp._w[5])
    args = (B, words, idx, lb["rec"], lb["stats"], sp.clip, sp.vf_coef, sp.ent_coef, sp._wf, bias, lb["Xw"], lb["H1"], lb["H2"],
            lb["dOut"], lb["dH2"], lb["dH1"], lb["scratch"], lb["terms"], lb["running"])
    plain = lambda: env.learn_chain(*args)
    for _ in range(3):
        plain()
    meds = [event_median(torch, plain) for _ in range(REPEATS)]
    out.append("%s tarok_learn_chain, B = %d: medians of %d launches, us: %s  (min %.1f, max %.1f)"
               % (label, B, LAUNCHES, " ".join("%.1f" % m for m in meds), min(meds), max(meds)))
    if distill:
        target = torch.zeros((M, 64), dtype=torch.bfloat16, device=env.device)
        sums, _ = env.playout_cards_det(8, 2)
        row = env.playout_targets(sums, buf["words"][T], 16, 8.0)
        target.view(T, N, 64)[:] = row                        # (every sample a real teacher's row)
        ds = torch.empty(((B + 95) // 96, 2), device=env.device)
        dt = torch.empty(2, device=env.device)
        dist = lambda: env.learn_chain_distill(*args, target, 1.0, ds, dt)
        for _ in range(3):
            dist()
        meds = [event_median(torch, dist) for _ in range(3)]
        out.append("%s tarok_learn_chain_distill, B = %d: medians, us: %s" % (label, B, " ".join("%.1f" % m for m in meds)))
        tg = lambda: env.playout_targets(sums, buf["words"][T], 16, 8.0, target_out=row)
        out.append("%s tarok_playout_targets, %d games: median %.1f us" % (label, N, event_median(torch, tg)))
        out.append("%s rollout T = %d at %d games, no teacher: median %.0f us" % (label, T, N, event_median(torch, lambda: sp.collect(T), 5)))
        env2 = tarok_amd.TarokVecEnv(N, seed=3, mix=K.MIX_ALL)
        sp2 = SP.SelfPlay(env2, hidden=256, seed=0, fused_learner=True, teacher=dict(worlds=8, samples=2))
        sp2.collect(T)
        out.append("%s rollout T = %d at %d games, teacher worlds = 8, samples = 2: median %.0f us"
                   % (label, T, N, event_median(torch, lambda: sp2.collect(T), 5)))
    return meds


def build_parent(rev):
    from tarok_amd import _native
    d = tempfile.mkdtemp(prefix="tarok_parent_")
    tar = subprocess.Popen(["git", "-C", ROOT, "archive", rev, "tarok_amd/csrc", "include"], stdout=subprocess.PIPE)
    subprocess.check_call(["tar", "-x", "-C", d], stdin=tar.stdout)
    assert tar.wait() == 0
    flags = [f if f != os.path.join(ROOT, "include") else os.path.join(d, "include") for f in _native.COMPILE_FLAGS]
    lib = os.path.join(d, "libtarokenv_parent.so")
    subprocess.check_call([_native.hipcc_path()] + flags + ["-shared", "-fPIC", "-o", lib, os.path.join(d, "tarok_amd", "csrc", "tarok_env.hip")])
    return lib


if __name__ == "__main__":
    a = sys.argv[1:]
    if len(a) >= 3 and a[0] == "--child":                     # the parent library's process
        lines = []
        chain_session(a[1], "parent", lines, False)
        with open(a[2], "a") as f:
            f.write("\n".join(lines) + "\n")
        sys.exit(0)
    out_path = a[0]
    parent_lib = a[a.index("--parent-lib") + 1] if "--parent-lib" in a else build_parent(a[a.index("--parent") + 1] if "--parent" in a else "HEAD^")
    import tarok_amd
    tarok_amd.build()
    lines = []
    chain_session(None, "this  ", lines, True)
    with open(out_path, "a") as f:
        f.write("\n".join(lines) + "\n")
    subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", os.path.abspath(parent_lib), out_path])
    lines = []
    chain_session(None, "this  ", lines, False)               # (again, after the parent: the session's drift shows here)
    with open(out_path, "a") as f:
        f.write("\n".join(lines) + "\n")
    print(open(out_path).read())
