"""Times tarok_front_lines at 65,536 games with HIP events (profiles/front_lines_times.txt), in one process:
  first     the call right after reset + prefetch (14 n lines to front)
  steady    the call behind the third of three rollouts of T = 48 policy_step launches (the lines dealt during it)
  chain     the existing chain on the n current games: bid_values + bid_round + exchange_values
  rollout   the 48 policy_step launches themselves
and reports us per fronted line against the chain's us per game.

usage: python tools/front_lines_time.py OUT"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tarok_amd
from tarok_amd import karte as K, selfplay as SP
from tarok_amd.bidding import pack_weights

out_path = sys.argv[1]
N, T, REPEATS = 65536, 48, 5
tarok_amd.build()


def net(seed):
    torch.manual_seed(seed)
    return [t.cuda() for t in pack_weights(SP.PolicyNet(256))]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


env = tarok_amd.TarokVecEnv(N, seed=0, mix=K.MIX_BOT)
dev = env.device
A, B, X = net(0), net(1), net(2)
kw = dict(bid=B, exchange=X, scale=70.0, contracts=K.BID_ALL_CONTRACTS)
count = torch.zeros(1, dtype=torch.int64, device=dev)
words = torch.zeros((2, N), dtype=torch.int64, device=dev)
act = torch.zeros(N, dtype=torch.uint8, device=dev)
env.front_lines_scratch()
first, steady, chain, rollout, fronted = [], [], [], [], []


def steps():
    for t in range(T):
        env.policy_step(A, words[t % 2], words[(t + 1) % 2], act)


def the_chain():
    values = env.bid_values(1, B, 70.0, contracts=K.BID_ALL_CONTRACTS)
    env.bid_round(1, values, 1, contracts=K.BID_ALL_CONTRACTS)
    env.exchange_values(X)


for r in range(REPEATS + 1):                              # (the first pass warms up and is dropped)
    words[0].copy_(env.reset(defer_exchange=True).words)
    c = timed(the_chain)
    words[0].copy_(env.exchange().words)
    env.prefetch()
    torch.cuda.synchronize()
    f = timed(lambda: env.front_lines(count_out=count, **kw))
    assert int(count) == 14 * N
    for _ in range(3):                                    # (the Bot's games of the reset are 48 cards long and end together: the
        ro = timed(steps)                                 # rollouts after the first play fronted games, whose ends have spread)
        s = timed(lambda: env.front_lines(count_out=count, **kw))
    if r:
        first.append(f); chain.append(c); rollout.append(ro); steady.append(s); fronted.append(int(count))
fmt = lambda xs: " ".join("%.1f" % x for x in xs)
lines = ["first   (14 n = %d lines), us: %s | us per line: %s" % (14 * N, fmt(first), " ".join("%.5f" % (x / (14 * N)) for x in first)),
         "steady  (lines: %s), us: %s | us per line: %s" % (" ".join(map(str, fronted)), fmt(steady),
                                                             " ".join("%.5f" % (x / max(1, k)) for x, k in zip(steady, fronted))),
         "chain   (bid_values + bid_round + exchange_values, n = %d games), us: %s | us per game: %s" % (
             N, fmt(chain), " ".join("%.5f" % (x / N) for x in chain)),
         "rollout (48 policy_step launches, eager), us: %s" % fmt(rollout)]
env.close()
with open(out_path, "a") as fh:
    for ln in lines:
        print(ln)
        fh.write(ln + "\n")
