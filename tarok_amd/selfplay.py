"""Self-play policy-gradient harness on top of the GPU env (BASELINE.json configs 4-5,
SURVEY §8f row 4).  Build-owned: the reference trains a double-Q LSTM agent with
pytorch-lightning (Igralec.py:545-714) and has no PPO, so nothing here is pinned to it —
this exists to show the env being driven by a learner and to exercise the one collective
of the whole build, the gradient all-reduce (RCCL over xGMI via torch.distributed).

Shape of the loop (per rank, one env shard each; games need no communication):

    obs  = env.observe()                        [N,256] bf16 features     (HIP kernel)
    pi,v = net(obs)                             small MLP, bf16           (torch / rocBLAS)
    a    = masked categorical sample            legal mask = observation word
    env.step(a, auto_reset=True)                                          (HIP kernel)
    ... T steps ...
    returns: every card is credited with its seat's final score of that game (Monte-Carlo,
    gamma = 1), or, with SelfPlay(gamma=..., gae_lambda=...), per-seat GAE bootstrapped from the
    seat's next decision; clipped-surrogate PPO update; gradients summed over ranks in ONE flattened
    all-reduce per minibatch (a few hundred KB: latency-bound, so one bucket, not many).

SelfPlay(env, opponent=snapshot) trains against a frozen opponent instead: per slot some seats are the learner's, the
others play the snapshot (tarok_policy_step_versus), and only the learner's samples reach the update.
"""
import time

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import karte as K
from . import playout
from . import sharding


class _LinearSplitK(torch.autograd.Function):
    """y = x W^T + b whose weight gradient is computed as a batch of partial products.

    dW = dY^T X has M = N = 256 or 64 and K = the minibatch (393,216 rows in the bench): as ONE
    GEMM it has 16 output tiles, i.e. 240 of the 256 CUs idle (hipBLASLt picks a 64x64x256 tile:
    0.81 ms, 2.5 % of the matrix peak, 44 % of the whole update).  Split along K into S batches
    (torch.bmm) it is S x 16 tiles; the partials are summed in f32."""

    @staticmethod
    def forward(ctx, x, w, b, relu):
        cd = torch.bfloat16 if (x.is_cuda and torch.is_autocast_enabled()) else x.dtype
        with torch.autocast(x.device.type, enabled=False):
            xq, wq, bq = x.to(cd), w.to(cd), b.to(cd)
            if relu and x.is_cuda:
                y = torch._addmm_activation(bq, xq, wq.t())      # bias + ReLU in the GEMM's epilogue
            else:
                y = F.linear(xq, wq, bq)
                if relu:
                    y = F.relu(y)
            ctx.save_for_backward(xq, wq, y if relu else None)
            ctx.out_dtypes = (x.dtype, w.dtype, b.dtype)
            return y

    @staticmethod
    def backward(ctx, gy):
        xq, wq, y = ctx.saved_tensors
        dx, dw, db = ctx.out_dtypes
        gy = gy.contiguous()
        if y is not None:
            gy = torch.ops.aten.threshold_backward(gy, y, 0)     # ReLU'
        gx = (gy @ wq).to(dx) if ctx.needs_input_grad[0] else None
        B = xq.shape[0]
        S = next((s for s in (32, 24, 16, 12, 8, 4, 2) if B % s == 0 and B // s >= 512), 1)      # S x 16 tiles >= 256 CUs
        if S > 1:
            gw = torch.bmm(gy.view(S, B // S, -1).transpose(1, 2), xq.view(S, B // S, -1)).sum(0, dtype=torch.float32)
        else:
            gw = (gy.t() @ xq).float()
        return gx, gw.to(dw), gy.sum(0, dtype=torch.float32).to(db), None


class PolicyNet(nn.Module):
    """256 features -> 2 x hidden ReLU -> one 64-wide head: outputs 0..53 = card logits, output
    54 = state value (the layout tarok_policy_mlp evaluates in one fused MFMA kernel when hidden = 256)."""

    def __init__(self, hidden=256):
        super().__init__()
        self.fc1 = nn.Linear(256, hidden)
        self.fc2 = nn.Linear(hidden, hidden)
        self.head = nn.Linear(hidden, 64)

    def forward_raw(self, x):
        """all 64 head outputs [N,64]"""
        if x.dim() == 2 and x.shape[0] >= 16384 and torch.is_grad_enabled():    # a training minibatch
            h = _LinearSplitK.apply(x, self.fc1.weight, self.fc1.bias, True)
            h = _LinearSplitK.apply(h, self.fc2.weight, self.fc2.bias, True)
            return _LinearSplitK.apply(h, self.head.weight, self.head.bias, False)
        h = F.relu(self.fc1(x))
        h = F.relu(self.fc2(h))
        return self.head(h)

    def forward(self, x):
        out = self.forward_raw(x)
        return out[..., :54], out[..., 54]


def legal_matrix(mask_words):
    """int64 [N] observation words -> bool [N,54] legal-card matrix."""
    bits = torch.arange(54, device=mask_words.device, dtype=torch.int64)
    return ((mask_words.unsqueeze(-1) >> bits) & 1).bool()


def sample_masked(logits, legal, generator=None):
    """Sample one legal card per row.  Returns (action int64 [N], log-prob f32 [N]).
    Rows without any legal card (finished games when auto-reset is off) get action 255."""
    none = ~legal.any(dim=-1)
    lg = logits.float().masked_fill(~legal, float("-inf"))
    lg = torch.where(none.unsqueeze(-1), torch.zeros_like(lg), lg)
    logp_all = F.log_softmax(lg, dim=-1)
    action = torch.multinomial(logp_all.exp(), 1, generator=generator).squeeze(-1)
    logp = logp_all.gather(-1, action.unsqueeze(-1)).squeeze(-1)
    return torch.where(none, torch.full_like(action, 255), action), torch.where(none, torch.zeros_like(logp), logp)


def learner_moves(seat, learner):
    """bool [T,N]: the seat that played at t is one of the learner's seats of its slot.  seat [T,N]; learner [N] uint8:
    one 4-bit seat set per slot (bit s: seat s is the learner's; bits 4..7 are ignored)."""
    return ((learner.to(device=seat.device, dtype=torch.int64).unsqueeze(0) >> seat.long()) & 1).bool()


def assign_returns(done, reward, seat, learner=None):
    """Credit every transition with its seat's final score of the game it belongs to.

    done [T,N] bool: the card played at t finished a game; reward [T,N,4]: scores by seat,
    valid where done; seat [T,N]: who played at t.  Returns (ret [T,N] f32, known [T,N] bool):
    `known` is False for the cards of games still unfinished when the rollout ends.
    learner ([N] uint8 seat sets, learner_moves): `known` is also False where another seat than the learner's played
    (tarok_learn_returns_seats); the returns are the same."""
    T, N = done.shape
    ret = torch.zeros((T, N), dtype=torch.float32, device=done.device)
    known = torch.zeros((T, N), dtype=torch.bool, device=done.device)
    cur = torch.zeros((N, 4), dtype=torch.float32, device=done.device)
    have = torch.zeros(N, dtype=torch.bool, device=done.device)
    for t in range(T - 1, -1, -1):
        d = done[t]
        cur = torch.where(d.unsqueeze(-1), reward[t].float(), cur)
        have = have | d
        ret[t] = cur.gather(-1, seat[t].long().unsqueeze(-1)).squeeze(-1)
        known[t] = have
    if learner is not None:
        known &= learner_moves(seat, learner)
    return ret, known


def assign_gae(done, reward, seat, val, gamma, lam, reward_scale, learner=None):
    """Returns by GAE(gamma, lam) per seat, bootstrapped from the value of the same seat's next decision inside the
    rollout: the plain torch statement of tarok_learn_returns_gae (include/tarok_env.h), the counterpart of
    assign_returns.

    done, reward, seat as in assign_returns, val [T,N]: the value at play time.  Per seat s the backward walk keeps what
    the seat's next decision left: nv (its value), na (its advantage), pr (the seat's final score * reward_scale if its
    game ended in between, else 0), have (there is such a decision, or the game ended).  gamma discounts per decision of
    the seat, not per lock-step.  Returns (ret [T,N] f32 = advantage + value, already scaled; known [T,N] bool):
    `known` is False only for a seat's last decision of a game still unfinished when the rollout ends.  The walk itself
    runs in float64 (this is the reference statement, not the hot path), so `ret` is the recursion's value rounded once.
    learner ([N] uint8 seat sets as in assign_returns): `known` is also False where another seat than the learner's
    played (tarok_learn_returns_seats with gae = 1).  The walk is the same for every seat — a seat's chain reads that
    seat's values only — so the returns are the same."""
    T, N = done.shape
    dev = done.device
    ret = torch.zeros((T, N), dtype=torch.float32, device=dev)
    known = torch.zeros((T, N), dtype=torch.bool, device=dev)
    nv = torch.zeros((N, 4), dtype=torch.float64, device=dev)
    na, pr = torch.zeros_like(nv), torch.zeros_like(nv)
    have = torch.zeros((N, 4), dtype=torch.bool, device=dev)
    seats = torch.arange(4, device=dev)
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    for t in range(T - 1, -1, -1):
        d = done[t].bool().unsqueeze(-1)
        pr = torch.where(d, reward[t].double() * reward_scale, pr)
        nv, na = torch.where(d, zero, nv), torch.where(d, zero, na)
        have = have | d
        s = seat[t].long().unsqueeze(-1)
        pick = lambda x: x.gather(-1, s).squeeze(-1)
        v = val[t].double()
        h = pick(have)
        a = torch.where(h, (pick(pr) + gamma * pick(nv) - v) + gamma * lam * pick(na), zero)
        ret[t], known[t] = (a + v).float(), h
        mine = seats == s
        nv, na, pr = torch.where(mine, v.unsqueeze(-1), nv), torch.where(mine, a.unsqueeze(-1), na), torch.where(mine, zero, pr)
        have = have | mine
    if learner is not None:
        known &= learner_moves(seat, learner)
    return ret, known


def assign_gae_seats(done, reward, seat, val, gamma, lam, reward_scale, learner=None):
    """assign_gae under its earlier name for the seat-masked call."""
    return assign_gae(done, reward, seat, val, gamma, lam, reward_scale, learner=learner)


def dw_ranges(B, cap=K.LEARN_MAX_BATCH):
    """The row ranges [(r0, r1), ...] over which update_fused computes the weight gradients of a minibatch of B
    samples: tarok_learn_dw takes at most `cap` samples per launch (32-bit buffer offsets), so a larger minibatch is
    split into ceil(B / cap) consecutive ranges of nearly equal size.  Exact: the gradient is linear in the samples
    and every range is scaled by the whole minibatch's 1 / sum w (terms[3])."""
    k = max(1, -(-B // cap))
    per = -(-B // k)
    return [(r0, min(r0 + per, B)) for r0 in range(0, B, per)]


def learn_dw_ranges(env, B, acts, terms, work, grad, gpart, cap=K.LEARN_MAX_BATCH):
    """env.learn_dw of a minibatch of B samples, one launch per row range of dw_ranges(B, cap): acts = (Xw, H1, H2, dOut,
    dH2, dH1) of the minibatch, passed as row-offset views; the first range writes `grad`, every later one `gpart`
    [MLP_PARAMS] f32 (unused when B <= cap), which is then added in, in range order."""
    for k, (r0, r1) in enumerate(dw_ranges(B, cap)):
        env.learn_dw(r1 - r0, *[a[r0:] if r0 else a for a in acts], terms, work, grad if k == 0 else gpart)
        if k:
            grad += gpart


def allreduce_flat(flat):
    """Average ONE flat gradient vector over all ranks in place (the fused learner's gradients already are one
    buffer: no gather, no scatter).  No-op without an initialised process group / with one rank."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return 0
    dist.all_reduce(flat, op=dist.ReduceOp.SUM)
    flat /= dist.get_world_size()
    return flat.numel() * flat.element_size()


def allreduce_gradients(params):
    """Sum the gradients of `params` over all ranks in ONE flattened all-reduce and
    average them.  No-op without an initialised process group / with one rank."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return 0
    grads = [p.grad for p in params if p.grad is not None]
    flat = torch.cat([g.reshape(-1) for g in grads])
    dist.all_reduce(flat, op=dist.ReduceOp.SUM)
    flat /= dist.get_world_size()
    off = 0
    for g in grads:
        n = g.numel()
        g.copy_(flat[off:off + n].view_as(g))
        off += n
    return flat.numel() * flat.element_size()


class SelfPlay:
    """All four seats of every game share one policy.

    The rollout is captured once into a graph (torch.cuda.graph: the library's kernels are
    launched on torch's capture stream) and replayed: per lock-step ONE tarok_policy_mlp launch
    (features -> MLP on the matrix cores -> masked sample, hidden = 256) and one tarok_step
    launch, both writing straight into their rows of static rollout buffers.  With another
    hidden size the policy runs as tarok_observe -> torch GEMMs -> tarok_sample_policy.

    opponent (a snapshot()): train against that frozen network instead of against oneself.  Per slot the seats of
    `learner_seats` play and learn the current weights, the others play the opponent (tarok_policy_step_versus: needs
    the fused policy and the fused step); only the learner's samples are `known` to the update
    (tarok_learn_returns_seats), and the fused update compacts them (tarok_learn_select) so that its minibatches hold
    nothing else.  learner_seats: an int 0..15 (one seat set for every slot) or a [N] uint8 tensor of sets; default:
    slot g owns the single seat (game_offset + g) % 4, so a sharded run seats the same games the same way.
    set_opponent() swaps the opponent's weights without a new graph capture.
    opponent=[snapshot, ...] (a list or tuple of 1..64 snapshots): a POOL of K frozen opponents in the same rollout
    (tarok_policy_step_pool, still one launch per lock-step in the one captured graph).  The object owns the six stacked
    tensors and a group_net tensor: step group g (slots 256 g .. 256 g + 255 of this env) meets opponent g % K, game after
    game.  self_play_groups = f in [0, 1] mixes plain self-play in: with P = max(1, round(1 / f)) every group with
    g % P == 0 plays the learner on all four seats instead (pool index K; its slots' learner sets become 15, so all four
    seats learn); the other groups keep opponent g % K; f = 0 (the default): no such group.  set_opponent(w, index=k)
    overwrites entry k in place.  iterate() adds learner_mean_score_by_opponent (K floats: learner_mean_score over the
    slots of each opponent's groups) and, with self-play groups, learner_mean_score_self.  A pool of K copies of one
    snapshot trains to the bits of opponent=snapshot.

    teacher = dict(worlds=W, samples=S, tau=tau, every=k, salt=...): learn from the playout teacher as well (expert
    iteration).  Before the policy launch of every k-th lock-step (every: default 1) the rollout runs one playout launch
    on the learner's seats — tarok_playout_cards_det with W worlds, or the open-hand tarok_playout_cards with worlds=0 —
    and one tarok_playout_targets on the words the policy is about to choose its cards on, into buf["teach"] [T,N,64] bf16
    (rows of the other lock-steps stay zero).  Both are stream-ordered and read-only on the env: they sit inside the one
    captured rollout graph and the rollout's own bytes do not change.  The update then adds distill_coef x the
    cross-entropy of the policy against those rows (tarok_learn_chain_distill; on the torch paths in torch) and the stats
    gain distill_ce and teacher_frac (the weighted mean of the rows' sums: about the share of weighted samples with a
    teacher).  distill_coef = 0 with a teacher measures the term without acting on it.  teacher=None: nothing changes.
    teacher = dict(..., worlds=W >= 1, voids=True): the rows come from the void-aware worlds — tarok_shown_voids, then
    tarok_playout_cards_voids, then tarok_playout_targets, still one stream-ordered chain inside the captured rollout.
    The env must keep the play history (TarokVecEnv(history=True)).
    teacher = dict(..., worlds=W >= 1, hidden=True): the rows come from worlds that also re-deal Klop's face-down talon and
    the declarer's discards — tarok_played_cards, then tarok_playout_cards_hidden, then tarok_playout_targets, recorded
    the same way.  Needs the play history too; not together with voids=True.
    teacher = dict(worlds=W >= 1, net=True, net_seats=15, tau=..., every=..., salt=...): the playouts of the W worlds are
    played by the LEARNER's own rollout weights — tarok_playout_cards_net on the weights the rollout plays with, the seats
    of net_seats greedy, the others the Bot — so the teacher improves with its student.  One playout per
    (card, world): `samples` is optional and must be 1; tarok_playout_targets divides by W.  Not together with voids or
    hidden; needs the fused policy (hidden = 256).  The launch's scratch is allocated before the rollout is captured, and
    a replayed graph reads the weights in place.  The launch is costly: `every` matters.
    teacher = dict(..., net=True, net_worlds="voids" | "hidden"): the network's playouts run in the void-aware worlds
    (tarok_shown_voids, then tarok_playout_cards_net_voids) or in the worlds that also re-deal Klop's talon and the
    declarer's discards (tarok_played_cards, then tarok_playout_cards_net_hidden), so the net seats never answer a hand
    the table knows to be impossible.  The words, the three launches and tarok_playout_targets are one
    stream-ordered chain inside the captured rollout; the env must keep the play history.  "det" (the default) is the
    launch above.  net=True with voids=True / hidden=True keeps raising, as it always has: net_worlds is the way in.
    teacher = dict(..., net=True, depth=D): the network's playouts stop at the mover's D-th next decision (1..12) and take
    the learner's own value head there, at value_scale = 1 / reward_scale — the head's unit turned back into points
    (tarok_playout_cards_net_value in the worlds of net_worlds).  The call sits inside the captured rollout
    on the live weights like the launch above; at D = 1 a playout is at most 6 cards long.  Without the key: as before.
    teacher = dict(halving=(w0, w1, ..), samples=S, tau=, every=, salt=, voids= | hidden=): the Bot-played worlds are spent by
    sequential halving (tarok_playout_cards_halving: 1..4 rounds, `worlds` omitted or their sum, samples optional: 1) and the
    rows come from tarok_playout_targets_counts on the launch's counts — both inside the captured rollout, the counts
    buffer allocated before capture.  Not with net=True.
    teacher = dict(net=True, net_halving=(w0, w1, ..), ...): the NETWORK's playouts are spent by sequential halving on a
    compacted item list (tarok_playout_cards_net_halving, DESIGN 8.21: `worlds` omitted, None or their sum; with net_seats,
    net_worlds and depth as above) and the rows come from tarok_playout_targets_counts.  The launch's scratch and the counts
    buffer are allocated before capture; a replayed graph reads the live rollout weights.
    teacher = dict(net=True, worlds=W, versus=(own_rel, opp_rel), ...) with opponent=<one snapshot>: the teacher's playouts seat
    TWO networks relative to each game's mover (tarok_playout_cards_net_versus) — the learner's live rollout
    weights on the relative seats of own_rel, the frozen opponent's tensors on those of opp_rel —, inside the captured rollout;
    (1, 14) makes the targets a search against the opponent actually at the table, and set_opponent() is picked up without a
    new capture.  It goes with net_worlds, depth and net_halving; net_seats is left out.  Without opponent=, or with a pool: a
    ValueError.
    teacher = dict(net=True, worlds=W, samples=S, temperature=t[, epsilon=e, versus=(1, 14), opp_temperature=, opp_epsilon=]): the
    teacher's networks play as they play AT THE TABLE (tarok_playout_cards_net_sampled) — the learner's weights draw
    from their softmax at temperature t (0: greedy), the Bot's card with probability e —, S playouts (default 1) per (card,
    world) on draws of their own, so the rows value the policy that goes on playing and more samples cut their variance.  The
    key `temperature` (or epsilon / opp_temperature / opp_epsilon) selects this launch: a dict without any of them is the
    greedy launch as before, where samples above 1 keeps raising.  With versus and no opp_temperature (no opp_epsilon), the
    frozen opponent's mode is the ENV'S CURRENT PLAY MODE (env.play_mode, read when the rollout is issued or captured): the
    mode the opponent actually plays at the table, which is the point of the launch; without versus the network sits on all
    four seats, (15, 0).  Inside the captured rollout, scratch allocated before capture.  Not with net_seats or net_halving.

    front = dict(bid=, exchange=, contracts=, margin=, pass_value=, every=1): the games auto-reset swaps in are bid and
    exchanged by the heads instead of the Bot (TarokVecEnv.front_lines).  bid / exchange: six tensors each
    (read in place) or a BidLearner / ExchangeLearner (its network, copied in place at the head of every rollout).  The
    run's first games go through bid_values -> bid_round -> reset(defer_exchange=True) -> exchange_values -> exchange, then
    prefetch and front_lines; every rollout then opens with one front_lines call inside the captured graph (every = k > 1:
    before every k-th rollout, outside it).  The heads sit on the learner's seats in opponent and pool mode and on all four
    in self-play.  T * every may not exceed FRONT_MAX_T = 48.  iterate() adds `fronted` (lines the rollout's call decided)
    and `front_contract_share` (ten shares).  front=None: the launches are the ones issued without it."""

    def __init__(self, env, hidden=256, lr=3e-4, clip=0.2, vf_coef=0.5, ent_coef=0.01, reward_scale=1.0 / 70.0, seed=0,
                 use_graph=True, fused=None, fused_loss=None, fused_step=None, fused_learner=None, max_grad_norm=1.0,
                 gamma=None, gae_lambda=None, opponent=None, learner_seats=None, teacher=None, distill_coef=0.0,
                 self_play_groups=0.0, front=None):
        self.front = self.check_front(front, env)
        if opponent is None and learner_seats is not None:
            raise ValueError("learner_seats says which seats learn against an opponent: pass opponent= (a snapshot()) as well")
        pool = self.is_pool(opponent)
        if pool and not 1 <= len(opponent) <= K.POOL_MAX:
            raise ValueError("opponent: a pool holds 1..%d snapshots, got %d" % (K.POOL_MAX, len(opponent)))
        if self_play_groups and not pool:
            raise ValueError("self_play_groups mixes plain self-play into an opponent POOL: pass opponent=[snapshot, ...] as well")
        self.pool_period(self_play_groups)            # (a ValueError outside 0..1)
        if opponent is not None:
            is_fused = (hidden == 256) if fused is None else bool(fused)
            if not is_fused or not (is_fused if fused_step is None else bool(fused_step)):
                raise RuntimeError("an opponent is seated by tarok_policy_step_versus, which needs the fused policy (hidden = 256) "
                                   "and the fused step")
            if isinstance(learner_seats, int) and not 0 <= learner_seats <= 15:
                raise ValueError("learner_seats: a seat set 0..15 or a [N] uint8 tensor of sets")
        self.teacher, self._player, self.distill_coef = None, None, float(distill_coef)
        if teacher is not None:                       # the card player is playout.card_player's; tau and every are the teacher's own
            unknown = set(teacher) - {"worlds", "samples", "tau", "every", "salt", "voids", "hidden", "net", "net_seats", "net_worlds", "depth",
                                      "halving", "net_halving", "versus"} - set(playout.SAMPLED_KEYS)
            net = bool(teacher.get("net", False))
            # the sampled launch is asked for by a play-mode key; `samples` then is its playouts per (card, world)
            sampled = {k: teacher[k] for k in playout.SAMPLED_KEYS[1:] if teacher.get(k) is not None}
            if sampled and not net:
                raise ValueError("teacher: temperature / epsilon / opp_temperature / opp_epsilon set how the NETWORK plays inside the "
                                 "playouts: they go with net=True")
            if sampled:
                sampled["samples"] = teacher.get("samples", 1)
            if unknown or ("samples" not in teacher and not net and "halving" not in teacher):
                raise ValueError("teacher: dict(worlds=W, samples=S, tau=tau, every=k, salt=...) or dict(halving=(w0, ..), ...): samples "
                                 "required unless net=True or halving= is given; unknown keys %s" % sorted(unknown))
            if "net_seats" in teacher and not net:
                raise ValueError("teacher: net_seats names the network's seats inside the playouts: it goes with net=True")
            versus = teacher.get("versus")
            if versus is not None and (opponent is None or pool):
                raise ValueError("teacher: versus=(own_rel, opp_rel) seats the frozen opponent inside the teacher's playouts: it goes with "
                                 "opponent= (ONE snapshot(), not a pool)")
            options = dict(halving=teacher.get("halving"), net_halving=teacher.get("net_halving"), net_versus=versus, net_sampled=sampled or None)
            p = playout.card_player(1 if sampled else int(teacher.get("samples", 1)), int(teacher.get("worlds") or 0), bool(teacher.get("voids", False)),
                                    bool(teacher.get("hidden", False)), net, int(teacher.get("net_seats", 15)), teacher.get("net_worlds", "det"),
                                    teacher.get("depth"), 1.0 / reward_scale if reward_scale else 0.0, int(teacher.get("salt", 0)),
                                    fused=(hidden == 256) if fused is None else bool(fused), history=getattr(env, "history", False), own=False,
                                    say=playout.spelling("teacher: ", net_depth="depth", net_value_scale="1 / reward_scale"), **options)
            tau, every = float(teacher.get("tau", 1.0)), int(teacher.get("every", 1))
            if not (every >= 1 and 0.0 <= tau < float("inf")):
                raise ValueError("teacher: tau >= 0 and finite, every >= 1")
            self._player = p                          # self.teacher: the same player as the dict it has always been
            self.teacher = dict(worlds=p.worlds, samples=p.samples, tau=tau, every=every, salt=p.salt, voids=p.kind == "voids" and not net,
                                hidden=p.kind == "hidden" and not net, net=net, net_seats=p.net_seats, net_worlds=p.kind if net else "det")
            if p.depth is not None:
                self.teacher["depth"] = p.depth
            if p.halving is not None:
                self.teacher["net_halving" if net else "halving"] = p.halving
            if versus is not None:
                self.teacher["versus"] = p.versus
            if sampled:
                self.teacher.update(temperature=p.modes[0], epsilon=p.modes[1], opp_temperature=sampled.get("opp_temperature"),
                                    opp_epsilon=sampled.get("opp_epsilon"))
        elif distill_coef:
            raise ValueError("distill_coef weighs the playout teacher's term: pass teacher= as well")
        self.env = env
        # returns: both None = every card credited with its seat's final score (Monte-Carlo: assign_returns /
        # tarok_learn_returns); either set = per-seat GAE(gamma, lambda), the other defaulting to 1.0 (assign_gae /
        # tarok_learn_returns_gae)
        self.gae = gamma is not None or gae_lambda is not None
        self.gamma = 1.0 if gamma is None else float(gamma)
        self.gae_lambda = 1.0 if gae_lambda is None else float(gae_lambda)
        self.device = env.device
        torch.manual_seed(seed)                       # same initial weights on every rank
        self.net = PolicyNet(hidden).to(self.device)
        self.lr, self.max_grad_norm = lr, max_grad_norm
        # ONE flat parameter vector (tarok_env.h TAROK_MLP_*): the module's parameters are views into it, so the
        # torch paths and the fused learner (tarok_learn_*: flat gradient, flat Adam state) see the same weights
        self.flat = None
        if hidden == 256:
            ps = [self.net.fc1.weight, self.net.fc1.bias, self.net.fc2.weight, self.net.fc2.bias, self.net.head.weight, self.net.head.bias]
            self.flat = torch.cat([p.detach().reshape(-1) for p in ps]).contiguous()
            assert self.flat.numel() == K.MLP_PARAMS
            off = 0
            for p in ps:
                p.data = self.flat[off:off + p.numel()].view_as(p)
                off += p.numel()
        self.opt = torch.optim.Adam(self.net.parameters(), lr=lr)
        self.clip, self.vf_coef, self.ent_coef, self.reward_scale = clip, vf_coef, ent_coef, reward_scale
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(1234 + 7919 * sharding.world()[0])
        self.hgen = torch.Generator()                 # host side: the fused learner's epoch permutations
        self.hgen.manual_seed(4321 + 7919 * sharding.world()[0])
        self.shuffle = "affine"
        self.obs_words = env.reset().words.clone()
        self.use_graph = use_graph
        self.fused = (hidden == 256) if fused is None else bool(fused)
        assert not self.fused or hidden == 256, "tarok_policy_mlp is built for hidden = 256"
        # the loss and its gradient in one kernel (tarok_ppo_loss) instead of ~40 framework kernels
        self.fused_loss = True if fused_loss is None else bool(fused_loss)
        # policy and env step in one launch per lock-step (tarok_policy_step)
        self.fused_step = self.fused if fused_step is None else bool(fused_step)
        # the whole update as tarok_learn_* launches: returns, forward + loss + backward chain, weight gradients,
        # clip + Adam on the flat vectors (update_fused)
        self.fused_learner = (self.fused and env.device.type == "cuda") if fused_learner is None else bool(fused_learner)
        assert not self.fused_learner or self.fused, "the fused learner is built for the fused policy (hidden = 256)"
        self._graph, self._buf, self._T = None, None, 0
        self._w = None                                # rollout copies of the weights (bf16) / biases (f32)
        # opponent mode: copies of the opponent's six tensors that belong to this object (the captured rollout reads them,
        # set_opponent writes them, no update ever does) and the learner's seat set of every slot
        # pool mode: _opp is the six STACKED tensors of the K opponents (tarok_policy_step_pool), _group_net the index of
        # every step group, K for a self-play group
        self._opp, self._seats, self._pool_k, self._group_net = None, None, 0, None
        if opponent is not None:
            if pool:
                self._pool_k = len(opponent)
                self._opp = [t.to(self.device) for t in env.stack_pool(opponent)]
                index = self.pool_group_net((env.n + 255) // 256, self._pool_k, self_play_groups)
                self._group_net = torch.tensor(index, dtype=torch.uint8, device=self.device)
            else:
                self._opp = [t.detach().to(self.device).clone().contiguous() for t in env.check_mlp_weights(opponent)]
            if learner_seats is None:
                learner_seats = (1 << ((torch.arange(env.n, dtype=torch.int64) + env.game_offset) % 4)).to(torch.uint8)
            elif not torch.is_tensor(learner_seats):
                learner_seats = torch.full((env.n,), int(learner_seats), dtype=torch.uint8)
            if learner_seats.dtype != torch.uint8 or tuple(learner_seats.shape) != (env.n,):
                raise ValueError("learner_seats: a seat set 0..15 or a [N] uint8 tensor of sets")
            self._seats = learner_seats.detach().to(self.device).clone().contiguous()
            if pool:                                  # a self-play group's four seats are all the learner's
                own = (self._group_net.long() >= self._pool_k).repeat_interleave(256)[:env.n]
                self._seats[own] = 15
        if self.front is not None:                    # the first games through the heads' existing chain, the lines behind them
            self._front_w = {k: ([t.detach().clone().contiguous() for t in self.front[k].weights()] if hasattr(self.front[k], "weights")
                                 else self.front[k]) for k in ("bid", "exchange")}
            self._front_count = torch.zeros(1, dtype=torch.int64, device=self.device)
            self._front_hist = torch.zeros(10, dtype=torch.int64, device=self.device)
            self._front_total = torch.zeros(11, dtype=torch.int64, device=self.device)     # lines and contracts over a rollout
            self.obs_words = self._front_start().words.clone()
        self._learn = None                           # the fused learner's buffers
        if self.fused_learner:
            dev = self.device
            bf = lambda k: torch.empty(k, dtype=torch.bfloat16, device=dev)
            self._wf = dict(w1=bf(65536), w2=bf(65536), w3=bf(16384), w3t=bf(16384), w2t=bf(65536))
            self.gflat = torch.zeros(K.MLP_PARAMS, dtype=torch.float32, device=dev)
            self.adam_m = torch.zeros_like(self.gflat)
            self.adam_v = torch.zeros_like(self.gflat)
            self.adam_step = torch.zeros(1, dtype=torch.int32, device=dev)
            self.sync_weights()
            f = self.flat
            sl = lambda a, k: f[a:a + k]
            # the rollout reads the learner's own copies: fragment-order weights, biases inside the flat vector
            self._w = [self._wf["w1"].view(256, 256), sl(K.MLP_B1, 256), self._wf["w2"].view(256, 256), sl(K.MLP_B2, 256),
                       self._wf["w3"].view(64, 256), sl(K.MLP_B3, 64)]

    FRONT_MAX_T = 48          # one-card launches between two front_lines calls that leave no game to start unfronted

    @staticmethod
    def check_front(front, env):
        """front=dict(bid=, exchange=, contracts=, margin=, pass_value=, every=) as SelfPlay keeps it, or a ValueError.  bid /
        exchange: six tensors as policy_mlp takes them (read in place by every rollout) or a BidLearner / ExchangeLearner
        (its network, copied into tensors of this object's at the head of every rollout); a BidLearner brings its scale,
        playouts_equiv, contracts and pass_value along (scale= / playouts= for plain tensors)."""
        if front is None:
            return None
        unknown = set(front) - {"bid", "exchange", "contracts", "margin", "pass_value", "every", "scale", "playouts"}
        if unknown:
            raise ValueError("front: dict(bid=, exchange=, contracts=, margin=, pass_value=, every=); unknown keys %s" % sorted(unknown))
        bid, exchange = front.get("bid"), front.get("exchange")
        if bid is None and exchange is None:
            raise ValueError("front: give bid= or exchange= (weights or a learner), or both")
        learner = hasattr(bid, "weights")
        f = dict(bid=bid, exchange=exchange, margin=int(front.get("margin", 0)), every=int(front.get("every", 1)),
                 contracts=int(front.get("contracts", bid.contracts if learner else K.BID_DEFAULT_CONTRACTS)),
                 pass_value=bool(front.get("pass_value", bid.pass_value if learner else False)),
                 scale=float(front.get("scale", bid.scale if learner else 0.0)),
                 playouts=int(front.get("playouts", bid.playouts_equiv if learner else 1)))
        if f["every"] < 1:
            raise ValueError("front: every >= 1 (rollouts per front_lines call)")
        if not 1 <= f["contracts"] <= K.BID_ALL_CONTRACTS:
            raise ValueError("front: contracts is a bit set within 1..0x3FF")
        if bid is not None and not 0.0 < f["scale"] <= 2.0 ** 20:
            raise ValueError("front: bid= as plain tensors needs scale= (bid_values' scale, 0 < scale <= 2**20)")
        if f["playouts"] < 1:
            raise ValueError("front: playouts >= 1")
        if bid is not None and env.mix != K.MIX_BOT:
            raise ValueError("front: bid= re-bids K.MIX_BOT's round: the env's mix must be K.MIX_BOT")
        for k in ("bid", "exchange"):
            if f[k] is not None and not hasattr(f[k], "weights"):
                f[k] = env.check_mlp_weights(f[k])
        return f

    def _front_args(self):
        f = self.front
        return dict(bid=self._front_w["bid"], exchange=self._front_w["exchange"], scale=f["scale"] if f["bid"] is not None else None,
                    contracts=f["contracts"], margin=f["margin"], pass_value=f["pass_value"], playouts=f["playouts"],
                    seats=15, seats_per_game=self._seats)

    @torch.no_grad()
    def _front_refresh(self):
        for k in ("bid", "exchange"):
            if hasattr(self.front[k], "weights"):
                for dst, src in zip(self._front_w[k], self.front[k].weights()):
                    dst.copy_(src)                    # in place: the captured rollout reads these tensors

    @torch.no_grad()
    def _front_start(self):
        """The run's first games through the heads' own chain (bid_values -> bid_round -> reset(defer_exchange=True) ->
        exchange_values -> exchange), then prefetch and the first front_lines: returns the first observation."""
        env, a = self.env, self._front_args()
        sets = dict(seats=a["seats"], seats_per_game=a["seats_per_game"])
        setup = {}
        if a["bid"] is not None:
            values = env.bid_values(0, a["bid"], a["scale"], contracts=a["contracts"], pass_value=a["pass_value"], **sets)
            c, d, k = env.bid_round(0, values, a["playouts"], threshold=a["margin"], contracts=a["contracts"], pass_value=a["pass_value"], **sets)
            setup = dict(contract=c, declarer=d, king_suit=k)
        env.reset(0, defer_exchange=True, **setup)
        obs = env.exchange(*env.exchange_values(a["exchange"], **sets)) if a["exchange"] is not None else env.exchange()
        env.prefetch()
        env.front_lines_scratch()                     # allocated here, before any capture
        env.front_lines(**a)
        return obs

    def _front_call(self):
        """front_lines at the head of a rollout; its count and contracts are the rollout's _front_total."""
        self._front_refresh()
        self.env.front_lines(count_out=self._front_count, hist_out=self._front_hist, **self._front_args())
        self._front_total[:1].copy_(self._front_count)
        self._front_total[1:].copy_(self._front_hist)

    def sync_weights(self):
        """Rebuild the kernels' bf16 fragment-order weight copies from the flat parameter vector (after loading a
        checkpoint or changing the parameters by hand; the fused Adam step keeps them current itself)."""
        self.env.learn_adam(self.flat, None, None, None, None, self._wf, apply=False)

    def _refresh_rollout_weights(self):
        if self.fused_learner:                        # (tarok_learn_adam wrote them with the update)
            return
        with torch.no_grad():
            n = self.net
            src = [(n.fc1.weight, torch.bfloat16), (n.fc1.bias, torch.float32), (n.fc2.weight, torch.bfloat16),
                   (n.fc2.bias, torch.float32), (n.head.weight, torch.bfloat16), (n.head.bias, torch.float32)]
            conv = (lambda p, dt: self.env.mfma_weight_order(p) if (self.fused and dt == torch.bfloat16)
                    else p.detach().to(dt).contiguous().clone())
            if self._w is None:
                self._w = [conv(p, dt) for p, dt in src]
            else:
                for d, (p, dt) in zip(self._w, src):
                    d.copy_(conv(p, dt))              # in place: the captured graph reads these tensors

    @torch.no_grad()
    def snapshot(self):
        """A detached copy of the current policy as the kernels read it (w1, b1, w2, b2, w3, b3: what evaluate()
        plays), safe to keep across later updates: evaluate(opponent=...) takes it."""
        if not self.fused:
            raise RuntimeError("snapshot() copies the weights of the fused policy, which is built for hidden = 256")
        if self._w is None or not self.fused_learner:
            self._refresh_rollout_weights()
        return tuple(t.detach().clone().contiguous() for t in self._w)

    @staticmethod
    def is_pool(opponent):
        """opponent= is a POOL when it is a list or tuple whose entries are not tensors (snapshots, or nothing at all); a
        single snapshot — six tensors — is today's one frozen opponent."""
        return isinstance(opponent, (list, tuple)) and not (len(opponent) and torch.is_tensor(opponent[0]))

    @staticmethod
    def pool_period(self_play_groups):
        """self_play_groups = f in [0, 1] -> the period P of the self-play groups: 0 (none) for f = 0, else
        max(1, round(1 / f)) — every P-th step group plays itself."""
        f = float(self_play_groups)
        if not 0.0 <= f <= 1.0:
            raise ValueError("self_play_groups: the share of step groups that play plain self-play, 0..1")
        return 0 if f == 0.0 else max(1, round(1.0 / f))

    @staticmethod
    def pool_group_net(groups, k, self_play_groups=0.0):
        """The pool index of every step group (group g = slots 256 g .. 256 g + 255), a list of `groups` ints: g % k,
        except that with P = pool_period(self_play_groups) > 0 every group with g % P == 0 gets k — the learner itself."""
        period = SelfPlay.pool_period(self_play_groups)
        return [k if period and g % period == 0 else g % k for g in range(groups)]

    @torch.no_grad()
    def set_opponent(self, weights, index=None):
        """Replace the frozen opponent by `weights` (a snapshot()): copied IN PLACE into the tensors the captured rollout
        graph reads, so the next collect() plays the new opponent without a new capture.  With a pool: entry `index`
        (required) of it."""
        if self._opp is None:
            raise RuntimeError("set_opponent() needs a SelfPlay made with opponent=")
        if self._pool_k:
            if index is None or not 0 <= int(index) < self._pool_k:
                raise ValueError("set_opponent() on a pool of %d needs index=0..%d" % (self._pool_k, self._pool_k - 1))
            for dst, src in zip(self._opp, self.env.check_mlp_weights(weights)):
                dst[int(index)].copy_(src)
            return
        if index is not None:
            raise ValueError("set_opponent(index=) names an entry of an opponent pool: this SelfPlay has one opponent")
        for dst, src in zip(self._opp, self.env.check_mlp_weights(weights)):
            dst.copy_(src)

    @torch.no_grad()
    def evaluate(self, n_games=4096, episodes=4, mix=K.MIX_BOT, opponent=None, greedy=False, temperature=None, epsilon=0.0,
                 versus_playout=None, playout_worlds=None, playout_voids=False, playout_exchange=None,
                 playout_hidden=False, playout_bidding=None, pass_value=False, playout_net=False, playout_net_seats=15,
                 playout_net_worlds="det", playout_net_depth=None, playout_halving=None, playout_net_halving=None,
                 playout_net_samples=None, playout_net_temperature=None, playout_net_epsilon=None):
        """Points per game against the Bot on duplicate deals (evaluate.evaluate_vs_bot: its dict), with the current
        weights.  Played on an env of its own: the training env and the captured rollout are left alone.  Per rank,
        and on the SAME deals on every rank (seed 0, game offset 0, whatever the training env's are): the figures of
        one run are comparable from call to call, and ranks holding the same weights return the same numbers —
        averaging them over ranks adds nothing.
        opponent (a snapshot()): points per game against that network instead (evaluate.evaluate_vs_policy: `bot_mean`
        is then the opponent's mean), on the same deals.  A LIST of snapshots: a list of such dicts, one per opponent,
        from one env that plays them all at once (evaluate.evaluate_vs_pool).
        greedy=True plays the network's best card (temperature 0) instead of a draw from its softmax, temperature a
        tempered draw, epsilon the Bot's card with that probability (TarokVecEnv.set_play_mode, on the evaluation's env
        only: the rollout keeps sampling at (1, 0)).
        versus_playout=samples: returns TWO dicts, (the policy's advantage over the Bot, the open-hand Monte-Carlo
        player's over the Bot on the same deals: evaluate.evaluate_playout_vs_bot with `samples` playouts per card).  The
        playout player sees the true hidden hands, so its figure is an upper-side yardstick, not a fair player's.
        playout_worlds=W (with versus_playout): the second dict is the determinized player's instead (W re-deals of the
        cards its seat cannot see, `samples` playouts per card in each).  Of the two, that one is the FAIR player: it uses
        only its seat's information, so its figure is one a policy can be held against.
        playout_voids=True (with playout_worlds): its worlds also honour the voids the table has seen.
        playout_hidden=True (with playout_worlds, not with playout_voids): its worlds also re-deal Klop's face-down talon
        and the declarer's discards (evaluate_playout_vs_bot(hidden=True)).
        playout_exchange=D (with playout_worlds): the fair player also makes its seat's talon exchange, valued by
        playouts over D discard sets per group (evaluate_playout_vs_bot(exchange=D)).
        playout_bidding=(W, S) (with playout_worlds and mix=K.MIX_BOT): the fair player also bids for its seat, every
        contract valued by playouts (evaluate_playout_vs_bot(bidding=(W, S))).
        pass_value=True (with playout_bidding): its pass is valued by playouts too and is the bar its bids have to clear
        (evaluate_playout_vs_bot(pass_value=True)).
        playout_net=True (with playout_worlds=W, versus_playout=1 and none of the other playout_ options): the second
        dict is the determinized player whose playouts are played by THIS learner's current weights
        (evaluate_playout_vs_bot(net=weights, net_seats=playout_net_seats)): one playout per (card, world).
        playout_net_worlds="voids" / "hidden" (with playout_net): those playouts run in the void-aware worlds or in the
        worlds that also re-deal the talon and the discards (evaluate_playout_vs_bot(net_worlds=...)); "det": as before.
        playout_net with playout_voids / playout_hidden keeps raising: playout_net_worlds is the way in.
        playout_net_depth=D (with playout_net; 1..12): those playouts stop at the player's D-th next decision and take this
        learner's value head there, in points (evaluate_playout_vs_bot(net_depth=D, net_value_scale=1 / reward_scale));
        None: they run to the last card, as before.
        playout_halving=(w0, w1, ..) (with versus_playout=S; playout_worlds None or their sum; with playout_voids /
        playout_hidden; not with playout_net, playout_exchange or playout_bidding): the fair player spends its worlds by
        sequential halving (evaluate_playout_vs_bot(halving=...)).
        playout_net_halving=(w0, w1, ..) (with playout_net; playout_worlds None or their sum; with playout_net_worlds and
        playout_net_depth): the network's playouts are spent by sequential halving on a compacted item list
        (evaluate_playout_vs_bot(net_halving=...)).  playout_halving with playout_net keeps raising.
        playout_net_samples=S, playout_net_temperature=t, playout_net_epsilon=e (with playout_net; any one given; not with
        playout_net_seats or playout_net_halving): inside those playouts the network plays as at the table — a draw from its
        softmax at t (default 1; 0: greedy), the Bot's card with probability e (default 0) —, S playouts (default 1) per
        (card, world) (evaluate_playout_vs_bot(net_samples=, net_temperature=, net_epsilon=)).  None: as before."""
        sampled = {k: v for k, v in dict(samples=playout_net_samples, temperature=playout_net_temperature,
                                         epsilon=playout_net_epsilon).items() if v is not None}
        playout.card_player(versus_playout, playout_worlds, playout_voids, playout_hidden, bool(playout_net), playout_net_seats,
                            playout_net_worlds, playout_net_depth, front=playout_exchange is not None or playout_bidding is not None,
                            say=playout.spelling(pattern="playout_%s", samples="versus_playout"), halving=playout_halving,
                            net_halving=playout_net_halving, net_sampled=sampled or None)
        if playout_halving is not None and versus_playout is None:
            raise ValueError("playout_halving goes with versus_playout=samples")
        if playout_bidding is not None and playout_worlds is None:
            raise ValueError("playout_bidding goes with playout_worlds=W")
        if playout_exchange is not None and playout_worlds is None:
            raise ValueError("playout_exchange goes with playout_worlds=W")
        if playout_worlds is not None and versus_playout is None:
            raise ValueError("playout_worlds goes with versus_playout=samples")
        if versus_playout is not None and opponent is not None:
            raise ValueError("versus_playout compares against the Bot: give it without opponent=")
        if greedy and temperature:
            raise ValueError("greedy=True is temperature 0: give one of the two")
        temperature = 0.0 if greedy else (1.0 if temperature is None else float(temperature))
        if not self.fused:
            raise RuntimeError("evaluate() plays tarok_policy_step_seats, which is built for hidden = 256")
        from .evaluate import evaluate_vs_bot, evaluate_vs_policy
        if self._w is None or not self.fused_learner:
            self._refresh_rollout_weights()
        if self.is_pool(opponent):                    # a list of snapshots: one dict per opponent, one launch per lock-step
            from .evaluate import evaluate_vs_pool
            return evaluate_vs_pool(self._w, opponent, n_games, episodes, mix=mix, device=self.env.device_index,
                                    temperature=temperature, epsilon=epsilon)
        if opponent is not None:
            return evaluate_vs_policy(self._w, opponent, n_games, episodes, mix=mix, device=self.env.device_index,
                                      temperature=temperature, epsilon=epsilon)
        own = evaluate_vs_bot(self._w, n_games, episodes, mix=mix, device=self.env.device_index, temperature=temperature,
                              epsilon=epsilon)
        if versus_playout is None:
            return own
        from .evaluate import evaluate_playout_vs_bot
        if playout_net:                               # what was left at its default is left out: the calls as they were
            more = dict({"net_" + k: v for k, v in sampled.items()}, net_worlds=None if playout_net_worlds == "det" else playout_net_worlds,
                        net_depth=playout_net_depth, net_value_scale=None if playout_net_depth is None else 1.0 / self.reward_scale,
                        net_halving=playout_net_halving)
            return own, evaluate_playout_vs_bot(None, n_games, episodes, mix=mix, device=self.env.device_index, worlds=playout_worlds,
                                                net=self._w, net_seats=playout_net_seats, **{k: v for k, v in more.items() if v is not None})
        return own, evaluate_playout_vs_bot(int(versus_playout), n_games, episodes, mix=mix, device=self.env.device_index,
                                            worlds=playout_worlds, voids=bool(playout_voids), exchange=playout_exchange,
                                            hidden=bool(playout_hidden), bidding=playout_bidding, pass_value=pass_value,
                                            **({} if playout_halving is None else dict(halving=playout_halving)))

    def _alloc(self, T):
        n, dev = self.env.n, self.device
        self._T = T
        # the network input of every step: as 4 x 64 feature bits per game on the fused path (expanded
        # per minibatch in update()), as [256] bf16 otherwise
        obs = (torch.empty((T, n, 4), dtype=torch.int64, device=dev) if self.fused
               else torch.empty((T, n, 256), dtype=torch.bfloat16, device=dev))
        self._buf = dict(obs=obs,
                         words=torch.empty((T + 1, n), dtype=torch.int64, device=dev),
                         act=torch.empty((T, n), dtype=torch.uint8, device=dev),
                         logp=torch.empty((T, n), dtype=torch.float32, device=dev),
                         val=torch.empty((T, n), dtype=torch.float32, device=dev),
                         done=torch.empty((T, n), dtype=torch.uint8, device=dev),
                         reward=torch.zeros((T, n, 4), dtype=torch.int16, device=dev))   # written only where done
        if self.teacher is not None:                  # the teacher's target rows, and the playout launch's own outputs
            self._buf["teach"] = torch.zeros((T, n, 64), dtype=torch.bfloat16, device=dev)
            self._teach_sums = torch.empty((n, K.PLAYOUT_RANKS, 4), dtype=torch.int32, device=dev)
            self._teach_act = torch.empty(n, dtype=torch.uint8, device=dev)
            dtype = self._player.words_dtype            # the voids / played words of the teacher's worlds
            self._teach_words = None if dtype is None else torch.empty(n, dtype=dtype, device=dev)
            self._player.prepare(self.env)            # the net launch's scratch: allocated here, before any capture
            if self._player.counts:                   # a halving teacher's playouts per card: its targets' divisors
                self._teach_counts = torch.empty((n, K.PLAYOUT_RANKS), dtype=torch.int32, device=dev)
        self._graph = None

    def teacher_modes(self):
        """(temperature, epsilon, opp_temperature, opp_epsilon) of a sampled teacher's next launch: the dict's own, and for a
        versus teacher that left the opponent's open, the env's current play mode — what the opponent plays at the table."""
        t, e = self.teacher["temperature"], self.teacher["epsilon"]
        ot, oe = self.env.play_mode if "versus" in self.teacher else (t, e)
        given_t, given_e = self.teacher["opp_temperature"], self.teacher["opp_epsilon"]
        return t, e, ot if given_t is None else float(given_t), oe if given_e is None else float(given_e)

    def _teach(self, t):
        """The teacher's rows of lock-step t: one playout launch on the learner's seats from the env's current positions,
        one tarok_playout_targets on the words of that lock-step.  Stream-ordered, read-only on the env, no allocation.
        A versus teacher's launch reads the live rollout weights as network A and the frozen opponent's own tensors (the ones
        set_opponent writes in place) as network B."""
        p, sets = self._player, dict(seats_per_game=self._seats)
        more = dict(count_out=self._teach_counts) if p.counts else {}
        if p.modes is not None:                       # B's mode, where the dict left it open, is the env's own
            more["modes"] = self.teacher_modes()
        p.launch(self.env, (self._w, self._opp if "versus" in self.teacher else None), sets, self._teach_words, self._teach_sums,
                 self._teach_act, **more)
        if p.counts:                                  # a halving launch: tarok_playout_targets_counts on its counts
            self.env.playout_targets_counts(self._teach_sums, self._teach_counts, self._buf["words"][t], self.teacher["tau"],
                                            target_out=self._buf["teach"][t], **sets)
        else:
            self.env.playout_targets(self._teach_sums, self._buf["words"][t], p.playouts, self.teacher["tau"], target_out=self._buf["teach"][t], **sets)

    def _rollout_body(self, T):
        env, buf, w = self.env, self._buf, self._w
        for t in range(T):
            if self.teacher is not None and t % self.teacher["every"] == 0:
                self._teach(t)
            if self._pool_k:                          # ... the others their step group's entry of the frozen pool
                env.policy_step(w, buf["words"][t], buf["words"][t + 1], buf["act"][t], buf["logp"][t], buf["val"][t],
                                feature_words_out=buf["obs"][t], reward_out=buf["reward"][t], done_out=buf["done"][t],
                                opponent_pool=self._opp, group_net=self._group_net, seats_per_game=self._seats)
                continue
            if self._opp is not None:                 # the learner's seats play w, the others the frozen opponent
                env.policy_step(w, buf["words"][t], buf["words"][t + 1], buf["act"][t], buf["logp"][t], buf["val"][t],
                                feature_words_out=buf["obs"][t], reward_out=buf["reward"][t], done_out=buf["done"][t],
                                opponent=self._opp, seats_per_game=self._seats)
                continue
            if self.fused and self.fused_step:
                env.policy_step(w, buf["words"][t], buf["words"][t + 1], buf["act"][t], buf["logp"][t], buf["val"][t],
                                feature_words_out=buf["obs"][t], reward_out=buf["reward"][t], done_out=buf["done"][t])
                continue
            if self.fused:
                env.policy_mlp(w, buf["words"][t], buf["act"][t], buf["logp"][t], buf["val"][t], feature_words_out=buf["obs"][t])
            else:
                env.observe(buf["obs"][t])
                h = F.relu(F.linear(buf["obs"][t], w[0], w[1].to(torch.bfloat16)))
                h = F.relu(F.linear(h, w[2], w[3].to(torch.bfloat16)))
                out = F.linear(h, w[4], w[5].to(torch.bfloat16))
                buf["val"][t].copy_(out[:, 54])
                env.sample_policy(out, buf["words"][t], buf["act"][t], buf["logp"][t])
            env.step(buf["act"][t], auto_reset=True, obs_out=buf["words"][t + 1], reward_out=buf["reward"][t],
                     done_out=buf["done"][t])

    def _collect_body(self, T):
        """Everything one rollout does on the device, in launch order (captured as ONE graph: the
        weight conversion and the buffer housekeeping are ~20 small launches that would otherwise
        cost more host time than the 48 lock-steps take on the GPU)."""
        buf = self._buf
        self._refresh_rollout_weights()
        buf["reward"].zero_()
        buf["words"][0].copy_(self.obs_words)
        if self.front is not None and self.front["every"] == 1:
            self._front_call()
        self._rollout_body(T)
        self.obs_words.copy_(buf["words"][T])

    @torch.no_grad()
    def collect(self, T):
        """T lock-steps of self-play into the static rollout buffers."""
        if self._buf is None or self._T != T:
            self._alloc(T)
        buf = self._buf
        if self.front is not None:
            if T * self.front["every"] > self.FRONT_MAX_T:
                raise ValueError("front: T * every = %d launches between two front_lines calls; more than %d may start a game that "
                                 "was never fronted" % (T * self.front["every"], self.FRONT_MAX_T))
            self._front_total.zero_()
            self._front_rollouts = getattr(self, "_front_rollouts", 0) + 1
            if self.front["every"] > 1 and (self._front_rollouts - 1) % self.front["every"] == 0:
                self._front_call()                    # (outside the captured rollout: the graph is the same for every rollout)
        if not self.use_graph:
            self._collect_body(T)
            return buf
        if self._graph is None:
            # warm up outside capture (lazy library / GEMM-workspace initialisation, rollout copies of
            # the weights allocated), then continue from the warmed-up env state
            s = torch.cuda.Stream(self.device)
            s.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(s):
                self._collect_body(2)                 # (any number: the refill-list parity lives on the device)
            torch.cuda.current_stream(self.device).wait_stream(s)
            torch.cuda.synchronize(self.device)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                self._collect_body(T)
            self._graph = g
        self._graph.replay()
        return buf

    def update(self, buf, epochs=2, minibatches=8):
        """Clipped-surrogate policy-gradient update on one rollout.  Returns stats."""
        T, n = buf["act"].shape
        words_t = buf["words"][:T]
        seat = (words_t >> K.OBS_SEAT_SHIFT) & 3
        if self.gae:
            ret, known = assign_gae(buf["done"].bool(), buf["reward"], seat, buf["val"], self.gamma, self.gae_lambda, self.reward_scale,
                                    learner=self._seats)
        else:
            ret, known = assign_returns(buf["done"].bool(), buf["reward"], seat, learner=self._seats)
            ret = ret * self.reward_scale
        flat = lambda x: x.reshape(T * n, *x.shape[2:])
        obs, words, act, logp0 = flat(buf["obs"]), flat(words_t), flat(buf["act"]).long(), flat(buf["logp"])
        val0 = flat(buf["val"]).float()
        ret, known = flat(ret), flat(known)
        adv = ret - val0
        m = known.float()
        mean = (adv * m).sum() / m.sum().clamp(min=1)
        std = (((adv - mean) ** 2 * m).sum() / m.sum().clamp(min=1)).sqrt().clamp(min=1e-6)
        adv = (adv - mean) / std
        stats = dict(loss=0.0, pi_loss=0.0, v_loss=0.0, entropy=0.0, allreduce_bytes=0, known_frac=float(m.mean()))
        teach = flat(buf["teach"]) if self.teacher is not None else None
        dsums = torch.zeros(2, dtype=torch.float32, device=self.device) if teach is not None else None
        if self._opp is not None:                     # (the weights m carry the seat mask: the opponent's samples count for nothing)
            stats["learner_samples"] = int(known.sum())
        sums = torch.zeros(4, dtype=torch.float32, device=self.device)     # loss terms summed on the device: no host sync per minibatch
        params = [p for p in self.net.parameters()]
        count = 0
        for _ in range(epochs):
            perm = torch.randperm(T * n, device=self.device, generator=self.gen)
            for idx in perm.chunk(minibatches):
                x = self.env.gather_features(obs, idx) if self.fused else obs[idx]
                w = m[idx]
                a = adv[idx]
                if self.fused_loss:
                    with torch.autocast("cuda", dtype=torch.bfloat16):
                        out = self.net.forward_raw(x)
                    out = out.to(torch.bfloat16).contiguous()
                    terms, dout = self.env.ppo_loss(out.detach(), words[idx], act[idx], logp0[idx], a, ret[idx], w,
                                                    self.clip, self.vf_coef, self.ent_coef)
                    pi_loss, v_loss, ent = terms[0], terms[1], terms[2]
                    loss = pi_loss + self.vf_coef * v_loss - self.ent_coef * ent
                    if teach is not None:                 # tarok_ppo_loss knows no teacher: the term in torch, added to dout
                        legal = legal_matrix(words[idx] & K.OBS_MASK)
                        lp = F.log_softmax(out[:, :54].float().masked_fill(~legal, float("-inf")), dim=-1)
                        lp = torch.where(legal, lp, torch.zeros_like(lp))
                        q = torch.where(legal, teach[idx][:, :54].float(), torch.zeros_like(lp))
                        S = q.sum(-1)
                        wsum = w.sum().clamp(min=1)
                        ce = (-(q * lp).sum(-1) * w).sum() / wsum
                        dsums += torch.stack([ce, (S * w).sum() / wsum])
                        loss = loss + self.distill_coef * ce
                        dd = torch.zeros_like(dout, dtype=torch.float32)
                        dd[:, :54] = (self.distill_coef * w / wsum).unsqueeze(-1) * (S.unsqueeze(-1) * lp.exp() * legal - q)
                        dout = (dout.float() + dd).to(torch.bfloat16)
                    self.opt.zero_grad(set_to_none=True)
                    out.backward(dout)
                else:
                    with torch.autocast("cuda", dtype=torch.bfloat16):
                        logits, val = self.net(x)
                    legal = legal_matrix(words[idx] & K.OBS_MASK)
                    lg = logits.float().masked_fill(~legal, float("-inf"))
                    logp_all = F.log_softmax(lg, dim=-1)
                    logp = logp_all.gather(-1, act[idx].clamp(max=53).unsqueeze(-1)).squeeze(-1)
                    wsum = w.sum().clamp(min=1)
                    ratio = (logp - logp0[idx]).exp()
                    pi_loss = -(torch.min(ratio * a, ratio.clamp(1 - self.clip, 1 + self.clip) * a) * w).sum() / wsum
                    v_loss = (((val.float() - ret[idx]) ** 2) * w).sum() / wsum
                    p = logp_all.exp()
                    ent = (-(p * torch.where(legal, logp_all, torch.zeros_like(logp_all))).sum(-1) * w).sum() / wsum
                    loss = pi_loss + self.vf_coef * v_loss - self.ent_coef * ent
                    if teach is not None:
                        q = torch.where(legal, teach[idx][:, :54].float(), torch.zeros_like(logp_all))
                        ce = (-(q * torch.where(legal, logp_all, torch.zeros_like(logp_all))).sum(-1) * w).sum() / wsum
                        dsums += torch.stack([ce.detach(), (q.sum(-1) * w).sum() / wsum])
                        loss = loss + self.distill_coef * ce
                    self.opt.zero_grad(set_to_none=True)
                    loss.backward()
                stats["allreduce_bytes"] = allreduce_gradients(params)
                nn.utils.clip_grad_norm_(params, 1.0)
                self.opt.step()
                count += 1
                sums += torch.stack([loss.detach().float(), pi_loss.detach().float(), v_loss.detach().float(), ent.detach().float()])
        for k, v in zip(("loss", "pi_loss", "v_loss", "entropy"), sums.tolist()):
            stats[k] = v / max(1, count)
        if teach is not None:
            stats["distill_ce"], stats["teacher_frac"] = (v / max(1, count) for v in dsums.tolist())
        return stats

    def _learn_bufs(self, M, B):
        """Buffers of the fused learner: per-sample records of a rollout of M samples, activations of a minibatch of
        at most B samples, the weight-gradient workspace."""
        lb = self._learn
        if lb is None or lb["M"] != M or lb["B"] < B:
            dev = self.device
            f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
            act = lambda k: torch.zeros((B + K.LEARN_PAD, k), dtype=torch.bfloat16, device=dev)
            lb = dict(M=M, B=B, rec=f32(M, 4), stats=f32(4), scratch=f32(max((self.env.n + 255) // 256, (B + 95) // 96), 4),
                      gpart=f32(K.MLP_PARAMS) if B > K.LEARN_MAX_BATCH else None,
                      H1=act(256), H2=act(256), dH2=act(256), dH1=act(256), dOut=act(64), terms=f32(4),
                      Xw=torch.zeros((B + K.LEARN_PAD, 4), dtype=torch.int64, device=dev),
                      running=torch.zeros(4, dtype=torch.float32, device=dev),
                      work=torch.empty(self.env.learn_workspace_bytes(), dtype=torch.uint8, device=dev))
            if self.teacher is not None:
                lb.update(dscratch=f32((B + 95) // 96, 2), dterms=f32(2), drunning=torch.zeros(2, dtype=torch.float32, device=dev))
            self._learn = lb
        return lb

    def _epoch_permutation(self, M):
        """The order in which an epoch visits the rollout's M samples: j -> (a j + b) mod M with a coprime to M and (a, b)
        drawn per epoch — a permutation whose consecutive entries lie a samples apart, so every minibatch (a run of it)
        spreads over all lock-steps and slots.  Three elementwise launches instead of torch.randperm's radix sort of M
        keys (0.18 ms of a 5 ms update at 3.1 M samples).  shuffle = "randperm" selects the latter."""
        if self.shuffle == "randperm":
            return torch.randperm(M, device=self.device, generator=self.gen)
        import math
        while True:
            a = int(torch.randint(M // 3, M, (1,), generator=self.hgen)) | 1
            if math.gcd(a, M) == 1:
                break
        b = int(torch.randint(0, M, (1,), generator=self.hgen))
        return (torch.arange(M, device=self.device, dtype=torch.int64) * a + b) % M

    def update_fused(self, buf, epochs=2, minibatches=8):
        """The update as fused launches (include/tarok_env.h tarok_learn_*): per rollout one returns kernel; per
        minibatch the forward + loss + backward chain (activations in LDS, bf16 MFMA), the three weight gradients
        as one split-K launch (one per row range of dw_ranges past TAROK_LEARN_MAX_BATCH samples), ONE flat gradient
        all-reduce, and clip + Adam + weight-copy refresh in one launch.  No host synchronisation until the statistics
        are read at the end.
        Opponent mode: tarok_learn_returns_seats knows the learner's samples only, tarok_learn_select compacts their
        numbers into a list, and ONE host read of the list's length follows — the single synchronisation opponent mode
        adds, per update: the epoch permutation runs over that many entries (not over M), and every minibatch's index
        is a run of it mapped through the list, so no launch computes an opponent's sample."""
        env = self.env
        T, n = buf["act"].shape
        M = T * n
        B = -(-M // minibatches)
        lb = self._learn_bufs(M, B)
        sel, count = None, M
        env.learn_returns_seats(T, buf["done"], buf["reward"], buf["words"][:T], buf["logp"], buf["val"], buf["act"], self.reward_scale,
                                lb["rec"], lb["stats"], lb["scratch"], gae=self.gae, gamma=self.gamma, lam=self.gae_lambda,
                                seats_per_game=self._seats)      # (None outside opponent mode: the unmasked kernel)
        if self._opp is not None:
            if "sel" not in lb:
                lb["sel"] = torch.empty(M, dtype=torch.int64, device=self.device)
                lb["sel_count"] = torch.zeros(1, dtype=torch.int64, device=self.device)
                lb["sel_scratch"] = torch.empty(env.learn_select_scratch_bytes(M), dtype=torch.uint8, device=self.device)
            env.learn_select(M, lb["rec"], lb["sel"], lb["sel_count"], lb["sel_scratch"])
            count = int(lb["sel_count"].item())       # the one host read
            sel = lb["sel"]
            if count == 0:                            # nothing of the learner's: no launch, no step
                none = dict(loss=0.0, pi_loss=0.0, v_loss=0.0, entropy=0.0, allreduce_bytes=0, known_frac=0.0, learner_samples=0)
                if self.teacher is not None:
                    none.update(distill_ce=0.0, teacher_frac=0.0)
                return none
        words = buf["obs"].view(M, 4)
        lb["running"].zero_()
        teach = None
        if self.teacher is not None:
            teach = buf["teach"].view(M, 64)
            lb["drunning"].zero_()
        nbytes = 0
        bias = (self._w[1], self._w[3], self._w[5])
        for _ in range(epochs):
            perm = self._epoch_permutation(count)
            for idx in perm.chunk(minibatches):
                if sel is not None:
                    idx = sel[idx]
                b = idx.numel()
                chain_args = (b, words, idx, lb["rec"], lb["stats"], self.clip, self.vf_coef, self.ent_coef, self._wf, bias,
                              lb["Xw"], lb["H1"], lb["H2"], lb["dOut"], lb["dH2"], lb["dH1"], lb["scratch"], lb["terms"], lb["running"])
                if teach is None:
                    env.learn_chain(*chain_args)
                else:
                    env.learn_chain_distill(*chain_args, teach, self.distill_coef, lb["dscratch"], lb["dterms"], lb["drunning"])
                learn_dw_ranges(env, b, [lb[a] for a in ("Xw", "H1", "H2", "dOut", "dH2", "dH1")], lb["terms"], lb["work"],
                                self.gflat, lb["gpart"])
                nbytes = allreduce_flat(self.gflat)
                env.learn_adam(self.flat, self.gflat, self.adam_m, self.adam_v, self.adam_step, self._wf, lr=self.lr,
                               max_norm=self.max_grad_norm)
        run = lb["running"].tolist()
        cnt = max(1.0, run[3])
        pi, v, ent = run[0] / cnt, run[1] / cnt, run[2] / cnt
        stats = dict(loss=pi + self.vf_coef * v - self.ent_coef * ent, pi_loss=pi, v_loss=v, entropy=ent, allreduce_bytes=nbytes,
                     known_frac=float(lb["stats"][2]))
        if sel is not None:
            stats["learner_samples"] = count
        if teach is not None:
            ce, frac = (v / cnt for v in lb["drunning"].tolist())
            stats.update(distill_ce=ce, teacher_frac=frac, loss=stats["loss"] + self.distill_coef * ce)
        return stats

    def iterate(self, T=48, epochs=2, minibatches=8):
        """One rollout + one update, timed.  Returns stats incl. env steps/s of the rollout and of the whole
        iteration (rollout + update)."""
        torch.cuda.synchronize(self.device)
        t0 = time.perf_counter()
        buf = self.collect(T)
        torch.cuda.synchronize(self.device)
        t1 = time.perf_counter()
        stats = (self.update_fused if self.fused_learner else self.update)(buf, epochs, minibatches)
        torch.cuda.synchronize(self.device)
        t2 = time.perf_counter()
        stats.update(rollout_s=t1 - t0, update_s=t2 - t1, env_steps=T * self.env.n,
                     rollout_steps_per_s=T * self.env.n / (t1 - t0), iteration_steps_per_s=T * self.env.n / (t2 - t0),
                     mean_score=float(buf["reward"].float().sum() / buf["done"].float().sum().clamp(min=1) / 4),
                     env_errors=int((buf["words"] < 0).any()))
        if self.front is not None:                    # the lines the rollout's front_lines call decided, and their contracts' shares
            tot = self._front_total.tolist()
            stats["fronted"] = tot[0]
            stats["front_contract_share"] = [c / max(1, tot[0]) for c in tot[1:]]
        if self._opp is not None:                     # mean final score over the learner's seats of the games that ended
            mine =((self._seats.long().unsqueeze(-1) >> torch.arange(4, device=self.device)) & 1).float()      # [N,4]
            w = buf["done"].float().unsqueeze(-1) * mine
            stats["learner_mean_score"] = float((buf["reward"].float() * w).sum() / w.sum().clamp(min=1))
            if self._pool_k:                          # ... and the same mean over the slots of each opponent's step groups
                k = self._pool_k
                net = self._group_net.long().clamp(max=k).repeat_interleave(256)[:self.env.n]              # [N], k = self
                zero = lambda: torch.zeros(k + 1, dtype=torch.float64, device=self.device)     # (integer sums: exact)
                num = zero().index_add_(0, net, (buf["reward"].double() * w.double()).sum((0, 2)))
                den = zero().index_add_(0, net, w.double().sum((0, 2)))
                mean = (num / den.clamp(min=1)).tolist()
                stats["learner_mean_score_by_opponent"] = mean[:k]
                if bool((self._group_net >= k).any()):
                    stats["learner_mean_score_self"] = mean[k]
        return stats
