"""The exchange head's learner: a network that picks the declarer's talon group and discards.

The teacher is TarokVecEnv.playout_exchange (tarok_playout_exchange): every candidate (group i, discard set d) played out
in determinized worlds, too slow for a self-play loop.  The head is a PolicyNet — the policy's 256 -> 256 -> 256 -> 64
network, so the rollout side is tarok_exchange_values, the policy's own MFMA forward — on one row per talon group.
Output 54 regresses on the group's mean scaled score under the Bot's random discards (a mean over the row's discard sets,
not their maximum: the maximum of noisy sums would be learned as a bias); output c < 54 regresses on the ADVANTAGE of
laying card c down, the mean scaled score of the row's candidates that discarded c minus the row's value target, for the
cards at least one candidate discarded.  Units: `reward_scale` points (1 / 70, as the policy's returns).

The update is plain torch autograd with Adam on purpose: an iteration is dominated by the teacher's launch, and
everything but collect() / exchange() runs on CPU tensors as well (ExchangeLearner(None)).
"""
import torch
import torch.nn.functional as F

from . import karte as K
from . import playout as P
from .bidding import pack_weights
from .env import TarokVecEnv
from .selfplay import PolicyNet

GROUPS = 6            # rows 0..5 of a game's eight can be live; rows 6 and 7 are padding
VALUE = 54            # the output that values a group (PolicyNet's value column)


def exchange_targets(feature_words, sums, cands, playouts, reward_scale):
    """The head's targets from feature words [N, 8, 4] int64 (exchange_values(feature_words=True)), the teacher's sums
    [N, 6 * D, 4] int and its candidates' discards [N, 6 * D, 3] uint8 (exchange_candidates).  Returns
      live  [N, 6] bool        the rows that exist (word 0 is non-zero)
      value [N, 6] float32     mean over d of sums[i * D + d][declarer] / playouts * reward_scale
      score [N, 6, 54] float32 per card c: the mean of the scaled sums of the row's candidates that laid c down, minus value
      known [N, 6, 54] bool    live, and at least one of the row's D candidates laid c down
    Entries outside live / known are zero.
    playouts: a number, or a halving launch's counts [N, 6 * D] — each candidate's sum is then divided by its own count, and
    a row with a candidate that was never played (count 0) is not live."""
    n = feature_words.shape[0]
    sets = sums.shape[1] // GROUPS
    w0 = feature_words[:, :GROUPS, 0]
    live = w0 != 0
    declarer = ((w0[:, 0] >> 55) & 1) + 2 * ((w0[:, 0] >> 56) & 1) + 3 * ((w0[:, 0] >> 57) & 1)        # one-hot bits 54..57
    own = sums.to(torch.float32).gather(2, declarer.view(n, 1, 1).expand(n, GROUPS * sets, 1)).view(n, GROUPS, sets)
    if torch.is_tensor(playouts):
        count = playouts.view(n, GROUPS, sets)
        scaled = own * float(reward_scale) / count.clamp(min=1).to(torch.float32)
        live = live & (count > 0).all(dim=2)
    else:
        scaled = own * (float(reward_scale) / float(playouts))
    value = scaled.mean(dim=2) * live
    c = cands.view(n, GROUPS, sets, 3).long()
    laid = torch.zeros((n, GROUPS, sets, 55), dtype=torch.float32, device=sums.device)
    laid.scatter_(3, c.clamp(max=54), 1.0)                           # 255 (no card) lands in column 54, dropped below
    laid = laid[..., :54]
    count = laid.sum(dim=2)
    known = (count > 0) & live.unsqueeze(-1)
    total = (laid * scaled.unsqueeze(-1)).sum(dim=2)
    score = torch.where(known, total / count.clamp(min=1.0) - value.unsqueeze(-1), torch.zeros_like(total))
    return live, value, score, known


def exchange_loss(out, live, value, score, known):
    """Huber loss (delta 1) of output 54 against `value` over the live rows plus that of outputs c < 54 against `score`
    over the known entries, each term averaged over its own entries (0 where it has none).  out [N, 6, 64]; no gradient
    flows through any other output."""
    out = out.float()
    zero = out.sum() * 0.0
    lv = F.huber_loss(out[..., VALUE][live], value[live], reduction="mean", delta=1.0) if bool(live.any()) else zero
    ls = F.huber_loss(out[..., :54][known], score[known], reduction="mean", delta=1.0) if bool(known.any()) else zero
    return lv + ls


class ExchangeLearner:
    """Regresses a PolicyNet on the playout teacher's exchange values.

    env: a TarokVecEnv, which collect() RESETS with the exchange deferred (give the learner an env of its own), or None
    for a learner on the CPU that is fed batches by hand (loss / step).  worlds, samples, discard_sets: the teacher's
    launch (playout_exchange).  worlds=None: 8, or with net_halving= the schedule's sum.  net: six tensors (policy_mlp's weights, read live at every collect()) — the teacher is then
    playout_exchange_net at (worlds, discard_sets) with the network's greedy card on the seats of net_seats inside the
    playouts, playouts = worlds; `samples` must be 1 or left unset.  net_depth: None, or 1..13 — the teacher is
    playout_exchange_net_value, whose playouts stop at the declarer's net_depth-th decision and read the value head of `net`
    there at net_value_scale points per unit (13 never stops).  net_list=True (with net=): the one teacher launch is
    playout_exchange_net_list, the same numbers from a compacted item list; nothing else changes.
    net_halving: a tuple of 1..4 positive world counts (with net=): the teacher is playout_exchange_net_halving, which spends
    later rounds' worlds on the leading candidates only; it names the worlds itself (`worlds` None or their sum), goes with
    net_depth, and collect() then returns the counts [N, 6 * D] in the place of the scalar playouts."""

    def __init__(self, env, worlds=None, samples=None, discard_sets=4, lr=1e-3, reward_scale=1.0 / 70.0, seed=0, net=None, net_seats=15,
                 net_halving=None, net_list=False, net_depth=None, net_value_scale=70.0):
        if not reward_scale > 0:
            raise ValueError("reward_scale > 0")
        self.net_halving = P.check_front_halving(net_halving, net, net_list, worlds, samples)
        worlds = (8 if worlds is None else worlds) if self.net_halving is None else sum(self.net_halving)
        if net_list and net is None:
            raise ValueError("net_list packs the network's playouts: it needs net=")
        if net_depth is not None:
            if net is None:
                raise ValueError("net_depth stops the network's playouts: it needs net=")
            P.check_depth(net_depth, net_value_scale, P.spelling(), max_depth=K.PLAYOUT_FRONT_MAX_DEPTH)
        if net is not None:
            if samples not in (None, 1):
                raise ValueError("net= runs one playout per (candidate, world): samples must be 1 or unset")
            if not (isinstance(net_seats, int) and 0 <= net_seats <= 15):
                raise ValueError("net_seats: a 4-bit seat set, 0..15")
            net = TarokVecEnv.check_mlp_weights(net)
        samples = (1 if net is not None else 2) if samples is None else samples
        self.net_weights, self.net_seats = net, int(net_seats)
        self.net_depth, self.net_value_scale = net_depth, float(net_value_scale)
        self.net_list = bool(net_list)
        self.env = env
        self.device = env.device if env is not None else torch.device("cpu")
        self.worlds, self.samples, self.discard_sets = int(worlds), int(samples), int(discard_sets)
        self.reward_scale = float(reward_scale)
        with torch.random.fork_rng(devices=[]):       # the initial weights are a function of `seed` alone
            torch.manual_seed(int(seed))
            self.net = PolicyNet(256)
        self.net.to(self.device)
        self.opt = torch.optim.Adam(self.net.parameters(), lr=float(lr))
        self.episode = 0
        self.salt = int(seed)

    # ---- the regression (any device)
    def outputs(self, feature_words):
        """The module's float outputs [N, 6, 64] on feature words [N, 8, 4] int64 (rows 6 and 7 are never live)."""
        fw = feature_words[:, :GROUPS]
        x = TarokVecEnv.expand_feature_words(fw.reshape(-1, 4), torch.float32)
        return self.net.forward_raw(x).view(fw.shape[0], GROUPS, 64)

    def loss(self, feature_words, sums, cands, playouts):
        """exchange_loss of the network on one batch: feature words [N, 8, 4], the teacher's sums [N, 6 * D, 4] at
        `playouts` and its candidates' discards [N, 6 * D, 3]."""
        return exchange_loss(self.outputs(feature_words), *exchange_targets(feature_words, sums, cands, playouts, self.reward_scale))

    def step(self, feature_words, sums, cands, playouts):
        """One Adam step on one batch; returns the loss before the step (a float)."""
        self.opt.zero_grad(set_to_none=True)
        loss = self.loss(feature_words, sums, cands, playouts)
        loss.backward()
        self.opt.step()
        return float(loss.detach())

    # ---- the launches (need the env)
    @torch.no_grad()
    def weights(self):
        return pack_weights(self.net)

    @torch.no_grad()
    def collect(self, episode):
        """(feature_words [N,8,4] int64, sums [N,6*D,4] int32, cands [N,6*D,3] uint8, playouts) of episode `episode`: a
        reset with the exchange deferred, the teacher's launch on every declarer, its candidates' discards and the head's
        launch for its input rows.  The games are left waiting for the exchange."""
        self.env.reset(episode=episode, defer_exchange=True)
        counts = None
        if self.net_halving is not None:
            sums, counts, _, _ = P.front_halving_launch(self.env, False)(self.net_weights, self.net_halving, self.discard_sets, self.net_depth,
                                                                        self.net_value_scale, net_seats=self.net_seats, salt=self.salt)
        elif self.net_list or self.net_weights is not None:
            launch = P.exchange_net_launch(self.env, self.net_list, True)
            sums, _, _ = launch(self.net_weights, self.worlds, self.discard_sets, self.net_depth, self.net_value_scale,
                                net_seats=self.net_seats, salt=self.salt)
        else:
            sums, _, _ = self.env.playout_exchange(self.worlds, self.samples, self.discard_sets, salt=self.salt)
        cands = self.env.exchange_candidates(self.discard_sets, salt=self.salt)
        _, _, _, fw = self.env.exchange_values(self.weights(), feature_words=True)
        return fw, sums, cands, self.worlds * self.samples if counts is None else counts

    def iterate(self):
        """collect() on a fresh episode and one step(); returns the loss before the step."""
        batch = self.collect(self.episode)
        self.episode += 1
        return self.step(*batch)

    @torch.no_grad()
    def exchange(self, seats=15, seats_per_game=None):
        """The exchange of the env's waiting games with the head on the declarers in `seats`, the Bot's own elsewhere:
        exchange_values, then env.exchange.  Returns the first observation."""
        choice, discards = self.env.exchange_values(self.weights(), seats=seats, seats_per_game=seats_per_game)
        return self.env.exchange(choice, discards)
