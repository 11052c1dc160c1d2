"""The bidding head's learner: a network that values every bid from the twelve cards of a hand.

The teacher is TarokVecEnv.playout_bids (tarok_playout_bids): 52-76 determinized playout sets per game, too slow for a
self-play loop.  The head is a PolicyNet — the policy's 256 -> 256 -> 256 -> 64 network, so the rollout side is
tarok_bid_values, the policy's own MFMA forward — whose outputs 0..18 regress on the teacher's mean score per row, in
units of `reward_scale` points (1 / 70, as the policy's returns).  TarokVecEnv.bid_values then writes the array
TarokVecEnv.bid_round reads, in the teacher's place.

The update is plain torch autograd with Adam on purpose: an iteration is dominated by the teacher's launch, not by a
regression on 4 rows per game, and everything but collect() / round() runs on CPU tensors as well (BidLearner(None)).
"""
import torch
import torch.nn.functional as F

from . import karte as K
from . import playout as P
from .env import TarokVecEnv
from .selfplay import PolicyNet

BID_OPTIONS = K.BID_ROWS - 1          # rows 0..18 are options, row 19 is padding


def row_mask(contracts, device=None):
    """[BID_OPTIONS] bool: the rows whose contract's bit is set in `contracts` (karte.bid_row_option)."""
    return torch.tensor([bool((int(contracts) >> K.bid_row_option(r)[0]) & 1) for r in range(BID_OPTIONS)], dtype=torch.bool,
                        device=device)


def bid_loss(out, sums, playouts, reward_scale, contracts, pass_value=False):
    """The head's loss from network outputs `out` [M, >= 19] and the teacher's sums [M, K.BID_ROWS] (int): target =
    sums / playouts * reward_scale, Huber loss (delta 1) over the rows whose contract is in `contracts`, averaged over
    those entries.  The other columns enter neither the value nor the gradient.
    pass_value=True (out [M, >= 20], sums from playout_bids(pass_value=True)): row K.BID_PASS_ROW joins those rows — output
    19 regresses on the value of a pass, same target, same loss.
    playouts: a number, or a halving launch's counts [M, K.BID_ROWS] — a row's target is then its sum over its own count, and
    a row with count 0 is not a target."""
    if torch.is_tensor(playouts):
        width = K.BID_ROWS if pass_value else BID_OPTIONS
        rows = torch.cat([row_mask(contracts, out.device), torch.ones(1, dtype=torch.bool, device=out.device)])[:width]
        count = playouts[:, :width]
        on = rows.unsqueeze(0) & (count > 0)
        target = sums[:, :width].to(torch.float32) * float(reward_scale) / count.clamp(min=1).to(torch.float32)
        return F.huber_loss(out[:, :width].float()[on], target[on], reduction="mean", delta=1.0)
    if not pass_value:
        rows = row_mask(contracts, out.device)
        target = sums[:, :BID_OPTIONS].to(torch.float32) * (float(reward_scale) / float(playouts))
        return F.huber_loss(out[:, :BID_OPTIONS].float()[:, rows], target[:, rows], reduction="mean", delta=1.0)
    rows = torch.cat([row_mask(contracts, out.device), torch.ones(1, dtype=torch.bool, device=out.device)])
    target = sums[:, :K.BID_ROWS].to(torch.float32) * (float(reward_scale) / float(playouts))
    return F.huber_loss(out[:, :K.BID_ROWS].float()[:, rows], target[:, rows], reduction="mean", delta=1.0)


def pack_weights(net):
    """A PolicyNet as tarok_bid_values / tarok_policy_mlp read it: (w1, b1, w2, b2, w3, b3), the weights bf16 in MFMA
    fragment order (TarokVecEnv.mfma_weight_order), the biases float32 — SelfPlay.snapshot()'s shape."""
    with torch.no_grad():
        order = TarokVecEnv.mfma_weight_order
        f = lambda b: b.detach().to(torch.float32).contiguous().clone()
        return (order(net.fc1.weight), f(net.fc1.bias), order(net.fc2.weight), f(net.fc2.bias), order(net.head.weight), f(net.head.bias))


class BidLearner:
    """Regresses a PolicyNet on the playout teacher's bid values.

    env: a TarokVecEnv (never reset by the learner: both launches come before reset()), or None for a learner on the
    CPU that is fed batches by hand (loss / step).  worlds, samples: the teacher's launch (playout_bids).  worlds=None: 8, or with
    net_halving= the schedule's sum.  contracts: the
    rows learned and bid.  playouts_equiv: the `playouts` bid_round() is told for the head's values, which are scaled to
    sums over that many playouts, so `threshold` stays in points per game as for the teacher.  pass_value=True: the teacher
    also values a pass (playout_bids(pass_value=True)), output 19 regresses on it, and round() holds every bid against the
    seat's own pass (bid_values / bid_round with pass_value=True; `threshold` is then the margin over the pass).  net: six
    tensors (policy_mlp's weights, read live at every collect()) — the teacher is then playout_bids_net at `worlds` with the
    network's greedy card on the seats of net_seats inside the playouts, playouts = worlds; `samples` must be 1 or left
    unset.  net_depth: None, or 1..13 — the teacher is playout_bids_net_value, whose playouts stop at the viewer's
    net_depth-th decision and read the value head of `net` there at net_value_scale points per unit (13 never stops).
    pass_value=True goes with net= only together with net_depth: the value launch plays the pass item too, and output 19
    regresses on its row 19; the plain net launch does not value the pass.  net_list=True (with net=): the one teacher
    launch is playout_bids_net_list, the same numbers from a compacted item list; it values the pass at any depth, so
    pass_value=True then needs no net_depth.  Nothing else changes.
    net_halving: a tuple of 1..4 positive world counts (with net=): the teacher is playout_bids_net_halving, which spends
    later rounds' worlds on a viewer's leading rows only; it names the worlds itself (`worlds` None or their sum), goes with
    net_depth and with pass_value at any depth, and collect() then returns the counts [N,4,20] in the place of the scalar
    playouts."""

    def __init__(self, env, worlds=None, samples=None, contracts=K.BID_DEFAULT_CONTRACTS, lr=1e-3, reward_scale=1.0 / 70.0,
                 playouts_equiv=16, seed=0, pass_value=False, net=None, net_seats=15, net_halving=None, net_list=False, net_depth=None,
                 net_value_scale=70.0):
        self.net_halving = P.check_front_halving(net_halving, net, net_list, worlds, samples)
        worlds = (8 if worlds is None else worlds) if self.net_halving is None else sum(self.net_halving)
        if net_list and net is None:
            raise ValueError("net_list packs the network's playouts: it needs net=")
        if net_depth is not None:
            if net is None:
                raise ValueError("net_depth stops the network's playouts: it needs net=")
            P.check_depth(net_depth, net_value_scale, P.spelling(), max_depth=K.PLAYOUT_FRONT_MAX_DEPTH)
        if net is not None:
            if pass_value and net_depth is None and not net_list and self.net_halving is None:
                raise ValueError("net= without net_depth does not value the pass: pass_value=True goes with the Bot's playouts "
                                 "or with net_depth")
            if samples not in (None, 1):
                raise ValueError("net= runs one playout per (option, world): samples must be 1 or unset")
            if not (isinstance(net_seats, int) and 0 <= net_seats <= 15):
                raise ValueError("net_seats: a 4-bit seat set, 0..15")
            net = TarokVecEnv.check_mlp_weights(net)
        samples = (1 if net is not None else 2) if samples is None else samples
        self.net_weights, self.net_seats = net, int(net_seats)
        self.net_depth, self.net_value_scale = net_depth, float(net_value_scale)
        self.net_list = bool(net_list)
        if not 1 <= int(contracts) <= K.BID_ALL_CONTRACTS:
            raise ValueError("contracts: a bit set within 1..0x3FF")
        if not (reward_scale > 0 and int(playouts_equiv) >= 1):
            raise ValueError("reward_scale > 0 and playouts_equiv >= 1")
        self.env = env
        self.device = env.device if env is not None else torch.device("cpu")
        self.worlds, self.samples, self.contracts = int(worlds), int(samples), int(contracts)
        self.reward_scale, self.playouts_equiv = float(reward_scale), int(playouts_equiv)
        self.pass_value = bool(pass_value)
        self.scale = self.playouts_equiv / self.reward_scale        # tarok_bid_values' scale: outputs -> sums over playouts_equiv
        if not self.scale <= 2.0 ** 20:
            raise ValueError("playouts_equiv / reward_scale exceeds tarok_bid_values' largest scale, 2**20")
        with torch.random.fork_rng(devices=[]):       # the initial weights are a function of `seed` alone
            torch.manual_seed(int(seed))
            self.net = PolicyNet(256)
        self.net.to(self.device)
        self.opt = torch.optim.Adam(self.net.parameters(), lr=float(lr))
        self.episode = 0
        self.salt = int(seed)

    # ---- the regression (any device)
    def outputs(self, feature_words):
        """The module's float outputs [M, 64] on feature words [M, 4] int64 (bid_values(feature_words=True) rows)."""
        x = TarokVecEnv.expand_feature_words(feature_words.reshape(-1, 4), torch.float32)
        return self.net.forward_raw(x)

    def loss(self, feature_words, sums, playouts):
        """bid_loss of the network on feature words [..., 4] and the teacher's sums [..., K.BID_ROWS] at `playouts`."""
        if torch.is_tensor(playouts):
            playouts = playouts.reshape(-1, K.BID_ROWS)
        return bid_loss(self.outputs(feature_words), sums.reshape(-1, K.BID_ROWS), playouts, self.reward_scale, self.contracts,
                        pass_value=self.pass_value)

    def step(self, feature_words, sums, playouts):
        """One Adam step on one batch; returns the loss before the step (a float)."""
        self.opt.zero_grad(set_to_none=True)
        loss = self.loss(feature_words, sums, playouts)
        loss.backward()
        self.opt.step()
        return float(loss.detach())

    # ---- the launches (need the env)
    @torch.no_grad()
    def weights(self):
        return pack_weights(self.net)

    @torch.no_grad()
    def collect(self, episode):
        """(feature_words [N,4,4] int64, sums [N,4,K.BID_ROWS] int32, playouts) of episode `episode`: the teacher's launch
        on every seat and the head's launch for its input rows."""
        counts = None
        if self.net_halving is not None:
            sums, counts, _ = P.front_halving_launch(self.env, True)(self.net_weights, episode, self.net_halving, self.net_depth,
                                                                     self.net_value_scale, pass_value=self.pass_value,
                                                                     net_seats=self.net_seats, contracts=self.contracts, salt=self.salt)
        elif self.net_list or self.net_weights is not None:
            launch = P.bids_net_launch(self.env, self.net_list, True)
            sums = launch(self.net_weights, episode, self.worlds, self.net_depth, self.net_value_scale, pass_value=self.pass_value,
                          net_seats=self.net_seats, contracts=self.contracts, salt=self.salt)
        else:
            sums = self.env.playout_bids(episode, self.worlds, self.samples, contracts=self.contracts, salt=self.salt,
                                         pass_value=self.pass_value)
        _, _, fw = self.env.bid_values(episode, self.weights(), self.scale, contracts=self.contracts, feature_words=True)
        return fw, sums, self.worlds * self.samples if counts is None else counts

    def iterate(self):
        """collect() on a fresh episode and one step(); returns the loss before the step."""
        fw, sums, playouts = self.collect(self.episode)
        self.episode += 1
        return self.step(fw, sums, playouts)

    @torch.no_grad()
    def round(self, episode, seats=15, threshold=0, deals=None, seats_per_game=None):
        """The bidding round with the head on `seats`: (contract, declarer, king_suit) as reset() takes them."""
        values = self.env.bid_values(episode, self.weights(), self.scale, contracts=self.contracts, deals=deals, seats=seats,
                                     seats_per_game=seats_per_game, pass_value=self.pass_value)
        return self.env.bid_round(episode, values, self.playouts_equiv, threshold=threshold, contracts=self.contracts, seats=seats,
                                  seats_per_game=seats_per_game, pass_value=self.pass_value)
