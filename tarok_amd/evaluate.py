"""How well does a policy play?  Duplicate evaluation of the learned policy against the Bot (evaluate_vs_bot) or
against a second network, such as an earlier checkpoint (evaluate_vs_policy: read "the Bot" below as that network).

The same deals are played five times: once with the Bot (Bot_igralec, Igralec.py:148-171: a uniformly random legal
card) on all four seats, and once with the network on each single seat and the Bot on the other three
(tarok_policy_step_seats).  Deals, contracts and the Bot's draws are functions of (seed, game index, episode, cards
played) alone, so the five tables of a deal differ only through the cards the network chose, and the score the
network's seat made is compared with the score the Bot made on that very seat of that very deal:

    advantage = mean over deals d and seats k of  score(network on k)[d, k] - score(Bot everywhere)[d, k]

in game points per game.  The four differences of a deal share its cards, so the standard error is taken over deals:
stderr = std over d of (mean over k of the difference) / sqrt(deals).
"""
import numpy as np
import torch

from . import karte as K
from . import playout
from .env import TarokVecEnv

PASS_SEATS = (0, 1, 2, 4, 8)      # the seat set of pass p: Bot everywhere, then the network on seat p - 1 alone
GAME_CARDS = 48


def duplicate_advantage(scores):
    """scores [5, D, 4] (numpy array or torch tensor): the final scores by seat of deal d in pass p — pass 0 the Bot on
    every seat, pass 1 + k the network on seat k only.  Returns a dict:
      policy_mean  mean over d, k of scores[1 + k, d, k]     bot_mean  the same entries of pass 0
      advantage    mean of the paired differences            by_seat   [4] the same per seat k
      stderr       sample standard deviation (n - 1) over deals of each deal's mean-over-k difference, divided by
                   sqrt(D); nan for a single deal
      deals        D"""
    if torch.is_tensor(scores):
        scores = scores.detach().cpu().numpy()
    s = np.asarray(scores, dtype=np.float64)
    if s.ndim != 3 or s.shape[0] != 5 or s.shape[2] != 4 or s.shape[1] < 1:
        raise ValueError("scores must be [5, deals, 4], got %s" % (s.shape,))
    k = np.arange(4)
    own = s[1 + k, :, k].T                    # [D, 4]: the network's seat in its pass
    bot = s[0][:, k]                          # [D, 4]: that seat with the Bot on it
    diff = own - bot
    deals = s.shape[1]
    per_deal = diff.mean(axis=1)
    stderr = float(per_deal.std(ddof=1) / np.sqrt(deals)) if deals > 1 else float("nan")
    return dict(policy_mean=float(own.mean()), bot_mean=float(bot.mean()), advantage=float(diff.mean()), stderr=stderr,
                by_seat=[float(x) for x in diff.mean(axis=0)], deals=int(deals))


def _empty(env, shape, dtype):
    with torch.cuda.device(env.device):
        return torch.empty(shape, dtype=dtype, device=env.device)


def _passes(n_games, episodes, front, cards, inspect=None, **env_args):
    """The duplicate-pass driver under every evaluate_* call: the five passes (PASS_SEATS) of every episode on an env of
    its own, made with env_args (device, seed, mix, history); returns scores [5, episodes * n_games, 4] i32.
    front, cards: who decides what, as makers that are called once with the env, before the first pass, where they
    allocate their buffers.  They return
      the front end    (env, episode, seats) -> (start, extras): the pass's reset and what goes before and after it (_front),
      the card player  (env, t, seats, action_row): lock-step t's launches — they leave a card per game in action_row [N] u8
                       and play it, without auto-reset (a finished game ignores its card; a Berac may end early).
    Per pass: the front end, 48 lock-steps, then ONE host synchronisation to read the slots' score sums.
    inspect (tests): a list that receives one dict per pass — episode, seats, start (the canonical lanes after the
    reset), actions [48, N] u8 and scores [N, 4] host arrays, and the front end's extras as host arrays — at the price of
    a second synchronisation per pass."""
    n = int(n_games)
    scores = np.zeros((len(PASS_SEATS), int(episodes) * n, 4), np.int32)
    env = TarokVecEnv(n, **env_args)
    try:
        actions = _empty(env, (GAME_CARDS, n), torch.uint8)
        front, cards = front(env), cards(env)
        for e in range(int(episodes)):
            for p, seats in enumerate(PASS_SEATS):
                start, extras = front(env, e, seats)
                for t in range(GAME_CARDS):
                    cards(env, t, seats, actions[t])
                _, ss = env.counters()                # (the pass's one synchronisation)
                scores[p, e * n:(e + 1) * n] = ss
                if inspect is not None:
                    inspect.append(dict(episode=e, seats=seats, start=start, actions=actions.cpu().numpy(), scores=ss.copy(),
                                        **{k: v.cpu().numpy() for k, v in extras.items()}))
    finally:
        env.close()
    return scores


def _front(want_start, bid=None, exchange=None):
    """The front end of a pass: the bid, if a maker of one is given (_bid_front, _bidnet_front), then the reset, which takes
    the bid's contract, declarer and king — with the exchange deferred if a maker of one is given (_exchange_front,
    _exchangenet_front), which then follows.  None: the mix's own contracts, the reset's own Bot exchange.
    want_start: read the canonical lanes right after the reset — BEFORE a deferred exchange (a synchronisation)."""
    def make(env):
        bid_, exchange_ = bid and bid(env), exchange and exchange(env)        # (None stays None)

        def front(env, episode, seats):
            setup, extras = bid_(env, episode, seats) if bid_ else ({}, {})
            env.reset(episode=episode, clear_counters=True, **setup, **({"defer_exchange": True} if exchange_ else {}))
            start = env.state() if want_start else None
            return start, dict(extras, **exchange_(env, seats)) if exchange_ else extras
        return front
    return make


def _bid_front(bidding, salt, threshold, contracts, pass_value=False):
    """The bid of a pass whose playout player bids: ONE tarok_playout_bids at bidding = (worlds, samples) with the pass's
    seat set, ONE tarok_bid_round — the Bot's own answers outside the set, so the empty set gives K.MIX_BOT's contract,
    declarer and king.  Returns them twice: as the keyword arguments reset() takes them as, and for `inspect`.  pass_value:
    both launches' _pass twins (the pass valued by playouts; `threshold` the margin over it)."""
    worlds, samples = bidding

    def make(env):
        sums = _empty(env, (env.n, 4, K.BID_ROWS), torch.int32)

        def bid(env, episode, seats):
            env.playout_bids(episode, worlds, samples, contracts=contracts, salt=salt, seats=seats, sum_out=sums, pass_value=pass_value)
            c, d, k = env.bid_round(episode, sums, int(worlds) * int(samples), threshold=threshold, contracts=contracts, seats=seats,
                                    pass_value=pass_value)
            setup = dict(contract=c, declarer=d, king_suit=k)
            return setup, setup
        return bid
    return make


def _net_front_args(net, net_seats, samples, what, net_depth=None, net_value_scale=70.0):
    """The checks of a front end whose playouts the network plays: net's six tensors, and the seat set to hand the launch
    for a pass (a function of the pass's seats: "own" is the pass's own set).  net_depth: None, or the front launches'
    1..13 with a finite net_value_scale > 0."""
    if net_depth is not None:
        playout.check_depth(net_depth, net_value_scale, playout.spelling(), max_depth=K.PLAYOUT_FRONT_MAX_DEPTH)
    if samples not in (None, 1):
        raise ValueError("net= runs one playout per (%s, world): samples must be None or 1" % what)
    if net_seats != "own" and not (isinstance(net_seats, int) and 0 <= net_seats <= 15):
        raise ValueError('net_seats: a 4-bit seat set, 0..15, or "own"')
    return TarokVecEnv.check_mlp_weights(net), (lambda seats: seats if net_seats == "own" else net_seats)


def _bid_net_front(net, net_seats, worlds, salt, threshold, contracts, net_depth=None, net_value_scale=70.0, pass_value=False,
                   net_list=False, net_halving=None):
    """_bid_front whose playouts the network plays: ONE tarok_playout_bids_net at `worlds` with the pass's seat set —
    net_seats inside the playouts, or the pass's own set for "own" — and ONE tarok_bid_round at playouts = worlds.
    net_depth: tarok_playout_bids_net_value in its place; pass_value (with net_depth only): its pass item, and
    tarok_bid_round_pass with `threshold` the margin over the pass, as for the Bot teacher.  net_list: the same arguments
    to tarok_playout_bids_net_list in either launch's place.  net_halving: ONE tarok_playout_bids_net_halving at that schedule
    in the launch's place, whose value_out is the round's sums at playouts = W, the schedule's sum."""
    def make(env):
        sums = _empty(env, (env.n, 4, K.BID_ROWS), torch.int32)
        raw, counts = ((_empty(env, (env.n, 4, K.BID_ROWS), torch.int32) for _ in range(2)) if net_halving is not None else (None, None))

        def bid(env, episode, seats):
            if net_halving is not None:                  # (sums holds value_out: what the round reads)
                playout.front_halving_launch(env, True)(
                    net, episode, net_halving, net_depth, net_value_scale, pass_value=pass_value, net_seats=net_seats(seats), contracts=contracts,
                    salt=salt, seats=seats, sum_out=raw, count_out=counts, value_out=sums)
                c, d, k = env.bid_round(episode, sums, sum(net_halving), threshold=threshold, contracts=contracts, seats=seats,
                                        pass_value=pass_value)
            elif net_depth is None:
                playout.bids_net_launch(env, net_list, False)(net, episode, worlds, net_seats=net_seats(seats), contracts=contracts, salt=salt, seats=seats, sum_out=sums)
                c, d, k = env.bid_round(episode, sums, int(worlds), threshold=threshold, contracts=contracts, seats=seats)
            else:
                playout.bids_net_launch(env, net_list, True)(
                    net, episode, worlds, net_depth, net_value_scale, pass_value=pass_value, net_seats=net_seats(seats), contracts=contracts,
                    salt=salt, seats=seats, sum_out=sums)
                c, d, k = env.bid_round(episode, sums, int(worlds), threshold=threshold, contracts=contracts, seats=seats,
                                        pass_value=pass_value)
            setup = dict(contract=c, declarer=d, king_suit=k)
            return setup, dict(setup, sums=sums)
        return bid
    return make


def _bidnet_front(weights, playouts_equiv, reward_scale, threshold, contracts, pass_value=False):
    """_bid_front with the bidding head in the playout teacher's place: ONE tarok_bid_values at scale = playouts_equiv /
    reward_scale with the pass's seat set and ONE tarok_bid_round at playouts = playouts_equiv; `inspect` also gets
    values [N,4,K.BID_ROWS] i32."""
    scale = float(int(playouts_equiv) / float(reward_scale))

    def make(env):
        values = _empty(env, (env.n, 4, K.BID_ROWS), torch.int32)

        def bid(env, episode, seats):
            env.bid_values(episode, weights, scale, contracts=contracts, seats=seats, value_out=values, pass_value=pass_value)
            c, d, k = env.bid_round(episode, values, int(playouts_equiv), threshold=threshold, contracts=contracts, seats=seats,
                                    pass_value=pass_value)
            setup = dict(contract=c, declarer=d, king_suit=k)
            return setup, dict(setup, values=values)
        return bid
    return make


def _exchange_front(worlds, samples, discard_sets, salt):
    """The talon exchange of a pass whose playout player makes it, after a reset that deferred it: ONE
    tarok_playout_exchange with the pass's seat set — its rows are the Bot's own exchange for a declarer outside the set —
    and one tarok_exchange that applies them.  Returns choice [N] i8 and discards [N,3] u8, for `inspect`."""
    def make(env):
        sums = _empty(env, (env.n, 6 * int(discard_sets), 4), torch.int32)
        chosen = dict(choice=_empty(env, env.n, torch.int8), discards=_empty(env, (env.n, 3), torch.uint8))

        def exchange(env, seats):
            env.playout_exchange(worlds, samples, discard_sets, salt=salt, seats=seats, sum_out=sums, choice_out=chosen["choice"],
                                 discards_out=chosen["discards"])
            env.exchange(chosen["choice"], chosen["discards"])
            return chosen
        return exchange
    return make


def _exchange_net_front(net, net_seats, worlds, discard_sets, salt, net_depth=None, net_value_scale=70.0, net_list=False,
                        net_halving=None):
    """_exchange_front whose playouts the network plays: ONE tarok_playout_exchange_net at (worlds, discard_sets) with the
    pass's seat set — net_seats inside the playouts, or the pass's own set for "own" — and one tarok_exchange.  net_depth:
    tarok_playout_exchange_net_value in its place.  net_list: the same arguments to tarok_playout_exchange_net_list in either
    launch's place.  net_halving: ONE tarok_playout_exchange_net_halving at that schedule in the launch's place; its choice
    and discards go to tarok_exchange."""
    def make(env):
        sums = _empty(env, (env.n, 6 * int(discard_sets), 4), torch.int32)
        chosen = dict(choice=_empty(env, env.n, torch.int8), discards=_empty(env, (env.n, 3), torch.uint8))
        counts = _empty(env, (env.n, 6 * int(discard_sets)), torch.int32) if net_halving is not None else None

        def exchange(env, seats):
            if net_halving is not None:
                playout.front_halving_launch(env, False)(
                    net, net_halving, discard_sets, net_depth, net_value_scale, net_seats=net_seats(seats), salt=salt, seats=seats, sum_out=sums,
                    count_out=counts, choice_out=chosen["choice"], discards_out=chosen["discards"])
            elif net_depth is None:
                playout.exchange_net_launch(env, net_list, False)(
                    net, worlds, discard_sets, net_seats=net_seats(seats), salt=salt, seats=seats, sum_out=sums, choice_out=chosen["choice"],
                    discards_out=chosen["discards"])
            else:
                playout.exchange_net_launch(env, net_list, True)(
                    net, worlds, discard_sets, net_depth, net_value_scale, net_seats=net_seats(seats), salt=salt, seats=seats, sum_out=sums,
                    choice_out=chosen["choice"], discards_out=chosen["discards"])
            env.exchange(chosen["choice"], chosen["discards"])
            return dict(chosen, sums=sums)
        return exchange
    return make


def _exchangenet_front(weights):
    """_exchange_front with the exchange head in the playout teacher's place: ONE tarok_exchange_values with the pass's
    seat set and one tarok_exchange."""
    def make(env):
        chosen = dict(choice=_empty(env, env.n, torch.int8), discards=_empty(env, (env.n, 3), torch.uint8))

        def exchange(env, seats):
            env.exchange_values(weights, seats=seats, choice_out=chosen["choice"], discards_out=chosen["discards"])
            env.exchange(chosen["choice"], chosen["discards"])
            return chosen
        return exchange
    return make


def _network_cards(weights, opponent, temperature, epsilon):
    """The card player of the network: the play mode, set once, and one tarok_policy_step_seats (_versus with an
    `opponent`) per lock-step."""
    def make(env):
        env.set_play_mode(temperature, epsilon)
        # the observation words go back and forth between the env's own buffer (reset() leaves the first ones there)
        # and a second one: the step's input and output may not alias
        words = [env.obs_words, _empty(env, env.n, torch.int64)]

        def cards(env, t, seats, row):
            env.policy_step(weights, words[t & 1], words[(t + 1) & 1], row, auto_reset=False, seats=seats, opponent=opponent)
        return cards
    return make


def _playout_cards(launch, words_dtype=None, counts=False):
    """A card player of two launches per lock-step: launch(env, seats, words, sums, row) — a playout launch that leaves
    its player's card on the pass's seats and the Bot's on the others in `row` — and one tarok_step that plays it.
    sums [N, K.PLAYOUT_RANKS, 4] i32 is the launch's sum_out; words [N], if a dtype is given, its history words; counts:
    the launch also takes count_out=[N, K.PLAYOUT_RANKS] i32 (a halving launch)."""
    def make(env):
        sums = _empty(env, (env.n, K.PLAYOUT_RANKS, 4), torch.int32)
        words = _empty(env, env.n, words_dtype) if words_dtype is not None else None
        more = dict(count_out=_empty(env, (env.n, K.PLAYOUT_RANKS), torch.int32)) if counts else {}

        def cards(env, t, seats, row):
            launch(env, seats, words, sums, row, **more)
            env.step(row, auto_reset=False)
        return cards
    return make


# the Bot's card on every seat: tarok_playout_cards with the empty seat set — no playout is run
_bot_cards = _playout_cards(lambda env, seats, words, sums, row: env.playout_cards(1, seats=0, sum_out=sums, action_out=row))


def _play_passes(weights, n_games, episodes, seed, mix, device, inspect=None, opponent=None):
    """_play_passes_mode at the play mode (1, 0): every network card one draw from its softmax."""
    return _play_passes_mode(weights, n_games, episodes, seed, mix, device, inspect=inspect, opponent=opponent)


def _play_passes_mode(weights, n_games, episodes, seed, mix, device, inspect=None, opponent=None, temperature=1.0, epsilon=0.0):
    """The five passes of every episode on an env of its own; returns scores [5, episodes * n_games, 4] i32.
    opponent: six tensors like `weights`, the network that takes the Bot's place on every seat outside the pass's set
    (tarok_policy_step_versus; None: the Bot, tarok_policy_step_seats).
    temperature, epsilon: the play mode of the env (TarokVecEnv.set_play_mode) — of every network seat, `opponent`'s
    too; the Bot's seats, hence the whole of evaluate_vs_bot's pass 0, do not depend on it.
    inspect (tests): a list that receives one dict per pass — episode, seats, start (the canonical lanes after the
    reset), actions [48, N] u8 and scores [N, 4] host arrays — at the price of a second synchronisation per pass."""
    return _passes(n_games, episodes, _front(inspect is not None), _network_cards(weights, opponent, temperature, epsilon), inspect,
                   device=device, seed=seed, mix=mix)


def evaluate_vs_bot(weights, n_games, episodes, seed=0, mix=K.MIX_BOT, device=0, temperature=1.0, epsilon=0.0):
    """Duplicate evaluation of `weights` (w1, b1, w2, b2, w3, b3 as tarok_policy_step takes them, on `device`)
    over n_games * episodes deals; returns duplicate_advantage's dict.  Deal e * n_games + i is game i of episode e
    of an env with this seed and game offset 0: the same arguments always play the same deals.

    Runs on an env of its own (a training env, its state and its captured graph are never touched).  Per episode and
    pass: reset with the score counters cleared, 48 one-card launches without auto-reset (a finished game ignores its
    card; a Berac may end early), then ONE host synchronisation to read the slots' score sums.

    temperature, epsilon: how the network's card is chosen (TarokVecEnv.set_play_mode, on the evaluation's own env).  The
    default (1, 0) samples the softmax, so the figure is that of the policy plus its sampling noise; temperature=0 plays
    the network's best card — the arg-max of Igralec.igraj_karto — and epsilon its random_card.  The Bot-everywhere pass
    is the same whatever the mode."""
    return duplicate_advantage(_play_passes_mode(weights, n_games, episodes, seed, mix, device, temperature=temperature,
                                                 epsilon=epsilon))


def evaluate_vs_policy(weights, opponent, n_games, episodes, seed=0, mix=K.MIX_BOT, device=0, temperature=1.0, epsilon=0.0):
    """Duplicate evaluation of `weights` against a second network, `opponent` (both as tarok_policy_step takes them, on
    `device`): evaluate_vs_bot with `opponent` in the Bot's place, one tarok_policy_step_versus launch per lock-step.
    Pass 0 plays `opponent` on all four seats, pass 1 + k `weights` on seat k alone and `opponent` on the other three,
    on the deals evaluate_vs_bot plays with the same arguments.  Returns duplicate_advantage's dict, unchanged:
    `bot_mean` is then the mean of the BASELINE policy (`opponent` on the seat in pass 0), `policy_mean` that of
    `weights`, and `advantage` is points per game of `weights` over `opponent` — exactly 0.0 for a network against
    itself, since a network's card on a position does not depend on who else sits at the table.
    temperature, epsilon: the play mode of BOTH networks (evaluate_vs_bot); a network against itself stays at 0.0 in
    every mode, the coin and the Bot's card being functions of the position too."""
    for name, ws in (("weights", weights), ("opponent", opponent)):
        if not isinstance(ws, (tuple, list)) or len(ws) != 6 or not all(torch.is_tensor(t) for t in ws):
            raise ValueError("%s: six tensors (w1, b1, w2, b2, w3, b3)" % name)
        TarokVecEnv.check_mlp_weights(ws)
    return duplicate_advantage(_play_passes_mode(weights, n_games, episodes, seed, mix, device, opponent=opponent,
                                                 temperature=temperature, epsilon=epsilon))


def _pool_cards(weights, pool, groups_per_block, temperature, epsilon):
    """_network_cards against a pool: one tarok_policy_step_pool per lock-step, the six stacked tensors `pool` in the
    opponent's place; step group g plays entry g // groups_per_block."""
    def make(env):
        env.set_play_mode(temperature, epsilon)
        words = [env.obs_words, _empty(env, env.n, torch.int64)]
        with torch.cuda.device(env.device):
            group_net = (torch.arange((env.n + 255) // 256, device=env.device) // groups_per_block).to(torch.uint8)

        def cards(env, t, seats, row):
            env.policy_step(weights, words[t & 1], words[(t + 1) & 1], row, auto_reset=False, seats=seats, opponent_pool=pool,
                            group_net=group_net)
        return cards
    return make


def pool_block_scores(scores, k, n_games, pool_size):
    """Block k's part of the scores of a pool evaluation ([5, episodes * pool_size * G, 4], G = n_games rounded up to a
    multiple of 256: episode-major, then slot): the first n_games slots of block k = slots [k G, (k + 1) G) of every
    episode, as [5, episodes * n_games, 4] in evaluate_vs_policy's order of deals."""
    n = int(n_games)
    G = -(-n // 256) * 256
    s = np.asarray(scores)
    return s.reshape(5, -1, int(pool_size), G, 4)[:, :, int(k), :n].reshape(5, -1, 4)


def evaluate_vs_pool(weights, pool, n_games, episodes, seed=0, mix=K.MIX_BOT, device=0, temperature=1.0, epsilon=0.0, inspect=None):
    """evaluate_vs_policy against every network of `pool` (a list of 1..64 weight sets) at once: ONE env of
    len(pool) * G slots, G = n_games rounded up to a multiple of 256 (whole step groups), block k = slots [k G, (k + 1) G)
    playing `weights` against pool[k] through tarok_policy_step_pool — one launch per lock-step for the whole pool, on
    the same five duplicate passes.  Returns a list of duplicate_advantage dicts, dict k from the first n_games slots of
    block k only (pool_block_scores).  Block k's deals are games k G .. of the seed: block 0's are evaluate_vs_policy's
    with the same arguments, so a pool of one returns that call's dict; the other blocks play deals of their own.
    temperature, epsilon: the play mode of every network.  inspect (tests): as in _play_passes_mode, over all slots."""
    if not isinstance(weights, (tuple, list)) or len(weights) != 6 or not all(torch.is_tensor(t) for t in weights):
        raise ValueError("weights: six tensors (w1, b1, w2, b2, w3, b3)")
    weights = TarokVecEnv.check_mlp_weights(weights)
    if not isinstance(pool, (tuple, list)) or not 1 <= len(pool) <= K.POOL_MAX:
        raise ValueError("pool: a list of 1..%d weight sets" % K.POOL_MAX)
    stacked = TarokVecEnv.stack_pool(pool)
    k, n = len(pool), int(n_games)
    G = -(-n // 256) * 256
    scores = _passes(k * G, episodes, _front(inspect is not None), _pool_cards(weights, stacked, G // 256, temperature, epsilon),
                     inspect, device=device, seed=seed, mix=mix)
    return [duplicate_advantage(pool_block_scores(scores, j, n, k)) for j in range(k)]


def _bid_args(bidding, mix):
    if bidding is None:
        return None
    if mix != K.MIX_BOT:
        raise ValueError("bidding=(worlds, samples) replaces the Bot's bidding round: it goes with mix=K.MIX_BOT")
    worlds, samples = bidding
    return int(worlds), int(samples)


def _playout_passes(samples, n_games, episodes, seed, mix, device, salt=0, inspect=None, worlds=None, voids=False, exchange=None,
                    hidden=False, bidding=None, threshold=0, contracts=K.BID_DEFAULT_CONTRACTS, pass_value=False, net=None,
                    net_seats=15, net_worlds="det", net_depth=None, net_value_scale=70.0, halving=None, net_halving=None, net_versus=None,
                    net_opponent=None, net_sampled=None):
    """_play_passes_mode with the Monte-Carlo player (TarokVecEnv.playout_cards) in the network's place: per lock-step
    one playout launch with the pass's seat set — tarok_playout_cards (open hands) for worlds=None,
    tarok_playout_cards_det (the fair player: `worlds` re-deals of the unseen cards) otherwise — whose action_out holds
    the playout player's card on its seats and the Bot's on the others, and one tarok_step that plays it.
    voids=True (with worlds): the env keeps the play history and every lock-step runs tarok_shown_voids and
    tarok_playout_cards_voids in tarok_playout_cards_det's place.
    hidden=True (with worlds, not with voids): the env keeps the play history and every lock-step runs tarok_played_cards
    and tarok_playout_cards_hidden in tarok_playout_cards_det's place.
    exchange=D (with worlds): every pass starts with _exchange_front at (worlds, samples, D) — the playout player makes
    its seat's talon exchange too; the inspected dicts then also hold choice [N] i8 and discards [N,3] u8, and `start`
    is the state BEFORE the exchange.  None: the reset's own Bot exchange, the code path as it was.
    bidding=(W, S) (with worlds): every pass starts with _bid_front at (W, S) — the playout player bids for its seat too;
    the inspected dicts then also hold contract, declarer and king_suit [N] i8.  None: the mix's own contracts.
    net=weights (with worlds, with nothing else): every lock-step runs tarok_playout_cards_net at `worlds` — the playouts
    are played by the network's greedy card on the seats of net_seats (a 4-bit set, or "own": the pass's seat set) and by
    the Bot elsewhere; `samples` is not taken.
    net_worlds="voids" / "hidden" (with net): the env keeps the play history and every lock-step runs tarok_shown_voids and
    tarok_playout_cards_net_voids / tarok_played_cards and tarok_playout_cards_net_hidden instead; "det" is the launch
    above.  (voids=True / hidden=True together with net= keep raising: net_worlds is the way in.)
    net_depth=D (with net): the launch is playout_cards_net_value at depth D and net_value_scale in the same worlds — the
    playouts stop at the player's D-th next decision and take the value head's estimate; None: the calls as they were.
    halving=(w0, ..): the launch is tarok_playout_cards_halving with that schedule, in the worlds voids / hidden name.
    net_halving=(w0, ..) (with net): the launch is tarok_playout_cards_net_halving with that schedule, in the worlds of
    net_worlds and at net_depth.
    net_versus=(own_rel, opp_rel) (with net): the launch is playout_cards_net_versus — `net` on the relative seats of own_rel,
    net_opponent (six tensors; required where opp_rel is not 0) on those of opp_rel, relative to the player's seat in every
    game —, in the worlds of net_worlds, at net_depth and with net_halving's schedule where one is given.
    net_sampled=dict(samples=, temperature=, epsilon=, opp_temperature=, opp_epsilon=) (with net, or with net and net_versus): the
    launch is playout_cards_net_sampled — the networks play under those play modes, `samples` playouts per (card, world);
    with net alone on the roles (15, 0).
    inspect: as in _play_passes_mode."""
    player = playout.card_player(samples, worlds, voids, hidden, net is not None, net_seats, net_worlds, net_depth, net_value_scale, salt,
                                 front=exchange is not None or bidding is not None, halving=halving, net_halving=net_halving,
                                 net_versus=net_versus, net_sampled=net_sampled)
    if net_opponent is not None and net_versus is None:
        raise ValueError("net_opponent is the second network of net_versus=(own_rel, opp_rel): give that as well")
    if net_versus is not None and player.versus[1] and net_opponent is None:
        raise ValueError("net_versus seats an opponent's network on the seats of opp_rel: give net_opponent= (six tensors) as well")
    if net is not None:
        if samples is not None:
            raise ValueError("net= runs one playout per (card, world): samples is not taken (pass None)")
        net = TarokVecEnv.check_mlp_weights(net)
    if net_opponent is not None:
        net_opponent = TarokVecEnv.check_mlp_weights(net_opponent)
    if exchange is not None and worlds is None:
        raise ValueError("exchange=D is the fair player's front end: give worlds= as well")
    if bidding is not None and worlds is None:
        raise ValueError("bidding=(W, S) is the fair player's front end: give worlds= as well")
    bidding = _bid_args(bidding, mix)
    cards = _playout_cards(lambda env, seats, words, sums, row, **more: player.launch(env, (net, net_opponent), dict(seats=seats), words, sums, row, **more),
                           words_dtype=player.words_dtype, counts=player.counts)
    front = _front(inspect is not None, bid=None if bidding is None else _bid_front(bidding, salt, threshold, contracts, pass_value),
                   exchange=None if exchange is None else _exchange_front(worlds, samples, exchange, salt))
    return _passes(n_games, episodes, front, cards, inspect, device=device, seed=seed, mix=mix, history=player.needs_history)


def evaluate_playout_vs_bot(samples, n_games, episodes, seed=0, mix=K.MIX_BOT, device=0, salt=0, inspect=None, worlds=None,
                            voids=False, exchange=None, hidden=False, bidding=None, threshold=0,
                            contracts=K.BID_DEFAULT_CONTRACTS, pass_value=False, net=None, net_seats=15, net_worlds="det",
                            net_depth=None, net_value_scale=70.0, halving=None, net_halving=None, net_versus=None, net_opponent=None,
                            net_samples=None, net_temperature=None, net_epsilon=None, net_opp_temperature=None, net_opp_epsilon=None):
    """evaluate_vs_bot with the open-hand Monte-Carlo player in the network's place: a strong reference player that needs
    no training.  On its seat it plays, at every move, the legal card with the best summed score over `samples` Bot
    playouts of each legal card (tarok_playout_cards; `salt` varies their draws).  The playouts see the TRUE hidden
    hands — perfect information — so the figure is an upper-side yardstick for a policy's own evaluate_vs_bot figure on
    the same deals (same seed, mix and sizes), not the strength of a fair player.
    worlds=W is the FAIR player: determinized playouts (tarok_playout_cards_det), W re-deals of the cards its seat cannot
    see and `samples` playouts of every legal card in each.  It uses only what its seat may know, so it is the honest
    fixed opponent to hold a learned policy against and a teacher the network could in principle reach.
    voids=True (with worlds=W): the fair player also uses the voids the table has seen — its worlds give no seat a card
    of a class it has shown to be out of (tarok_shown_voids, tarok_playout_cards_voids; the env keeps the history).
    hidden=True (with worlds=W, not with voids=True): the fair player's worlds also re-deal what only other seats have
    seen — Klop's face-down talon and the declarer's discards (tarok_played_cards, tarok_playout_cards_hidden; the env
    keeps the history).  It composes with exchange=D, which runs before the first card.
    exchange=D (with worlds=W): the fair player makes BOTH of its seat's decisions — before the first card of a game it
    declared it picks the talon group and the discards by playouts over D discard sets per group
    (tarok_playout_exchange at (W, samples, D)); the other declarers exchange as the Bot does.  None (the default): every
    declarer exchanges as the Bot does, as before.
    bidding=(Wb, Sb) (with worlds=W and mix=K.MIX_BOT): the fair player also BIDS for its seat — tarok_playout_bids at
    (Wb, Sb) over `contracts` and tarok_bid_round with `threshold` decide contract, declarer and called king before the
    reset; the other seats bid as the Bot does, so pass 0 is unchanged.  It composes with exchange=D.  None (the default):
    the Bot's bidding round on every seat, as before.  pass_value=True (with bidding): the pass is valued by playouts too
    and is the bar a bid has to clear (tarok_playout_bids_pass, tarok_bid_round_pass; `threshold` the margin over it).
    net=weights (with worlds=W; `samples` must be None; with none of voids, hidden, exchange, bidding): the fair player
    whose playouts are played by a policy network (tarok_playout_cards_net) — weights = policy_mlp's six tensors.  Inside
    the playouts the seats of net_seats (a 4-bit set; 15, the default: every seat) play the network's greedy card, the
    others the Bot's; net_seats="own" makes the set the player's own seat, a best response to a table of Bots.
    net_worlds="voids" / "hidden" (with net=weights; "det", the default, is the call as it was): the network's playouts run
    in the void-aware worlds (tarok_shown_voids, tarok_playout_cards_net_voids) or in the worlds that also re-deal Klop's
    talon and the declarer's discards (tarok_played_cards, tarok_playout_cards_net_hidden); the env keeps the history.
    The spellings net= with voids=True / hidden=True keep raising ValueError, as they always have: net_worlds is the way in.
    net_depth=D (with net=weights; 1..12): the network's playouts stop at the player's D-th next decision and take the value
    head's estimate times net_value_scale (points per unit of the head: 1 / the learner's reward_scale) for the rest of the
    game (tarok_playout_cards_net_value, in the worlds of net_worlds) — at D = 1 at most 6 cards per playout where a fresh
    deal takes 47.  None (the default): the playouts run to the last card, the calls as they were.
    halving=(w0, w1, ..) (1..4 positive world counts; `worlds` None or their sum; with voids / hidden as worlds=W is; not with
    net=, exchange or bidding): the fair player spends its worlds by sequential halving (tarok_playout_cards_halving) —
    every legal card in the first w0 worlds, then the better half in w1 fresh ones, and so on: the finalists are compared
    over all the worlds at a fraction of the playouts.  None (the default): the calls as they were.
    net_halving=(w0, w1, ..) (with net=weights; `worlds` None or their sum; with net_worlds and net_depth; not with exchange
    or bidding): the network's playouts are spent by sequential halving on a compacted item list
    (tarok_playout_cards_net_halving).  None (the default): the calls as they were.  halving= with net= keeps raising.
    net_versus=(own_rel, opp_rel) with net_opponent=weights (with net=weights; net_seats left out; with net_worlds, net_depth and
    net_halving): the playouts seat TWO networks relative to the player's seat (tarok_playout_cards_net_versus) — `net` on the
    relative seats of own_rel, net_opponent on those of opp_rel, the Bot elsewhere; (1, 14): the player models the whole table
    as net_opponent and plays `net` against it.  net_opponent may be left out where opp_rel is 0.  None (the default): the
    calls as they were.
    net_samples=S, net_temperature=t, net_epsilon=e [, net_opp_temperature=, net_opp_epsilon=] (with net=weights, alone or with
    net_versus; any one of them given; not with net_seats, net_halving, exchange or bidding): the networks inside the playouts
    play as at the table — a draw from the softmax at the temperature (default 1; 0: the greedy card), the Bot's card with
    probability epsilon (default 0) — and every (card, world) gets S playouts (default 1) on draws of their own
    (tarok_playout_cards_net_sampled); net_opponent's mode defaults to net's.  All None (the default): the calls as they were.
    The same five duplicate passes (PASS_SEATS) on an env of its own; returns duplicate_advantage's dict, `policy_mean`
    being the playout player's.  inspect (tests): a list that receives one dict per pass, as in _play_passes_mode."""
    sampled = {k: v for k, v in dict(samples=net_samples, temperature=net_temperature, epsilon=net_epsilon,
                                     opp_temperature=net_opp_temperature, opp_epsilon=net_opp_epsilon).items() if v is not None}
    return duplicate_advantage(_playout_passes(samples, n_games, episodes, seed, mix, device, salt=salt, inspect=inspect,
                                               worlds=worlds, voids=voids, exchange=exchange, hidden=hidden, bidding=bidding,
                                               threshold=threshold, contracts=contracts, pass_value=pass_value, net=net,
                                               net_seats=net_seats, net_worlds=net_worlds, net_depth=net_depth,
                                               net_value_scale=net_value_scale, halving=halving, net_halving=net_halving,
                                               net_versus=net_versus, net_opponent=net_opponent, net_sampled=sampled or None))


def _front_cards(cards):
    """The card player of the front-end evaluations: the Bot on every seat, or — cards=weights — the network's greedy card
    (_network_cards at temperature 0) on the pass's seats in the Bot's place."""
    return _bot_cards if cards is None else _network_cards(TarokVecEnv.check_mlp_weights(cards), None, 0.0, 0.0)


def evaluate_exchange_vs_bot(worlds, samples, discard_sets, n_games, episodes, seed=0, mix=K.MIX_BOT, device=0, salt=0, inspect=None):
    """What is the talon exchange alone worth?  The five duplicate passes with the Bot playing EVERY card on every seat;
    in pass 1 + k the games seat k declared get their exchange from tarok_playout_exchange at (worlds, samples,
    discard_sets) — the talon group and discards with the best summed score over determinized playouts — and every
    other declarer exchanges as the Bot does (group 0, random discards).  Pass 0 is the Bot everywhere: the scores of
    evaluate_vs_bot's and evaluate_playout_vs_bot's pass 0 on the same deals.  Returns duplicate_advantage's dict,
    `policy_mean` being that of the seat whose exchanges the playouts chose.  (The same with the playouts played by a
    network: evaluate_exchange_net_vs_bot.)"""
    front = _front(inspect is not None, exchange=_exchange_front(worlds, samples, discard_sets, salt))
    return duplicate_advantage(_passes(n_games, episodes, front, _bot_cards, inspect, device=device, seed=seed, mix=mix))


def evaluate_exchange_net_vs_bot(net, worlds, discard_sets, n_games, episodes, seed=0, mix=K.MIX_BOT, device=0, salt=0, inspect=None,
                                 net_seats=15, cards=None, net_halving=None, net_list=False, net_depth=None, net_value_scale=70.0):
    """evaluate_exchange_vs_bot with the playouts played by a network: net = policy_mlp's six tensors; in pass 1 + k the
    games seat k declared get their exchange from ONE tarok_playout_exchange_net at (worlds, discard_sets) — one playout
    per (candidate, world), the network's greedy card on the seats of net_seats (a 4-bit set of absolute seats; "own":
    the pass's seat set) inside them, the Bot's on the others — in tarok_playout_exchange's place; the inspected dicts
    also hold the launch's sums.  cards=weights: the pass's seats also PLAY the network's greedy card, in the Bot's place.
    Pass 0 is the Bot everywhere either way: evaluate_exchange_vs_bot's pass 0 on the same deals.  (A function of its own,
    not arguments of evaluate_exchange_vs_bot: that call's parameter list is pinned as it stands.)  net_depth: None, or
    1..13 — tarok_playout_exchange_net_value: the playouts stop at the declarer's net_depth-th decision and read the value
    head of `net` there at net_value_scale points per unit.  net_list=True: the launch is tarok_playout_exchange_net_list
    with the same arguments — the same numbers from a compacted item list.  net_halving: a tuple of 1..4 positive world
    counts — the launch is tarok_playout_exchange_net_halving, which spends later rounds' worlds on the leading candidates;
    it names the worlds itself (`worlds` None or their sum), goes with net_depth and is not given with net_list=True."""
    if net_list and net is None:
        raise ValueError("net_list packs the network's playouts: it needs net=")
    net_halving = playout.check_front_halving(net_halving, net, net_list, worlds, None)
    exchange = _exchange_net_front(*_net_front_args(net, net_seats, None, "candidate", net_depth, net_value_scale), worlds, discard_sets,
                                   salt, net_depth, net_value_scale, bool(net_list), net_halving)
    front = _front(inspect is not None, exchange=exchange)
    return duplicate_advantage(_passes(n_games, episodes, front, _front_cards(cards), inspect, device=device, seed=seed, mix=mix))


def evaluate_exchangenet_vs_bot(weights, n_games, episodes, seed=0, mix=K.MIX_BOT, device=0, inspect=None):
    """What is the exchange head's exchange worth?  evaluate_exchange_vs_bot with tarok_exchange_values in
    tarok_playout_exchange's place: the five duplicate passes with the Bot playing EVERY card on every seat; in pass
    1 + k the games seat k declared get their talon group and discards from the network — weights = (w1, b1, w2, b2, w3,
    b3) as tarok_exchange_values takes them (exchange.ExchangeLearner.weights()) — and every other declarer exchanges as
    the Bot does.  Pass 0 is the Bot's own exchange everywhere: evaluate_exchange_vs_bot's pass 0 on the same deals.
    Returns duplicate_advantage's dict, `policy_mean` being that of the seat whose exchanges the head chose."""
    front = _front(inspect is not None, exchange=_exchangenet_front(TarokVecEnv.check_mlp_weights(weights)))
    return duplicate_advantage(_passes(n_games, episodes, front, _bot_cards, inspect, device=device, seed=seed, mix=mix))


def evaluate_bidding_vs_bot(worlds, samples, n_games, episodes, seed=0, device=0, salt=0, threshold=0,
                            contracts=K.BID_DEFAULT_CONTRACTS, inspect=None, pass_value=False, net=None, net_seats=15, cards=None,
                            net_halving=None, net_list=False, net_depth=None, net_value_scale=70.0):
    """What is the bid alone worth?  The five duplicate passes on K.MIX_BOT's deals with the Bot making EVERY exchange and
    playing EVERY card; in pass 1 + k seat k bids by playouts — tarok_playout_bids at (worlds, samples) over `contracts`,
    then tarok_bid_round with `threshold` — against three Bot bidders, and calls its king by the same sums.  Pass 0 is the
    Bot's own bidding round on every seat: the scores of evaluate_vs_bot's pass 0 on the same deals.  Returns
    duplicate_advantage's dict, `policy_mean` being that of the seat that bid by playouts.  pass_value=True: the seat's
    pass is valued by playouts as well (tarok_playout_bids_pass) and is the bar its bids have to clear
    (tarok_bid_round_pass, `threshold` the margin over it); pass 0 is unchanged.
    net=weights (policy_mlp's six tensors; `samples` None or 1; not with pass_value=True): the playouts are played by the
    network — one tarok_playout_bids_net at `worlds` in tarok_playout_bids' place, the network's greedy card on the seats
    of net_seats (a 4-bit set of absolute seats; "own": the pass's seat set) inside them, and tarok_bid_round at playouts =
    worlds; the inspected dicts then also hold the launch's sums.  cards=weights: the pass's seats also PLAY the network's
    greedy card, in the Bot's place.  net_depth (with net): None, or 1..13 — tarok_playout_bids_net_value: the playouts stop
    at the viewer's net_depth-th decision and read the value head of `net` there at net_value_scale points per unit; then
    pass_value=True is allowed too — the launch plays the pass item, and tarok_bid_round_pass holds every bid against it as
    for the Bot teacher.  net_list=True (with net): the launch is tarok_playout_bids_net_list with the same arguments — the
    same numbers from a compacted item list.  net_halving (with net): a tuple of 1..4 positive world counts — the launch is
    tarok_playout_bids_net_halving, which spends later rounds' worlds on a viewer's leading rows; its value_out goes to the
    round at playouts = the schedule's sum; it names the worlds itself (`worlds` None or their sum), goes with net_depth,
    values the pass at any depth, and is not given with net_list=True.  With the defaults the call issues the launches it
    always did."""
    net_halving = playout.check_front_halving(net_halving, net, net_list, worlds, samples)
    if net is None:
        if net_depth is not None:
            raise ValueError("net_depth stops the network's playouts: it needs net=")
        if net_list:
            raise ValueError("net_list packs the network's playouts: it needs net=")
        bid = _bid_front((worlds, samples), salt, threshold, contracts, pass_value)
    else:
        if pass_value and net_depth is None and net_halving is None:
            raise ValueError("net= without net_depth does not value the pass: pass_value=True goes with the Bot's playouts or "
                             "with net_depth")
        bid = _bid_net_front(*_net_front_args(net, net_seats, samples, "option", net_depth, net_value_scale), worlds, salt, threshold,
                             contracts, net_depth, net_value_scale, bool(pass_value), bool(net_list), net_halving)
    front = _front(inspect is not None, bid=bid)
    return duplicate_advantage(_passes(n_games, episodes, front, _front_cards(cards), inspect, device=device, seed=seed, mix=K.MIX_BOT))


def evaluate_bidnet_vs_bot(bid_weights, n_games, episodes, seed=0, device=0, threshold=0, contracts=K.BID_DEFAULT_CONTRACTS,
                           playouts_equiv=16, reward_scale=1.0 / 70.0, inspect=None, pass_value=False):
    """What is the bidding head's bid worth?  evaluate_bidding_vs_bot with tarok_bid_values in tarok_playout_bids' place:
    the five duplicate passes on K.MIX_BOT's deals with the Bot making EVERY exchange and playing EVERY card; in pass
    1 + k seat k bids from the network's values — bid_weights = (w1, b1, w2, b2, w3, b3) as tarok_bid_values takes them
    (bidding.BidLearner.weights()), scaled to sums over `playouts_equiv` playouts of `reward_scale` points, so that
    `threshold` is in points per game as for the teacher — against three Bot bidders.  Pass 0 is the Bot's own round on
    every seat: evaluate_bidding_vs_bot's pass 0 on the same deals.  Returns duplicate_advantage's dict, `policy_mean`
    being that of the seat the head bid for.  pass_value=True: output 19 is the seat's value of a pass and the bar its bids
    have to clear (tarok_bid_values_pass, tarok_bid_round_pass; a head trained by BidLearner(pass_value=True))."""
    front = _front(inspect is not None, bid=_bidnet_front(TarokVecEnv.check_mlp_weights(bid_weights), playouts_equiv, reward_scale,
                                                          threshold, contracts, pass_value))
    return duplicate_advantage(_passes(n_games, episodes, front, _bot_cards, inspect, device=device, seed=seed, mix=K.MIX_BOT))
