"""The playout card player, described once: what SelfPlay(teacher=dict(...)), SelfPlay.evaluate(playout_*=...) and
evaluate.evaluate_playout_vs_bot(...) each spell in their own words.  card_player() holds every rule of the options and
returns a CardPlayer — ONE class for every kind of launch, the options a kind does not have None —; the CardPlayer knows
what its launch needs (history, the words tensor, the net scratch, the divisor of tarok_playout_targets or a count per
card) and issues it, with one signature, through the env's public method of its launch_kind.  A door keeps only the rules
that are its own (tau and every; versus_playout; exchange and bidding) and names the options its way through spelling()."""
import collections
import numbers

import torch

from . import karte as K

WORLDS = ("det", "voids", "hidden")               # the fair world kinds; the position is tarok_playout_cards_net_value's `kind`
WORDS_DTYPE = dict(voids=torch.int32, hidden=torch.int64)      # the per-game words a kind reads: shown_voids() / played_cards()
OPTIONS = ("samples", "worlds", "voids", "hidden", "exchange", "bidding", "net", "net_seats", "net_worlds", "net_depth", "net_value_scale",
           "halving", "net_halving", "net_versus", "net_sampled")


def spelling(prefix="", pattern="%s", **other):
    """How a door words a refusal: `prefix`, then the text with every {option} of OPTIONS replaced by other[option] or
    pattern % option.  The default is evaluate_playout_vs_bot's spelling."""
    names = {k: other.get(k, pattern % k) for k in OPTIONS}
    return lambda text: prefix + text.format(**names)


def exchange_net_launch(env, net_list, value):
    """The env's net-played exchange launch: the compacted list's; else, `value`: the one that takes (depth, value_scale)."""
    return env.playout_exchange_net_list if net_list else env.playout_exchange_net_value if value else env.playout_exchange_net


def bids_net_launch(env, net_list, value):
    """The env's net-played bid launch: the compacted list's; else, `value`: the one that takes (depth, value_scale, pass_value)."""
    return env.playout_bids_net_list if net_list else env.playout_bids_net_value if value else env.playout_bids_net


def front_halving_launch(env, bids):
    """The env's sequential-halving launch over the net-played front lists: the bid launch's, else the exchange's."""
    return env.playout_bids_net_halving if bids else env.playout_exchange_net_halving


def check_front_halving(net_halving, net, net_list, worlds, samples, say=spelling()):
    """net_halving= of the exchange and bid doors -> its schedule as a tuple (None stays None).  It needs {net}=, is itself a
    list launch (no net_list=True beside it), names the worlds itself — `worlds` None or the schedule's sum — and runs one
    playout per (arm, world): samples None or 1."""
    if net_halving is None:
        return None
    schedule = check_halving(net_halving, say, "{net_halving}")
    if net is None or net is False:
        raise ValueError(say("{net_halving}= spends the worlds of the network's playouts: it goes with {net}="))
    if net_list:
        raise ValueError(say("{net_halving}= is already a list launch: leave net_list out"))
    if worlds is not None and int(worlds) != sum(schedule):
        raise ValueError(say("{net_halving}= names the worlds of every round: {worlds} is optional and must be their sum"))
    if samples not in (None, 1):
        raise ValueError(say("{net_halving}= runs one playout per (arm, world): {samples} is optional and must be 1"))
    return schedule


def one_world_kind(voids, hidden, say=spelling()):
    if voids and hidden:
        raise ValueError(say("{hidden}=True is not built together with {voids}=True: give one of the two"))


def check_depth(depth, value_scale, say=spelling(net_depth="depth", net_value_scale="value_scale"), max_depth=K.PLAYOUT_MAX_DEPTH):
    """max_depth: K.PLAYOUT_FRONT_MAX_DEPTH for the exchange and bid launches, whose items start at 0 cards played."""
    if isinstance(depth, bool) or not isinstance(depth, numbers.Integral) or not 1 <= depth <= max_depth:
        raise ValueError(say("{net_depth}: None or 1..%d viewer decisions" % max_depth))
    if not 0 < float(value_scale) < float("inf"):
        raise ValueError(say("{net_value_scale}: finite and > 0"))


def check_halving(halving, say=spelling(), option="{halving}"):
    """A sequential-halving schedule as a tuple: 1..K.PLAYOUT_MAX_ROUNDS positive ints, at most K.PLAYOUT_MAX_WORLDS in all.
    option: the name the refusal gives it ("{net_halving}" for the net-played launch's)."""
    ok = isinstance(halving, (tuple, list)) and 1 <= len(halving) <= K.PLAYOUT_MAX_ROUNDS and \
        all(isinstance(w, numbers.Integral) and not isinstance(w, bool) and w >= 1 for w in halving)
    if not ok or sum(halving) > K.PLAYOUT_MAX_WORLDS:
        raise ValueError(say(option + ": 1..%d positive world counts, one per round, at most %d in all" % (K.PLAYOUT_MAX_ROUNDS, K.PLAYOUT_MAX_WORLDS)))
    return tuple(int(w) for w in halving)


def check_versus(net_versus, say=spelling()):
    """The roles of a two-network net playout as (own_rel, opp_rel): two disjoint 4-bit sets over the seats RELATIVE to the
    viewer (bit r: the seat r places after the viewer; bit 0 the viewer itself) — network A's seats and network B's."""
    ok = isinstance(net_versus, (tuple, list)) and len(net_versus) == 2 and \
        all(isinstance(r, numbers.Integral) and not isinstance(r, bool) and 0 <= r <= 15 for r in net_versus)
    if not ok or net_versus[0] & net_versus[1]:
        raise ValueError(say("{net_versus}: (own_rel, opp_rel), two disjoint 4-bit sets (0..15) over the seats relative to the viewer"))
    return int(net_versus[0]), int(net_versus[1])


def check_play_mode(temperature, epsilon, say=spelling(), names=("temperature", "epsilon")):
    """A play mode as tarok_set_play_mode takes it: temperature 0 (greedy) or within [1e-6, 1e6], epsilon within [0, 1]."""
    ok = all(isinstance(x, numbers.Real) and not isinstance(x, bool) and x == x for x in (temperature, epsilon))
    if not ok or not (temperature == 0 or 1e-6 <= temperature <= 1e6) or not 0 <= epsilon <= 1:
        raise ValueError(say("%s: 0 (greedy) or within 1e-6..1e6; %s: within 0..1" % names))
    return float(temperature), float(epsilon)


def check_play_modes(temperature, epsilon, opp_temperature=None, opp_epsilon=None, say=spelling()):
    """The two play modes of a sampled net playout as (temperature, epsilon, opp_temperature, opp_epsilon): network A's, then
    network B's, whose values default — each on its own — to A's."""
    t, e = check_play_mode(temperature, epsilon, say)
    return (t, e) + check_play_mode(t if opp_temperature is None else opp_temperature, e if opp_epsilon is None else opp_epsilon, say,
                                    ("opp_temperature", "opp_epsilon"))


SAMPLED_KEYS = ("samples", "temperature", "epsilon", "opp_temperature", "opp_epsilon")


def check_sampled(net_sampled, say=spelling()):
    """net_sampled=dict(samples=1, temperature=1.0, epsilon=0.0, opp_temperature=None, opp_epsilon=None) -> (samples, modes):
    the playouts per (card, world) and check_play_modes' four numbers."""
    if not isinstance(net_sampled, dict) or set(net_sampled) - set(SAMPLED_KEYS):
        raise ValueError(say("{net_sampled}: a dict with keys among %s" % ", ".join(SAMPLED_KEYS)))
    samples = net_sampled.get("samples", 1)
    if not (isinstance(samples, numbers.Integral) and not isinstance(samples, bool) and 1 <= samples <= K.PLAYOUT_MAX_SAMPLES):
        raise ValueError(say("{net_sampled}: samples 1..%d" % K.PLAYOUT_MAX_SAMPLES))
    return int(samples), check_play_modes(net_sampled.get("temperature", 1.0), net_sampled.get("epsilon", 0.0),
                                          net_sampled.get("opp_temperature"), net_sampled.get("opp_epsilon"),
                                          lambda text: say("{net_sampled}: " + text))


class CardPlayer(collections.namedtuple("CardPlayer", "kind worlds samples net net_seats depth value_scale salt halving versus modes",
                                        defaults=(None, None, None))):
    """kind: "open" (the true hands) or one of WORLDS; worlds as the door gave it (None or 0 for "open"), samples per
    (card, world); net: the playouts are played by a network on net_seats (a set 0..15, or "own": the launch's own seats),
    stopped at the viewer's depth-th decision (None: never) with the value head at value_scale points per unit.
    halving: None, or the worlds of every round of sequential halving, worlds their sum — the Bot-played launch's, with net the
    net-played one's.  versus: None, or (own_rel, opp_rel): the playouts seat TWO networks relative to each game's viewer, the
    player's own and an opponent's; net_seats is then not read.  modes: None, or (temperature, epsilon,
    opp_temperature, opp_epsilon): the networks play under a play mode each, `samples` playouts per (card, world) (DESIGN
    8.25); versus is then (15, 0) where the door gave net= alone, and halving is None (no such launch)."""
    __slots__ = ()

    needs_history = property(lambda self: self.kind in WORDS_DTYPE)
    words_dtype = property(lambda self: WORDS_DTYPE.get(self.kind))
    playouts = property(lambda self: max(1, self.worlds or 0) * self.samples)       # tarok_playout_targets' divisor
    # the rows have a count per card (count_out), not one divisor: the targets are tarok_playout_targets_counts'
    counts = property(lambda self: self.halving is not None)

    @property
    def launch_kind(self):
        """The env method of the launch: fair | halving | net | net_value | net_halving | versus | sampled."""
        if self.modes is not None:
            return "sampled"
        if self.versus is not None:
            return "versus"
        if not self.net:
            return "fair" if self.halving is None else "halving"
        return "net_halving" if self.halving is not None else "net" if self.depth is None else "net_value"

    def prepare(self, env):
        """What has to exist before the launch is captured into a graph: a net-played launch's scratch."""
        if self.modes is not None:
            env.playout_net_sampled_scratch(self.worlds, self.samples)
        elif self.net and self.halving is not None:
            env.playout_net_halving_scratch(self.halving)
        elif self.net:
            env.playout_net_scratch(self.worlds)

    def launch(self, env, nets, sets, words, sum_out, action_out, count_out=None, modes=None):
        """The player's launch on `env`, through the env's public method of its launch_kind; returns what that returns.
        nets = (weights, opponent): the six tensors of the player's network and of the opponent's, each None where the kind
        does not read it; sets = dict(seats=...) or dict(seats_per_game=...); words the caller's tensor of words_dtype (None
        where there is none); count_out: the caller's [N,12] int32 tensor where the player `counts` (None: a new one per
        call); modes: the four numbers in self.modes' place (a caller that fixes the opponent's mode late)."""
        weights, opponent = nets
        kind = self.launch_kind
        world = dict(voids=self.kind == "voids", hidden=self.kind == "hidden", words=words)
        out = dict(salt=self.salt, sum_out=sum_out, action_out=action_out, **sets)
        value = dict(depth=self.depth, value_scale=self.value_scale)
        if kind == "fair":
            return env.playout_cards_fair(self.worlds, self.samples, **world, **out)
        if kind == "halving":
            return env.playout_cards_halving(self.halving, self.samples, count_out=count_out, **world, **out)
        if kind == "sampled":
            t, e, ot, oe = self.modes if modes is None else modes
            return env.playout_cards_net_sampled(weights, opponent, self.worlds, self.samples, *self.versus, temperature=t, epsilon=e,
                                                 opp_temperature=ot, opp_epsilon=oe, **value, **world, **out)
        if kind == "versus":
            more = {} if self.halving is None else dict(count_out=count_out)
            return env.playout_cards_net_versus(weights, opponent, self.worlds, *self.versus, halving=self.halving, **value, **world, **more, **out)
        net_seats = sets["seats"] if self.net_seats == "own" else self.net_seats
        if kind == "net_halving":
            return env.playout_cards_net_halving(weights, self.halving, net_seats, count_out=count_out, **value, **world, **out)
        if self.needs_history:
            out.update({self.kind: True, "words": words})
        if kind == "net":
            return env.playout_cards_net(weights, self.worlds, net_seats=net_seats, **out)
        return env.playout_cards_net_value(weights, self.worlds, self.depth, self.value_scale, net_seats=net_seats, **out)


def card_player(samples=None, worlds=None, voids=False, hidden=False, net=False, net_seats=15, net_worlds="det", net_depth=None,
                net_value_scale=70.0, salt=0, front=False, fused=True, history=None, own=True, say=spelling(), halving=None,
                net_halving=None, net_versus=None, net_sampled=None):
    """The one validator of a card player's options, in evaluate_playout_vs_bot's names: a CardPlayer, or a ValueError in
    the door's words (say: spelling()).  samples None: 1.  front: the door also asked for a playout-valued exchange or
    bidding.  fused: the door's policy is the fused one.  history: whether the env at hand keeps the play history (None:
    the door makes its env as needs_history says).  own: the door takes net_seats="own".
    halving: a tuple of 1..4 positive world counts, one per round of sequential halving (tarok_playout_cards_halving): it names the worlds
    itself — `worlds` None (or 0) or their sum —, goes with voids / hidden as worlds does, and is not built for net=, the
    exchange, the bidding or open hands.
    net_halving: such a tuple for the NET-played launch (tarok_playout_cards_net_halving; the player's `halving`): it requires
    net=, names the worlds itself as halving does, goes with net_worlds and net_depth, and takes what net= takes — samples
    None or 1, no exchange, no bidding.  halving= together with net= keeps raising.
    net_versus: (own_rel, opp_rel) — the player's `versus` (tarok_playout_cards_net_versus): the playouts seat the player's network on
    the relative seats of own_rel and an opponent's on those of opp_rel, relative to each game's viewer.  It requires net=, goes
    with net_worlds, net_depth and net_halving, and seats the networks itself: net_seats stays at its default.
    net_sampled: dict(samples=, temperature=, epsilon=, opp_temperature=, opp_epsilon=) on top of net= or net_versus= — the
    player's `modes` (tarok_playout_cards_net_sampled): the networks play under those play modes (the opponent's default to the
    player's), `samples` playouts per (card, world).  With net= alone the network sits on all four seats, (own_rel, opp_rel) =
    (15, 0): net_seats stays at its default.  Not built, and refused by name: net_halving, the exchange and the bidding."""
    sampled = None
    if net_sampled is not None:
        sampled = check_sampled(net_sampled, say)
        if not net:
            raise ValueError(say("{net_sampled}= sets how the networks play inside the network's playouts: it goes with {net}="))
        if net_halving is not None:
            raise ValueError(say("{net_sampled}= is not built for {net_halving}: the sampled launch has no halving form"))
        if front:
            raise ValueError(say("{net_sampled}= is not built for the {exchange} and {bidding} launches: the card launch alone is sampled"))
        if net_seats != 15:
            raise ValueError(say("{net_sampled}= seats the network relative to the viewer, on all four seats or as {net_versus} says: "
                                 "leave {net_seats} out"))
    if net_versus is not None:
        net_versus = check_versus(net_versus, say)
        if not net:
            raise ValueError(say("{net_versus}= seats two networks inside the network's playouts: it goes with {net}="))
        if net_seats != 15:
            raise ValueError(say("{net_versus}= seats the networks itself, relative to the viewer: leave {net_seats} out"))
    if halving is not None:
        halving = check_halving(halving, say)
        if net or front:
            raise ValueError(say("{halving}= is the Bot-played card launch's: no {net}, {exchange} or {bidding}"))
        if worlds and int(worlds) != sum(halving):
            raise ValueError(say("{halving}= names the worlds of every round: {worlds} is optional and must be their sum"))
        worlds = sum(halving)
    if net_halving is not None:
        net_halving = check_halving(net_halving, say, "{net_halving}")
        if not net:
            raise ValueError(say("{net_halving}= spends the worlds of the network's playouts: it goes with {net}="))
        if worlds and int(worlds) != sum(net_halving):
            raise ValueError(say("{net_halving}= names the worlds of every round: {worlds} is optional and must be their sum"))
        worlds = sum(net_halving)
    if net_depth is not None:
        if not net:
            raise ValueError(say("{net_depth} stops the network's playouts: it goes with {net}="))
        check_depth(net_depth, net_value_scale, say)
    if net_worlds not in WORLDS:
        raise ValueError(say("{net_worlds}: one of %s" % ", ".join('"%s"' % w for w in WORLDS)))
    if net_worlds != "det" and not net:
        raise ValueError(say("{net_worlds} names the worlds of the network's playouts: it goes with {net}="))
    if net:
        if not worlds:
            raise ValueError(say("{net}= plays the determinized player's playouts: give {worlds}= as well"))
        if samples not in (None, 1):
            raise ValueError(say("{net}= runs one playout per (card, world): {samples} is optional and must be 1"))
        if voids or hidden or front:
            raise ValueError(say("{net}= composes with nothing else yet: no {voids}, {hidden}, {exchange} or {bidding}"))
        if not (own and net_seats == "own") and not (isinstance(net_seats, int) and 0 <= net_seats <= 15):
            raise ValueError(say("{net_seats}: a 4-bit seat set, 0..15" + ', or "own"' * own))
        if not fused:
            raise ValueError(say("{net}= plays tarok_playout_cards_net, which needs the fused policy (hidden = 256)"))
    if voids and not worlds:
        raise ValueError(say("{voids}=True constrains the re-deals: give {worlds}= as well"))
    if hidden and not worlds:
        raise ValueError(say("{hidden}=True widens the re-deals: give {worlds}= as well"))
    one_world_kind(voids, hidden, say)
    samples, worlds = 1 if samples is None else int(samples), None if worlds is None else int(worlds)
    if not (0 <= (worlds or 0) <= K.PLAYOUT_MAX_WORLDS and 1 <= samples <= K.PLAYOUT_MAX_SAMPLES):
        raise ValueError(say("{worlds} 0..%d, {samples} 1..%d" % (K.PLAYOUT_MAX_WORLDS, K.PLAYOUT_MAX_SAMPLES)))
    kind = "open" if not worlds else "voids" if voids else "hidden" if hidden else net_worlds
    if kind in WORDS_DTYPE and history is not None and not history:
        raise ValueError(say("the %s worlds read the play history: TarokVecEnv(history=True)" % kind))
    samples, modes = (samples, None) if sampled is None else sampled
    if modes is not None and net_versus is None:
        net_versus = (15, 0)
    return CardPlayer(kind, worlds, samples, bool(net), net_seats, net_depth, float(net_value_scale), int(salt),
                      halving if net_halving is None else net_halving, net_versus, modes)
