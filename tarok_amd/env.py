"""TarokVecEnv — N lock-stepped 4-player Tarok games on one MI355X.

Host-side mirror of what the reference does with N `Igra` objects inside
`Tarok.paralel_start` (Tarok.py:30-62): `reset()` deals and sets the contracts
up (Igra.razdeli + engine constructors + talon exchange), `legal_actions()` is
`mozne_karte` for the seat to move, `step()` is one `next(g)` per game.  All
compute is in libtarokenv.so (HIP, gfx950); torch only provides device memory
and streams.  There is no CPU path: constructing an env without the library or
without a GPU raises.
"""
import ctypes as C

import numpy as np
import torch

from . import _native
from . import karte as K
from . import playout as P


def _u64(t):
    """int64 torch tensor -> numpy uint64 (host)."""
    return t.detach().cpu().numpy().view(np.uint64)


def _salt(salt):
    """A salt as the ABI's uint64."""
    return int(salt) & ((1 << 64) - 1)


_SIZES = dict(worlds=(K.PLAYOUT_MAX_WORLDS, "worlds: 1..%d" % K.PLAYOUT_MAX_WORLDS),
              samples=(K.PLAYOUT_MAX_SAMPLES, "samples: 1..%d" % K.PLAYOUT_MAX_SAMPLES),
              discard_sets=(K.EXCHANGE_MAX_SETS, "discard_sets: 1..%d" % K.EXCHANGE_MAX_SETS),
              contracts=(K.BID_ALL_CONTRACTS, "contracts: a bit set within 1..0x3FF"))


def _sizes(**given):
    """worlds=, discard_sets=, contracts= of a scratch method as ints, each within 1..its maximum (else a ValueError)."""
    for name, value in given.items():
        if not 1 <= int(value) <= _SIZES[name][0]:
            raise ValueError(_SIZES[name][1])
    return [int(value) for value in given.values()]


class Obs:
    """Per-game observation words (include/tarok_env.h TAROK_OBS_*) as an int64
    device tensor with decoded views."""

    def __init__(self, words):
        self.words = words

    @property
    def mask(self):            # legal-card mask of the seat to move (= `mozne`)
        return self.words & K.OBS_MASK

    @property
    def seat(self):
        return (self.words >> K.OBS_SEAT_SHIFT) & 3

    @property
    def step(self):            # cards played so far in the game
        return (self.words >> K.OBS_STEP_SHIFT) & 63

    @property
    def done(self):
        return ((self.words >> K.OBS_DONE_BIT) & 1).bool()

    @property
    def error(self):
        return self.words < 0   # bit 63

    def mask_numpy(self):
        return _u64(self.mask)


def playout_values(sum, words, samples):
    """TarokVecEnv.playout_cards' sums as per-card values: [N,54] float32, for every legal card of the seat to move (the
    legal mask and seat of the observation words `words` [N] int64 the playouts started from) the mean final score of
    that seat over the `samples` open-hand playouts, -inf elsewhere.  Rank j of `sum` [N,12,4] is the j-th lowest legal
    card.  Pure torch, on whatever device the inputs are; the values inherit the playouts' perfect information.
    `samples` is the divisor, the number of playouts per card: for the sums of a determinized launch
    (playout_cards_det) pass worlds * samples; those values use the mover's own information only."""
    cards = torch.arange(54, device=words.device, dtype=torch.int64)
    legal = ((words.to(torch.int64).unsqueeze(1) >> cards) & 1).bool()                  # [N,54]
    rank = (torch.cumsum(legal.to(torch.int64), dim=1) - 1).clamp_(0, K.PLAYOUT_RANKS - 1)
    seat = ((words.to(torch.int64) >> K.OBS_SEAT_SHIFT) & 3).view(-1, 1, 1).expand(-1, K.PLAYOUT_RANKS, 1)
    # the correctly rounded float32 quotient on every device: a float32 division by a scalar may be carried out as a
    # multiplication by its reciprocal, which is an ulp off for some sums; in float64 either way rounds to the same float32
    own = (torch.gather(sum, 2, seat).squeeze(2).to(torch.float64) / float(samples)).to(torch.float32)      # [N,12]
    return torch.where(legal, torch.gather(own, 1, rank), torch.full((), float("-inf"), device=words.device))


class TarokVecEnv:
    def __init__(self, n_games, device=0, seed=0, mix=K.MIX_ALL, game_offset=0, history=False, refill_fan=None, lazy_refill=None):
        """refill_fan, lazy_refill: launch tuning (tarok_set_option; None = the library's default for the batch size);
        results never depend on them."""
        self._h = None
        L = _native.lib()
        if not torch.cuda.is_available() or L.tarok_device_count() == 0:
            raise _native.TarokNativeError("TarokVecEnv needs an MI355X: no GPU is visible and there is no CPU fallback")
        self.L = L
        self.n = int(n_games)
        self.device_index = int(device)
        self.device = torch.device("cuda", self.device_index)
        self.seed, self.mix, self.game_offset = int(seed), int(mix), int(game_offset)
        h = C.c_void_p()
        self.history = bool(history)
        _native.check(L.tarok_create(C.byref(h), self.device_index, self.n, self.game_offset, self.seed, self.mix,
                                     K.HISTORY if history else 0))
        self._h = h
        self._net_scratch = {}          # the scratch tensors of the launches that take one, by (name, shape): _scratch
        self.set_option(refill_fan, lazy_refill)
        with torch.cuda.device(self.device):
            self.obs_words = torch.zeros(self.n, dtype=torch.int64, device=self.device)
            self.reward = torch.zeros((self.n, 4), dtype=torch.int16, device=self.device)
            self.done = torch.zeros(self.n, dtype=torch.uint8, device=self.device)
            self.action = torch.full((self.n,), 255, dtype=torch.uint8, device=self.device)
            self.trick = None     # allocated by step(..., tricks=True)

    # ------------------------------------------------------------------
    def set_option(self, refill_fan=None, lazy_refill=None):
        """Launch tuning (tarok_set_option) at any point of a run; results never depend on it.  A change of the refill fan
        after the first step launch synchronises the device (include/tarok_env.h)."""
        if refill_fan is not None:
            _native.check(self.L.tarok_set_option(self._h, K.OPT_REFILL_FAN, int(refill_fan)))
        if lazy_refill is not None:
            _native.check(self.L.tarok_set_option(self._h, K.OPT_LAZY_REFILL, int(lazy_refill)))

    def set_play_mode(self, temperature=1.0, epsilon=0.0):
        """How sample_policy, policy_mlp and policy_step choose the card from the logits (tarok_set_play_mode): a draw
        from the softmax at `temperature` (0: greedy, the lowest-numbered legal card at the maximum), and with probability
        `epsilon` the Bot's uniformly random legal card instead — (0, random_card) is Igralec.igraj_karto's selection.
        (1, 0), a new env's mode, is the plain draw.  logp_out is the log-probability of the played card under the whole
        mode.  Read when a launch is issued: a graph captured around launches keeps the mode it was captured with."""
        _native.check(self.L.tarok_set_play_mode(self._h, float(temperature), float(epsilon)))

    @property
    def play_mode(self):
        """(temperature, epsilon) as set (tarok_get_play_mode)."""
        t, e = C.c_float(), C.c_float()
        _native.check(self.L.tarok_get_play_mode(self._h, C.byref(t), C.byref(e)))
        return t.value, e.value

    def refill_selftest(self, kind, per_slot, episode0=100, order=0, reps=1):
        """tarok_debug_refill_selftest (tests only; reset() afterwards): (wrong lines, [first records])."""
        import numpy as np
        rep = np.zeros(49, np.uint64)
        with torch.cuda.device(self.device):
            torch.cuda.synchronize(self.device)
            _native.check(self.L.tarok_debug_refill_selftest(self._h, int(kind), int(per_slot), int(episode0), int(order), int(reps),
                                                             rep.ctypes.data))
        return int(rep[0]), rep[1:].reshape(8, 6)[: min(8, int(rep[0]))]

    def close(self):
        if self._h is not None:
            torch.cuda.synchronize(self.device)
            self.L.tarok_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _dev(self, x, dtype, shape):
        """None -> NULL; tensor / array -> contiguous device tensor of dtype."""
        if x is None:
            return None
        t = torch.as_tensor(x)
        t = t.to(device=self.device, dtype=dtype).contiguous()
        if tuple(t.shape) != tuple(shape):
            raise ValueError("expected shape %s, got %s" % (tuple(shape), tuple(t.shape)))
        return t

    @staticmethod
    def _p(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def _empty(self, t, shape, dtype):
        """An output the caller gave, or where it gave None a new uninitialised tensor on the env's device."""
        return torch.empty(shape, dtype=dtype, device=self.device) if t is None else t

    # ------------------------------------------------------------------
    def reset(self, episode=0, deals=None, contract=None, declarer=None, king_suit=None,
              talon_choice=None, discards=None, defer_exchange=False, clear_counters=True):
        """Deal + set up all N games (Igra.py:38-55,65-73; Navadna_igra.py:20-68).
        Returns the first observation."""
        n = self.n
        deals = self._dev(deals, torch.uint8, (n, 54))
        contract = self._dev(contract, torch.int8, (n,))
        declarer = self._dev(declarer, torch.int8, (n,))
        king_suit = self._dev(king_suit, torch.int8, (n,))
        talon_choice = self._dev(talon_choice, torch.int8, (n,))
        discards = self._dev(discards, torch.uint8, (n, 3))
        flags = (K.DEFER_EXCHANGE if defer_exchange else 0) | (K.CLEAR_COUNTERS if clear_counters else 0)
        with torch.cuda.device(self.device):
            _native.check(self.L.tarok_reset(self._h, int(episode), self._p(deals), self._p(contract), self._p(declarer),
                                             self._p(king_suit), self._p(talon_choice), self._p(discards), flags,
                                             self._stream()))
        return self.legal_actions()

    def exchange(self, talon_choice=None, discards=None):
        """menjaj_iz_talona for games still waiting (Navadna_igra.py:60-66)."""
        talon_choice = self._dev(talon_choice, torch.int8, (self.n,))
        discards = self._dev(discards, torch.uint8, (self.n, 3))
        with torch.cuda.device(self.device):
            _native.check(self.L.tarok_exchange(self._h, self._p(talon_choice), self._p(discards), self._stream()))
        return self.legal_actions()

    def legal_actions(self):
        with torch.cuda.device(self.device):
            _native.check(self.L.tarok_legal_actions(self._h, self._p(self.obs_words), None, self._stream()))
        return Obs(self.obs_words)

    def _trick_buf(self, tricks):
        if tricks and self.trick is None:
            with torch.cuda.device(self.device):
                self.trick = torch.zeros(self.n, dtype=torch.int16, device=self.device)
        return self.trick if tricks else None

    def step(self, action, auto_reset=False, tricks=False, obs_out=None, reward_out=None, done_out=None, reward_ref=False):
        """One card per game.  Returns (Obs, reward[N,4] i16 — valid where done, done[N] u8).
        reward_ref=True: reward carries what rezultat_igre folds into the last transition (Igralec.py:421-437:
        the scores, but -20 / +20 for the defenders of a Berac) instead of the plain scores.
        tricks=True also fills self.trick [N] i16: 0, or 0x8000 | vrednost_stiha<<4 | winner seat
        for games whose trick this card completed (what rezultat_stiha is told).
        obs_out / reward_out / done_out: caller-owned device tensors to write into instead of
        the env's own buffers (e.g. rows of a rollout buffer)."""
        a = self._dev(action, torch.uint8, (self.n,))
        ob = self.obs_words if obs_out is None else obs_out
        rw = self.reward if reward_out is None else reward_out
        dn = self.done if done_out is None else done_out
        with torch.cuda.device(self.device):
            _native.check(self.L.tarok_step(self._h, self._p(a), self._p(rw), self._p(dn),
                                            self._p(self._trick_buf(tricks)), self._p(ob),
                                            (K.AUTO_RESET if auto_reset else 0) | (K.REWARD_REF if reward_ref else 0),
                                            self._stream()))
        return Obs(ob), rw, dn

    def sample_policy(self, logits, obs_words, action_out=None, logp_out=None):
        """Masked categorical sample from bf16 logits [N,64] (tarok_sample_policy)."""
        assert logits.dtype == torch.bfloat16 and logits.is_contiguous() and tuple(logits.shape) == (self.n, 64)
        with torch.cuda.device(self.device):
            action_out = self._empty(action_out, self.n, torch.uint8)
            logp_out = self._empty(logp_out, self.n, torch.float32)
            _native.check(self.L.tarok_sample_policy(self._h, self._p(logits), self._p(obs_words), self._p(action_out),
                                                     self._p(logp_out), self._stream()))
        return action_out, logp_out

    def policy_random(self, obs=None):
        """Bot_igralec.igraj_karto on device (Igralec.py:158-159)."""
        words = self.obs_words if obs is None else obs.words
        with torch.cuda.device(self.device):
            _native.check(self.L.tarok_policy_random(self._h, self._p(words), self._p(self.action), self._stream()))
        return self.action

    def step_random(self, auto_reset=False, tricks=False, reward_ref=False):
        with torch.cuda.device(self.device):
            _native.check(self.L.tarok_step_random(self._h, self._p(self.action), self._p(self.reward), self._p(self.done),
                                                   self._p(self._trick_buf(tricks)), self._p(self.obs_words),
                                                   (K.AUTO_RESET if auto_reset else 0) | (K.REWARD_REF if reward_ref else 0),
                                                   self._stream()))
        return Obs(self.obs_words), self.reward, self.done

    def prefetch(self):
        """Fill every next-game line that reset() emptied (reset() calls it itself; afterwards the step
        launches keep the slots' seven dealt-ahead games full on their own: callers never need this)."""
        with torch.cuda.device(self.device):
            _native.check(self.L.tarok_prefetch(self._h, self._stream()))

    def _krog_bufs(self, cards):
        if getattr(self, "_kb_cards", 0) != cards:
            with torch.cuda.device(self.device):
                self._kb = dict(action=torch.full((cards, self.n), 255, dtype=torch.uint8, device=self.device),
                                reward=torch.zeros((cards, self.n, 4), dtype=torch.int16, device=self.device),
                                done=torch.zeros((cards, self.n), dtype=torch.uint8, device=self.device),
                                trick=torch.zeros((cards, self.n), dtype=torch.int16, device=self.device),
                                obs=torch.zeros((cards, self.n), dtype=torch.int64, device=self.device))
            self._kb_cards = cards
        return self._kb

    def krog_random(self, cards=4, auto_reset=False, reward_ref=False, tricks=True):
        """`cards` cards of every game in one launch, Bot policy in-kernel (cards=4: one trick =
        one pass of the reference's krog).  Returns dict of [cards,N] tensors: action, reward
        [cards,N,4] (valid where done), done, trick, obs (observation words); also updates
        self.obs_words to the last row.  tricks=False: no per-trick rows (trick_out = NULL: the
        set of outputs tarok_run_random asks for, i.e. the card loop the bench times)."""
        kb = self._krog_bufs(cards)
        with torch.cuda.device(self.device):
            _native.check(self.L.tarok_krog_random(self._h, int(cards), self.n, self._p(kb["action"]), self._p(kb["reward"]),
                                                   self._p(kb["done"]), self._p(kb["trick"]) if tricks else None, self._p(kb["obs"]),
                                                   (K.AUTO_RESET if auto_reset else 0) | (K.REWARD_REF if reward_ref else 0),
                                                   self._stream()))
            self.obs_words.copy_(kb["obs"][cards - 1])
        return kb

    def run_random(self, n_steps, fused=False, graph_chunk=0, auto_reset=True, prefetch_every=0, cards_per_launch=None, done_rows=True):
        """n_steps lock-steps of the random policy launched from C (optionally graph-replayed).
        cards_per_launch: 0 = policy + step kernels, 1 = fused one-card kernel, >= 2 = that many
        cards per launch (tarok_krog_random); default from `fused`.  done_rows=False (one-card modes): done_out = NULL —
        a consumer reads "finished by this step" off bit 62 of the observation word instead of a byte row."""
        cards = (1 if fused else 0) if cards_per_launch is None else int(cards_per_launch)
        with torch.cuda.device(self.device):
            if cards >= 2:
                kb = self._krog_bufs(cards)
                _native.check(self.L.tarok_run_random(self._h, int(n_steps), cards, int(graph_chunk), int(prefetch_every),
                                                      self._p(kb["action"]), self._p(kb["reward"]), self._p(kb["done"]),
                                                      self._p(kb["obs"]), K.AUTO_RESET if auto_reset else 0, self._stream()))
                self.obs_words.copy_(kb["obs"][cards - 1])
            else:
                _native.check(self.L.tarok_run_random(self._h, int(n_steps), cards, int(graph_chunk), int(prefetch_every),
                                                      self._p(self.action), self._p(self.reward), self._p(self.done) if done_rows else None,
                                                      self._p(self.obs_words), K.AUTO_RESET if auto_reset else 0,
                                                      self._stream()))

    def rollout_random(self, episode=0, trace=False):
        """Whole random-policy games in one launch.  Returns dict of device tensors:
        scores [N,4] i16, nsteps [N] i16 and, with trace, step-major seats/masks/actions [48,N]."""
        n = self.n
        with torch.cuda.device(self.device):
            out = dict(scores=torch.empty((n, 4), dtype=torch.int16, device=self.device),
                       nsteps=torch.empty(n, dtype=torch.int16, device=self.device))
            if trace:
                out["seats"] = torch.empty((48, n), dtype=torch.int8, device=self.device)
                out["masks"] = torch.empty((48, n), dtype=torch.int64, device=self.device)
                out["actions"] = torch.empty((48, n), dtype=torch.uint8, device=self.device)
            _native.check(self.L.tarok_rollout_random(self._h, int(episode), self._p(out["scores"]), self._p(out["nsteps"]),
                                                      self._p(out.get("seats")), self._p(out.get("masks")),
                                                      self._p(out.get("actions")), self._stream()))
        return out

    def _cards(self, worlds, samples, salt, seats, seats_per_game, sum_out, action_out, voids=False, hidden=False, words=None):
        """The one card launch under the Bot-played playout_cards* methods (`samples` playouts per card and world): picks the
        native entry point of the world kind — worlds None: open hands; voids / hidden True: the env's own words, written into
        the caller's `words` tensor (None: a new one); a tensor or an array in their place: the words themselves, which need
        no history.  Returns (sum_out, action_out), allocated where None."""
        kind, words = TarokVecEnv._world_words(self, worlds is not None, voids, hidden, words)
        words = words()
        name = "tarok_playout_cards" + ("" if kind == "open" else "_" + kind)
        with torch.cuda.device(self.device):
            sum_out, action_out = TarokVecEnv._card_outputs(self, sum_out, action_out)
            _native.check(getattr(self.L, name)(self._h, *[int(c) for c in (worlds, samples) if c is not None], _salt(salt),
                                                int(seats), self._p(self._seat_sets(seats_per_game)), *([] if words is None else [self._p(words)]),
                                                self._p(sum_out), self._p(action_out), self._stream()))
        return sum_out, action_out

    def _net_cards(self, name, order, sizes, given, scratch, weights, net_seats, depth, value_scale, voids, hidden, words, salt, seats,
                   seats_per_game, sum_out, action_out, count_out=False, opponent=False, opp_rel=0):
        """The one card launch under the five playout_cards_net* methods.  name: the native entry point ({kind}: "", "_voids" or
        "_hidden", for the entries that have the world kind in their name); order: its arguments between the env and the
        scratch, as the names of their groups — sizes (`sizes` as ints: worlds, samples), sets (salt, seats, the per-game
        sets), kind (the kind's number and the words), words (the words alone, where there are any), net_seats, value (depth,
        value_scale), nets (the six pointers of `weights`; then, with opponent other than False, the six of `opponent` — six
        NULLs for None, which opp_rel 0 allows) and whatever `given` holds (roles, schedule, modes).  scratch: a call that makes
        the launch's scratch tensor; count_out other than False: the launch writes a count per card.  voids / hidden / words:
        as in _world_words.  Every refusal comes before the first launch.  Returns the outputs, allocated where None."""
        kind, words = TarokVecEnv._world_words(self, True, voids, hidden, words)
        net_seats, depth, value_scale, nets = TarokVecEnv._net_args(self, weights, net_seats, depth, value_scale)
        if opponent is not False:
            if opponent is None and opp_rel:
                raise ValueError("opp_rel seats the opponent's network: give its six tensors")
            nets = nets + ([None] * 6 if opponent is None else [self._p(t) for t in self.check_mlp_weights(opponent)])
        scratch = scratch()
        words = words()
        with torch.cuda.device(self.device):
            outs = TarokVecEnv._card_outputs(self, sum_out, action_out, count_out)
            groups = dict(given, sizes=[int(c) for c in sizes], sets=[_salt(salt), int(seats), self._p(self._seat_sets(seats_per_game))],
                          kind=[P.WORLDS.index(kind), self._p(words)], words=[] if words is None else [self._p(words)],
                          net_seats=[net_seats], value=[depth, value_scale], nets=nets)
            _native.check(getattr(self.L, name.format(kind="" if kind == "det" else "_" + kind))(
                self._h, *[x for group in order.split() for x in groups[group]], self._p(scratch), scratch.numel(),
                *[self._p(t) for t in outs], self._stream()))
        return tuple(outs)

    def _world_words(self, fair, voids, hidden, words):
        """(kind, words) of a card launch, `words` a call that makes its per-game words tensor (None for a kind without),
        so that every refusal comes before the first launch.  fair False: "open", the true hands.  voids / hidden True: the
        env's own words — which need the play history — written into the caller's `words` tensor (None: a new one); a
        tensor or an array in their place: the words themselves, which need no history."""
        is_words = lambda x: x is not None and not isinstance(x, (bool, int))          # a tensor or an array
        want_v, want_h = is_words(voids) or bool(voids), is_words(hidden) or bool(hidden)
        P.one_world_kind(want_v, want_h)
        kind = "open" if not fair else "voids" if want_v else "hidden" if want_h else "det"
        if kind not in P.WORDS_DTYPE:
            return kind, lambda: None
        given = voids if want_v else hidden
        if is_words(given):
            return kind, lambda: self._dev(given, P.WORDS_DTYPE[kind], (self.n,))
        if not self.history:
            raise ValueError("%s=True goes with the play history: TarokVecEnv(history=True)" % kind)
        return kind, lambda: self._dev((self.shown_voids if want_v else self.played_cards)(words), P.WORDS_DTYPE[kind], (self.n,))

    def _card_outputs(self, sum_out, action_out, count_out=False):
        """A card launch's outputs — sum [N,12,4] int32, count [N,12] int32 unless False, action [N] uint8 — each the
        caller's, or where it gave None a new tensor."""
        counts = [] if count_out is False else [self._empty(count_out, (self.n, K.PLAYOUT_RANKS), torch.int32)]
        return [self._empty(sum_out, (self.n, K.PLAYOUT_RANKS, 4), torch.int32)] + counts + [self._empty(action_out, self.n, torch.uint8)]

    def _exchange_outputs(self, discard_sets, sum_out, choice_out, discards_out):
        """An exchange launch's outputs (sum [N, 6 * discard_sets, 4] int32, choice [N] int8, discards [N,3] uint8)."""
        return (self._empty(sum_out, (self.n, 6 * int(discard_sets), 4), torch.int32), self._empty(choice_out, self.n, torch.int8),
                self._empty(discards_out, (self.n, 3), torch.uint8))

    def _net_args(self, weights, net_seats, depth, value_scale, max_depth=K.PLAYOUT_MAX_DEPTH):
        """What the net-played launches check and pass alike: (net_seats in 0..15, depth as the ABI's list and halving
        entries take it — None becomes 0, to the last card; else checked within 1..max_depth with its value_scale —,
        value_scale, the six weights' pointers)."""
        depth, value_scale = TarokVecEnv._list_value(net_seats, depth, value_scale, max_depth)
        return int(net_seats), depth, value_scale, [self._p(t) for t in self.check_mlp_weights(weights)]

    @staticmethod
    def _list_value(net_seats, depth, value_scale, max_depth=K.PLAYOUT_FRONT_MAX_DEPTH):
        """_net_args' checks, which read nothing of an env -> (depth, value_scale) as the ABI takes them (depth 0: to the end)."""
        if not 0 <= int(net_seats) <= 15:
            raise ValueError("net_seats: a 4-bit seat set, 0..15")
        if depth is not None:
            P.check_depth(depth, value_scale, max_depth=max_depth)
        return (0 if depth is None else int(depth)), float(value_scale)

    def playout_cards_fair(self, worlds, samples, *, voids=False, hidden=False, words=None, salt=0, seats=15, seats_per_game=None,
                           sum_out=None, action_out=None):
        """The card launch a player's settings name: worlds None / 0 -> playout_cards (open hands); voids=True ->
        playout_cards_voids on shown_voids(words); hidden=True -> playout_cards_hidden on played_cards(words); otherwise
        playout_cards_det.  words: the caller's scratch tensor for the voids / played words ([N] int32 / int64; None: a
        new one per call), so that a captured rollout allocates nothing.  Everything else as for the launch chosen."""
        return self._cards(worlds or None, samples, salt, seats, seats_per_game, sum_out, action_out, bool(voids), bool(hidden), words)

    def playout_cards(self, samples, salt=0, seats=15, seats_per_game=None, sum_out=None, action_out=None):
        """Open-hand Monte-Carlo value of every legal card of the seat to move (tarok_playout_cards): each legal card is
        played and the game finished `samples` times by the Bot, from the env's current positions.  The playouts see the
        TRUE hidden hands (perfect information): an upper-side yardstick and a teacher signal, not a fair player.
        The fair sibling is playout_cards_det.
        Returns (sum [N,12,4] int32 — row j: the four final scores summed over the playouts of the j-th lowest legal card,
        zero rows beyond the legal cards and for games that do not take part — and action [N] uint8: the first card at
        the maximum of the mover's sums, the Bot's card where the mover is outside `seats` / `seats_per_game` (as in
        policy_step), 255 where nothing is to be played).  Read-only on the env; `salt` varies the playouts' draws."""
        return self._cards(None, samples, salt, seats, seats_per_game, sum_out, action_out)

    def playout_cards_det(self, worlds, samples, salt=0, seats=15, seats_per_game=None, sum_out=None, action_out=None):
        """Determinized Monte-Carlo value of every legal card of the seat to move (tarok_playout_cards_det): the FAIR
        sibling of playout_cards.  The cards the mover cannot see are re-dealt `worlds` times (1..64) among the other
        seats, hand sizes kept, and every legal card is played out `samples` times by the Bot in every world, so the sums
        are over worlds * samples playouts (playout_values' divisor) and depend on the mover's information set alone:
        its hand, the table, the won piles, the talon ids, the contract, the declarer and the called suit.  Where a
        called king is among the unseen cards the world's team is the declarer and whoever was dealt it.
        Outputs, `seats` / `seats_per_game`, `salt` and the read-only contract: as for playout_cards."""
        return self._cards(worlds, samples, salt, seats, seats_per_game, sum_out, action_out)

    def playout_cards_halving(self, round_worlds, samples=1, *, voids=False, hidden=False, words=None, salt=0, seats=15, seats_per_game=None,
                              sum_out=None, count_out=None, action_out=None):
        """playout_cards_fair with sequential halving (tarok_playout_cards_halving), in one launch: round r plays the cards
        still alive `samples` times in each of round_worlds[r] fresh worlds (1..4 rounds, sum(round_worlds) <= 64), and
        after every round but the last the better half by the mover's sum stays alive, ties to the lower rank.  voids /
        hidden / words: the worlds' kind and the caller's scratch tensor for its words, as in playout_cards_fair; the worlds
        and the playouts' keys are that launch's, so round_worlds=(W,) gives its bytes.
        Returns (sum [N,12,4] int32, count [N,12] int32 — the playouts behind every row, 0 beyond the legal cards and for
        games that do not take part —, action [N] uint8: the first card at the maximum among the cards alive at the end)."""
        schedule = P.check_halving(round_worlds)
        kind, words = TarokVecEnv._world_words(self, True, voids, hidden, words)
        words = words()
        with torch.cuda.device(self.device):
            sum_out, count_out, action_out = TarokVecEnv._card_outputs(self, sum_out, action_out, count_out)
            _native.check(self.L.tarok_playout_cards_halving(self._h, P.WORLDS.index(kind), self._p(words), len(schedule),
                                                             (C.c_int * len(schedule))(*schedule), int(samples), _salt(salt),
                                                             int(seats), self._p(self._seat_sets(seats_per_game)), self._p(sum_out),
                                                             self._p(count_out), self._p(action_out), self._stream()))
        return sum_out, count_out, action_out

    def playout_net_halving_scratch(self, round_worlds):
        """The scratch tensor of playout_cards_net_halving at a schedule (uint8, tarok_playout_net_halving_scratch_bytes: the
        largest round's item arrays at its bound, the per-game words, the running sums and counts, the scan's partials), cached
        on the env per schedule — the size depends on no world kind —: a caller that captures the launch asks for it BEFORE
        the capture."""
        schedule = P.check_halving(round_worlds)
        return self._scratch(("cards_halving", schedule), self.L.tarok_playout_net_halving_scratch_bytes, len(schedule),
                             (C.c_int * len(schedule))(*schedule))

    def playout_cards_net_halving(self, weights, round_worlds, net_seats=15, voids=False, hidden=False, words=None, depth=None,
                                  value_scale=70.0, salt=0, seats=15, seats_per_game=None, scratch=None, sum_out=None, count_out=None,
                                  action_out=None):
        """playout_cards_net / playout_cards_net_value with sequential halving on a compacted item list
        (tarok_playout_cards_net_halving): round r plays the cards still alive once in each of round_worlds[r] fresh worlds,
        the playouts played by `weights` on the seats of net_seats and by the Bot on the others, and after every round but
        the last the better half by the mover's sum stays alive, ties to the lower rank.  A round's items are packed without
        gaps, so its forward rows are its alive cards' alone; round_worlds=(W,) is playout_cards_net(weights, W) to the byte,
        with no dead rows.  voids / hidden / words: the worlds' kind and the caller's scratch tensor for its words, as in
        playout_cards_halving; depth / value_scale: playout_cards_net_value's stop (None: to the last card).  scratch: the
        caller's uint8 tensor of at least playout_net_halving_scratch(round_worlds).numel() bytes (None: that cached one).
        Returns (sum [N,12,4] int32, count [N,12] int32 — the worlds behind every row —, action [N] uint8: the first card
        at the maximum among the cards alive at the end)."""
        schedule = P.check_halving(round_worlds)
        return TarokVecEnv._net_cards(self, "tarok_playout_cards_net_halving", "kind schedule sets net_seats nets value", (),
                                      dict(schedule=[len(schedule), (C.c_int * len(schedule))(*schedule)]),
                                      lambda: self.playout_net_halving_scratch(schedule) if scratch is None else scratch, weights, net_seats,
                                      depth, value_scale, voids, hidden, words, salt, seats, seats_per_game, sum_out, action_out, count_out)

    def playout_net_scratch(self, worlds):
        """The scratch tensor of playout_cards_net at `worlds` (uint8, tarok_playout_net_scratch bytes), cached on the env
        per `worlds`: a caller that captures the launch into a graph asks for it BEFORE the capture."""
        worlds, = _sizes(worlds=worlds)
        return self._scratch(("cards", worlds), self.L.tarok_playout_net_scratch, worlds)

    def playout_cards_net(self, weights, worlds, net_seats=15, salt=0, seats=15, seats_per_game=None, sum_out=None, action_out=None,
                          voids=False, hidden=False, words=None):
        """playout_cards_det whose playouts are played by a policy network (tarok_playout_cards_net): one playout per
        (legal card, world); after the candidate card the seats of `net_seats` (a 4-bit set of absolute seats) play the
        GREEDY card of `weights` (policy_mlp's six tensors, read when the launch runs) on the playout's own position,
        the other seats the Bot's card.  The sums are over `worlds` playouts (playout_values' divisor).  net_seats=15:
        the learned policy with one ply of search on top; net_seats=0: playout_cards_det(worlds, 1) to the byte; one
        seat: a best response to a table of Bots.  Worlds, outputs, `seats` / `seats_per_game`, `salt` and the
        read-only contract: as for playout_cards_det.  The scratch is playout_net_scratch(worlds).
        voids=True: the worlds honour shown voids (tarok_playout_cards_net_voids on shown_voids(words)), so the network
        never plays from a hand the table knows to be impossible; hidden=True: the worlds also re-deal Klop's face-down
        talon and the declarer's discards (tarok_playout_cards_net_hidden on played_cards(words)).  Either needs
        TarokVecEnv(history=True); a tensor in their place ([N] int32 / int64) is taken as the words themselves, as
        playout_cards_voids(voids=...) takes them, and needs no history.  words: the caller's scratch tensor for the
        env's own words (None: a new one per call), so that a captured launch allocates nothing.  Not both: the two
        kinds do not compose.  The defaults issue tarok_playout_cards_net."""
        return TarokVecEnv.playout_cards_net_value(self, weights, worlds, None, 0.0, net_seats, salt, seats, seats_per_game, sum_out, action_out,
                                                   voids, hidden, words)

    def playout_cards_net_value(self, weights, worlds, depth, value_scale=70.0, net_seats=15, salt=0, seats=15, seats_per_game=None,
                                sum_out=None, action_out=None, voids=False, hidden=False, words=None):
        """playout_cards_net whose playouts stop at the VIEWER's `depth`-th next decision (tarok_playout_cards_net_value;
        the viewer is the seat to move, the seat the playouts are for): there the value head of `weights` (output 54 of
        policy_mlp's forward on the stop position's own features, whether or not the viewer is in net_seats) times
        `value_scale`, rounded half-even into int16 range, is the viewer's result and the other three columns get 0; a
        playout whose game ends first keeps its true scores.  Only the viewer's column of the sums is meaningful; the card
        rule reads no other.  depth: 1..12 — depth 1 plays at most 6 cards per playout where a fresh deal takes 47; depth
        12 never stops and gives playout_cards_net's bytes.  value_scale: points per unit of the value head (a learner
        trained on returns * reward_scale wants 1 / reward_scale; 70 is SelfPlay's default reward_scale inverted).
        Everything else — worlds, voids= / hidden= / words=, the scratch, the outputs — is playout_cards_net's; depth=None
        IS playout_cards_net."""
        if depth is not None:
            P.check_depth(depth, value_scale)         # (before anything of the env is read)
        name, order = ("tarok_playout_cards_net{kind}", "sizes sets words net_seats nets") if depth is None else \
            ("tarok_playout_cards_net_value", "sizes sets kind net_seats value nets")
        return TarokVecEnv._net_cards(self, name, order, (worlds,), {}, lambda: self.playout_net_scratch(worlds), weights, net_seats, depth,
                                      value_scale, voids, hidden, words, salt, seats, seats_per_game, sum_out, action_out)

    def playout_cards_net_versus(self, weights, opponent, worlds, own_rel=1, opp_rel=14, depth=None, value_scale=70.0, voids=False,
                                 hidden=False, words=None, halving=None, salt=0, seats=15, seats_per_game=None, sum_out=None,
                                 action_out=None, count_out=None):
        """playout_cards_net / playout_cards_net_value whose playouts seat TWO networks relative to each game's VIEWER — the
        seat to move, the seat the playouts are for (tarok_playout_cards_net_versus).  own_rel / opp_rel: two
        disjoint 4-bit sets over the relative seats r = (seat - viewer) & 3 (bit 0: the viewer itself); after the candidate
        card the seats of own_rel play the greedy card of `weights`, those of opp_rel the greedy card of `opponent` (both
        policy_mlp's six tensors, read when the launch runs), the rest the Bot's card.  The defaults (1, 14): `weights` plays
        the viewer and `opponent` the table — the playouts of a best response to `opponent`, one launch for every game's own
        viewer.  (15, 0) is playout_cards_net(weights, worlds) to the byte, (0, 15) the same on `opponent`, (0, 0)
        playout_cards_det(worlds, 1); opponent may be None where opp_rel is 0.  depth / value_scale: playout_cards_net_value's
        stop (None: to the last card), with the value head of the VIEWER'S OWN network — `opponent` if opp_rel holds bit 0,
        else `weights`.  voids / hidden / words: the worlds' kind, as in playout_cards_net.  Returns (sum, action).
        halving=(w0, w1, ..): the worlds are spent by sequential halving on a compacted item list
        (tarok_playout_cards_net_versus_halving; `worlds` None or their sum), as in playout_cards_net_halving; returns (sum,
        count, action), and count_out is taken.  The scratch is playout_net_scratch(worlds) or
        playout_net_halving_scratch(halving)."""
        own_rel, opp_rel = P.check_versus((own_rel, opp_rel), P.spelling(net_versus="(own_rel, opp_rel)"))
        schedule = None if halving is None else P.check_halving(halving)
        if schedule is not None and worlds and int(worlds) != sum(schedule):
            raise ValueError("halving= names the worlds of every round: worlds is optional and must be their sum")
        if schedule is None and count_out is not None:
            raise ValueError("count_out holds the worlds behind every row of a halving launch: it goes with halving=")
        roles = dict(roles=[own_rel, opp_rel])
        if schedule is None:
            return TarokVecEnv._net_cards(self, "tarok_playout_cards_net_versus", "sizes sets kind roles value nets", (worlds,), roles,
                                          lambda: self.playout_net_scratch(worlds), weights, 0, depth, value_scale, voids, hidden, words, salt,
                                          seats, seats_per_game, sum_out, action_out, opponent=opponent, opp_rel=opp_rel)
        return TarokVecEnv._net_cards(self, "tarok_playout_cards_net_versus_halving", "kind schedule sets roles nets value", (),
                                      dict(roles, schedule=[len(schedule), (C.c_int * len(schedule))(*schedule)]),
                                      lambda: self.playout_net_halving_scratch(schedule), weights, 0, depth, value_scale, voids, hidden, words,
                                      salt, seats, seats_per_game, sum_out, action_out, count_out, opponent, opp_rel)

    def playout_net_sampled_scratch(self, worlds, samples):
        """The scratch tensor of playout_cards_net_sampled at (worlds, samples) (uint8, tarok_playout_cards_net_sampled_scratch
        bytes: 48 per item), cached on the env per shape: a caller that captures the launch asks for it BEFORE the capture."""
        worlds, samples = _sizes(worlds=worlds, samples=samples)
        return self._scratch(("cards_sampled", worlds, samples), self.L.tarok_playout_cards_net_sampled_scratch, worlds, samples)

    def playout_cards_net_sampled(self, weights, opponent, worlds, samples, own_rel=15, opp_rel=0, temperature=1.0, epsilon=0.0,
                                  opp_temperature=None, opp_epsilon=None, depth=None, value_scale=70.0, voids=False, hidden=False,
                                  words=None, salt=0, seats=15, seats_per_game=None, sum_out=None, action_out=None):
        """playout_cards_net_versus whose networks play as they play AT THE TABLE, `samples` playouts per (legal card, world)
        (tarok_playout_cards_net_sampled).  The seats of own_rel play `weights` under the play mode (temperature,
        epsilon), those of opp_rel play `opponent` under (opp_temperature, opp_epsilon) — each None: `weights`' value —, the
        rest the Bot: set_play_mode's two numbers, with its checks — a draw from the softmax at the temperature (0: the greedy
        card), and with probability epsilon the Bot's card instead —, on the draws of the item's own key, so a second sample of
        a world is another playout.  The env's own play mode is neither read nor written.  All samples of a world start from
        the same dealt position; the sums are over worlds * samples playouts (playout_values' divisor).  samples = 1 at
        temperature 0 and epsilon 0 on both networks is playout_cards_net_versus to the byte; (0, 0), or epsilon 1 on both
        networks, is playout_cards_det / _voids / _hidden(worlds, samples).  opponent may be None where opp_rel is 0.  depth /
        value_scale, voids / hidden / words, seats / seats_per_game, salt and the outputs: as in playout_cards_net_versus; no
        halving form.  The scratch is playout_net_sampled_scratch(worlds, samples).  Returns (sum, action)."""
        own_rel, opp_rel = P.check_versus((own_rel, opp_rel), P.spelling(net_versus="(own_rel, opp_rel)"))
        modes = P.check_play_modes(temperature, epsilon, opp_temperature, opp_epsilon)
        return TarokVecEnv._net_cards(self, "tarok_playout_cards_net_sampled", "sizes sets kind roles value modes nets", (worlds, samples),
                                      dict(roles=[own_rel, opp_rel], modes=modes), lambda: self.playout_net_sampled_scratch(worlds, samples),
                                      weights, 0, depth, value_scale, voids, hidden, words, salt, seats, seats_per_game, sum_out, action_out,
                                      opponent=opponent, opp_rel=opp_rel)

    def playout_exchange(self, worlds, samples, discard_sets=4, salt=0, seats=15, seats_per_game=None, sum_out=None,
                         choice_out=None, discards_out=None):
        """The declarer's talon exchange valued by determinized playouts (tarok_playout_exchange), for the games that
        wait for it (reset(defer_exchange=True)) with their declarer in `seats` / `seats_per_game`.  Candidate (i, d):
        talon group i with the d-th of `discard_sets` (1..8) draws of the Bot's discard sampler; every candidate is
        played to the end `samples` times by the Bot in each of `worlds` (1..64) re-deals of the three hands the
        declarer cannot see.  Returns (sum [N, 6 * discard_sets, 4] int32 — row i * discard_sets + d, zero rows for
        groups the contract does not have and for games that do not take part —, choice [N] int8 and discards [N,3]
        uint8: the first candidate at the maximum of the declarer's sums; the Bot's own exchange where a game waits
        with its declarer outside the set; -1 and 255s elsewhere).  exchange(choice, discards) applies them — a mixed
        table in one call.  Read-only on the env; `salt` varies the draws."""
        with torch.cuda.device(self.device):
            sum_out, choice_out, discards_out = TarokVecEnv._exchange_outputs(self, discard_sets, sum_out, choice_out, discards_out)
            _native.check(self.L.tarok_playout_exchange(self._h, int(worlds), int(samples), int(discard_sets),
                                                        _salt(salt), int(seats),
                                                        self._p(self._seat_sets(seats_per_game)), self._p(sum_out),
                                                        self._p(choice_out), self._p(discards_out), self._stream()))
        return sum_out, choice_out, discards_out

    def playout_bids(self, episode, worlds, samples, contracts=K.BID_DEFAULT_CONTRACTS, deals=None, salt=0, seats=15,
                     seats_per_game=None, sum_out=None, pass_value=False):
        """Every bid of every seat valued by determinized playouts (tarok_playout_bids), BEFORE reset(): the game valued
        is the one reset(episode, deals) would deal.  For every viewer seat in `seats` / `seats_per_game` and each of
        `worlds` (1..64) re-deals of the 42 cards it does not hold, every option in `contracts` (bit code: Klop 0 ..
        Odprti_berac 9) — each of Tri / Dve / Ena with each of the four kings — is played to the end `samples` times by
        the Bot with the viewer as declarer.  Returns sum [N, 4, K.BID_ROWS] int32: the viewer's summed score per row
        (karte.bid_row), zeros for seats outside the set, options outside `contracts` and row 19.  bid_round() turns the
        sums into a contract, a declarer and a king.  Does not read or write the env's games; `salt` varies the draws.
        pass_value=True (tarok_playout_bids_pass): row K.BID_PASS_ROW also holds the viewer's summed score of PASSING, over
        the same worlds: three Bots bid with the viewer silent (seat 0 is left the forced Klop when all pass), and the game
        they arrive at is played out by the Bot.  Rows 0..18 are the same bytes either way."""
        deals = self._dev(deals, torch.uint8, (self.n, 54))
        launch = self.L.tarok_playout_bids_pass if pass_value else self.L.tarok_playout_bids
        with torch.cuda.device(self.device):
            sum_out = self._empty(sum_out, (self.n, 4, K.BID_ROWS), torch.int32)
            _native.check(launch(self._h, int(episode), self._p(deals), int(worlds), int(samples), int(contracts),
                                 _salt(salt), int(seats),
                                 self._p(self._seat_sets(seats_per_game)), self._p(sum_out), self._stream()))
        return sum_out

    def _scratch(self, key, size_fn, *sizes):
        """The cached scratch tensor of a launch that takes one: `key` names the launch and its shape in _net_scratch."""
        cache = self._net_scratch
        if key not in cache:
            size = int(size_fn(self._h, *sizes))
            if size < 0:
                _native.check(size)
            with torch.cuda.device(self.device):
                cache[key] = torch.empty(size, dtype=torch.uint8, device=self.device)
        return cache[key]

    def playout_exchange_net_scratch(self, worlds, discard_sets=4):
        """The scratch tensor of playout_exchange_net at (worlds, discard_sets) (uint8, tarok_playout_exchange_net_scratch
        bytes), cached on the env per shape: a caller that captures the launch asks for it BEFORE the capture."""
        worlds, discard_sets = _sizes(worlds=worlds, discard_sets=discard_sets)
        return self._scratch(("exchange", worlds, discard_sets), self.L.tarok_playout_exchange_net_scratch, worlds, discard_sets)

    def playout_exchange_net(self, weights, worlds, discard_sets=4, net_seats=15, salt=0, seats=15, seats_per_game=None, sum_out=None,
                             choice_out=None, discards_out=None):
        """playout_exchange whose playouts are played by a policy network (tarok_playout_exchange_net): one playout per
        (candidate, world), the seats of `net_seats` (a 4-bit set of absolute seats) playing the GREEDY card of `weights`
        (policy_mlp's six tensors, read when the launch runs), the other seats the Bot's card.  The sums are over `worlds`
        playouts.  net_seats=0: playout_exchange(worlds, 1, discard_sets) to the byte.  Candidates, worlds, the three
        outputs, `seats` / `seats_per_game`, `salt` and the read-only contract: as for playout_exchange.  The scratch is
        playout_exchange_net_scratch(worlds, discard_sets)."""
        return TarokVecEnv._exchange_net(self, "tarok_playout_exchange_net", weights, worlds, discard_sets, None, 0.0, net_seats, salt, seats, seats_per_game,
                                         sum_out, choice_out, discards_out)

    def _exchange_net(self, name, weights, worlds, discard_sets, depth, value_scale, net_seats, salt, seats, seats_per_game, sum_out,
                      choice_out, discards_out):
        """The call under playout_exchange_net, _net_value and _net_list.  name: the native function — the _list one takes
        (depth, value_scale) at any depth (0: to the last card) and has its own scratch; the dense _value one is only
        called with a depth."""
        net_seats, d, value_scale, w = TarokVecEnv._net_args(self, weights, net_seats, depth, value_scale, K.PLAYOUT_FRONT_MAX_DEPTH)
        is_list = name.endswith("_list")
        value = (d, value_scale) if is_list or depth is not None else ()
        scratch = (self.playout_exchange_net_list_scratch if is_list else self.playout_exchange_net_scratch)(worlds, discard_sets)
        with torch.cuda.device(self.device):
            sum_out, choice_out, discards_out = TarokVecEnv._exchange_outputs(self, discard_sets, sum_out, choice_out, discards_out)
            _native.check(getattr(self.L, name)(self._h, int(worlds), int(discard_sets), _salt(salt), int(seats),
                                                self._p(self._seat_sets(seats_per_game)), net_seats, *value, *w, self._p(scratch),
                                                scratch.numel(), self._p(sum_out), self._p(choice_out), self._p(discards_out),
                                                self._stream()))
        return sum_out, choice_out, discards_out

    def playout_exchange_net_value(self, weights, worlds, discard_sets, depth, value_scale=70.0, net_seats=15, salt=0, seats=15,
                                   seats_per_game=None, sum_out=None, choice_out=None, discards_out=None):
        """playout_exchange_net whose playouts stop at the DECLARER's `depth`-th decision (tarok_playout_exchange_net_value):
        there the value head of `weights` times `value_scale`, rounded half-even into int16 range, is the declarer's result
        and the other three columns get 0, as playout_cards_net_value stops a card's playouts; only the declarer's column of
        the sums is meaningful, and the choice reads no other.  depth: 1..13 — a candidate is a game at 0 cards played, so
        the declarer has 12 decisions ahead: 13 never stops and gives playout_exchange_net's bytes, 12 stops at the forced
        last card, 1 runs at most 4 card rounds.  At depth 1 with the declarer on lead nothing is played and a candidate's
        number is the same in every world.  Everything else, the scratch included, is playout_exchange_net's; depth=None IS
        playout_exchange_net."""
        return TarokVecEnv._exchange_net(self, "tarok_playout_exchange_net" + ("" if depth is None else "_value"), weights, worlds, discard_sets, depth, value_scale, net_seats, salt, seats, seats_per_game,
                                         sum_out, choice_out, discards_out)

    def playout_bids_net_scratch(self, worlds):
        """The scratch tensor of playout_bids_net at `worlds` (uint8, tarok_playout_bids_net_scratch bytes: 3,840 * worlds
        + 40 per game), cached on the env per `worlds`: a caller that captures the launch asks for it BEFORE the capture."""
        worlds, = _sizes(worlds=worlds)
        return self._scratch(("bids", worlds), self.L.tarok_playout_bids_net_scratch, worlds)

    def playout_bids_net(self, weights, episode, worlds, net_seats=15, contracts=K.BID_DEFAULT_CONTRACTS, deals=None, salt=0, seats=15,
                         seats_per_game=None, sum_out=None):
        """playout_bids whose playouts are played by a policy network (tarok_playout_bids_net): one playout per (viewer,
        option, world), the seats of `net_seats` (a 4-bit set of absolute seats) playing the GREEDY card of `weights`, the
        other seats the Bot's card; the exchange inside a playout stays the Bot's.  The sums are over `worlds` playouts.
        net_seats=0: playout_bids(episode, worlds, 1) to the byte.  Row K.BID_PASS_ROW is 0: the pass is not valued here.
        Everything else as for playout_bids.  The scratch is playout_bids_net_scratch(worlds); nothing is allocated by
        the launch itself."""
        return TarokVecEnv._bids_net(self, "tarok_playout_bids_net", weights, episode, worlds, None, 0.0, False, net_seats, contracts, deals, salt, seats,
                                     seats_per_game, sum_out)

    def _bids_net(self, name, weights, episode, worlds, depth, value_scale, pass_value, net_seats, contracts, deals, salt, seats,
                  seats_per_game, sum_out):
        """The call under playout_bids_net, _net_value and _net_list.  name: the native function — the _list one takes
        (depth, value_scale, pass_value) at any depth (0: to the last card) and has its own scratch; the dense _value one
        is only called with a depth."""
        net_seats, d, value_scale, w = TarokVecEnv._net_args(self, weights, net_seats, depth, value_scale, K.PLAYOUT_FRONT_MAX_DEPTH)
        is_list = name.endswith("_list")
        value = (d, value_scale, int(bool(pass_value))) if is_list or depth is not None else ()
        scratch = self.playout_bids_net_list_scratch(worlds, contracts, seats, seats_per_game is not None, pass_value) if is_list else \
            self.playout_bids_net_scratch(worlds)
        deals = self._dev(deals, torch.uint8, (self.n, 54))
        with torch.cuda.device(self.device):
            sum_out = self._empty(sum_out, (self.n, 4, K.BID_ROWS), torch.int32)
            _native.check(getattr(self.L, name)(self._h, int(episode), self._p(deals), int(worlds), int(contracts), _salt(salt),
                                                int(seats), self._p(self._seat_sets(seats_per_game)), net_seats, *value, *w,
                                                self._p(scratch), scratch.numel(), self._p(sum_out), self._stream()))
        return sum_out

    def playout_bids_net_value(self, weights, episode, worlds, depth, value_scale=70.0, pass_value=False, net_seats=15,
                               contracts=K.BID_DEFAULT_CONTRACTS, deals=None, salt=0, seats=15, seats_per_game=None, sum_out=None):
        """playout_bids_net whose playouts stop at the VIEWER's `depth`-th decision (tarok_playout_bids_net_value; the viewer
        is the seat whose row it is, in the Klop row too): there the value head of `weights` times `value_scale`, rounded
        half-even into int16 range, is the viewer's result, as playout_cards_net_value stops a card's playouts.  depth:
        1..13 — an option is a game at 0 cards played: 13 never stops and gives playout_bids_net's bytes, 12 stops at the
        forced last card, 1 runs at most 4 card rounds.  pass_value=True: row K.BID_PASS_ROW also holds the viewer's value
        of PASSING — playout_bids(pass_value=True)'s pass playout (three Bots bid with the viewer silent) at sample 0, played
        and stopped like every other row; bid_round(pass_value=True) takes the sums.  Without it row 19 is 0.  Everything
        else, the scratch included, is playout_bids_net's; depth=None IS playout_bids_net, where a pass is not valued."""
        if depth is None and pass_value:
            raise ValueError("pass_value=True needs a depth: the plain net launch does not value the pass")
        return TarokVecEnv._bids_net(self, "tarok_playout_bids_net" + ("" if depth is None else "_value"), weights, episode, worlds, depth, value_scale, pass_value, net_seats, contracts, deals, salt, seats,
                                     seats_per_game, sum_out)

    def playout_exchange_net_list_scratch(self, worlds, discard_sets=4):
        """The scratch tensor of playout_exchange_net_list at (worlds, discard_sets) (uint8,
        tarok_playout_exchange_net_list_scratch bytes: the dense launch's item arrays — the host cannot read the contracts,
        so they do not shrink — plus 8 bytes per (game, group), the scan's partials and the total word), cached on the env
        per shape: a caller that captures the launch asks for it BEFORE the capture."""
        worlds, discard_sets = _sizes(worlds=worlds, discard_sets=discard_sets)
        return self._scratch(("exchange_list", worlds, discard_sets), self.L.tarok_playout_exchange_net_list_scratch, worlds, discard_sets)

    def playout_exchange_net_list(self, weights, worlds, discard_sets=4, depth=None, value_scale=70.0, net_seats=15, salt=0, seats=15,
                                  seats_per_game=None, sum_out=None, choice_out=None, discards_out=None):
        """playout_exchange_net / playout_exchange_net_value on a compacted item list (tarok_playout_exchange_net_list): the
        same three outputs to the byte, for any weights, with the items of Klop games, of games that do not take part and of
        the groups a Tri or a Dve does not have left out of the play launch's forward rows.  depth=None or 13: to the last
        card; 1..12: playout_exchange_net_value's stop at value_scale.  The scratch is
        playout_exchange_net_list_scratch(worlds, discard_sets); the launch allocates nothing and reads nothing back."""
        return TarokVecEnv._exchange_net(self, "tarok_playout_exchange_net_list", weights, worlds, discard_sets, depth, value_scale, net_seats, salt, seats, seats_per_game,
                                         sum_out, choice_out, discards_out)

    def playout_bids_net_list_scratch(self, worlds, contracts=K.BID_DEFAULT_CONTRACTS, seats=15, per_game=False, pass_value=False):
        """The scratch tensor of playout_bids_net_list (uint8, tarok_playout_bids_net_list_scratch bytes): 48 bytes for every
        item the seat set can hold — games x viewers in `seats` (4 with per_game=True, a seats_per_game launch) x the rows of
        `contracts` (+ 1 with pass_value) x worlds — plus 72 bytes per game and the scan's words: 624 * worlds per game for
        one viewer at the default contracts, against playout_bids_net_scratch's 3,840 * worlds.  Cached on the env per
        shape: a caller that captures the launch asks for it BEFORE the capture."""
        (worlds, contracts), seats = _sizes(worlds=worlds, contracts=contracts), int(seats)
        if not 0 <= seats <= 15:
            raise ValueError("seats: a 4-bit seat set, 0..15")
        key = ("bids_list", worlds, contracts, 15 if per_game else seats, bool(per_game), bool(pass_value))
        return self._scratch(key, self.L.tarok_playout_bids_net_list_scratch, worlds, contracts, seats, int(bool(per_game)),
                             int(bool(pass_value)))

    def playout_bids_net_list(self, weights, episode, worlds, depth=None, value_scale=70.0, pass_value=False, net_seats=15,
                              contracts=K.BID_DEFAULT_CONTRACTS, deals=None, salt=0, seats=15, seats_per_game=None, sum_out=None):
        """playout_bids_net / playout_bids_net_value on a compacted item list (tarok_playout_bids_net_list): the same sums to
        the byte, for any weights, with the slots of rows outside `contracts`, of viewers outside the seat set and of
        invalid deal rows neither allocated nor run through the play launch's forward.  depth=None or 13: to the last card;
        1..12: playout_bids_net_value's stop at value_scale.  pass_value=True is taken at ANY depth: with depth=None it is
        playout_bids_net_value(depth=13, pass_value=True).  The scratch is playout_bids_net_list_scratch(worlds, contracts,
        seats, seats_per_game is not None, pass_value); the launch allocates nothing and reads nothing back."""
        return TarokVecEnv._bids_net(self, "tarok_playout_bids_net_list", weights, episode, worlds, depth, value_scale, pass_value, net_seats, contracts, deals, salt, seats,
                                     seats_per_game, sum_out)

    def playout_exchange_net_halving_scratch(self, round_worlds, discard_sets=4):
        """The scratch tensor of playout_exchange_net_halving at (schedule, discard_sets) (uint8,
        tarok_playout_exchange_net_halving_scratch_bytes: the largest round's item arrays at its bound, every row's running sums
        and count, 12 bytes per (game, group), the scan's partials and the total word), cached on the env per shape: a caller
        that captures the launch asks for it BEFORE the capture."""
        schedule, (discard_sets,) = P.check_halving(round_worlds, option="round_worlds"), _sizes(discard_sets=discard_sets)
        return self._scratch(("exchange_halving", schedule, discard_sets), self.L.tarok_playout_exchange_net_halving_scratch_bytes,
                             len(schedule), (C.c_int * len(schedule))(*schedule), discard_sets)

    def playout_exchange_net_halving(self, weights, round_worlds, discard_sets=4, depth=None, value_scale=70.0, net_seats=15, salt=0,
                                     seats=15, seats_per_game=None, scratch=None, sum_out=None, count_out=None, choice_out=None,
                                     discards_out=None):
        """playout_exchange_net_list with sequential halving over a game's candidates (tarok_playout_exchange_net_halving):
        round r plays the candidates still alive once in each of round_worlds[r] fresh worlds, and after every round but the
        last the better half by the declarer's sum stays alive, ties to the lower row.  round_worlds=(W,) is
        playout_exchange_net_list(weights, W) to the byte.  depth / value_scale / net_seats and everything else: the list
        launch's.  scratch: the caller's uint8 tensor of at least playout_exchange_net_halving_scratch(round_worlds,
        discard_sets).numel() bytes (None: that cached one).  Returns (sum [N, 6 * discard_sets, 4] int32, count [N, 6 *
        discard_sets] int32 — the worlds behind every row —, choice [N] int8 and discards [N,3] uint8: the first candidate at
        the maximum of the declarer's sums among the candidates alive at the end)."""
        schedule = P.check_halving(round_worlds, option="round_worlds")
        net_seats, d, value_scale, w = TarokVecEnv._net_args(self, weights, net_seats, depth, value_scale, K.PLAYOUT_FRONT_MAX_DEPTH)
        scratch = self.playout_exchange_net_halving_scratch(schedule, discard_sets) if scratch is None else scratch
        with torch.cuda.device(self.device):
            sum_out, choice_out, discards_out = TarokVecEnv._exchange_outputs(self, discard_sets, sum_out, choice_out, discards_out)
            count_out = self._empty(count_out, (self.n, 6 * int(discard_sets)), torch.int32)
            _native.check(self.L.tarok_playout_exchange_net_halving(
                self._h, len(schedule), (C.c_int * len(schedule))(*schedule), int(discard_sets), _salt(salt), int(seats),
                self._p(self._seat_sets(seats_per_game)), net_seats, d, value_scale, *w, self._p(scratch), scratch.numel(),
                self._p(sum_out), self._p(count_out), self._p(choice_out), self._p(discards_out), self._stream()))
        return sum_out, count_out, choice_out, discards_out

    def playout_bids_net_halving_scratch(self, round_worlds, contracts=K.BID_DEFAULT_CONTRACTS, seats=15, per_game=False, pass_value=False):
        """The scratch tensor of playout_bids_net_halving (uint8, tarok_playout_bids_net_halving_scratch_bytes: the largest
        round's item arrays at its bound, every row's running sum and count, the deal, 12 bytes per (game, viewer), the scan's
        partials and the total word), cached on the env per shape as playout_bids_net_list_scratch caches its own: a caller
        that captures the launch asks for it BEFORE the capture."""
        schedule, (contracts,), seats = P.check_halving(round_worlds, option="round_worlds"), _sizes(contracts=contracts), int(seats)
        if not 0 <= seats <= 15:
            raise ValueError("seats: a 4-bit seat set, 0..15")
        key = ("bids_halving", schedule, contracts, 15 if per_game else seats, bool(per_game), bool(pass_value))
        return self._scratch(key, self.L.tarok_playout_bids_net_halving_scratch_bytes, len(schedule), (C.c_int * len(schedule))(*schedule),
                             contracts, seats, int(bool(per_game)), int(bool(pass_value)))

    def playout_bids_net_halving(self, weights, episode, round_worlds, depth=None, value_scale=70.0, pass_value=False, net_seats=15,
                                 contracts=K.BID_DEFAULT_CONTRACTS, deals=None, salt=0, seats=15, seats_per_game=None, scratch=None,
                                 sum_out=None, count_out=None, value_out=None):
        """playout_bids_net_list with sequential halving over a viewer's rows (tarok_playout_bids_net_halving): round r plays
        the rows still alive once in each of round_worlds[r] fresh worlds, and after every round but the last the better half
        by the viewer's sum stays alive, ties to the lower row.  With pass_value=True row K.BID_PASS_ROW is not in the race: it
        is played in every round its viewer plays.  round_worlds=(W,) is playout_bids_net_list(weights, episode, W) to the
        byte.  Returns (sum [N,4,20] int32, count [N,4,20] int32 — the worlds behind every row —, value [N,4,20] int32: sum x W
        / count to the nearest integer, which bid_round takes as its sums at playouts = W = sum(round_worlds))."""
        schedule = P.check_halving(round_worlds, option="round_worlds")
        net_seats, d, value_scale, w = TarokVecEnv._net_args(self, weights, net_seats, depth, value_scale, K.PLAYOUT_FRONT_MAX_DEPTH)
        if scratch is None:
            scratch = self.playout_bids_net_halving_scratch(schedule, contracts, seats, seats_per_game is not None, pass_value)
        deals = self._dev(deals, torch.uint8, (self.n, 54))
        with torch.cuda.device(self.device):
            sum_out, count_out, value_out = (self._empty(t, (self.n, 4, K.BID_ROWS), torch.int32) for t in (sum_out, count_out, value_out))
            _native.check(self.L.tarok_playout_bids_net_halving(
                self._h, int(episode), self._p(deals), len(schedule), (C.c_int * len(schedule))(*schedule), int(contracts), _salt(salt),
                int(seats), self._p(self._seat_sets(seats_per_game)), net_seats, d, value_scale, int(bool(pass_value)), *w,
                self._p(scratch), scratch.numel(), self._p(sum_out), self._p(count_out), self._p(value_out), self._stream()))
        return sum_out, count_out, value_out

    def bid_round(self, episode, sums, playouts, threshold=0, contracts=K.BID_DEFAULT_CONTRACTS, seats=15, seats_per_game=None,
                  pass_value=False):
        """The bidding round of every game on the device (tarok_bid_round; Igra.licitacija's control flow): the seats of
        `seats` / `seats_per_game` answer from playout_bids()' sums — the best-valued contract that beats the standing
        bid, if its sum exceeds threshold * playouts (playouts = worlds * samples of the launch that made the sums) and,
        for the holder, the sum of standing — and the other seats as the Bot does.  Returns (contract, declarer,
        king_suit), three [N] int8 device tensors that reset(episode, deals, contract=, declarer=, king_suit=) takes
        unchanged.  seats=0 is the Bot's own round (K.MIX_BOT's contract, declarer and king); sums may then be None.
        pass_value=True (tarok_bid_round_pass): a seat's bar is the value of its own pass, sums[g, seat, K.BID_PASS_ROW] +
        threshold * playouts: `threshold` is then the margin, in points per game, a bid has to beat the pass by."""
        sums = self._dev(sums, torch.int32, (self.n, 4, K.BID_ROWS))
        launch = self.L.tarok_bid_round_pass if pass_value else self.L.tarok_bid_round
        with torch.cuda.device(self.device):
            out = [torch.empty(self.n, dtype=torch.int8, device=self.device) for _ in range(3)]
            _native.check(launch(self._h, int(episode), self._p(sums), int(playouts), int(threshold), int(contracts),
                                 int(seats), self._p(self._seat_sets(seats_per_game)), self._p(out[0]),
                                 self._p(out[1]), self._p(out[2]), self._stream()))
        return tuple(out)

    def bid_values(self, episode, weights, scale, contracts=K.BID_DEFAULT_CONTRACTS, deals=None, seats=15, seats_per_game=None,
                   value_out=None, raw=False, feature_words=False, pass_value=False):
        """The bidding head (tarok_bid_values): playout_bids()' array written by a network from the twelve cards of each
        hand, BEFORE reset(), for the game reset(episode, deals) would deal.  weights = (w1, b1, w2, b2, w3, b3) as
        policy_mlp takes them; the input row of seat v is the hand, the one-hot seat and the tarok / suit-length / king /
        trula features of include/tarok_env.h, and output o < 19 of the network is bid row o (karte.bid_row).  Returns
        value [N, 4, K.BID_ROWS] int32 = the outputs times `scale` (0 < scale <= 2**20), clamped to +-2**30 and rounded to
        even, with playout_bids()' zeros (seats outside `seats` / `seats_per_game`, options outside `contracts`, row 19,
        an invalid deal): bid_round(episode, value, playouts, ...) takes it as its sums.  raw=True also returns the
        unscaled float32 outputs [N, 4, K.BID_ROWS] (same zeros), feature_words=True the input rows as bits
        [N, 4, 4] int64 (expand_feature_words; every seat, in the set or not): (value, raw, feature_words), None for what
        was not asked for.  Does not read or write the env's games.
        pass_value=True (tarok_bid_values_pass): row K.BID_PASS_ROW of value and raw is output 19, the value of a pass,
        scaled, clamped and rounded as the other rows and whatever `contracts` holds; rows 0..18 are the same bytes."""
        w1, b1, w2, b2, w3, b3 = self.check_mlp_weights(weights)
        deals = self._dev(deals, torch.uint8, (self.n, 54))
        launch = self.L.tarok_bid_values_pass if pass_value else self.L.tarok_bid_values
        with torch.cuda.device(self.device):
            value_out = self._empty(value_out, (self.n, 4, K.BID_ROWS), torch.int32)
            raw_out = torch.empty((self.n, 4, K.BID_ROWS), dtype=torch.float32, device=self.device) if raw else None
            fw_out = torch.empty((self.n, 4, 4), dtype=torch.int64, device=self.device) if feature_words else None
            _native.check(launch(self._h, int(episode), self._p(deals), self._p(w1), self._p(b1), self._p(w2),
                                 self._p(b2), self._p(w3), self._p(b3), float(scale), int(contracts), int(seats),
                                 self._p(self._seat_sets(seats_per_game)), self._p(value_out), self._p(raw_out),
                                 self._p(fw_out), self._stream()))
        if not raw and not feature_words:
            return value_out
        return value_out, raw_out, fw_out

    def exchange_values(self, weights, seats=15, seats_per_game=None, raw=False, feature_words=False, choice_out=None,
                        discards_out=None):
        """The exchange head (tarok_exchange_values): playout_exchange()'s choice and discards from a network, for the
        games that wait for the exchange (reset(defer_exchange=True)) with their declarer in `seats` / `seats_per_game`.
        weights = (w1, b1, w2, b2, w3, b3) as policy_mlp takes them.  Row i < 8 of a game is "pick up talon group i" (the
        features of include/tarok_env.h: what the declarer would hold, what stays in the talon, the group, the called
        king's whereabouts, the shape of the new hand); output 54 of the network is the group's value, output c < 54 the
        discard score of card c.  Returns choice [N] int8 and discards [N, 3] uint8 as playout_exchange() does — the
        group of the largest value and its best-scored discardable cards; the Bot's own exchange where a game waits with
        its declarer outside the set; -1 and 255s elsewhere — so exchange(choice, discards) applies them.  raw=True also
        returns the float32 outputs [N, 8, 64] (zeros for rows that are not live), feature_words=True the input rows as
        bits [N, 8, 4] int64 (expand_feature_words; zeros where not live): (choice, discards, raw, feature_words), None
        for what was not asked for.  Read-only on the env."""
        w1, b1, w2, b2, w3, b3 = self.check_mlp_weights(weights)
        with torch.cuda.device(self.device):
            choice_out = self._empty(choice_out, self.n, torch.int8)
            discards_out = self._empty(discards_out, (self.n, 3), torch.uint8)
            raw_out = torch.empty((self.n, 8, 64), dtype=torch.float32, device=self.device) if raw else None
            fw_out = torch.empty((self.n, 8, 4), dtype=torch.int64, device=self.device) if feature_words else None
            _native.check(self.L.tarok_exchange_values(self._h, self._p(w1), self._p(b1), self._p(w2), self._p(b2), self._p(w3),
                                                       self._p(b3), int(seats), self._p(self._seat_sets(seats_per_game)),
                                                       self._p(raw_out), self._p(choice_out), self._p(discards_out),
                                                       self._p(fw_out), self._stream()))
        if not raw and not feature_words:
            return choice_out, discards_out
        return choice_out, discards_out, raw_out, fw_out

    def front_lines_scratch(self):
        """The scratch tensor of front_lines (uint8, tarok_front_lines_scratch_bytes), cached on the env: a caller that
        captures the call asks for it BEFORE the capture."""
        return self._scratch(("front_lines",), lambda h, n: self.L.tarok_front_lines_scratch_bytes(n), self.n)

    def front_lines(self, bid=None, exchange=None, scale=None, contracts=K.BID_DEFAULT_CONTRACTS, margin=0, pass_value=False, seats=15,
                    seats_per_game=None, count_out=None, hist_out=None, playouts=1):
        """The bid and exchange heads on the games auto-reset has dealt ahead (tarok_front_lines): every next-game line
        that is valid now and has not been fronted yet is decided again in place — the deal of its key, the bidding round
        of bid_round(pass_value=) with the seats of `seats` / `seats_per_game` answering from bid_values(bid, scale,
        contracts)' values at threshold `margin` and `playouts` (BidLearner.round's: scale = learner.scale, playouts =
        learner.playouts_equiv), the game set up, and exchange_values(exchange)' choice and discards applied where the
        declarer is in the set (the Bot's exchange elsewhere) — and marked.  bid, exchange: six tensors each as policy_mlp
        takes them, read when the launches run; one of the two may be None (bid=None keeps the env's own contracts, and
        only then may the env's mix be another than K.MIX_BOT).  With the empty set the lines keep their bytes and gain
        the mark.  Stream-ordered and capturable between two step launches; lines on a pending refill list are left to
        the next call.  count_out [1] int64 / hist_out [10] int64 device tensors, if given, receive the number of lines
        fronted by this call and their contracts.  Returns (count_out, hist_out)."""
        if bid is None and exchange is None:
            raise ValueError("front_lines: give bid= or exchange= (six tensors as policy_mlp takes them), or both")
        if not 0 <= int(seats) <= 15:
            raise ValueError("seats: a 4-bit seat set, 0..15")
        none = (None,) * 6
        b = none
        if bid is not None:
            if scale is None or not 0.0 < float(scale) <= 2.0 ** 20:
                raise ValueError("front_lines: bid= needs bid_values' scale, 0 < scale <= 2**20")
            if not 1 <= int(contracts) <= K.BID_ALL_CONTRACTS:
                raise ValueError("contracts: a bit set within 1..0x3FF")
            if int(playouts) < 1:
                raise ValueError("playouts: >= 1")
            if self.mix != K.MIX_BOT:
                raise ValueError("front_lines: bid= re-bids K.MIX_BOT's round: the env's mix must be K.MIX_BOT")
            b = self.check_mlp_weights(bid)
        x = none if exchange is None else self.check_mlp_weights(exchange)
        spg = self._seat_sets(seats_per_game)
        for name, t, k in (("count_out", count_out, 1), ("hist_out", hist_out, 10)):
            if t is not None and not (torch.is_tensor(t) and t.device == self.device and t.dtype == torch.int64 and t.is_contiguous()
                                      and t.numel() == k):
                raise ValueError("%s: a contiguous int64 tensor of %d on the env's device" % (name, k))
        scratch = self.front_lines_scratch()
        with torch.cuda.device(self.device):
            _native.check(self.L.tarok_front_lines(self._h, *[self._p(t) for t in b], float(scale) if bid is not None else 1.0,
                                                   int(playouts), int(margin), int(contracts), int(bool(pass_value)),
                                                   *[self._p(t) for t in x], int(seats), self._p(spg), self._p(scratch),
                                                   scratch.numel(), self._p(count_out), self._p(hist_out), self._stream()))
        return count_out, hist_out

    def get_lines(self, lanes=False):
        """The next-game lines (tarok_get_lines): a [N, K.GAMES_AHEAD, 6] uint64 numpy array — a line's four packed words,
        its key, and episode tag | front mark << 32.  lanes=True: (lines, lanes [10, N, K.GAMES_AHEAD] uint64), each line's
        game as state()'s ten lanes (meaningful where the tag is valid)."""
        with torch.cuda.device(self.device):
            out = torch.empty((self.n, K.GAMES_AHEAD, 6), dtype=torch.int64, device=self.device)
            lan = torch.empty((10, self.n, K.GAMES_AHEAD), dtype=torch.int64, device=self.device) if lanes else None
            _native.check(self.L.tarok_get_lines(self._h, self._p(out), self._p(lan), self._stream()))
        lines = out.cpu().numpy().view("uint64")
        return (lines, lan.cpu().numpy().view("uint64")) if lanes else lines

    def exchange_candidates(self, discard_sets=4, salt=0, seats=15, seats_per_game=None):
        """The cards playout_exchange()'s candidates laid down (tarok_exchange_candidates): [N, 6 * discard_sets, 3] uint8,
        row i * discard_sets + d the discards of candidate (i, d) of a launch with the same discard_sets, salt and seat set
        (255 beyond the group size; 255s for groups the contract does not have and games that do not take part).
        Read-only on the env."""
        with torch.cuda.device(self.device):
            out = torch.empty((self.n, 6 * int(discard_sets), 3), dtype=torch.uint8, device=self.device)
            _native.check(self.L.tarok_exchange_candidates(self._h, int(discard_sets), _salt(salt), int(seats),
                                                           self._p(self._seat_sets(seats_per_game)), self._p(out), self._stream()))
        return out

    def shown_voids(self, out=None):
        """[N] int32 device tensor (tarok_shown_voids; the bits of a u32): bit 5 * seat + class of a game's word is set
        iff the play so far has shown that seat to hold no card of that class (class = min(card >> 3, 4): the four suits,
        the taroks); 0 for a game that is not in play.  Needs TarokVecEnv(history=True).  Read-only, stream-ordered."""
        if not self.history:
            raise ValueError("shown_voids reads the play history: TarokVecEnv(history=True)")
        with torch.cuda.device(self.device):
            out = self._empty(out, self.n, torch.int32)
            _native.check(self.L.tarok_shown_voids(self._h, self._p(out), self._stream()))
        return out

    def playout_cards_voids(self, worlds, samples, salt=0, seats=15, seats_per_game=None, voids=None, sum_out=None, action_out=None):
        """playout_cards_det whose worlds honour shown voids (tarok_playout_cards_voids): every world is uniform over the
        re-deals that keep the hand sizes and give no other seat a card of a class `voids` marks it void in.
        voids: [N] int32 words as shown_voids() returns them (any words of the caller's are accepted; all zero gives
        playout_cards_det's bytes); None: shown_voids() of the current positions.  Needs TarokVecEnv(history=True).
        Everything else as for playout_cards_det; world w is another deal than there unless the game shows no void."""
        if not self.history:
            raise ValueError("playout_cards_voids goes with the play history: TarokVecEnv(history=True)")
        return self._cards(worlds, samples, salt, seats, seats_per_game, sum_out, action_out, voids=self.shown_voids() if voids is None else voids)

    def played_cards(self, out=None):
        """[N] int64 device tensor (tarok_played_cards; the bits of a u64): bit c of a game's word is set iff card c is in
        the play history of the slot's current game, the cards on the table included; 0 for a game that waits for the
        exchange or has just been re-dealt.  Needs TarokVecEnv(history=True).  Read-only, stream-ordered."""
        if not self.history:
            raise ValueError("played_cards reads the play history: TarokVecEnv(history=True)")
        with torch.cuda.device(self.device):
            out = self._empty(out, self.n, torch.int64)
            _native.check(self.L.tarok_played_cards(self._h, self._p(out), self._stream()))
        return out

    def playout_cards_hidden(self, worlds, samples, salt=0, seats=15, seats_per_game=None, played=None, sum_out=None, action_out=None):
        """playout_cards_det whose worlds also re-deal what only other seats have seen (tarok_playout_cards_hidden): in a
        Klop the face-down talon cards not yet given away, in Tri .. Solo_ena the declarer's discards when another seat
        is to move.  Where nothing more is hidden the bytes are playout_cards_det's.
        played: [N] int64 words as played_cards() returns them; None: played_cards() of the current positions.  Needs
        TarokVecEnv(history=True).  Everything else as for playout_cards_det."""
        if not self.history:
            raise ValueError("playout_cards_hidden goes with the play history: TarokVecEnv(history=True)")
        return self._cards(worlds, samples, salt, seats, seats_per_game, sum_out, action_out, hidden=self.played_cards() if played is None else played)

    def playout_targets(self, sums, obs_words, playouts, tau, seats=15, seats_per_game=None, target_out=None):
        """A playout launch's sums as a teacher's target rows (tarok_playout_targets): target [N,64] bf16, for a game with
        a teacher the softmax over its legal cards of (the mover's sum) / (playouts * tau) at the cards' columns (tau = 0:
        1.0 at the playout launch's card), 0 everywhere else; a zero row for a game without one.  sums [N,12,4] int32
        (playout_cards / playout_cards_det), obs_words [N] the observation words the playouts started from, playouts =
        samples (x worlds), seats / seats_per_game as given to the playout launch.  Stream-ordered; allocates nothing when
        target_out is given."""
        with torch.cuda.device(self.device):
            target_out = self._empty(target_out, (self.n, 64), torch.bfloat16)
            _native.check(self.L.tarok_playout_targets(self._h, self._p(sums), self._p(obs_words), int(playouts), float(tau), int(seats),
                                                       self._p(self._seat_sets(seats_per_game)), self._p(target_out), self._stream()))
        return target_out

    def playout_targets_counts(self, sums, counts, obs_words, tau, seats=15, seats_per_game=None, target_out=None):
        """playout_targets for sums with a count per card (tarok_playout_targets_counts): the softmax is over (the mover's
        sum) / (the card's count) / tau on the cards with a count, 0 on a card without playouts; tau = 0: 1.0 at the first
        card at the maximal mean among the cards of maximal count — on playout_cards_halving's (sum, count) that
        launch's card.  counts [N,12] int32.  Stream-ordered; allocates nothing when target_out is given."""
        with torch.cuda.device(self.device):
            target_out = self._empty(target_out, (self.n, 64), torch.bfloat16)
            _native.check(self.L.tarok_playout_targets_counts(self._h, self._p(sums), self._p(counts), self._p(obs_words), float(tau), int(seats),
                                                              self._p(self._seat_sets(seats_per_game)), self._p(target_out), self._stream()))
        return target_out

    def observe(self, out=None):
        """[N,256] bf16 features of the seat to move (include/tarok_env.h tarok_observe)."""
        with torch.cuda.device(self.device):
            out = self._empty(out, (self.n, 256), torch.bfloat16)
            _native.check(self.L.tarok_observe(self._h, self._p(out), self._stream()))
        return out

    def observe_ref(self, out=None, meta=None):
        """The reference's own observation layout for the seat to move (tarok_observe_ref;
        Igralec.py:453-533).  Returns (record [N, REF_RECORD_BYTES] u8, meta [N,4] i32 = T, type, rows
        used, seat); `ref_views` slices the record into the reference's tensors."""
        with torch.cuda.device(self.device):
            out = self._empty(out, (self.n, K.REF_RECORD_BYTES), torch.uint8)
            meta = self._empty(meta, (self.n, 4), torch.int32)
            _native.check(self.L.tarok_observe_ref(self._h, self._p(out), self._p(meta), self._stream()))
        return out, meta

    @staticmethod
    def ref_views(record):
        """[N, REF_RECORD_BYTES] record -> dict of views named as in Igralec.py:455-519."""
        n = record.shape[0]
        cut = lambda a, b: record[:, a:b]
        return {"input_layer_nasprotiki": cut(K.REF_OPP, K.REF_OWN).reshape(n, K.REF_ROWS, 3, 54),
                "roka_input": cut(K.REF_OWN, K.REF_TALON).reshape(n, K.REF_ROWS, 54),
                "talon_input": cut(K.REF_TALON, K.REF_KING).reshape(n, 6, 55),
                "talon_input_klop": cut(K.REF_TALON, K.REF_TALON + 54),
                "barva_kralja": cut(K.REF_KING, K.REF_INDEX), "index_tistega_ki_igra": cut(K.REF_INDEX, K.REF_DISCARDS),
                "zalozil": cut(K.REF_DISCARDS, K.REF_LEGAL), "mozne_vec": cut(K.REF_LEGAL, K.REF_LEGAL + 54)}

    def observe_exchange_ref(self, out=None):
        """menjaj_talon_v_vektor (Igralec.py:535-543) for the games waiting for the exchange:
        [N, REF_EXCHANGE_BYTES] u8 = roka 54 | talon (54,6) | igra 15 | pad."""
        with torch.cuda.device(self.device):
            out = self._empty(out, (self.n, K.REF_EXCHANGE_BYTES), torch.uint8)
            _native.check(self.L.tarok_observe_exchange_ref(self._h, self._p(out), self._stream()))
        return out

    def observe_hands_ref(self, out=None):
        """The bidding input (Igralec.py:278-281): [N,4,54] u8, every seat's hand one-hot."""
        with torch.cuda.device(self.device):
            out = self._empty(out, (self.n, 4, 54), torch.uint8)
            _native.check(self.L.tarok_observe_hands_ref(self._h, self._p(out), self._stream()))
        return out

    def get_history(self):
        """[48,N] u8 device tensor: card p of every slot's current game (TarokVecEnv(history=True))."""
        with torch.cuda.device(self.device):
            h = torch.empty((48, self.n), dtype=torch.uint8, device=self.device)
            _native.check(self.L.tarok_get_history(self._h, self._p(h), self._stream()))
        return h

    def set_history(self, hist):
        h = self._dev(hist, torch.uint8, (48, self.n))
        with torch.cuda.device(self.device):
            _native.check(self.L.tarok_set_history(self._h, self._p(h), self._stream()))

    @staticmethod
    def mfma_weight_order(weight):
        """torch.nn.Linear.weight [out, 256] -> the bf16 fragment order tarok_policy_mlp reads
        (include/tarok_env.h): [out/32, 16 k-steps, 2 halves, 32 rows, 8] flattened."""
        out = weight.shape[0]
        assert weight.shape[1] == 256 and out % 32 == 0
        return weight.detach().to(torch.bfloat16).view(out // 32, 32, 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous().view(out, 256)

    @staticmethod
    def check_mlp_weights(weights):
        """(w1, b1, w2, b2, w3, b3) as the policy kernels read them, or an AssertionError / ValueError."""
        w1, b1, w2, b2, w3, b3 = weights
        for w, shp in ((w1, (256, 256)), (w2, (256, 256)), (w3, (64, 256))):
            assert w.dtype == torch.bfloat16 and w.is_contiguous() and tuple(w.shape) == shp
        for b, k in ((b1, 256), (b2, 256), (b3, 64)):
            assert b.dtype == torch.float32 and b.is_contiguous() and tuple(b.shape) == (k,)
        return w1, b1, w2, b2, w3, b3

    def policy_mlp(self, weights, obs_words, action_out=None, logp_out=None, value_out=None, features_out=None,
                   feature_words_out=None):
        """Fused learned-policy step (tarok_policy_mlp).  weights = (w1, b1, w2, b2, w3, b3): w* bf16 in
        mfma_weight_order() ([256,256], [256,256], [64,256]), b* f32; returns (action u8 [N], logp f32 [N],
        value f32 [N]).  features_out [N,256] bf16 and/or feature_words_out [N,4] int64 (the same features
        as bits: expand_feature_words) receive the network input for the learner."""
        w1, b1, w2, b2, w3, b3 = self.check_mlp_weights(weights)
        with torch.cuda.device(self.device):
            action_out = self._empty(action_out, self.n, torch.uint8)
            logp_out = self._empty(logp_out, self.n, torch.float32)
            value_out = self._empty(value_out, self.n, torch.float32)
            _native.check(self.L.tarok_policy_mlp(self._h, self._p(w1), self._p(b1), self._p(w2), self._p(b2), self._p(w3),
                                                  self._p(b3), self._p(obs_words), self._p(action_out), self._p(logp_out),
                                                  self._p(value_out), self._p(features_out), self._p(feature_words_out),
                                                  self._stream()))
        return action_out, logp_out, value_out

    POOL_MAX = K.POOL_MAX
    POOL_SHAPES = ((256, 256), (256,), (256, 256), (256,), (64, 256), (64,))

    @staticmethod
    def check_pool_weights(pool):
        """Six stacked tensors (w1 [K,256,256], b1 [K,256], w2 [K,256,256], b2 [K,256], w3 [K,64,256], b3 [K,64]), entry k
        as check_mlp_weights takes one network, 1 <= K <= 64 — or a ValueError.  Returns (K, the six)."""
        if not isinstance(pool, (list, tuple)) or len(pool) != 6 or not all(torch.is_tensor(t) for t in pool):
            raise ValueError("opponent_pool: six stacked tensors (w1, b1, w2, b2, w3, b3), each with a leading K")
        k = pool[0].shape[0] if pool[0].dim() else 0
        if not 1 <= k <= TarokVecEnv.POOL_MAX:
            raise ValueError("opponent_pool: 1..%d networks, got %d" % (TarokVecEnv.POOL_MAX, k))
        for i, (t, shp) in enumerate(zip(pool, TarokVecEnv.POOL_SHAPES)):
            want = torch.float32 if i & 1 else torch.bfloat16
            if t.dtype != want or not t.is_contiguous() or tuple(t.shape) != (k,) + shp:
                raise ValueError("opponent_pool[%d]: a contiguous %s tensor %s, got %s %s" % (i, want, (k,) + shp, t.dtype, tuple(t.shape)))
        return k, tuple(pool)

    @staticmethod
    def stack_pool(weight_sets):
        """A list of weight sets (each six tensors as check_mlp_weights takes them) -> the six stacked tensors of an
        opponent pool, entry k = weight_sets[k] (new memory: the sets are copied)."""
        sets = [TarokVecEnv.check_mlp_weights(w) for w in weight_sets]
        if not 1 <= len(sets) <= TarokVecEnv.POOL_MAX:
            raise ValueError("stack_pool: 1..%d weight sets, got %d" % (TarokVecEnv.POOL_MAX, len(sets)))
        return tuple(torch.stack([s[i] for s in sets]).contiguous() for i in range(6))

    def _group_net(self, group_net):
        """group_net as tarok_policy_step_pool takes it: None, or a contiguous uint8 tensor [ceil(N / 256)] on the device."""
        g = group_net
        if g is not None and not (torch.is_tensor(g) and g.device == self.device and g.dtype == torch.uint8
                                  and g.is_contiguous() and tuple(g.shape) == ((self.n + 255) // 256,)):
            raise ValueError("group_net: a contiguous uint8 tensor [ceil(N / 256)] on the env's device")
        return g

    def policy_step(self, weights, obs_words, obs_out, action_out, logp_out=None, value_out=None, feature_words_out=None,
                    reward_out=None, done_out=None, auto_reset=True, seats=None, seats_per_game=None, tricks=None, opponent=None,
                    opponent_pool=None, group_net=None):
        """policy_mlp + step in one launch (tarok_policy_step): samples a card per game from the MLP
        policy on `obs_words` and plays it; obs_out receives the next observation words.
        seats (a 4-bit set, bit s: seat s plays the network) or seats_per_game ([N] uint8 device tensor of such sets):
        the mixed table of tarok_policy_step_seats — the other seats play the Bot's card (step_random's) with
        logp 0.  tricks: a [N] int16 device tensor that receives trick_out (see step()).
        opponent (six tensors like `weights`): a second network in the Bot's place (tarok_policy_step_versus) — the
        seats of the set play `weights`, the others `opponent`, each with its own card, logp and value; without
        seats / seats_per_game the set is 15.
        opponent_pool (six STACKED tensors, stack_pool()) instead of opponent: a pool of K frozen networks
        (tarok_policy_step_pool) — the other seats of step group g (slots 256 g .. 256 g + 255) play pool entry
        group_net[g] (a [ceil(N / 256)] uint8 device tensor; None: g % K); an index >= K is `weights` itself."""
        flags = K.AUTO_RESET if auto_reset else 0
        if opponent_pool is not None:
            if opponent is not None:
                raise ValueError("policy_step: opponent and opponent_pool exclude each other")
            k, pool = TarokVecEnv.check_pool_weights(opponent_pool)      # (before the env is touched)
            gn = self._group_net(group_net)
            with torch.cuda.device(self.device):
                _native.check(self.L.tarok_policy_step_pool(
                    self._h, 15 if seats is None else int(seats), self._p(self._seat_sets(seats_per_game)),
                    *[self._p(t) for t in self.check_mlp_weights(weights)], k, *[self._p(t) for t in pool], self._p(gn),
                    self._p(obs_words), self._p(action_out), self._p(logp_out), self._p(value_out), self._p(feature_words_out),
                    self._p(reward_out), self._p(done_out), self._p(tricks), self._p(obs_out), flags, self._stream()))
            return action_out
        if group_net is not None:
            raise ValueError("policy_step: group_net needs opponent_pool")
        plain =opponent is None and seats is None and seats_per_game is None
        sets = () if plain else (15 if seats is None else int(seats), self._p(self._seat_sets(seats_per_game)))
        nets = [weights] if opponent is None else [self.check_mlp_weights(weights), self.check_mlp_weights(opponent)]
        fn = self.L.tarok_policy_step if plain else self.L.tarok_policy_step_seats if opponent is None else self.L.tarok_policy_step_versus
        with torch.cuda.device(self.device):
            _native.check(fn(self._h, *sets, *[self._p(t) for net in nets for t in net], self._p(obs_words), self._p(action_out),
                             self._p(logp_out), self._p(value_out), self._p(feature_words_out), self._p(reward_out), self._p(done_out),
                             self._p(tricks), self._p(obs_out), flags, self._stream()))
        return action_out

    def _seat_sets(self, seats_per_game):
        """seats_per_game as the C entry points take it: None, or a contiguous uint8 tensor [N] on the env's device."""
        spg = seats_per_game
        if spg is not None and not (torch.is_tensor(spg) and spg.device == self.device and spg.dtype == torch.uint8
                                    and spg.is_contiguous() and tuple(spg.shape) == (self.n,)):
            raise ValueError("seats_per_game: a contiguous uint8 tensor [N] on the env's device")
        return spg

    def ppo_loss(self, out, obs_words, action, logp_old, advantage, ret, weight, clip, vf_coef, ent_coef):
        """tarok_ppo_loss: (loss terms f32 [3] = weighted means of the policy loss, the squared value
        error and the entropy; d loss / d out [B,64] bf16) for loss = pi + vf_coef v - ent_coef H."""
        B = out.shape[0]
        assert out.dtype == torch.bfloat16 and out.is_contiguous() and tuple(out.shape) == (B, 64)
        f = lambda t: t.to(torch.float32).contiguous()
        logp_old, advantage, ret, weight = f(logp_old), f(advantage), f(ret), f(weight)
        action = action.to(torch.int64).contiguous()
        obs_words = obs_words.to(torch.int64).contiguous()
        with torch.cuda.device(self.device):
            inv = (1.0 / weight.sum().clamp(min=1.0)).reshape(1).contiguous()
            dout = torch.empty_like(out)
            part = torch.empty(((B + 255) // 256, 4), dtype=torch.float32, device=self.device)
            _native.check(self.L.tarok_ppo_loss(self._h, int(B), self._p(out), self._p(obs_words), self._p(action),
                                                self._p(logp_old), self._p(advantage), self._p(ret), self._p(weight),
                                                float(clip), float(vf_coef), float(ent_coef), self._p(inv), self._p(dout),
                                                self._p(part), self._stream()))
            terms = part.sum(0)[:3] * inv
        return terms, dout

    def targets_ref(self, obs_before, action, trick, done, reward, next_q=None, factor=0.1):
        """The reference agent's transition targets (tarok_targets_ref; Igralec.py:387-446) of a recorded rollout:
        rows [T,N] (reward [T,N,4] recorded with reward_ref=True), T a multiple of 4 from a trick boundary.
        Returns (dy [T/4,N,4,54] f32, meta [T/4,N,4] u8)."""
        Tn = obs_before.shape[0]
        with torch.cuda.device(self.device):
            dy = torch.empty((Tn // 4, self.n, 4, 54), dtype=torch.float32, device=self.device)
            meta = torch.empty((Tn // 4, self.n, 4), dtype=torch.uint8, device=self.device)
            c = lambda t: None if t is None else t.contiguous()
            _native.check(self.L.tarok_targets_ref(self._h, int(Tn), self._p(c(obs_before)), self._p(c(action)), self._p(c(trick)),
                                                   self._p(c(done)), self._p(c(reward)), self._p(c(next_q)), float(factor),
                                                   self._p(dy), self._p(meta), self._stream()))
        return dy, meta

    # ---- the fused learner (include/tarok_env.h tarok_learn_*; driven by tarok_amd.selfplay.SelfPlay.update_fused)
    def _learn_returns(self, T, done, reward, words, logp, val, act, reward_scale, rec, stats, scratch, gae, gamma, lam, seats, seats_per_game):
        with torch.cuda.device(self.device):
            _native.check(self.L.tarok_learn_returns_seats(self._h, int(T), self._p(done), self._p(reward), self._p(words), self._p(logp),
                                                           self._p(val), self._p(act), float(reward_scale), 1 if gae else 0, float(gamma),
                                                           float(lam), int(seats), self._p(self._seat_sets(seats_per_game)), self._p(rec),
                                                           self._p(stats), self._p(scratch), self._stream()))

    def learn_returns(self, T, done, reward, words, logp, val, act, reward_scale, rec, stats, scratch):
        """The record and advantage statistics of tarok_learn_returns: every card credited with its seat's final score."""
        self._learn_returns(T, done, reward, words, logp, val, act, reward_scale, rec, stats, scratch, False, 1.0, 1.0, 15, None)

    def learn_returns_gae(self, T, done, reward, words, logp, val, act, reward_scale, gamma, lam, rec, stats, scratch):
        """The record of learn_returns with per-seat GAE(gamma, lam) returns (tarok_learn_returns_gae)."""
        self._learn_returns(T, done, reward, words, logp, val, act, reward_scale, rec, stats, scratch, True, gamma, lam, 15, None)

    def learn_returns_seats(self, T, done, reward, words, logp, val, act, reward_scale, rec, stats, scratch, gae=False, gamma=1.0,
                            lam=1.0, seats=15, seats_per_game=None):
        """tarok_learn_returns_seats: the record of learn_returns (gae=False) or learn_returns_gae (gae=True) with `known`
        masked by the learner's seats: seats (a 4-bit set for every slot) or seats_per_game ([N] uint8 device tensor of
        sets), as in policy_step.  The set 15 without seats_per_game masks nothing: the unmasked kernel runs."""
        self._learn_returns(T, done, reward, words, logp, val, act, reward_scale, rec, stats, scratch, gae, gamma, lam, seats, seats_per_game)

    def learn_select_scratch_bytes(self, M):
        return int(self.L.tarok_learn_select_scratch_bytes(int(M)))

    def learn_select(self, M, rec, index_out, count_out, scratch):
        """tarok_learn_select: index_out[:count] (int64 [M]) = the numbers of the known samples of rec [M,4], ascending;
        count_out int64 [1] on the device; scratch: learn_select_scratch_bytes(M) bytes.  No host synchronisation."""
        with torch.cuda.device(self.device):
            _native.check(self.L.tarok_learn_select(self._h, int(M), self._p(rec), self._p(index_out), self._p(count_out),
                                                    self._p(scratch), self._stream()))

    def learn_chain(self, B, words, index, rec, stats, clip, vf_coef, ent_coef, wf, bias, Xw, H1, H2, dOut, dH2, dH1, scratch, terms,
                    running=None):
        """wf: dict of the bf16 fragment-order weight copies (w1, w2, w3, w3t, w2t: learn_adam), bias: (b1, b2, b3) f32."""
        with torch.cuda.device(self.device):
            _native.check(self.L.tarok_learn_chain(self._h, int(B), self._p(words), self._p(index), self._p(rec), self._p(stats),
                                                   float(clip), float(vf_coef), float(ent_coef), self._p(wf["w1"]), self._p(bias[0]),
                                                   self._p(wf["w2"]), self._p(bias[1]), self._p(wf["w3"]), self._p(bias[2]),
                                                   self._p(wf["w3t"]), self._p(wf["w2t"]), self._p(Xw), self._p(H1), self._p(H2), self._p(dOut),
                                                   self._p(dH2), self._p(dH1), self._p(scratch), self._p(terms), self._p(running),
                                                   self._stream()))

    def learn_chain_distill(self, B, words, index, rec, stats, clip, vf_coef, ent_coef, wf, bias, Xw, H1, H2, dOut, dH2, dH1, scratch, terms,
                            running, target, distill_coef, distill_scratch, distill_out, distill_running=None):
        """learn_chain with the distillation term (tarok_learn_chain_distill): target [M,64] bf16 rows by sample number (as
        rec), distill_scratch [ceil(B/96),2] f32, distill_out [2] f32 = {weighted mean cross-entropy, weighted mean of the
        rows' sums}, distill_running [2] f32 or None: += distill_out."""
        with torch.cuda.device(self.device):
            _native.check(self.L.tarok_learn_chain_distill(
                self._h, int(B), self._p(words), self._p(index), self._p(rec), self._p(stats), float(clip), float(vf_coef),
                float(ent_coef), self._p(wf["w1"]), self._p(bias[0]), self._p(wf["w2"]), self._p(bias[1]), self._p(wf["w3"]),
                self._p(bias[2]), self._p(wf["w3t"]), self._p(wf["w2t"]), self._p(Xw), self._p(H1), self._p(H2), self._p(dOut),
                self._p(dH2), self._p(dH1), self._p(scratch), self._p(terms), self._p(running), self._p(target), float(distill_coef),
                self._p(distill_scratch), self._p(distill_out), self._p(distill_running), self._stream()))

    def learn_workspace_bytes(self):
        return int(self.L.tarok_learn_workspace_bytes(self._h))

    def learn_dw(self, B, Xw, H1, H2, dOut, dH2, dH1, terms, work, grad):
        with torch.cuda.device(self.device):
            _native.check(self.L.tarok_learn_dw(self._h, int(B), self._p(Xw), self._p(H1), self._p(H2), self._p(dOut),
                                                self._p(dH2), self._p(dH1), self._p(terms), self._p(work), self._p(grad), self._stream()))

    def learn_adam(self, param, grad, m, v, step, wf, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=1.0, gnorm=None, apply=True):
        wf = wf or {}
        with torch.cuda.device(self.device):
            _native.check(self.L.tarok_learn_adam(self._h, self._p(param), self._p(grad), self._p(m), self._p(v), self._p(step), float(lr),
                                                  float(beta1), float(beta2), float(eps), float(max_norm), self._p(wf.get("w1")),
                                                  self._p(wf.get("w2")), self._p(wf.get("w3")), self._p(wf.get("w3t")),
                                                  self._p(wf.get("w2t")), self._p(gnorm), 1 if apply else 0, self._stream()))

    def gather_features(self, feature_words, index=None, out=None):
        """tarok_expand_features: [M,4] int64 feature words (+ optional int64 sample index [B]) ->
        [B,256] bf16 network input, gather and bit expansion in one kernel."""
        fw = feature_words.contiguous()
        B = fw.shape[0] if index is None else index.shape[0]
        with torch.cuda.device(self.device):
            out = self._empty(out, (B, 256), torch.bfloat16)
            idx = None if index is None else index.to(torch.int64).contiguous()
            _native.check(self.L.tarok_expand_features(self._h, int(B), self._p(fw), self._p(idx), self._p(out), self._stream()))
        return out

    @staticmethod
    def expand_feature_words(words, dtype=torch.bfloat16):
        """[..., 4] int64 feature words (tarok_policy_mlp feature_words_out) -> [..., 256] 0/1 features."""
        b = words.contiguous().view(torch.uint8).view(*words.shape[:-1], 32, 1)
        shifts = torch.arange(8, device=words.device, dtype=torch.uint8)
        return ((b >> shifts) & 1).view(*words.shape[:-1], 256).to(dtype)

    def state(self):
        """Canonical lanes [10,N] (H0-3, P0-3, TAL, META) as host numpy uint64."""
        with torch.cuda.device(self.device):
            lanes = torch.empty((10, self.n), dtype=torch.int64, device=self.device)
            _native.check(self.L.tarok_get_state(self._h, self._p(lanes), self._stream()))
        return _u64(lanes)

    def set_state(self, lanes):
        """Restore from canonical lanes [10,N] (numpy uint64 / int64 tensor): inverse of state()."""
        if isinstance(lanes, np.ndarray):
            lanes = torch.from_numpy(np.ascontiguousarray(lanes).view(np.int64))
        lanes = self._dev(lanes, torch.int64, (10, self.n))
        with torch.cuda.device(self.device):
            _native.check(self.L.tarok_set_state(self._h, self._p(lanes), self._stream()))
        return self.legal_actions()

    def counters(self):
        """(episode[N] int64, score_sum[N,4] int32) host numpy."""
        with torch.cuda.device(self.device):
            ep = torch.empty(self.n, dtype=torch.int32, device=self.device)
            ss = torch.empty((self.n, 4), dtype=torch.int32, device=self.device)
            _native.check(self.L.tarok_get_counters(self._h, self._p(ep), self._p(ss), self._stream()))
        return ep.cpu().numpy().astype(np.int64), ss.cpu().numpy()
