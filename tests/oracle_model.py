"""TEST INFRASTRUCTURE — a per-slot model of the step launches that predicts EVERY output row.

One `SlotModel` is one slot of a TarokVecEnv played on the CPU oracle (oracle/tarok_oracle.c, the restatement of
the reference rules): `card()` plays one card the way one row of a step launch does (include/tarok_env.h:
tarok_step, tarok_step_random, tarok_krog_random, tarok_run_random, tarok_policy_step) and returns the full row a
learner reads — action_out, done_out, reward_out, trick_out, obs_out and the history byte — not only the state.
The expectations come from the oracle and from oracle/encoder_spec.py, never from the code under test.

No GPU in here: tests/test_oracle_model.py replays the games recorded from the reference through it.
"""
import ctypes as C

from oracle import encoder_spec as E
from oracle import oracle as O
from oracle import tarok_spec as S

PHASE_PLAY, PHASE_DONE = 2, 3
NO_CARD = 255                    # action_out where nothing is to be played


class Row:
    """What one card of one slot writes.
    action    the card (the Bot policy's or the caller's); NO_CARD from the Bot policy where no game is in play
    done      1 iff the game finished by this card
    reward    [4] by seat, only where done (None otherwise: the launch writes no reward row)
    trick     0, or 0x8000 | vrednost_stiha << 4 | seat that took the trick this card completed
    obs       the observation word for the NEXT move (DONE kept across an auto-reset)
    hist_pos  index of the history byte this card wrote (= cards played before it), None for a rejected card
    rejected  the card was not played: illegal, garbage, or no game in play"""
    __slots__ = ("action", "done", "reward", "trick", "obs", "hist_pos", "rejected")

    def __init__(self):
        self.action, self.done, self.reward, self.trick, self.obs, self.hist_pos, self.rejected = NO_CARD, 0, None, 0, 0, None, True


def reward_row(game, reward_ref):
    """reward_out of a game that has just finished: the plain scores, or with TAROK_REWARD_REF what
    rezultat_igre folds into each seat's last transition (oracle/encoder_spec.rezultat_igre_st_tock)."""
    g = game.g
    scores = game.scores
    if not reward_ref:
        return scores
    tip = E.TIP_IZBIRE[int(g.contract)]
    left = 12 - int(g.trick_no)                       # cards left in every hand when the game ended
    return [E.rezultat_igre_st_tock(scores[s], tip, s == int(g.declarer), left) for s in range(4)]


class SlotModel:
    """Slot `index` of an env (seed, mix): its current game, episode number, score sums and play history."""

    def __init__(self, seed, index, mix, episode=0, game=None, game_of=None):
        """game: an oracle Game to play instead of the slot's synthetic one (no spec RNG key: explicit cards only,
        no auto-reset).
        game_of(index, episode): the game the slot starts at `episode`, as (a fresh oracle Game, its key), or None for
        the synthetic one — a next-game line that tarok_front_lines decided again (tests/front_lines_model.py).  The key
        is the one the line carries, S.game_key(seed, index, episode): the Bot policy's draws stay on it."""
        self.seed, self.i, self.mix, self.game_of = seed, index, mix, game_of
        self.sum = [0, 0, 0, 0]
        self.fin = False
        self.hist = [0] * 48
        if game is None:
            self.new_game(episode)
        else:
            self.ep, self.g, self.key, self.played = episode, game, None, 0

    def new_game(self, ep):
        self.ep = ep
        given = None if self.game_of is None else self.game_of(self.i, ep)
        if given is None:
            self.g, self.key = O.Game.synth(self.seed, self.i, ep, self.mix), S.game_key(self.seed, self.i, ep)
        else:
            self.g, self.key = given
            assert int(self.key) == S.game_key(self.seed, self.i, ep), "a given game plays under the key its line carries"
        self.played = 0                               # rows [0, played) of the history belong to the current game

    def reset(self, ep):
        self.new_game(ep)
        self.sum = [0, 0, 0, 0]
        self.fin = False

    def legal(self):
        return self.g.legal() if self.g.g.phase == PHASE_PLAY else 0

    def obs_word(self):
        return int(O.lib().to_obs_word(C.byref(self.g.g), 1 if self.fin else 0))

    def card(self, a=None, auto=False, reward_ref=False):
        """One card (a = None: the Bot policy's, uniform among the legal cards on the spec RNG).  Mirrors one row of a
        step launch: the card, trick resolution and scoring, then the auto-reset, then the observation word."""
        game, g = self.g, self.g.g
        row = Row()
        self.fin = False
        if g.phase == PHASE_PLAY:
            pos = g.trick_no * 4 + g.n_in_trick
            if a is None:
                a = int(O.lib().to_policy_action(self.key, pos, game.legal()))
            row.action = int(a)
            r = game.step(a)
            if r >= 0:
                row.rejected = False
                row.hist_pos = pos
                self.hist[pos] = int(a)
                self.played = pos + 1
                row.trick = int(g.last_trick)
            if r == 1:
                self.fin = True
                row.done = 1
                for s in range(4):
                    self.sum[s] += g.score[s]
                row.reward = reward_row(game, reward_ref)
        elif a is not None:
            row.action = int(a)
        if auto and g.phase == PHASE_DONE:
            self.new_game(self.ep + 1)
        row.obs = self.obs_word()
        return row
