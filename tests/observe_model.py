"""TEST INFRASTRUCTURE — the 256 observation features of the seat to move, stated once on the CPU oracle.

What tarok_observe writes, and what the fused policy launches feed their network and write to features_out and
feature_words_out (include/tarok_env.h at tarok_observe): four 64-bit words, each a 54-bit card set and ten flag bits
from bit 54,

  word 0   own hand               | contract one-hot (10)
  word 1   legal cards            | declarer seat relative to the mover one-hot (4), cards on the table one-hot (4),
                                    mover on the declarer's team, the contract calls a king
  word 2   cards on the table     | called-king suit one-hot (4), trick number in binary (4)
  word 3   cards already taken    | game live

"Cards already taken" are the oracle's four piles: a seat's won tricks, Klop's gifted talon cards with the trick they
went to, and the declarer's discards.  The seat to move is (leader + cards on the table) % 4 in every phase.  For a game
that is NOT in play — waiting for the exchange, or finished — the legal region and the live bit are 0 and every other
region is what the oracle's state holds: the 12 dealt cards of seat 0 and no card taken for a waiting game; for a
finished game the cards left in the hand of the seat that took the last trick (none after 12 tricks), the trick number
at which it ended, an empty table.

Everything is read off an oracle Game (oracle/oracle.py); nothing comes from the code under test.  `Statement` holds
the parts as methods so that tests/test_observe_model_cpu.py can swap one part for a wrong one (its mutants).
"""
import numpy as np

DECK = (1 << 54) - 1
PHASE_EXCHANGE, PHASE_PLAY, PHASE_DONE = 1, 2, 3
BF16_ZERO, BF16_ONE = 0x0000, 0x3F80


class Statement:
    """The feature words of an oracle Game.  `after`, where a caller has it, is the same slot's Game once the card of
    this position has been played and an auto-reset has renewed a finished game; the statement does not read it."""

    def hand(self, game, seat):
        return int(game.g.hand[seat])

    def legal(self, game):
        return game.legal() if game.g.phase == PHASE_PLAY else 0

    def table_onehot(self, nt):
        return 1 << nt

    def team_bit(self, game, seat):
        return (int(game.g.team) >> seat) & 1

    def trick_number(self, game, after):
        return int(game.g.trick_no)

    def taken(self, game):
        p = game.g.pile
        return int(p[0]) | int(p[1]) | int(p[2]) | int(p[3])

    def live(self, game):
        return 1 if game.g.phase == PHASE_PLAY else 0

    def words(self, game, after=None):
        g = game.g
        nt = int(g.n_in_trick)
        seat = (int(g.leader) + nt) & 3
        king = int(g.king)
        table = 0
        for j in range(nt):
            table |= 1 << int(g.trick[j])
        f1 = (1 << ((int(g.declarer) - seat) & 3)) | (self.table_onehot(nt) << 4) | (self.team_bit(game, seat) << 8) | \
             ((1 if king >= 0 else 0) << 9)
        f2 = ((1 << king) if king >= 0 else 0) | (self.trick_number(game, after) << 4)
        return [self.hand(game, seat) | (1 << (54 + int(g.contract))), self.legal(game) | (f1 << 54), table | (f2 << 54),
                self.taken(game) | (self.live(game) << 54)]


feature_words = Statement().words


def words_array(rows):
    """[m][4] Python ints -> [m, 4] uint64."""
    return np.array([[int(w) for w in ws] for ws in rows], dtype=np.uint64).reshape(len(rows), 4)


def expand(words):
    """[m][4] feature words -> [m, 256] float64 0 / 1 (feature f = bit f % 64 of word f // 64)."""
    w = words_array(words) if not isinstance(words, np.ndarray) else words.astype(np.uint64).reshape(-1, 4)
    bits = (w[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)
    return bits.reshape(len(w), 256).astype(np.float64)


def from_bf16(raw):
    """[m, 256] raw 16-bit words of a bf16 feature array -> float64 0 / 1.  Only the two patterns 0x0000 (0.0) and
    0x3F80 (1.0) are features: anything else (a negative zero, a denormal, 0x3F81) is an AssertionError."""
    raw = np.asarray(raw)
    assert raw.dtype == np.uint16, raw.dtype
    one = raw == BF16_ONE
    bad = ~one & (raw != BF16_ZERO)
    assert not bad.any(), ("not a 0.0 / 1.0 bf16 pattern", [(int(i), int(j), hex(int(raw[i, j]))) for i, j in np.argwhere(bad)[:8]])
    return one.astype(np.float64)
