"""TEST INFRASTRUCTURE — the plan of the two-network net playouts' comparison (weight sets, shapes, positions, roles), shared
by tests/test_playout_net_versus_cpu.py (the model alone) and tests/test_gpu_playout_net_versus.py (the kernels against the
model and against the existing launches).  No GPU."""
import playout_net_value_cases as PC
import playout_net_versus_model as XM

SEED, EPISODE, OFFSET, SALT = PC.SEED, PC.EPISODE, PC.OFFSET, PC.SALT
SHAPES = PC.SHAPES                                # (5, 3): 180 item slots, a full tile of 128 and a partial one; (1, 1): one partial tile
POSITIONS = PC.POSITIONS                          # per world kind: (mix, cards) — MIX_ALL after 0, 9, 24, 40 and 44 cards among them
SCALES = PC.SCALES
DEPTHS = (0, 1, 3)                                # of the comparison with the model
BYTE_DEPTHS = (0, 1, 3, 12)                       # of the byte equalities with the existing launches
MIXED = ((1, 14), (14, 1), (3, 8))                # A the viewer and B the table; the reverse (the viewer's value from B); two, a Bot, one
CASES = [(kind, at) for kind in ("det", "voids", "hidden") for at in range(len(POSITIONS[kind]))]


def weight_sets():
    """Two exactly summable integer sets that play differently, each with a value row of its own: A is
    playout_net_value_cases' V (set R, row 54 redrawn), B its P with row 54 and b3[54] redrawn from another stream (W3[54] in
    {-8..8} 2^-10, b3[54] = -2.25), so that A's and B's stop values differ in sign and size over the positions."""
    import torch
    sets = PC.weight_sets()
    WA, WB = sets["V"], [t.clone() for t in sets["P"]]
    g = torch.Generator(); g.manual_seed(1454)
    WB[4][54] = torch.randint(-8, 9, (256,), generator=g).double() * 2.0 ** -10
    WB[5][54] = -2.25
    return dict(A=WA, B=WB)


def rotate(m, v):
    """The absolute seat set m as seen by viewer v: bit r of the result is bit (r + v) & 3 of m."""
    return sum(((m >> ((r + v) & 3)) & 1) << r for r in range(4))


def model(kind, at, n, worlds, W, own_rel, opp_rel, depth, value_scale=1.0, rule="spec"):
    """The model's (games, words, sums, cards, info) of case (kind, at) at n games."""
    games, words, _ = PC.games_at(kind, at, n)
    sums, acts, info = XM.playout_cards(kind, games, SEED, SALT, 15, worlds, W["A"], W["B"], own_rel, opp_rel, depth, value_scale, words, rule)
    return games, words, sums, acts, info
