"""TEST INFRASTRUCTURE — tarok_learn_select (include/tarok_env.h) as numpy: the stable compaction of the known samples
of a record the way the library's three launches decompose it (count per tile, exclusive scan of the tile counts,
scatter by rank inside round, wave and tile), so that tests/test_opponent_cpu.py can hold the decomposition against
np.flatnonzero and tests/test_gpu_learner_opponent.py the kernels against both — the scratch rows included.
"""
import numpy as np

KNOWN_BIT = 1 << 8                 # of the record's fourth word: card | known << 8
WAVES, LANES = 4, 64               # a workgroup of the library: 256 threads


def rec_of(known, seed=0):
    """A record [M,4] f32 whose known bits are `known` (bool [M]) and whose other fields are noise: a card byte in 0..53
    in the low bits of the fourth word, anything in the three floats."""
    known = np.asarray(known, bool)
    rnd = np.random.RandomState(seed)
    rec = rnd.randn(known.size, 4).astype(np.float32)
    bits = rnd.randint(0, 54, known.size).astype(np.uint32) | np.where(known, KNOWN_BIT, 0).astype(np.uint32)
    rec[:, 3] = bits.view(np.float32)
    return rec


def known_of(rec):
    return (np.ascontiguousarray(rec[:, 3]).view(np.uint32) & KNOWN_BIT) != 0


def scratch_bytes(M, tile):
    """tile_off [tiles] i64 then tile_cnt [tiles] u32, rounded up to 16 bytes."""
    tiles = -(-M // tile)
    return -(-tiles * 12 // 16) * 16


def select_model(rec, tile, fill=-1):
    """Returns dict(index [M] i64 with `fill` in the entries that are not written, count, tile_cnt [tiles] u32,
    tile_off [tiles] i64)."""
    known = known_of(rec)
    M = known.size
    tiles = -(-M // tile)
    rounds = tile // (WAVES * LANES)
    assert rounds * WAVES * LANES == tile
    padded = np.zeros(tiles * tile, bool)
    padded[:M] = known
    k = padded.reshape(tiles, WAVES, rounds, LANES)            # sample = ((tile * WAVES + wave) * rounds + round) * LANES + lane
    tile_cnt = k.sum(axis=(1, 2, 3)).astype(np.uint32)
    tile_off = np.concatenate([[0], np.cumsum(tile_cnt.astype(np.int64))[:-1]]).astype(np.int64)
    index = np.full(M, fill, np.int64)
    for t in range(tiles):
        at = int(tile_off[t])
        for w in range(WAVES):
            for r in range(rounds):
                ballot = k[t, w, r]
                below = np.cumsum(ballot) - ballot                 # mbcnt: known lanes below the lane
                lanes = np.nonzero(ballot)[0]
                index[at + below[lanes]] = ((t * WAVES + w) * rounds + r) * LANES + lanes
                at += int(ballot.sum())
    return dict(index=index, count=int(tile_cnt.sum()), tile_cnt=tile_cnt, tile_off=tile_off)


def known_patterns(M, tile, seed=0):
    """The known patterns of the compaction tests for M samples, as (name, bool [M])."""
    rnd = np.random.RandomState(seed + M)
    z = lambda: np.zeros(M, bool)
    pats = [("half", rnd.rand(M) < 0.5), ("all", np.ones(M, bool)), ("none", z())]
    a = z(); a[0] = True; pats.append(("first", a))
    a = z(); a[M - 1] = True; pats.append(("last", a))
    a = np.ones(M, bool); a[tile:2 * tile] = False; pats.append(("empty tile", a))       # (M <= tile: all set)
    a = rnd.rand(M) < 0.5; a[min(M, 128):min(M, 192)] = False; pats.append(("empty wave round", a))
    return pats
