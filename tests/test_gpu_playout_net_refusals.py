"""GPU: what the net-played and halving playout entries REFUSE, through the C ABI itself.  For each of the twelve entry
points and their scratch-size functions one accepted call (TAROK_OK, or a positive size) on a 5-game env, then one call per
refusal clause of the entry, each the accepted call with one argument changed: every one returns TAROK_EINVAL, before
any launch.  The table is the host layer's contract as include/tarok_env.h words it: the entries' depth ranges differ
(1..12 cards value, 1..13 exchange / bid value, 0..12 net halving, 0..13 the lists), the halving and list entries refuse
a bad value_scale even at depth 0 (the plain dense entries take none), tarok_playout_cards_net_value refuses DET with
words, the halving entries (kind == DET) != !words, and the Bot exchange takes no outputs at all where the net exchange
does not.

Run on the GPU box:  python -m pytest tests/test_gpu_playout_net_refusals.py -m gpu -q
"""
import ctypes
import types

import pytest

import gpu_harness as H
from gpu_harness import T  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu
OK, EINVAL = 0, -1
N, WORLDS, SETS, CONTRACTS = 5, 2, 2, 0x3FF
DET, VOIDS, HIDDEN = 0, 1, 2
SEED, OFFSET, EPISODE = 41, 1000, 3
WEIGHTS = ("w1", "b1", "w2", "b2", "w3", "b3")
BAD_SCALES = (0.0, -1.0, float("inf"), float("nan"))


def ints(*v):
    return (ctypes.c_int * len(v))(*v)


@pytest.fixture(scope="module")
def X(T):
    """The env (5 games, history on, 5 Bot cards in), the integer weight set R, the words and the output tensors, as the
    pointers the ABI takes."""
    import torch
    import playout_net_value_cases as NV
    import policy_exact_ref as PE
    from oracle import tarok_spec as S
    env = H.make_env(T, N, S.MIX_ALL, 5, history=True, seed=SEED, offset=OFFSET, episode=EPISODE)
    dev = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device="cuda")
    keep = dict(kw=PE.kernel_weights(T, NV.weight_sets()["R"]), voids=env.shown_voids(), played=env.played_cards(),
                sum=dev((N, 12, 4), torch.int32), count=dev((N, 12), torch.int32), action=dev(N, torch.uint8),
                xsum=dev((N, 6 * SETS, 4), torch.int32), choice=dev(N, torch.int8), discards=dev((N, 3), torch.uint8),
                bsum=dev((N, 4, 20), torch.int32), scratch=dev(1 << 20, torch.uint8))
    p = {k: v.data_ptr() for k, v in keep.items() if k != "kw"}
    p.update(zip(WEIGHTS, (t.data_ptr() for t in keep["kw"])))
    assert p["scratch"] % 16 == 0
    torch.cuda.synchronize()
    yield types.SimpleNamespace(env=env, L=env.L, h=env._h, stream=env._stream(), keep=keep, **p)
    torch.cuda.synchronize()
    env.close()


def run(X, entry, spec, refusals, accepted=OK):
    """The accepted call, then every refusal: (label, the arguments it changes)."""
    import torch
    names = [k for k, _ in spec]
    f = getattr(X.L, entry)

    def call(**over):
        assert set(over) <= set(names), (entry, sorted(set(over) - set(names)))
        vals = dict(spec, **over)
        return int(f(*[vals[k] for k in names]))

    got = call()
    torch.cuda.synchronize()
    assert got == accepted, (entry, "the accepted call returned", got)
    labels = [label for label, _ in refusals]
    assert len(set(labels)) == len(labels), (entry, "a clause is listed twice")
    bad = [(label, r) for label, over in refusals for r in [call(**over)] if r != EINVAL]
    assert not bad, (entry, "not refused with TAROK_EINVAL", bad)
    torch.cuda.synchronize()
    return call


def size_of(X, entry, *args):
    size = int(getattr(X.L, entry)(X.h, *args))
    assert 0 < size <= X.keep["scratch"].numel() - 16, (entry, size)
    return size


# ---- the clauses the entries share
def c_env():
    return [("NULL env", dict(e=None))]


def c_worlds():
    return [("worlds 0", dict(worlds=0)), ("worlds 65", dict(worlds=65))]


def c_seats():
    return [("seats 16", dict(seats=16)), ("seats -1", dict(seats=-1))]


def c_net():
    return [("net_seats 16", dict(net_seats=16)), ("net_seats -1", dict(net_seats=-1))] + \
           [("%s NULL" % w, {w: None}) for w in WEIGHTS]


def c_scratch(X, need):
    return [("scratch NULL", dict(scratch=None)), ("scratch misaligned by 8", dict(scratch=X.scratch + 8)),
            ("scratch_bytes one short", dict(scratch_bytes=need - 1))]


def c_sets():
    return [("discard_sets 0", dict(discard_sets=0)), ("discard_sets 9", dict(discard_sets=9))]


def c_contracts():
    return [("contracts 0", dict(contracts=0)), ("contracts 0x400", dict(contracts=0x400))]


def c_depth(lo, hi):
    return [("depth %d" % lo, dict(depth=lo)), ("depth %d" % hi, dict(depth=hi))]


def c_scale(**more):
    """A bad value_scale; more: the depth it is refused at where that is not the accepted call's."""
    return [("value_scale %r%s" % (v, "".join(" at %s %r" % kv for kv in more.items())), dict(more, value_scale=v)) for v in BAD_SCALES]


def c_schedule():
    return [("rounds 0", dict(rounds=0)), ("rounds 5", dict(rounds=5, round_worlds=ints(1, 1, 1, 1, 1))),
            ("schedule NULL", dict(round_worlds=None)), ("a round of 0 worlds", dict(round_worlds=ints(1, 0))),
            ("a round of -1 worlds", dict(round_worlds=ints(-1, 2))), ("a schedule of 65 worlds", dict(round_worlds=ints(64, 1))),
            ("a schedule of 65 worlds in 4 rounds", dict(rounds=4, round_worlds=ints(16, 16, 16, 17)))]


def c_kind_halving(X):
    """The halving entries: (kind == DET) != !words."""
    return [("kind -1", dict(kind=-1)), ("kind 3", dict(kind=3)), ("DET with words", dict(words=X.voids)),
            ("VOIDS without words", dict(kind=VOIDS, words=None)), ("HIDDEN without words", dict(kind=HIDDEN, words=None))]


def none_of(*outs):
    return [("all outputs NULL", {o: None for o in outs})]


# ---- the scratch-size functions
def test_scratch_sizes(X):
    s = lambda *more: [("e", X.h)] + list(more)
    for entry in ("tarok_playout_net_scratch", "tarok_playout_bids_net_scratch"):
        run(X, entry, s(("worlds", WORLDS)), c_env() + c_worlds(), size_of(X, entry, WORLDS))
    for entry in ("tarok_playout_exchange_net_scratch", "tarok_playout_exchange_net_list_scratch"):
        run(X, entry, s(("worlds", WORLDS), ("discard_sets", SETS)), c_env() + c_worlds() + c_sets(), size_of(X, entry, WORLDS, SETS))
    assert size_of(X, "tarok_playout_net_scratch", WORLDS) == N * 12 * WORLDS * 48
    assert size_of(X, "tarok_playout_exchange_net_scratch", WORLDS, SETS) == N * 6 * SETS * WORLDS * 48
    assert size_of(X, "tarok_playout_bids_net_scratch", WORLDS) == N * 80 * WORLDS * 48 + N * 40
    rw = ints(1, 2)
    run(X, "tarok_playout_net_halving_scratch_bytes", s(("rounds", 2), ("round_worlds", rw)), c_env() + c_schedule(),
        size_of(X, "tarok_playout_net_halving_scratch_bytes", 2, rw))
    entry, args = "tarok_playout_bids_net_list_scratch", (WORLDS, CONTRACTS, 15, 0, 1)
    run(X, entry, s(("worlds", WORLDS), ("contracts", CONTRACTS), ("seats", 15), ("per_game_seats", 0), ("pass_value", 1)),
        c_env() + c_worlds() + c_contracts() + c_seats() +
        [("per_game_seats 2", dict(per_game_seats=2)), ("per_game_seats -1", dict(per_game_seats=-1)),
         ("pass_value 2", dict(pass_value=2)), ("pass_value -1", dict(pass_value=-1))], size_of(X, entry, *args))


# ---- the card entries
def cards_spec(X, mid, need):
    head = [("e", X.h), ("worlds", WORLDS), ("salt", 3), ("seats", 15), ("seats_per_game", None)]
    tail = [(w, getattr(X, w)) for w in WEIGHTS] + [("scratch", X.scratch), ("scratch_bytes", need), ("sum_out", X.sum),
                                                     ("action_out", X.action), ("stream", X.stream)]
    return head + mid + tail


def cards_clauses(X, need):
    return c_env() + c_worlds() + c_seats() + c_net() + c_scratch(X, need) + none_of("sum_out", "action_out")


@pytest.mark.parametrize("kind", ("det", "voids", "hidden"))
def test_cards_net(X, kind):
    need = size_of(X, "tarok_playout_net_scratch", WORLDS)
    words = dict(det=[], voids=[("voids", X.voids)], hidden=[("played", X.played)])[kind]
    entry = "tarok_playout_cards_net" + ("" if kind == "det" else "_" + kind)
    call = run(X, entry, cards_spec(X, words + [("net_seats", 15)], need),
               cards_clauses(X, need) + [("%s NULL" % k, {k: None}) for k, _ in words])
    assert call(action_out=None) == OK and call(sum_out=None) == OK          # one output is enough


def test_cards_net_value(X):
    need = size_of(X, "tarok_playout_net_scratch", WORLDS)
    mid = [("kind", VOIDS), ("words", X.voids), ("net_seats", 15), ("depth", 2), ("value_scale", 70.0)]
    call = run(X, "tarok_playout_cards_net_value", cards_spec(X, mid, need),
               cards_clauses(X, need) + c_depth(0, 13) + c_scale() +
               [("kind -1", dict(kind=-1)), ("kind 3", dict(kind=3)), ("DET with words", dict(kind=DET)),
                ("VOIDS without words", dict(words=None)), ("HIDDEN without words", dict(kind=HIDDEN, words=None))])
    assert call(kind=DET, words=None, depth=1) == OK and call(kind=HIDDEN, words=X.played, depth=12) == OK


# ---- the exchange entries
def exchange_spec(X, value, need):
    return [("e", X.h), ("worlds", WORLDS), ("discard_sets", SETS), ("salt", 3), ("seats", 15), ("seats_per_game", None),
            ("net_seats", 15)] + value + [(w, getattr(X, w)) for w in WEIGHTS] + \
           [("scratch", X.scratch), ("scratch_bytes", need), ("sum_out", X.xsum), ("choice_out", X.choice), ("discards_out", X.discards),
            ("stream", X.stream)]


def exchange_clauses(X, need):
    return c_env() + c_worlds() + c_sets() + c_seats() + c_net() + c_scratch(X, need) + none_of("sum_out", "choice_out", "discards_out")


def test_exchange_net(X):
    need = size_of(X, "tarok_playout_exchange_net_scratch", WORLDS, SETS)
    run(X, "tarok_playout_exchange_net", exchange_spec(X, [], need), exchange_clauses(X, need))
    call = run(X, "tarok_playout_exchange_net_value", exchange_spec(X, [("depth", 2), ("value_scale", 70.0)], need),
               exchange_clauses(X, need) + c_depth(0, 14) + c_scale())
    assert call(depth=1) == OK and call(depth=13) == OK


def test_exchange_net_list(X):
    need = size_of(X, "tarok_playout_exchange_net_list_scratch", WORLDS, SETS)
    call = run(X, "tarok_playout_exchange_net_list", exchange_spec(X, [("depth", 0), ("value_scale", 70.0)], need),
               exchange_clauses(X, need) + c_depth(-1, 14) + c_scale() + c_scale(depth=2))
    assert call(depth=13) == OK and call(depth=2) == OK


def test_the_bot_exchange_takes_no_outputs(X):
    """tarok_playout_exchange with every output NULL is TAROK_OK — nothing to do — where the net entries refuse it; its
    arguments are checked first all the same."""
    spec = [("e", X.h), ("worlds", WORLDS), ("samples", 1), ("discard_sets", SETS), ("salt", 3), ("seats", 15), ("seats_per_game", None),
            ("sum_out", X.xsum), ("choice_out", X.choice), ("discards_out", X.discards), ("stream", X.stream)]
    call = run(X, "tarok_playout_exchange", spec, c_env() + c_worlds() + c_sets() + c_seats() +
               [("samples 0", dict(samples=0)), ("samples 1025", dict(samples=1025))])
    none = dict(sum_out=None, choice_out=None, discards_out=None)
    assert call(**none) == OK
    assert call(worlds=0, **none) == EINVAL and call(discard_sets=9, **none) == EINVAL


# ---- the bid entries
def bids_spec(X, value, need):
    return [("e", X.h), ("episode", EPISODE), ("deals", None), ("worlds", WORLDS), ("contracts", CONTRACTS), ("salt", 3), ("seats", 15),
            ("seats_per_game", None), ("net_seats", 15)] + value + [(w, getattr(X, w)) for w in WEIGHTS] + \
           [("scratch", X.scratch), ("scratch_bytes", need), ("sum_out", X.bsum), ("stream", X.stream)]


def bids_clauses(X, need):
    return c_env() + c_worlds() + c_contracts() + c_seats() + c_net() + c_scratch(X, need) + none_of("sum_out")


C_PASS = [("pass_value 2", dict(pass_value=2)), ("pass_value -1", dict(pass_value=-1))]


def test_bids_net(X):
    need = size_of(X, "tarok_playout_bids_net_scratch", WORLDS)
    run(X, "tarok_playout_bids_net", bids_spec(X, [], need), bids_clauses(X, need))
    call = run(X, "tarok_playout_bids_net_value", bids_spec(X, [("depth", 2), ("value_scale", 70.0), ("pass_value", 1)], need),
               bids_clauses(X, need) + c_depth(0, 14) + c_scale() + C_PASS)
    assert call(depth=13, pass_value=0) == OK


def test_bids_net_list(X):
    need = size_of(X, "tarok_playout_bids_net_list_scratch", WORLDS, CONTRACTS, 15, 0, 1)
    call = run(X, "tarok_playout_bids_net_list", bids_spec(X, [("depth", 0), ("value_scale", 70.0), ("pass_value", 1)], need),
               bids_clauses(X, need) + c_depth(-1, 14) + c_scale() + c_scale(depth=2) + C_PASS)
    assert call(depth=13, pass_value=0) == OK and call(depth=2) == OK


# ---- the halving entries
def test_cards_halving(X):
    spec = [("e", X.h), ("kind", DET), ("words", None), ("rounds", 2), ("round_worlds", ints(1, 2)), ("samples", 1), ("salt", 3),
            ("seats", 15), ("seats_per_game", None), ("sum_out", X.sum), ("count_out", X.count), ("action_out", X.action),
            ("stream", X.stream)]
    call = run(X, "tarok_playout_cards_halving", spec,
               c_env() + c_kind_halving(X) + c_schedule() + c_seats() + [("samples 0", dict(samples=0)), ("samples 1025", dict(samples=1025))] +
               none_of("sum_out", "count_out", "action_out"))
    assert call(kind=VOIDS, words=X.voids) == OK and call(kind=HIDDEN, words=X.played, sum_out=None, action_out=None) == OK


def test_cards_net_halving(X):
    rw = ints(1, 2)
    need = size_of(X, "tarok_playout_net_halving_scratch_bytes", 2, rw)
    spec = [("e", X.h), ("kind", DET), ("words", None), ("rounds", 2), ("round_worlds", rw), ("salt", 3), ("seats", 15),
            ("seats_per_game", None), ("net_seats", 15)] + [(w, getattr(X, w)) for w in WEIGHTS] + \
           [("depth", 0), ("value_scale", 70.0), ("scratch", X.scratch), ("scratch_bytes", need), ("sum_out", X.sum), ("count_out", X.count),
            ("action_out", X.action), ("stream", X.stream)]
    call = run(X, "tarok_playout_cards_net_halving", spec,
               c_env() + c_kind_halving(X) + c_schedule() + c_seats() + c_net() + c_scratch(X, need) + c_depth(-1, 13) + c_scale() +
               c_scale(depth=2) + none_of("sum_out", "count_out", "action_out"))
    assert call(kind=VOIDS, words=X.voids, depth=2) == OK and call(kind=HIDDEN, words=X.played, depth=12) == OK
