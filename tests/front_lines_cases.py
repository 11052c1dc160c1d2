"""TEST INFRASTRUCTURE — the fronted next-game lines of tests/test_gpu_front_lines.py and tests/test_gpu_front_rows.py: the
envs' constants, random head weights, the front_lines call and the twin chain its lines are held to."""
import numpy as np


N, SEED, OFFSET = 300, 7, 9000
AHEAD = 14


def random_weights(seed, gain=1.0):
    """Six tensors as policy_mlp takes them: a PolicyNet of `seed`, its head scaled so that bids and passes both occur."""
    import torch
    from tarok_amd.bidding import pack_weights
    from tarok_amd.selfplay import PolicyNet
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        net = PolicyNet(256)
        with torch.no_grad():
            net.head.weight.mul_(gain)
            net.head.bias.normal_(0.0, 0.05 * gain)
    return [t.cuda() for t in pack_weights(net)]


def make_env(T, mix=None, n=N):
    from tarok_amd import karte as K
    env = T.TarokVecEnv(n, seed=SEED, mix=K.MIX_BOT if mix is None else mix, game_offset=OFFSET)
    env.reset(episode=0)
    env.prefetch()
    return env


def sets_tensor(n):
    import torch
    return torch.from_numpy(((np.arange(n) * 7 + 3) % 16).astype(np.uint8)).cuda()


def front(env, **kw):
    """front_lines with count_out, hist_out and the scratch inside guard bands: (count, hist [10])."""
    import torch
    from guarded import Guarded, assert_guards_intact
    from tarok_amd import _native
    count = Guarded("count_out", 1, 1, np.int64, device="cuda")
    hist = Guarded("contract_hist_out", 1, 10, np.int64, device="cuda")
    nbytes = int(env.L.tarok_front_lines_scratch_bytes(env.n))
    assert nbytes == 128 + 8 * AHEAD * env.n, "not true: nbytes == 128 + 8 * AHEAD * env.n"
    scratch = Guarded("scratch", 1, nbytes, np.uint8, device="cuda")
    none = [None] * 6
    b, x = kw.get("bid") or none, kw.get("exchange") or none
    with torch.cuda.device(env.device):
        _native.check(env.L.tarok_front_lines(env._h, *[env._p(t) for t in b], float(kw.get("scale", 1.0)), int(kw.get("playouts", 1)),
                                              int(kw.get("margin", 0)), int(kw.get("contracts", 0xF)), int(kw.get("pass_value", False)),
                                              *[env._p(t) for t in x], int(kw.get("seats", 15)), env._p(kw.get("seats_per_game")),
                                              scratch.ptr, nbytes, count.ptr, hist.ptr, env._stream()))
        torch.cuda.synchronize()
    assert_guards_intact([count, hist, scratch], sorted(kw))
    (c, cw), (h, hw) = count.host(), hist.host()
    assert cw.all() and hw.all(), "count_out and every entry of contract_hist_out are written"
    return int(c[0, 0]), h[0].astype(np.int64)


def split(lines):
    """(packed [n,14,4], key [n,14], nep [n,14], mark [n,14]) of get_lines()' array."""
    tag = lines[:, :, 5]
    return lines[:, :, :4], lines[:, :, 4], (tag & np.uint64(0xFFFFFFFF)).astype(np.int64), (tag >> np.uint64(32)).astype(np.int64)


def valid_lines(env, nep):
    ep = env.counters()[0]
    b = np.arange(AHEAD)[None, :]
    return (nep > ep[:, None]) & (nep <= ep[:, None] + AHEAD) & (nep % AHEAD == b)


def twin_chain(T, episode, kw, mix=None, n=N, seed=SEED, offset=OFFSET):
    """(state lanes [10, n], keys) of a twin env taken through the existing chain at `episode`."""
    from tarok_amd import karte as K
    from oracle import tarok_spec as S
    env = T.TarokVecEnv(n, seed=seed, mix=K.MIX_BOT if mix is None else mix, game_offset=offset)
    sets = dict(seats=kw.get("seats", 15), seats_per_game=kw.get("seats_per_game"))
    setup = {}
    if kw.get("bid") is not None:
        pv = bool(kw.get("pass_value", False))
        vals = env.bid_values(episode, kw["bid"], kw["scale"], contracts=kw.get("contracts", 0xF), pass_value=pv, **sets)
        c, d, k = env.bid_round(episode, vals, kw.get("playouts", 1), threshold=kw.get("margin", 0), contracts=kw.get("contracts", 0xF),
                                pass_value=pv, **sets)
        setup = dict(contract=c, declarer=d, king_suit=k)
    env.reset(episode, defer_exchange=True, **setup)
    if kw.get("exchange") is not None:
        env.exchange(*env.exchange_values(kw["exchange"], **sets))
    else:
        env.exchange()
    lanes = env.state()
    env.close()
    keys = np.array([S.game_key(seed, offset + j, episode) for j in range(n)], np.uint64)
    return lanes, keys


def assert_lines_are_twins(T, env, taken, kw, mix=None):
    """Every line of the bool mask `taken` [n,14] holds the twin chain's game of its episode, under its key, marked."""
    lines, lanes = env.get_lines(lanes=True)
    _, key, nep, mark = split(lines)
    assert (mark[taken] == nep[taken]).all(), "not true: (mark[taken] == nep[taken]).all()"
    for e in np.unique(nep[taken]):
        want, keys = twin_chain(T, int(e), kw, mix=mix, n=env.n)
        j, b = np.nonzero(taken & (nep == e))
        assert (lanes[:, j, b] == want[:, j]).all(), ("episode", int(e), np.nonzero((lanes[:, j, b] != want[:, j]).any(0))[0][:8])
        assert (key[j, b] == keys[j]).all(), "not true: (key[j, b] == keys[j]).all()"
