"""GPU: tarok_amd.exchange.ExchangeLearner — the exchange head regressed on the playout teacher's sums and its
candidates' discards — on 256 games with a (2, 1, 2) teacher: the held-out loss falls, exchange() leaves clean games, the
targets equal the numpy statement on the launches' own arrays, and weights() fed to tarok_exchange_values reproduces the
module's float outputs within tests/exchange_head_model.py's derived bound.

Run on the GPU box:  python -m pytest tests/test_gpu_exchange_learner.py -m gpu -q -s
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, HELD_OUT = 256, 1000
U = np.uint64


@pytest.fixture(scope="module")
def trained():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import tarok_amd
    tarok_amd.build()
    from tarok_amd import exchange as X, karte as K
    env = tarok_amd.TarokVecEnv(N, seed=9, mix=K.MIX_BOT)
    lr = X.ExchangeLearner(env, worlds=2, samples=1, discard_sets=2, seed=0)
    held = lr.collect(HELD_OUT)
    with torch.no_grad():
        before = float(lr.loss(*held))
    losses = [lr.iterate() for _ in range(30)]
    with torch.no_grad():
        after = float(lr.loss(*held))
    yield dict(env=env, lr=lr, held=held, before=before, after=after, losses=losses)
    env.close()


def test_training_lowers_the_held_out_loss(trained):
    """30 iterations on fresh episodes 0..29; the loss on episode 1000, which no iteration saw, before and after."""
    print("held-out loss before %.5f, after %.5f; training losses first %.5f last %.5f" % (
        trained["before"], trained["after"], trained["losses"][0], trained["losses"][-1]))
    assert trained["lr"].episode == 30 and len(trained["losses"]) == 30 and all(np.isfinite(trained["losses"]))
    assert trained["after"] < trained["before"]


def test_the_targets_and_the_loss_equal_the_numpy_statement(trained):
    import torch
    import exchange_head_model as EM
    from tarok_amd import exchange as X
    lr = trained["lr"]
    fw, sums, cands, playouts = trained["held"]
    assert playouts == 2 and tuple(sums.shape) == (N, 12, 4) and tuple(cands.shape) == (N, 12, 3)
    live, value, score, known = [t.cpu().numpy() for t in X.exchange_targets(fw, sums, cands, playouts, lr.reward_scale)]
    wl, wv, ws, wk = EM.targets(fw.cpu().numpy().view(np.uint64), sums.cpu().numpy(), cands.cpu().numpy(), playouts, lr.reward_scale)
    assert (live == wl).all() and (known == wk).all() and live.sum() > N and known.sum() >= live.sum()
    assert np.abs(value - wv).max() < 1e-5 and np.abs(score - ws).max() < 1e-5
    with torch.no_grad():
        out = lr.outputs(fw).double().cpu().numpy()
        got = float(lr.loss(*trained["held"]))
    assert got == pytest.approx(EM.loss(out, wl, wv, ws, wk), rel=1e-4, abs=1e-6)


def test_exchange_leaves_clean_games(trained):
    env, lr = trained["env"], trained["lr"]
    for seats in (15, 4):
        env.reset(episode=HELD_OUT, defer_exchange=True)
        waiting = ((env.state()[9] >> U(52)) & U(3)) == 1
        assert waiting.any()
        lr.exchange(seats=seats)
        meta = env.state()[9]
        assert not ((meta >> U(54)) & U(1)).any() and (((meta >> U(52)) & U(3)) == 2).all()
        for _ in range(48):
            env.step_random(auto_reset=False)
        meta = env.state()[9]
        assert (((meta >> U(52)) & U(3)) == 3).all() and not ((meta >> U(54)) & U(1)).any()


def test_the_packed_weights_reproduce_the_module(trained):
    """exchange_values(weights(), raw=True) against the float64 forward of the module's weights rounded to bf16, without
    the activation stores, on the live rows; the bound is forward_bound's: float32 accumulation over 256 products and a
    bias per output, and the two bf16 stores."""
    import torch
    import exchange_head_model as EM
    env, lr = trained["env"], trained["lr"]
    env.reset(episode=HELD_OUT, defer_exchange=True)
    _, _, raw, fw = env.exchange_values(lr.weights(), raw=True, feature_words=True)
    assert torch.equal(fw, trained["held"][0])
    net = lr.net
    bf = lambda t: t.detach().to(torch.bfloat16).double().cpu()
    f64 = lambda t: t.detach().double().cpu()
    W = [bf(net.fc1.weight), f64(net.fc1.bias), bf(net.fc2.weight), f64(net.fc2.bias), bf(net.head.weight), f64(net.head.bias)]
    words = fw.cpu().numpy().view(np.uint64)
    live = words[:, :, 0] != 0
    x = EM.expand(words[live])
    y = EM.forward(x, W, stores=False)[0][:, :55]
    bound = EM.forward_bound(x, W)[:, :55]
    got = raw.cpu().numpy()
    err = np.abs(got[live][:, :55].astype(np.float64) - y)
    print("kernel against the bf16-weight module: max error %.3g, max bound %.3g, max |y| %.3g" % (err.max(), bound.max(), np.abs(y).max()))
    assert (err <= bound).all() and bound.max() < np.abs(y).max()
    assert not got[~live].any()
