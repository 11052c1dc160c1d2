"""GPU: tarok_amd.bidding.BidLearner — the bidding head regressed on the playout teacher's sums — on 256 games with a
(2, 1) teacher: the held-out loss falls, round() bids inside its mask and its outputs reset cleanly, and weights() fed to
tarok_bid_values reproduces the module's float outputs within tests/bid_head_model.py's derived bound.

Run on the GPU box:  python -m pytest tests/test_gpu_bid_learner.py -m gpu -q -s
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
    from tarok_amd import bidding as B, karte as K
    env = tarok_amd.TarokVecEnv(N, seed=9, mix=K.MIX_BOT)
    lr = B.BidLearner(env, worlds=2, samples=1, seed=0)
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


def test_round_bids_inside_the_mask_and_resets_cleanly(trained):
    from tarok_amd import karte as K
    env, lr = trained["env"], trained["lr"]
    for seats in (15, 4):
        c, d, k = lr.round(HELD_OUT, seats=seats)
        cn = c.cpu().numpy()
        assert ((cn >= 0) & (cn <= 3)).all(), "the default mask is Klop .. Ena"
        assert ((d.cpu().numpy() >= 0) & (d.cpu().numpy() <= 3)).all() and ((k.cpu().numpy() >= 0) & (k.cpu().numpy() <= 3)).all()
        env.reset(episode=HELD_OUT, contract=c, declarer=d, king_suit=k)
        meta = env.state()[9]
        assert not ((meta >> U(54)) & U(1)).any() and (((meta >> U(33)) & U(15)).astype(np.int8) == cn).all()
        for _ in range(48):
            env.step_random(auto_reset=False)
        meta = env.state()[9]
        assert (((meta >> U(52)) & U(3)) == 3).all() and not ((meta >> U(54)) & U(1)).any()
    assert lr.scale == pytest.approx(16 * 70.0) and K.BID_DEFAULT_CONTRACTS == lr.contracts


def test_the_packed_weights_reproduce_the_module(trained):
    """bid_values(weights(), raw=True) against the module's own float outputs on the collected features.  The packed
    weights are the module's rounded to bf16, so the reference is the float64 forward of THOSE weights without the
    activation stores (the module's arithmetic on the weights the kernel is given), and the bound is forward_bound's:
    float32 accumulation over 256 products and a bias per output, and the two bf16 stores."""
    import torch
    import bid_head_model as HM
    env, lr = trained["env"], trained["lr"]
    fw = trained["held"][0]
    _, raw, fw2 = env.bid_values(HELD_OUT, lr.weights(), lr.scale, raw=True, feature_words=True)
    assert torch.equal(fw, fw2)
    net = lr.net
    bf = lambda t: t.detach().to(torch.bfloat16).double().cpu()
    f64 = lambda t: t.detach().double().cpu()
    W = [bf(net.fc1.weight), f64(net.fc1.bias), bf(net.fc2.weight), f64(net.fc2.bias), bf(net.head.weight), f64(net.head.bias)]
    x = HM.expand(fw.cpu().numpy().view(np.uint64).reshape(-1, 4))
    y = HM.forward(x, W, stores=False)[0].reshape(N, 4, 64)[:, :, :13]
    bound = HM.forward_bound(x, W).reshape(N, 4, 64)[:, :, :13]
    got = raw.cpu().numpy()[:, :, :13].astype(np.float64)
    err = np.abs(got - y)
    print("kernel against the bf16-weight module: max error %.3g, max bound %.3g, max |y| %.3g" % (err.max(), bound.max(), np.abs(y).max()))
    assert (err <= bound).all() and bound.max() < np.abs(y).max()
    assert not raw.cpu().numpy()[:, :, 13:].any()
    # the module in float32 with its unrounded weights differs by the weights' rounding only: a loose sanity figure, printed
    with torch.no_grad():
        mod = lr.outputs(fw)[:, :13].double().cpu().numpy().reshape(N, 4, 13)
    print("float32 module against the kernel: max difference %.3g" % np.abs(mod - got).max())
