"""TEST INFRASTRUCTURE — the exactly summable weight sets of the bidding head (tests/test_gpu_bid_values.py and
tests/test_gpu_bid_values_pass.py)."""


def weight_sets():
    """{name: float64 weight set}: R, two sets P and H (see the module's docstring)."""
    import torch
    import policy_exact_ref as PE
    g = torch.Generator(); g.manual_seed(5)
    H = [t.clone() for t in PE.weights_p(0, 1, 0)]
    H[4] = (H[4] * 8).round()
    H[5] = torch.randint(-4, 5, (64,), generator=g).double() + 0.5
    return dict(R=PE.weights_r(), P1=PE.weights_p(*PE.P_PARAMS[1]), P8=PE.weights_p(*PE.P_PARAMS[8]), H=H)
