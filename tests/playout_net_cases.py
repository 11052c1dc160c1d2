"""TEST INFRASTRUCTURE — what the CPU tests of the net-played playouts share: a network with given logits, the stand-in
envs that record the launches of the Python surface, and the fixture that hides the device.  No GPU."""
import contextlib

import numpy as np


def zero_net(b3):
    """A network whose 54 card logits are b3 on every position."""
    import torch
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    bias = z(64)
    bias[:54] = torch.as_tensor(np.asarray(b3, np.float64))
    return [z(256, 256), z(256), z(256, 256), z(256), z(64, 256), bias]


def weights():
    import torch
    return [torch.zeros(256, 256, dtype=torch.bfloat16), torch.zeros(256), torch.zeros(256, 256, dtype=torch.bfloat16), torch.zeros(256),
            torch.zeros(64, 256, dtype=torch.bfloat16), torch.zeros(64)]


class NoHistory:
    history = False


class WithHistory:
    history = True


class Calls:
    """Records name(args) of everything called through it; tensors are shown by dtype and shape."""

    def __init__(self):
        self.calls = []

    def show(self, x):
        import torch
        if torch.is_tensor(x):
            return "%s%s" % (str(x.dtype).replace("torch.", ""), list(x.shape))
        return repr(x)

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)

        def f(*args, **kwargs):
            self.calls.append("%s(%s)" % (name, ", ".join([self.show(a) for a in args] + ["%s=%s" % (k, self.show(v)) for k, v in sorted(kwargs.items())])))
            return 0
        return f


@contextlib.contextmanager
def no_device():
    import torch
    saved = torch.cuda.device
    torch.cuda.device = lambda d: contextlib.nullcontext()
    try:
        yield
    finally:
        torch.cuda.device = saved
