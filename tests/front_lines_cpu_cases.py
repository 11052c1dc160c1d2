"""TEST INFRASTRUCTURE — the model-side constants and head weights of tests/test_front_lines_cpu.py, shared with
tests/test_oracle_model.py.  No GPU."""
import torch


SEED, GIDX = 3, 77


def zero_weights():
    return [torch.zeros((256, 256), dtype=torch.bfloat16), torch.zeros(256), torch.zeros((256, 256), dtype=torch.bfloat16),
            torch.zeros(256), torch.zeros((64, 256), dtype=torch.bfloat16), torch.zeros(64)]


def model_weights(seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: (torch.randint(-4, 5, s, generator=g).double() / 16)
    return (r(256, 256), r(256), r(256, 256) / 16, r(256), r(64, 256) / 16, r(64))
