"""TEST INFRASTRUCTURE — output arrays with guard bands.

A `Guarded` array is one output of a launch ([rows, stride, *inner], of which the columns [0, n) of every row are
the caller's) allocated INSIDE a larger byte tensor: a guard band in front and behind (at least one 4 KiB page and
at least one full row of the output), everything filled with the byte SENTINEL_BYTE.  No kernel legitimately writes
an element made of that byte (a card id 165, a done byte 165, a trick word 0xA5A5 worth 602 points, a score of
-23,131, an observation word with 27 legal cards, seat -91), so after a launch

  * a guard byte or a byte of a padding column [n, stride) that is not the sentinel is a stray store, and
  * an element of the payload that still IS the sentinel was not written.

Works on any torch device: the checker itself is tested on the CPU (tests/test_oracle_model.py).
"""
import ctypes as C

import numpy as np

SENTINEL_BYTE = 0xA5
PAGE = 4096


class Guarded:
    def __init__(self, name, rows, n, np_dtype, inner=(), stride=None, device="cpu"):
        import torch
        self.name, self.rows, self.n = name, int(rows), int(n)
        self.stride = self.n if stride is None else int(stride)
        assert self.stride >= self.n
        self.inner = tuple(int(k) for k in inner)
        self.dtype = np.dtype(np_dtype)
        self.elem = self.dtype.itemsize * int(np.prod(self.inner, dtype=np.int64))     # bytes per (row, column)
        self.row_bytes = self.stride * self.elem
        self.payload_bytes = self.rows * self.row_bytes
        self.guard_bytes = -(-max(PAGE, self.row_bytes) // PAGE) * PAGE               # whole pages: the payload stays aligned
        self.raw = torch.empty(2 * self.guard_bytes + self.payload_bytes, dtype=torch.uint8, device=device)
        assert self.raw.data_ptr() % 16 == 0
        self.fill()

    def fill(self):
        self.raw.fill_(SENTINEL_BYTE)
        self._host = None                             # (the host copy is taken once per fill: read after the launch)

    @property
    def ptr(self):
        return C.c_void_p(self.raw.data_ptr() + self.guard_bytes)

    def payload(self):
        """The payload as a torch byte view (for uploads into an INPUT that sits between guards)."""
        return self.raw[self.guard_bytes:self.guard_bytes + self.payload_bytes]

    def _split(self):
        if self._host is None:
            self._host = self.raw.cpu().numpy()
        h = self._host
        gb = self.guard_bytes
        return h[:gb], h[gb:gb + self.payload_bytes].reshape(self.rows, self.stride, self.elem), h[gb + self.payload_bytes:]

    def host(self):
        """(values [rows, n, *inner] of the dtype, written [rows, n] bool: the element is not all sentinel bytes)."""
        _, mid, _ = self._split()
        cols = np.ascontiguousarray(mid[:, :self.n, :])
        vals = cols.view(self.dtype).reshape((self.rows, self.n) + self.inner)
        return vals, (cols != SENTINEL_BYTE).any(axis=2)

    def violations(self, limit=8):
        """Stray stores: [(where, byte offset within that region, value)], at most `limit` per region."""
        front, mid, back = self._split()
        out = []
        for where, region in (("front guard", front), ("back guard", back), ("padding columns", mid[:, self.n:, :].reshape(-1))):
            bad = np.nonzero(region != SENTINEL_BYTE)[0]
            out += [("%s: %s" % (self.name, where), int(b), int(region[b])) for b in bad[:limit]]
        return out


def assert_guards_intact(arrays, tag=None):
    bad = [v for a in arrays if a is not None for v in a.violations()]
    assert not bad, ("stray stores", tag, bad)
