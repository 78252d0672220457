"""Device plumbing shared by tests/test_heads_kernels_gpu.py and tests/test_opt_kernel_gpu.py: guarded buffers,
sentinel-framed workspaces, and the per-element comparison that records error / bound ratios."""
import numpy as np
import pytest
import torch

GUARD = 16  # guard elements on both sides of every buffer
WS_GUARD = 4096  # sentinel bytes on both sides of every workspace
SENT = 0xA5
TD = {0: torch.float32, 1: torch.float16, 2: torch.bfloat16}
DN = {0: "f32", 1: "f16", 2: "bf16"}
U = 2.0 ** -24
UT = {0: 2.0 ** -24, 1: 2.0 ** -11, 2: 2.0 ** -8}  # unit roundoff of the one store
TINY = {0: 2.0 ** -150, 1: 2.0 ** -25, 2: 2.0 ** -134}  # half the smallest subnormal


def lib():
    import datou_gomoku_muzero_amd._lib as L
    return L


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


class Buf:
    """A device tensor of ``n`` elements inside a larger allocation: GUARD NaN (or ``fill`` for integers) elements
    before and after it, the tensor itself ``off`` elements off the allocation's 16-byte grid.  ``data`` (float64 or
    integer numpy) is copied in; without it the tensor holds the fill too (an output: NaN until written)."""

    def __init__(self, n, dtype, off=0, fill=float("nan"), data=None):
        self.raw = torch.full((n + 2 * GUARD + 8,), fill, dtype=dtype, device="cuda")
        self.lo, self.n, self.fill = GUARD + off, n, fill
        self.t = self.raw[self.lo:self.lo + n]
        if data is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(data)).reshape(-1).to(dtype))

    def _is_fill(self, g):
        return bool(torch.isnan(g).all()) if self.fill != self.fill else bool((g == self.fill).all())

    def intact(self):
        return self._is_fill(torch.cat([self.raw[:self.lo], self.raw[self.lo + self.n:]]))

    def untouched(self):
        return self._is_fill(self.t)

    def f64(self):
        return self.t.double().cpu().numpy()


class Workspace:
    """``nbytes`` of workspace (0xFF bytes: NaN as floats, or zeros with ``zero``) between two sentinel regions."""

    def __init__(self, nbytes, zero=False):
        self.raw = torch.full((WS_GUARD + nbytes + WS_GUARD,), SENT, dtype=torch.uint8, device="cuda")
        self.t = self.raw[WS_GUARD:WS_GUARD + nbytes]
        self.t.fill_(0 if zero else 0xFF)
        self.nbytes = nbytes
        assert self.t.data_ptr() % 16 == 0

    def intact(self):
        return bool((self.raw[:WS_GUARD] == SENT).all()) and bool((self.raw[WS_GUARD + self.nbytes:] == SENT).all())


def f32_in(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def bits(t):
    return t.contiguous().view(torch.uint8).cpu()


def same(a, b):
    return torch.equal(bits(a), bits(b))


def within(ratios, name, dt, got, want, bound):
    """|got - want| <= bound, element by element; records the largest error / bound in ``ratios``."""
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), "%s: %d elements not written" % (name, int((~np.isfinite(got)).sum()))
    err = np.abs(got - want)
    bound = np.broadcast_to(bound, err.shape)
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))))
    print("%s %s: max error / bound = %.3g (max error %.3g)" % (name, DN[dt], ratio, float(err.max())))
    key = "%s %s" % (name, DN[dt])
    ratios[key] = max(ratios.get(key, 0.0), ratio)
    i = int(np.argmax(err - bound))
    assert ratio <= 1.0, "%s: error %.3g > bound %.3g at flat index %d (got %r, want %r)" % (
        name, err.flat[i], bound.flat[i], i, got.flat[i], np.asarray(want).flat[i])
