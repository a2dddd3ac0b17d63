"""Helpers shared by the GPU tests that compare bit for bit inside sentinel frames (tests/test_gpu_reduce_routes.py,
tests/test_gpu_elementwise_routes.py, tests/test_gpu_spmm_routes.py, tests/test_gpu_graph_prep.py: there a 1-D array is a one-row
frame)."""
import numpy as np

SENTINEL = np.float32(12345.0)
# one sentinel per element type a frame can hold: float32 rows, bf16 result rows (uint16), bit images (uint32 / int32)
SENTINELS = {np.dtype(np.float32): SENTINEL, np.dtype(np.uint16): np.uint16(0xABCD), np.dtype(np.uint32): np.uint32(0x5EA7BEEF),
             np.dtype(np.int32): np.int32(0x5EA7BEEF)}
_UINT = {2: np.uint16, 4: np.uint32}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(got, want):
    """Same shape and the same float32 bit patterns."""
    return got.shape == want.shape and np.array_equal(bits(got), bits(want))


def _pattern(a, dtype):
    """The bit patterns of `a` as elements of `dtype`."""
    a = np.ascontiguousarray(a, dtype=dtype)
    return a.view(_UINT[a.dtype.itemsize])


class Frame:
    """An [n, f] view of row stride ld, `lead` elements into a flat device buffer of sentinels (`data`: the view's content;
    `dtype`: float32, uint16, uint32 or int32).
    check(want): the view holds `want` bit for bit and every element outside it is still the sentinel.
    untouched(): the whole buffer is what the constructor uploaded (for input operands)."""

    def __init__(self, ctx, n, f, ld, lead, data=None, tail=9, dtype=np.float32):
        from gcnx.device import DeviceArray
        assert ld >= f
        self.dtype = np.dtype(dtype)
        self.sentinel = SENTINELS[self.dtype]
        self.ctx, self.n, self.f, self.ld, self.lead = ctx, n, f, ld, lead
        host = np.full(lead + n * ld + tail, self.sentinel, self.dtype)
        if data is not None:
            self._body(host)[:, :f] = np.asarray(data, self.dtype).reshape(n, f)
        self._initial = host
        self.buf = ctx.to_device(host)
        self.view = DeviceArray(ctx, self.buf.ptr + self.dtype.itemsize * lead, (n, f), self.dtype, ld=ld, base=self.buf)

    def _body(self, flat):
        return flat[self.lead:self.lead + self.n * self.ld].reshape(self.n, self.ld)

    def row(self, i):
        """Row i of the view as a 1-D array."""
        from gcnx.device import DeviceArray
        return DeviceArray(self.ctx, self.view.ptr + self.dtype.itemsize * i * self.ld, (self.f,), self.dtype, base=self.buf)

    def aligned(self):
        return self.view.ptr % 16 == 0 and self.ld * self.dtype.itemsize % 16 == 0

    def _outside_intact(self, got):
        s = _pattern(self.sentinel, self.dtype)
        g = _pattern(got, self.dtype)
        body = self._body(g)
        return bool((body[:, self.f:] == s).all() and (g[:self.lead] == s).all() and (g[self.lead + self.n * self.ld:] == s).all())

    def numpy(self):
        """The view's content on the host, after asserting that nothing outside it was written."""
        got = self.buf.numpy()
        assert self._outside_intact(got), "written outside the view"
        return self._body(got)[:, :self.f].copy()

    def check(self, want, what=""):
        got = self.buf.numpy()
        body = self._body(got)
        want = np.asarray(want, self.dtype).reshape(self.n, self.f)
        assert np.array_equal(_pattern(body[:, :self.f], self.dtype), _pattern(want, self.dtype)), what
        assert self._outside_intact(got), (what, "written outside the view")

    def untouched(self, what=""):
        """Nothing was written at all: the body holds the initial data, everything else the sentinel."""
        assert np.array_equal(_pattern(self.buf.numpy(), self.dtype), _pattern(self._initial, self.dtype)), (what, "an input frame was written")
