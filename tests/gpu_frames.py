"""Helpers shared by the GPU tests that compare bit for bit inside sentinel frames (tests/test_gpu_reduce_routes.py,
tests/test_gpu_elementwise_routes.py)."""
import numpy as np

SENTINEL = np.float32(12345.0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(got, want):
    """Same shape and the same float32 bit patterns."""
    return got.shape == want.shape and np.array_equal(bits(got), bits(want))


class Frame:
    """An [n, f] view of row stride ld, `lead` floats into a flat device buffer of sentinels (`data`: the view's content).
    check(want): the view holds `want` bit for bit and every float outside it is still the sentinel."""

    def __init__(self, ctx, n, f, ld, lead, data=None, tail=9):
        from gcnx.device import DeviceArray
        assert ld >= f
        self.ctx, self.n, self.f, self.ld, self.lead = ctx, n, f, ld, lead
        host = np.full(lead + n * ld + tail, SENTINEL, np.float32)
        if data is not None:
            self._body(host)[:, :f] = data
        self.buf = ctx.to_device(host)
        self.view = DeviceArray(ctx, self.buf.ptr + 4 * lead, (n, f), np.float32, ld=ld, base=self.buf)

    def _body(self, flat):
        return flat[self.lead:self.lead + self.n * self.ld].reshape(self.n, self.ld)

    def row(self, i):
        """Row i of the view as a 1-D array."""
        from gcnx.device import DeviceArray
        return DeviceArray(self.ctx, self.view.ptr + 4 * i * self.ld, (self.f,), np.float32, base=self.buf)

    def aligned(self):
        return self.view.ptr % 16 == 0 and self.ld % 4 == 0

    def check(self, want, what=""):
        got = self.buf.numpy()
        body = self._body(got)
        assert same(body[:, :self.f], np.asarray(want, np.float32).reshape(self.n, self.f)), what
        assert (body[:, self.f:] == SENTINEL).all() and (got[:self.lead] == SENTINEL).all() \
            and (got[self.lead + self.n * self.ld:] == SENTINEL).all(), (what, "written outside the view")
