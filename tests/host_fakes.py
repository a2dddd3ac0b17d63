"""NumPy-backed stand-ins for gcnx.Context and gcnx.device.DeviceArray, for the host tests that build layers and models without a
device: build(), state_dict(), load_state_dict() and everything else that only places, uploads and reads parameters."""
import numpy as np


class HostArray:
    """Stands in for DeviceArray: flat / cols views share the buffer; every flat() is recorded in ``views`` as (offset, n, shape)
    and the last upload is kept in ``uploaded``."""

    def __init__(self, base, arr):
        self.base, self.arr, self.shape, self.size = base, arr, arr.shape, arr.size
        self.uploaded, self.views = None, []

    @property
    def offset(self):
        """Of the first element, in floats from the start of the buffer."""
        return (self.arr.__array_interface__["data"][0] - self.base.__array_interface__["data"][0]) // 4

    def flat(self, off, n, shape=None):
        assert self.arr.flags.c_contiguous and off + n <= self.size
        self.views.append((off, n, tuple(shape or (n,))))
        return HostArray(self.base, self.arr.reshape(-1)[off:off + n].reshape(shape or (n,)))

    def cols(self, c0, c1):
        assert self.arr.ndim == 2 and 0 <= c0 <= c1 <= self.shape[1]
        return HostArray(self.base, self.arr[:, c0:c1])

    def copy_from_host(self, host, wait=True):
        host = np.ascontiguousarray(host, np.float32)
        assert host.shape == tuple(self.shape) and self.arr.flags.c_contiguous, (host.shape, self.shape)
        self.uploaded = host.copy()
        self.arr[...] = self.uploaded

    def numpy(self):
        return self.arr.copy()


class HostContext:
    """Stands in for gcnx.Context: host arrays behind zeros(n), each kept in ``buffers``."""

    def __init__(self):
        self.buffers = []

    def zeros(self, n, dtype=np.float32):
        base = np.zeros(int(n), np.float32)
        self.buffers.append(HostArray(base, base))
        return self.buffers[-1]
