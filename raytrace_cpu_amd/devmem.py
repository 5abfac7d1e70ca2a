"""DeviceScope: the device buffers of one piece of work, over the C ABI's own allocator (kr_malloc / kr_free, include/kr_trace.h).

    with DeviceScope(lib) as dev:
        d_rays = dev.alloc(n * RAY_F64.itemsize)
        d_out = dev.zeros(nw * 8)
        ... launches ...
        words = dev.fetch(d_out, nw)
    # every buffer of the scope has been freed, also when a call raised

The scope does not synchronise: the copies are hipMemcpy on the null stream.  Scopes nest; an inner one frees its buffers when it ends.
"""
import ctypes as C

import numpy as np

from .capi import check


class DeviceScope:
    def __init__(self, lib):
        self.lib, self._owned = lib, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        """kr_free of every buffer handed out, once."""
        while self._owned:
            self.lib.kr_free(self._owned.pop())

    def alloc(self, nbytes):
        d = C.c_void_p()
        check(self.lib, self.lib.kr_malloc(C.byref(d), nbytes), "kr_malloc")
        self._owned.append(d)
        return d

    def zero(self, d, nbytes):
        """kr_memset(d, 0, nbytes) of a buffer that exists (a scratch that is reused)."""
        check(self.lib, self.lib.kr_memset(d, 0, nbytes), "kr_memset")
        return d

    def zeros(self, nbytes):
        return self.zero(self.alloc(nbytes), nbytes)

    def upload(self, array):
        """A device copy of a C-contiguous host array."""
        d = self.alloc(array.nbytes)
        if array.nbytes:
            check(self.lib, self.lib.kr_memcpy_h2d(d, array.ctypes.data_as(C.c_void_p), array.nbytes), "kr_memcpy_h2d")
        return d

    def fetch(self, d, count, dtype=np.float64):
        """`count` items of `dtype` read back from d, as a new host array."""
        return self.fetch_into(d, np.zeros(count, dtype=dtype))

    def fetch_into(self, d, array):
        if array.nbytes:
            check(self.lib, self.lib.kr_memcpy_d2h(array.ctypes.data_as(C.c_void_p), d, array.nbytes), "kr_memcpy_d2h")
        return array
