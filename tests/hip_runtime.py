"""hipMalloc / hipHostMalloc / hipMemcpy for the GPU tests that hand raw device addresses to the library's launch entries
(fe_launch_copy, fe_launch_book)."""
import ctypes as C

import numpy as np

from msckf_stereo_c_amd import capi


class Hip:
    """hipMalloc / hipHostMalloc / hipMemcpy of the HIP runtime the library itself is linked against."""

    def __init__(self):
        capi.lib()
        path = None
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64.so" in line:
                    path = line.split()[-1]
                    break
        assert path, "the library's HIP runtime is not loaded"
        L = self.L = C.CDLL(path)
        L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        L.hipHostMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
        L.hipFree.argtypes = [C.c_void_p]
        L.hipHostFree.argtypes = [C.c_void_p]
        L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        L.hipGetLastError.argtypes = []
        self.owned = []

    def _ok(self, rc, what):
        assert rc == 0, "%s failed: %d" % (what, rc)

    def alloc(self, n, pinned):
        p = C.c_void_p()
        self._ok(self.L.hipHostMalloc(C.byref(p), n, 0) if pinned else self.L.hipMalloc(C.byref(p), n), "allocation")
        self.owned.append((p.value, pinned))
        return p.value

    def put(self, ptr, data):
        self._ok(self.L.hipMemcpy(ptr, data.ctypes.data, data.nbytes, 4), "hipMemcpy")           # hipMemcpyDefault

    def get(self, ptr, n):
        out = np.empty(n, np.uint8)
        self._ok(self.L.hipMemcpy(out.ctypes.data, ptr, n, 4), "hipMemcpy")
        return out

    def last_error(self):
        """hipGetLastError: 0, or the code of the last error of this thread's HIP calls and launches (and clears it)."""
        return self.L.hipGetLastError()

    def free(self):
        for p, pinned in self.owned:
            (self.L.hipHostFree if pinned else self.L.hipFree)(p)
        self.owned = []
