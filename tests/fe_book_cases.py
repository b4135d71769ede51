"""The named edge cases of the front-end's bookkeeping (tests/cpp/fe_book_device_cases.cpp) for the CPU and the GPU test: builds
the helper library with g++ (once per process and host item order), and wraps its C interface.  Python never mirrors
FeBookDev: it asks for sizeof(FeBookDev), the arena size and a filled descriptor as bytes."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"]

_dir = None
_libs = {}


def build_dir():
    global _dir
    if _dir is None:
        _dir = tempfile.mkdtemp(prefix="fe_book_cases_")
        atexit.register(shutil.rmtree, _dir, True)
    return _dir


def host_libdir():
    from msckf_stereo_c_amd import build
    _, host = build.build_all()
    return os.path.dirname(host)


def build_program(order):
    """fe_book_test (the random frames against ref_frame) with the host running the items of a phase in `order`."""
    exe = os.path.join(build_dir(), "fe_book_test_%d" % order)
    if not os.path.exists(exe):
        libdir = host_libdir()
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unused-variable", "-DFB_HOST_ORDER=%d" % order, "-I", ROOT,
                               "-o", exe, os.path.join(ROOT, "tests", "cpp", "fe_book_test.cpp"), "-L" + libdir, "-lmskf_host", "-lmskf_hip",
                               "-Wl,-rpath," + libdir])
    return exe


class Lib:
    def __init__(self, order):
        libdir = host_libdir()
        so = os.path.join(build_dir(), "libfe_book_cases_%d.so" % order)
        subprocess.check_call(["g++"] + FLAGS + ["-shared", "-fPIC", "-DFB_HOST_ORDER=%d" % order, "-I", ROOT, "-o", so,
                                                 os.path.join(ROOT, "tests", "cpp", "fe_book_device_cases.cpp"), "-L" + libdir, "-lmskf_host", "-lmskf_hip",
                                                 "-Wl,-rpath," + libdir])
        L = self.L = C.CDLL(so)
        L.fbc_case_name.restype = L.fbc_case_set.restype = L.fbc_census_names.restype = L.fbc_error.restype = C.c_char_p
        L.fbc_run.restype = C.c_void_p
        L.fbc_free.argtypes = L.fbc_error.argtypes = L.fbc_n_frames.argtypes = L.fbc_arena_size.argtypes = L.fbc_scratch_bytes.argtypes = [C.c_void_p]
        L.fbc_initial.argtypes = L.fbc_n_arrays.argtypes = [C.c_void_p]
        L.fbc_desc_size.restype = L.fbc_arena_size.restype = L.fbc_scratch_bytes.restype = C.c_size_t
        L.fbc_initial.restype = L.fbc_snapshot.restype = C.c_void_p
        L.fbc_snapshot.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.fbc_census.argtypes = [C.c_void_p, C.c_int]
        L.fbc_census.restype = C.POINTER(C.c_int)
        L.fbc_input_range.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.fbc_array.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.fbc_array.restype = C.c_char_p
        L.fbc_desc.argtypes = [C.c_void_p, C.c_int, C.c_ulonglong, C.c_void_p]
        L.fbc_check_desc.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_ulonglong, C.c_size_t, C.c_size_t, C.c_char_p, C.c_size_t]
        assert L.fbc_host_order() == order
        self.census_names = L.fbc_census_names().decode().split()
        assert len(self.census_names) == L.fbc_census_words()
        self.cases = [(L.fbc_case_set(i).decode(), L.fbc_case_name(i).decode()) for i in range(L.fbc_n_cases())]
        self.sets = []
        for s, _ in self.cases:
            if s not in self.sets:
                self.sets.append(s)

    def index(self, name):
        return [n for _, n in self.cases].index(name)

    def of_set(self, case_set):
        return [i for i, (s, _) in enumerate(self.cases) if s == case_set]

    def run(self, i):
        return Run(self, i)


class Run:
    """One case run on the host: the arena before the first frame, four snapshots per frame (inputs of fe_book1 written, after
    fe_book1, inputs of fe_book2 written, after fe_book2), the census per frame, and descriptors for any base address."""

    def __init__(self, lib, i):
        L = self.L = lib.L
        self.name = lib.cases[i][1]
        self.h = L.fbc_run(i)
        assert self.h
        self.error = L.fbc_error(self.h).decode()
        self.n_frames = L.fbc_n_frames(self.h)
        self.size = L.fbc_arena_size(self.h)
        self.scratch_bytes = L.fbc_scratch_bytes(self.h)
        self.desc_size = L.fbc_desc_size()
        self.initial = self._bytes(L.fbc_initial(self.h))
        self.census = [dict(zip(lib.census_names, L.fbc_census(self.h, f)[:len(lib.census_names)])) for f in range(self.n_frames)] if not self.error else []
        lo, hi = C.c_size_t(), C.c_size_t()
        self.ranges = []
        for which in (0, 1):
            L.fbc_input_range(self.h, which, C.byref(lo), C.byref(hi))
            self.ranges.append((lo.value, hi.value))
        self.arrays = []
        off, nbytes, elem = C.c_size_t(), C.c_size_t(), C.c_size_t()
        for k in range(L.fbc_n_arrays(self.h)):
            name = L.fbc_array(self.h, k, C.byref(off), C.byref(nbytes), C.byref(elem)).decode()
            self.arrays.append((name, off.value, nbytes.value, elem.value))

    def _bytes(self, p):
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (self.size,)).copy()

    def snapshot(self, frame, which):
        return self._bytes(self.L.fbc_snapshot(self.h, frame, which))

    def desc(self, frame, base):
        out = np.zeros(self.desc_size, np.uint8)
        self.L.fbc_desc(self.h, frame, base, out.ctypes.data)
        return out

    def check_desc(self, frame, desc, base, size, lds_budget=150 * 1024):
        """None, or what is wrong with the descriptor."""
        why = C.create_string_buffer(128)
        rc = self.L.fbc_check_desc(self.h, frame, desc.ctypes.data, base, size, lds_budget, why, 128)
        return None if rc == 0 else "check %d: %s" % (rc, why.value.decode())

    def where(self, got, want):
        """None if the two arenas are equal, else the array and index of the first differing byte."""
        bad = np.flatnonzero(got != want)
        if bad.size == 0:
            return None
        b = int(bad[0])
        for k, (name, off, nbytes, elem) in enumerate(self.arrays):         # (in arena order)
            end = self.arrays[k + 1][1] if k + 1 < len(self.arrays) else self.size
            if off <= b < end:
                if b < off + nbytes:
                    return "%s[%d] (byte %d of the arena, %d bytes differ in all)" % (name, (b - off) // elem, b, bad.size)
                return "canary after %s (byte %d of the arena, %d bytes differ in all)" % (name, b, bad.size)
        return "byte %d of the arena" % b

    def close(self):
        if self.h:
            self.L.fbc_free(self.h)
            self.h = None

    def __del__(self):
        self.close()


def lib(order=0):
    if order not in _libs:
        _libs[order] = Lib(order)
    return _libs[order]
