"""Loader of the CPU model libraries (tests/emul*/libaisx_<name>.so): TEST INFRASTRUCTURE for the -m "not gpu" suite.
One function for every model: rebuild when stale, load, declare the entry points."""
import ctypes as C
import glob
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "gr-ais_amd", "csrc")
vp, i32, f32, f64, u32, u64, lng = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_uint, C.c_uint64, C.c_long
_LIBS = {}


def load(name, table, extra_deps=()):
    """tests/<name>/libaisx_<name>.so, rebuilt by its Makefile when it is older than a header of the product's csrc, the
    shared model sources (tests/emul), its own source or one of `extra_deps` (paths below csrc).  `table` rows are
    (entry point, restype or None, argtypes); an entry point that is not listed keeps ctypes' defaults."""
    if name not in _LIBS:
        d = os.path.join(HERE, name)
        so = os.path.join(d, "libaisx_%s.so" % name)
        deps = glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(HERE, "emul", "emul*")) + \
            [os.path.join(d, name + ".cpp")] + [os.path.join(CSRC, e) for e in extra_deps]
        if (not os.path.exists(so)) or any(os.path.getmtime(x) > os.path.getmtime(so) for x in deps):
            subprocess.check_call(["make", "-C", d, "-s", "-B"])
        L = C.CDLL(so)
        for fn, restype, argtypes in table:
            f = getattr(L, fn)
            if restype is not None:
                f.restype = restype
            f.argtypes = argtypes
        _LIBS[name] = L
    return _LIBS[name]
