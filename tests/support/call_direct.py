"""TEST INFRASTRUCTURE: direct pga_call_bubbles cases for tests/test_call_gpu.py, run in a child process of their own so that the test
can bound them with a timeout.  The product library (the HIP kernels of k_call.hpp behind pga_host_call.hpp) gets walks and bubbles
no GFA reaches (tests/support/call_cases.py), and the plain restatement (tests/support/call_ref.py) checks all six output arrays for
exact equality.  PANGENE_CALL_HASH_BITS is read by the library from the environment; the expected arrays do not depend on it.
Prints one line per case and "ALL OK" at the end; exits 1 at the first difference.

    python tests/support/call_direct.py {exhaustive|edges|pileup|graphlike|refusals}"""
import ctypes as C
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import call_cases as cc  # noqa: E402
import call_ref as cr  # noqa: E402

PGA_ERR_RANGE, PGA_ERR_ARG = -2, -3


class pga_call_rec_t(C.Structure):
    _fields_ = [("bo", C.c_int32), ("walk", C.c_int32), ("st_off", C.c_int32), ("en_off", C.c_int32)]


class pga_call_in_t(C.Structure):
    _fields_ = [("step", C.c_void_p), ("walk_off", C.c_void_p), ("n_walk", C.c_int32), ("n_seg", C.c_int32),
                ("bub_vs", C.c_void_p), ("bub_ve", C.c_void_p), ("n_bub", C.c_int32)]


class pga_call_out_t(C.Structure):
    _fields_ = [("n_rec", C.c_int64), ("rec", C.POINTER(pga_call_rec_t)), ("rep", C.POINTER(C.c_int32)), ("cnt", C.POINTER(C.c_int32)),
                ("n_gene", C.c_int64), ("gene_bub", C.POINTER(C.c_int32)), ("gene_seg", C.POINTER(C.c_int32)), ("gene_first", C.POINTER(C.c_int64))]


def _copy(ptr, n, dtype, width=1):
    """n * width items behind a pointer of the backend, copied out: they are the backend's until its next call"""
    if n == 0:
        return np.zeros((0, width) if width > 1 else 0, dtype=dtype)
    a = np.frombuffer(C.string_at(ptr, n * width * np.dtype(dtype).itemsize), dtype=dtype).copy()
    return a.reshape(n, width) if width > 1 else a


def call(lib, step, walk_off, n_seg, bub_vs, bub_ve, n_walk=None):
    """(rc, outputs as in call_ref.walk_side)"""
    step = np.ascontiguousarray(step, dtype=np.int32)
    walk_off = np.ascontiguousarray(walk_off, dtype=np.int64)
    bub_vs, bub_ve = np.ascontiguousarray(bub_vs, dtype=np.int32), np.ascontiguousarray(bub_ve, dtype=np.int32)
    a = pga_call_in_t(step.ctypes.data, walk_off.ctypes.data, len(walk_off) - 1 if n_walk is None else n_walk, n_seg,
                      bub_vs.ctypes.data, bub_ve.ctypes.data, len(bub_vs))
    out = pga_call_out_t()
    rc = lib.pga_call_bubbles(C.byref(a), C.byref(out))
    R, H = int(out.n_rec), int(out.n_gene)
    if rc != 0:
        return rc, dict(n_rec=R, n_gene=H)
    return rc, dict(rec=_copy(out.rec, R, np.int32, 4), rep=_copy(out.rep, R, np.int32), cnt=_copy(out.cnt, R, np.int32),
                    gene_bub=_copy(out.gene_bub, H, np.int32), gene_seg=_copy(out.gene_seg, H, np.int32), gene_first=_copy(out.gene_first, H, np.int64))


def check(lib, label, case, want=None):
    t0 = time.perf_counter()
    want = cr.walk_side(*case) if want is None else want
    t_ref = time.perf_counter() - t0
    t0 = time.perf_counter()
    rc, got = call(lib, *case)
    t_lib = time.perf_counter() - t0
    ok = rc == 0 and all(got[k].shape == want[k].shape and got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]) for k in cr.KEYS)
    n_int = int(np.maximum(want["rec"][:, 3].astype(np.int64) - want["rec"][:, 2] - 1, 0).sum())
    print("%s: N=%d R=%d I=%d alleles=%d genes=%d, restatement %.2f s, library %.3f s: %s" % (
        label, len(case[0]), len(want["rec"]), n_int, int((want["cnt"] > 0).sum()), len(want["gene_seg"]), t_ref, t_lib, "ok" if ok else "DIFFERENT"), flush=True)
    if not ok:
        print("  rc = %d" % rc)
        for k in cr.KEYS if rc == 0 else ():
            if got[k].shape != want[k].shape:
                print("  %s: shape %s, want %s" % (k, got[k].shape, want[k].shape))
            elif not np.array_equal(got[k], want[k]):
                bad = np.argwhere(got[k] != want[k])
                print("  %s: %d differ, first at %s: got %s, want %s" % (k, len(bad), bad[0].tolist(), got[k][bad[0][0]].tolist(), want[k][bad[0][0]].tolist()))
        sys.exit(1)


def refusals(lib):
    """argument errors, found before any device work; a good call straight afterwards is still right"""
    (label, good, _), = cc.exhaustive()
    step, off, n_seg, vs, ve = good
    want = cr.walk_side(*good)
    check(lib, "before the refusals", good, want)
    bad = []
    for at, v in ((0, 2 * n_seg), (len(step) - 1, 2 * n_seg), (len(step) // 2, -1)):
        s = step.copy()
        s[at] = v
        bad.append(("step[%d] = %d" % (at, v), (s, off, n_seg, vs, ve), {}, PGA_ERR_ARG))
    for at, v in ((len(vs) - 1, 2 * n_seg), (3, 2 * n_seg + 5)):
        x = vs.copy()
        x[at] = v
        bad.append(("bub_vs[%d] = %d" % (at, v), (step, off, n_seg, x, ve), {}, PGA_ERR_ARG))
    for at, v in ((2, 2 * n_seg), (5, -1)):
        x = ve.copy()
        x[at] = v
        bad.append(("bub_ve[%d] = %d" % (at, v), (step, off, n_seg, vs, x), {}, PGA_ERR_ARG))
    bad.append(("n_walk = -1", good, dict(n_walk=-1), PGA_ERR_RANGE))
    for what, case, kw, want_rc in bad:
        rc, got = call(lib, *case, **kw)
        ok = rc == want_rc and got["n_rec"] == 0 and got["n_gene"] == 0
        print("refusal %s: rc = %d, want %d: %s" % (what, rc, want_rc, "ok" if ok else "DIFFERENT"), flush=True)
        if not ok:
            sys.exit(1)
        check(lib, "after the refusal", good, want)


def main():
    which = sys.argv[1]
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    from pangene_amd import capi
    lib = C.CDLL(capi.LIB_HIP)
    lib.pga_call_bubbles.restype = C.c_int
    lib.pga_call_bubbles.argtypes = [C.POINTER(pga_call_in_t), C.POINTER(pga_call_out_t)]
    print("PANGENE_CALL_HASH_BITS = %s" % os.environ.get("PANGENE_CALL_HASH_BITS", "(unset)"), flush=True)
    if which == "refusals":
        refusals(lib)
    elif which in cc.WHICH:
        for label, case, _ in cc.cases(which):
            check(lib, label, case)
    else:
        sys.exit("unknown case " + which)
    print("ALL OK", flush=True)


if __name__ == "__main__":
    main()
