"""TEST INFRASTRUCTURE: stage A of the HIP backend against the plain restatement (tests/support/stage_a_ref.py), for
tests/test_stage_a_gpu.py, run in a child process of its own: the switches that choose the route (PANGENE_GLOBAL_SORT, PANGENE_BINS,
PANGENE_BIN_CAP, PANGENE_Y_FIXUP, PANGENE_RANK_BY_SORT, PANGENE_POISON) are read once per process.  For every shard: pga_create,
pga_begin, pga_selftest_stage_a, then pga_begin and the hook again, pga_destroy.  Every exported array must equal the restatement
exactly (rk, word 0 of record B: by its properties, stage_a_ref.check_rk), and the second export the first.  Prints one line per shard
and "ALL OK"; exits 1 at the first difference, naming shard, array and first index.

    python tests/support/stage_a_direct.py [--routes default|global|bincap|bins0] [--dump FILE.npz] [shard ...]

--routes: which routes the hook must report (default: the table of stage_a_ref.expected_route; global: 0 everywhere; bincap: manyctg
takes contig bins; bins0: the bins shard takes the radix path).  --dump: the order of rk of every shard (stage_a_ref.rk_order)."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import stage_a_ref as sr  # noqa: E402


class Export(C.Structure):  # pga_selftest_stage_a_t (pga_host_selftest.hpp)
    _fields_ = [(k, C.c_void_p) for k in ("recA", "recB", "recC", "flags", "fidx", "gnm", "yperm", "headpos")] + \
               [(k, C.c_uint32) for k in ("f_head", "f_multi", "f_cstie")] + [("route", C.c_int32), ("n_unit", C.c_int32 * 3), ("n_cu", C.c_int32)]


def fail(shard, what):
    print("%s: DIFFERENT: %s" % (shard, what), flush=True)
    sys.exit(1)


def export(lib, ctx, sh):
    N = sh.N
    arr = {k: np.full((N, 4), -1, np.int32) for k in ("recA", "recB", "recC")}
    arr["flags"] = np.full(N, 0xffffffff, np.uint32)
    arr.update({k: np.full(N, -1, np.int32) for k in ("fidx", "gnm", "yperm")})
    arr["headpos"] = np.full(sh.G + 1, -1, np.int32)
    e = Export(**{k: v.ctypes.data for k, v in arr.items()})
    rc = lib.pga_selftest_stage_a(ctx, C.byref(e))
    if rc != 0:
        fail(sh.name, "pga_selftest_stage_a returned %d" % rc)
    return arr, e


def compare(sh, want, got, e, by_sort):
    def eq(name, g, w):
        g, w = np.asarray(g, np.int64), np.asarray(w, np.int64)
        if g.shape != w.shape or not np.array_equal(g, w):
            bad = np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1))
            k = int(bad[0])
            fail(sh.name, "%s at %d (of %d; %d differ): got %s, want %s" % (name, k, len(g), len(bad), g[k].tolist(), w[k].tolist()))
    if bin(e.f_head).count("1") != 1 or bin(e.f_multi).count("1") != 1 or bin(e.f_cstie).count("1") != 1 or len({e.f_head, e.f_multi, e.f_cstie, sr.PGA_F_REV}) != 4:
        fail(sh.name, "the internal flag bits %#x %#x %#x are not three bits of their own" % (e.f_head, e.f_multi, e.f_cstie))
    flags = want["rev"] | np.where(want["multi"], e.f_multi, 0) | np.where(want["head"], e.f_head, 0) | np.where(want["cstie"], e.f_cstie, 0)
    for w, name in enumerate(("cs", "seg", "ce", "pm")):
        eq("recA." + name, got["recA"][:, w], want["recA"][:, w])
    for w, name in ((1, "gid"), (2, "cds"), (3, "pid")):
        eq("recB." + name, got["recB"][:, w], want["recB"][:, w])
    for w, name in enumerate(("rank", "n_exon", "off_exon", "score_ori")):
        eq("recC." + name, got["recC"][:, w], want["recC"][:, w])
    eq("flags", got["flags"], flags)
    for name in ("fidx", "gnm", "yperm"):
        eq(name, got[name], want[name])
    if sh.N:
        eq("headpos", got["headpos"], want["headpos"])
    err = sr.check_rk(got["recB"][:, 0], want, by_sort)
    if err:
        fail(sh.name, "recB.rk: " + err)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--routes", default="")
    ap.add_argument("--dump", default="")
    ap.add_argument("shards", nargs="*")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    from pangene_amd import capi
    lib = capi.load()
    lib.pga_create.restype = lib.pga_begin.restype = lib.pga_selftest_stage_a.restype = C.c_int
    lib.pga_begin.argtypes = [C.c_void_p]
    lib.pga_selftest_stage_a.argtypes = [C.c_void_p, C.c_void_p]
    lib.pga_destroy.restype, lib.pga_destroy.argtypes = None, [C.c_void_p]
    by_sort = os.environ.get("PANGENE_RANK_BY_SORT") is not None
    dump = {}
    t_all = time.time()
    for name in a.shards or sr.NAMES:
        t0 = time.time()
        sh = sr.make(name, n_cu)
        want = sr.restate(sh)
        t1 = time.time()
        ctx = C.c_void_p()
        rc = lib.pga_create(C.byref(ctx), C.byref(sh.c), C.byref(sh.par))
        if rc != 0:
            fail(name, "pga_create returned %d" % rc)
        first = None
        for turn in range(2):
            rc = lib.pga_begin(ctx)
            if rc != 0:
                fail(name, "pga_begin returned %d (turn %d)" % (rc, turn))
            got, e = export(lib, ctx, sh)
            if e.n_cu != n_cu:
                fail(name, "the context counts %d CUs, the device has %d" % (e.n_cu, n_cu))
            compare(sh, want, got, e, by_sort)
            if first is None:
                first = got
            else:
                for k in got:
                    if not np.array_equal(got[k], first[k]):
                        fail(name, "%s: the second pga_begin leaves another array than the first, first at %d" % (k, int(np.flatnonzero((got[k] != first[k]).reshape(len(got[k]), -1).any(axis=1))[0])))
        lib.pga_destroy(ctx)
        route, units = e.route, tuple(e.n_unit)
        if a.routes == "default":
            w_route, w_units = sr.expected_route(name, n_cu)
            ok = route == w_route and (w_units is None or (units[1:] == w_units[1:] and (units[0] >= w_units[0] if name == "crowd" else units[0] == w_units[0])))
            if name == "few":
                ok = ok and units[0] == 0
            if not ok:
                fail(name, "route %d, units %s: expected route %d, units %s" % (route, units, w_route, w_units))
        elif (a.routes == "global" and route != 0) or (a.routes == "bincap" and name == "manyctg" and route != 2) or (a.routes == "bins0" and name == "bins" and route != 0):
            fail(name, "route %d is not the one this environment asks for (%s)" % (route, a.routes))
        dump[name] = sr.rk_order(got["recB"][:, 0])
        print("%s: ok  %d hits, %d genomes, key bits (cs, cm, contig) %s, route %d, units %s  [%.2f s, %.2f s of them the restatement]" % (
            name, sh.N, sh.G, sh.key_bits, route, units, time.time() - t0, t1 - t0), flush=True)
    if a.dump:
        np.savez(a.dump, **dump)
    print("%.1f s" % (time.time() - t_all))
    print("ALL OK", flush=True)


if __name__ == "__main__":
    main()
