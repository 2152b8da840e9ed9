"""TEST INFRASTRUCTURE for tests/test_loop_lean_gpu.py, in a child process of its own: the MODE-0 sweep that evaluates its open hits itself
(k_sweep_rounds<., 1>, PANGENE_SWEEP_INLINE=1 -- read at every call) against the list form with its k_sweep_slow (=0) and against the plain-C oracle,
on the shards of loop_lean_cases.py, through the script of tests/support/sweep_direct.py (stage A, pg_post_process, flag_vtx, pg_shadow(0), the
filter; every per-hit array compared for every hit after every download).

For every shard: (1) from the shard alone, the kernel's window arithmetic restated (loop_lean_cases.open_hits): at least one hit is open; (2) the
script in both forms against the oracle -- the route hook must report no inline sweep in the list form, and in the inline form one sweep and exactly
the open hits that are not filtered when pg_shadow(0) runs (the oracle's flags say which); (3) four sweeps over one context in the forms list, inline,
inline, list and once more inline, list, list, inline (the two-counter protocol of dcnt[12] / dcnt[13] across every change of form), every download
equal to the oracle's after as many pg_shadow(0).  Prints one line per shard and "ALL OK"; exits 1 at the first difference.

    python tests/support/loop_lean_sweep.py [shard ...]"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import loop_lean_cases as lc  # noqa: E402
import stage_a_ref as sr  # noqa: E402
import sweep_direct as sd  # noqa: E402
import sweep_ref as sw  # noqa: E402


def routed(api, hip, sh, form):
    """sweep_direct.run with PANGENE_SWEEP_INLINE=form; the hook's words as they stand when the script sets the shadow filter (right behind pg_shadow(0))"""
    os.environ["PANGENE_SWEEP_INLINE"] = form
    route = np.full(10, -7, np.int32)
    real = api._set_filter

    def set_filter(ctx, which):
        if which == sd.FLT_SHADOW and hip.pga_selftest_loop_route(ctx, route.ctypes.data) != 0:
            sd.fail(sh.name, "pga_selftest_loop_route failed")
        return real(ctx, which)
    api._set_filter = set_filter
    try:
        out = sd.run(api, sh)
    finally:
        api._set_filter = real
    return out, route.tolist()


def sequence(api, sh, forms):
    """create, begin, ingest, flag_vtx, then one pg_shadow(0) and one download of flags / pid_dom per entry of forms (None: the oracle, no switch)"""
    api.shard = sh.name
    _, _, g2s, n_seg = sd.drawn(sh)
    ctx = C.c_void_p()
    api.create(C.byref(ctx), C.byref(sh.c), C.byref(sh.par))
    api.begin(ctx)
    api.ingest(ctx, None)
    api.flag_vtx(ctx, sd.ptr(g2s), n_seg, 1)
    got = []
    for f in forms:
        if f is not None:
            os.environ["PANGENE_SWEEP_INLINE"] = f
        stats = np.full((sh.G, 2), -1, np.int32)
        api.shadow(ctx, 0, sd.ptr(stats))
        a = {k: np.full(sh.N, -9, np.int32) for k in sd.STATE[1:7]}
        a["flags"], a["flt_x_bits"] = np.full(sh.N, 0xffffffff, np.uint32), np.full((sh.N + 63) // 64, 0xffffffffffffffff, np.uint64)
        api.download(ctx, C.byref(sr.HitState(**{k: sd.ptr(v) for k, v in a.items()})))
        got.append((a["flags"] & sw.PUBLIC, a["pid_dom"].copy(), stats))
    api.destroy(ctx)
    return got


def main():
    from pangene_amd import capi
    hip = C.CDLL(capi.LIB_HIP, mode=os.RTLD_LOCAL | os.RTLD_NOW)
    ora = C.CDLL(os.path.join(ROOT, "oracle", "liboracle.so"), mode=os.RTLD_LOCAL | os.RTLD_NOW)
    dev_api, ora_api = sd.Api(hip, "pga"), sd.Api(ora, "pgo")
    hip.pga_selftest_loop_route.restype, hip.pga_selftest_loop_route.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
    for name in sys.argv[1:] or lc.NAMES:
        sh = lc.shard(name)
        opn = lc.open_hits(sh)
        if not opn.any():
            sd.fail(sh.name, "no hit of the shard is open: the case proves nothing")
        want = sd.run(ora_api, sh)
        # the open hits that are not filtered when pg_shadow(0) runs (the sweep leaves flt alone: the flags behind it say which), by X position
        live = (want["3a", "flags"] & sw.F_FLT) == 0
        goff = np.asarray(sh.goff, np.int64)
        gx = goff[np.searchsorted(goff, np.arange(sh.N), side="right") - 1] + want["3a", "pos_x"]  # (the downloads are in file order; pos_x counts inside the genome)
        n_want = int((opn[gx] & live).sum())
        if n_want == 0:
            sd.fail(sh.name, "every open hit is filtered before pg_shadow(0): the case proves nothing")
        for form in ("0", "1"):
            got, route = routed(dev_api, hip, sh, form)
            sd.compare(sh, got, want)
            if route[1] != int(form) or route[2] != (n_want if form == "1" else 0):
                sd.fail(sh.name, "form %s: the hook reports %d inline sweeps and %d inline hits, expected %d and %d (route %s)" % (form, route[1], route[2], int(form), n_want if form == "1" else 0, route))
        for forms in (("0", "1", "1", "0"), ("1", "0", "0", "1")):
            w = sequence(ora_api, sh, (None,) * 4)
            g = sequence(dev_api, sh, forms)
            for k, (a, b) in enumerate(zip(g, w)):
                for what, x, y in zip(("flags", "pid_dom", "stats"), a, b):
                    if not np.array_equal(x, y):
                        sd.fail(sh.name, "sequence %s, sweep %d, %s: first difference at %d" % ("".join(forms), k, what, int(np.flatnonzero((x != y).reshape(len(x), -1).any(axis=1))[0])))
        print("%s: ok  %d hits, %d open, %d of them evaluated by the inline form" % (sh.name, sh.N, int(opn.sum()), n_want), flush=True)
    print("ALL OK", flush=True)


if __name__ == "__main__":
    main()
