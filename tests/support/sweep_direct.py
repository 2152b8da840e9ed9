"""TEST INFRASTRUCTURE: the overlap sweep and stage A's filters of the HIP backend against the plain-C oracle on the shards of
tests/support/sweep_ref.py, for tests/test_sweep_gpu.py, run in a child process of its own: the switches that choose the route (PANGENE_SWEEP_LISTS,
PANGENE_MERGE_LITERAL, PANGENE_FILTERS, PANGENE_POISON) are read once per process.  Both libraries are loaded, and for every shard the same script
is driven through pga_* and pgo_* from the same ctypes structs:

    1  create, begin (set_head where the shard names a head), ingest(stats[4 G]); download, hazards, hazard_segs
    2  post_partials, fetch of max_ori[P] and sums[6 P]; post_apply(rep, pj, &n_pseudo) with rep / pj drawn from the shard's name;
       set_filter(PSEUDO), shadow(1, stats[2 G]); download
    3  flag_vtx(g2s, n_seg, then_filter = 1), about 70 % of the genes with a segment; shadow(0, stats[2 G]); download;
       set_filter(SHADOW); download; hazards, hazard_segs
    4  begin again, ingest(NULL); download -- on the HIP side it must equal the download of step 1
    5  destroy

After every download all eight arrays are compared for EVERY hit, filtered ones included (flags: the public bits), and the statistics, n_pseudo,
max_ori and sums, all with integer equality.  Hazards: h1, h2_cm, h2_cs equal; h3 of the device >= the oracle's and, while both lists are complete,
its segments a superset of the oracle's (the device also reports ties among keys that do not end as the maximum); both 0 on halo* and round.
The hook pga_selftest_sweep_route says which builds ran.  Prints one line per shard and "ALL OK"; exits 1 at the first difference, naming shard,
step, array and first index.

    python tests/support/sweep_direct.py [--lists auto|lds|global] [--filters global|k32|k64] [shard ...]

--lists / --filters: what the hook must report for the environment the child runs in."""
import argparse
import ctypes as C
import os
import sys
import time
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import stage_a_ref as sr  # noqa: E402
import sweep_ref as sw  # noqa: E402

HAZARD_CAP = 4096
FLT_PSEUDO, FLT_SHADOW = 0, 3
STATE = ("flags", "rank", "score_dom", "pid_dom", "pid_dom0", "pos_x", "pos_y", "flt_x_bits")


class Hazard(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("h1", "h2_cm", "h2_cs", "h3")]


class Api:
    SIG = dict(create=[C.c_void_p, C.c_void_p, C.c_void_p], begin=[C.c_void_p], ingest=[C.c_void_p, C.c_void_p], post_partials=[C.c_void_p, C.c_void_p, C.c_void_p],
               fetch=[C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t], post_apply=[C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], set_filter=[C.c_void_p, C.c_int32],
               shadow=[C.c_void_p, C.c_int32, C.c_void_p], flag_vtx=[C.c_void_p, C.c_void_p, C.c_int32, C.c_int32], set_head=[C.c_void_p, C.c_void_p],
               download=[C.c_void_p, C.c_void_p], hazards=[C.c_void_p, C.c_void_p], hazard_segs=[C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p])

    def __init__(self, lib, pfx):
        self.pfx = pfx
        for k, args in self.SIG.items():
            f = getattr(lib, "%s_%s" % (pfx, k))
            f.restype, f.argtypes = C.c_int, args
            setattr(self, "_" + k, f)
        self.destroy = getattr(lib, pfx + "_destroy")
        self.destroy.restype, self.destroy.argtypes = None, [C.c_void_p]

    def __getattr__(self, k):  # every call must answer 0
        f = object.__getattribute__(self, "_" + k)

        def call(*a):
            rc = f(*a)
            if rc != 0:
                fail(self.shard, "%s_%s returned %d" % (self.pfx, k, rc))
        return call


def fail(shard, what):
    print("%s: DIFFERENT: %s" % (shard, what), flush=True)
    sys.exit(1)


def ptr(a):
    return a.ctypes.data


def drawn(sh):
    """rep / pj / g2s of a shard, from its name"""
    rng = np.random.default_rng(zlib.crc32(sh.name.encode()))
    rep, pj = (rng.random(sh.P) < 0.7).astype(np.uint8), (rng.random(sh.P) < 0.2).astype(np.uint8)
    keep = rng.random(sh.Q) < 0.7
    for g, k in getattr(sh, "g2s_force", {}).items():
        keep[g] = k
    g2s = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    return rep, pj, g2s, int(keep.sum())


def run(api, sh):
    """the script through one backend: {(step, name): array}"""
    api.shard = sh.name
    out = {}
    N, G, P = sh.N, sh.G, sh.P
    rep, pj, g2s, n_seg = drawn(sh)

    def download(step):
        a = {k: np.full(N, -9, np.int32) for k in STATE[1:7]}
        a["flags"], a["flt_x_bits"] = np.full(N, 0xffffffff, np.uint32), np.full((N + 63) // 64, 0xffffffffffffffff, np.uint64)
        st = sr.HitState(**{k: ptr(v) for k, v in a.items()})
        api.download(ctx, C.byref(st))
        a["flags"] = a["flags"] & sw.PUBLIC
        for k in STATE:
            out[step, k] = a[k]

    def hazards(step):
        hz, segs, n_tot = Hazard(), np.full(HAZARD_CAP, -1, np.int32), C.c_int64(-1)
        api.hazards(ctx, C.byref(hz))
        api.hazard_segs(ctx, ptr(segs), HAZARD_CAP, C.byref(n_tot))
        out[step, "hazards"] = np.array([hz.h1, hz.h2_cm, hz.h2_cs, hz.h3], np.int64)
        out[step, "hazard_segs"] = (int(n_tot.value), segs[:max(0, min(HAZARD_CAP, int(n_tot.value)))].copy())

    def begin():
        api.begin(ctx)
        if hasattr(sh, "head_file"):
            api.set_head(ctx, ptr(sh.head_file))

    ctx = C.c_void_p()
    api.create(C.byref(ctx), C.byref(sh.c), C.byref(sh.par))
    begin()
    stats = np.full((G, 4), -1, np.int32)
    api.ingest(ctx, ptr(stats))
    out["1", "stats"] = stats
    download("1")
    hazards("1")
    p_max, p_sums = C.c_void_p(), C.c_void_p()
    api.post_partials(ctx, C.byref(p_max), C.byref(p_sums))
    max_ori, sums = np.full(P, -1, np.int32), np.full(6 * P, -1, np.int64)
    api.fetch(ctx, ptr(max_ori), p_max, max_ori.nbytes)
    api.fetch(ctx, ptr(sums), p_sums, sums.nbytes)
    out["2", "max_ori"], out["2", "sums"] = max_ori, sums
    n_pseudo = C.c_int64(-1)
    api.post_apply(ctx, ptr(rep), ptr(pj), C.byref(n_pseudo))
    out["2", "n_pseudo"] = np.array([n_pseudo.value])
    api.set_filter(ctx, FLT_PSEUDO)
    stats = np.full((G, 2), -1, np.int32)
    api.shadow(ctx, 1, ptr(stats))
    out["2", "stats"] = stats
    download("2")
    api.flag_vtx(ctx, ptr(g2s), n_seg, 1)
    stats = np.full((G, 2), -1, np.int32)
    api.shadow(ctx, 0, ptr(stats))
    out["3a", "stats"] = stats
    download("3a")
    api.set_filter(ctx, FLT_SHADOW)
    download("3b")
    hazards("3b")
    begin()
    api.ingest(ctx, None)
    download("4")
    api.destroy(ctx)
    return out


def compare(sh, dev, ora):
    name = sh.name
    for key, w in ora.items():
        g = dev[key]
        what = "step %s, %s" % key
        if key[1] == "hazards":
            if not np.array_equal(g[:3], w[:3]):
                fail(name, "%s: h1, h2_cm, h2_cs are %s on the device, %s in the oracle" % (what, g[:3].tolist(), w[:3].tolist()))
            if g[3] < w[3]:
                fail(name, "%s: h3_dom_tie is %d on the device, below the oracle's %d" % (what, g[3], w[3]))
            if (name.startswith("halo") or name == "round") and (g[3] or w[3]):
                fail(name, "%s: h3_dom_tie is %d / %d on a shard without ties" % (what, g[3], w[3]))
            continue
        if key[1] == "hazard_segs":
            if g[0] < w[0]:
                fail(name, "%s: %d events on the device, %d in the oracle" % (what, g[0], w[0]))
            if g[0] <= HAZARD_CAP and w[0] <= HAZARD_CAP and not set(w[1].tolist()) <= set(g[1].tolist()):
                fail(name, "%s: the oracle's segments %s are not among the device's" % (what, sorted(set(w[1].tolist()) - set(g[1].tolist()))[:10]))
            continue
        g2, w2 = g.reshape(len(g), -1), w.reshape(len(w), -1)
        if g2.shape != w2.shape or not np.array_equal(g2, w2):
            bad = np.flatnonzero((g2 != w2).any(axis=1))
            k = int(bad[0])
            extra = ""
            if len(g) == sh.N and key[1] != "flt_x_bits":
                extra = ", flags there %#x (%d of the %d are filtered hits)" % (int(ora[key[0], "flags"][k]), int((ora[key[0], "flags"][bad] & sw.F_FLT != 0).sum()), len(bad))
            fail(name, "%s at %d (of %d; %d differ): device %s, oracle %s%s" % (what, k, len(g), len(bad), g2[k].tolist(), w2[k].tolist(), extra))
    if name.startswith("head"):  # overlap.c:108, said outright: after the winners are filtered only the hit at index 0 keeps the SHADOW bit of the sweep before
        f = {k: int(sh.goff[-2] + sh.genomes[-1].file_of[v - sw.PRE]) for k, v in sh.mark.items()}
        kept, cleared = ("h1", "h0") if name == "head2" else ("h0", "h1")
        for side, o in (("device", dev), ("oracle", ora)):
            b2, b3 = o["2", "flags"], o["3a", "flags"]
            if not (b2[f["h0"]] & b2[f["h1"]] & sw.F_SHADOW and b3[f["w0"]] & b3[f["w1"]] & sw.F_FLT and b3[f[kept]] & sw.F_SHADOW and not b3[f[cleared]] & (sw.F_SHADOW | sw.F_FLT)):
                fail(name, "step 3a, %s: SHADOW of %s must stand and that of %s be cleared once their winners are filtered: flags %#x %#x (step 2: %#x %#x)" % (
                    side, kept, cleared, int(b3[f[kept]]), int(b3[f[cleared]]), int(b2[f[kept]]), int(b2[f[cleared]])))
    for k in STATE:  # the run without statistics and the second pass over one upload leave what the first left
        if not np.array_equal(dev["4", k], dev["1", k]):
            fail(name, "step 4, %s: the second begin + ingest(NULL) leaves another array than the first begin + ingest(stats), first at %d" % (k, int(np.flatnonzero(dev["4", k] != dev["1", k])[0])))


def check_route(sh, route, a):
    lists_in_lds, density_known, any_multi, exon_regular, gf_ok, gf_k32 = route
    multi = int(any((g.nex != 1).any() for g in sh.genomes))
    bad = []
    if any_multi != multi:
        bad.append("any_multi %d" % any_multi)
    if exon_regular != (sh.name != "odd"):
        bad.append("exon_regular %d" % exon_regular)
    if multi and not density_known:
        bad.append("density_known 0")
    if multi and a.lists == "lds" and not lists_in_lds or multi and a.lists == "global" and lists_in_lds:
        bad.append("lists_in_lds %d under PANGENE_SWEEP_LISTS=%s" % (lists_in_lds, a.lists))
    if a.lists == "auto" and sh.name in ("exons", "sparse") and lists_in_lds != (sh.name == "exons"):
        bad.append("lists_in_lds %d by the sampled density" % lists_in_lds)
    if a.filters == "global" and gf_ok or a.filters != "global" and not gf_ok:
        bad.append("gf_ok %d" % gf_ok)
    if a.filters == "k32" and gf_k32 != (sh.name not in ("filters_neg", "filters_big")) or a.filters in ("k64", "") and gf_k32:
        bad.append("gf_k32 %d" % gf_k32)
    if bad:
        fail(sh.name, "the route is not the one this environment asks for: %s (hook: %s)" % (", ".join(bad), list(route)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lists", default="")
    ap.add_argument("--filters", default="")
    ap.add_argument("shards", nargs="*")
    a = ap.parse_args()
    from pangene_amd import capi
    hip = C.CDLL(capi.LIB_HIP, mode=os.RTLD_LOCAL | os.RTLD_NOW)
    ora = C.CDLL(os.path.join(ROOT, "oracle", "liboracle.so"), mode=os.RTLD_LOCAL | os.RTLD_NOW)
    dev_api, ora_api = Api(hip, "pga"), Api(ora, "pgo")
    hip.pga_selftest_sweep_route.restype, hip.pga_selftest_sweep_route.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
    t_all = time.time()
    for name in a.shards or sw.NAMES:
        t0 = time.time()
        sh = sw.make(name)
        t1 = time.time()
        want = run(ora_api, sh)
        t2 = time.time()
        route = np.full(6, -1, np.int32)
        real_destroy = dev_api.destroy

        def destroy(ctx):  # the hook reads the context at the end of the script
            if hip.pga_selftest_sweep_route(ctx, route.ctypes.data) != 0:
                fail(name, "pga_selftest_sweep_route failed")
            real_destroy(ctx)
        dev_api.destroy = destroy
        got = run(dev_api, sh)
        dev_api.destroy = real_destroy
        t3 = time.time()
        compare(sh, got, want)
        check_route(sh, route.tolist(), a)
        n_flt = [int((want[s, "flags"] & sw.F_FLT != 0).sum()) for s in ("1", "2", "3a", "3b")]
        print("%s: ok  %d hits, filtered after each step %s, shadowed %d, h3 %d / %d, route %s  [%.2f s: shard %.2f, oracle %.2f, device %.2f]" % (
            name, sh.N, n_flt, int(want["2", "stats"][:, 1].sum()), int(got["3b", "hazards"][3]), int(want["3b", "hazards"][3]), route.tolist(), time.time() - t0, t1 - t0, t2 - t1, t3 - t2), flush=True)
    print("%.1f s" % (time.time() - t_all))
    print("ALL OK", flush=True)


if __name__ == "__main__":
    main()
