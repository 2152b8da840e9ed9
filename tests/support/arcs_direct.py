"""TEST INFRASTRUCTURE: the vertex step and a host-driven arc and branch round of the HIP backend against the plain-C oracle on the shards of
tests/support/arcs_ref.py, for tests/test_arcs_gpu.py, run in a child process of its own (the switches that choose the route are read once per process).
Both libraries are loaded, and for every shard the same script is driven through pga_* and pgo_* from the same ctypes structs:

    0  create, begin, ingest, post_partials, post_apply(rep, pj), set_filter(PSEUDO), shadow(1): where the driver is before the vertex step
    1  vtx_partials; fetch of cnt[2 Q] and the records
    2  flag_vtx(g2s, n_seg, 1); download
    3  arc_round_local(use_ori, n_seg, seg_cnt, deg); arc_table + fetch; hazards; download
    4  on a fresh begin .. step 2: the deferred form arc_round_local(NULL, NULL), rep_pos queued behind it, arc_round_finish -- status 1: a plain
       arc_round_local and rep_pos again; arc_table + fetch
    5  arc_round (the exchange form) + fetch of seg_cnt and its table; arc_set_current with it: deg
    6  rep_pos; hazards
    7  n_local over the shard's pair list, once for each of its (local_dist, local_count, frag_mode)
    8  branch_pairs(NULL, NULL, n_arc, seg_gid, ...) + branch_decide: n_pairs, arc_weak[n_arc], n_dist_loci[2 S], n_flt1, n_flt2
    9  mark_hits(NULL, NULL, n_arc, &n_marked, 1); download
   10  the second round: arc_round_local, arc_table + fetch, download; set_filter(SHADOW); download
   11  (the hook pga_selftest_arc_route, HIP side only) destroy

Compared with integer equality: cnt and the vertex records after canonicalisation (the sets of a (sub, dom) key ORed, sorted by key; on the device's raw
records the sets of equal keys must be disjoint), seg_cnt, deg, n_arc and every field of every arc record, after every download all eight state arrays for
EVERY hit (flags: the public bits, weak bits included), h2_cm (step 3: equal, or twice the oracle's where the device repeats the round; later: zero
together, see compare), h2_cs, n_pairs, arc_weak, n_dist_loci, n_flt1, n_flt2, n_marked.  n_local: cnt > 0 element by
element -- the ABI specifies no more --, on local* (every pair comparable in one genome only) cnt itself; the device's h2_cs increase <= the oracle's (it
stops at the first certain genome), equal on local*, and above its value after rep_pos on reps* (the H2b events are there).  Steps 4 and 5 must give step 3's table, counters and degrees.  Prints one line per shard and
"ALL OK"; exits 1 at the first difference, naming shard, step, array and first index.

    python tests/support/arcs_direct.py [--sort-path] [--live 0|1] [--walk 1|4] [--table-log2 N] [--lds-vtx 1] [--lib PATH] [shard ...]

The options say what the hook and the statuses must report for the environment the child runs in; --lib: another build of the HIP library (a scratch
build with a deliberately wrong kernel must fail here)."""
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
import arcs_ref as ar  # noqa: E402

PUBLIC = 0x7ff
FLT_PSEUDO, FLT_SHADOW = 0, 3
STATE = ("flags", "rank", "score_dom", "pid_dom", "pid_dom0", "pos_x", "pos_y", "flt_x_bits")
ARC = np.dtype([("x", np.uint64), ("n_genome", np.int32), ("tot_cnt", np.int32), ("sum_dist", np.uint64), ("sum_s1", np.int64), ("sum_s2", np.int64)])  # pga_arc_part_t
assert ARC.itemsize == 40
RP_FULL, RP_COMPACT, RP_WIDE = 0, 1, 2
ROUTE = ("n_big", "overflowed", "table_sparse", "live_on", "NL", "rp_form", "walk_ipt", "lds_vtx")


class Hazard(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("h1", "h2_cm", "h2_cs", "h3")]


P, I32, I64, F64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double


class Api:
    SIG = dict(create=[P, P, P], begin=[P], ingest=[P, P], post_partials=[P, P, P], fetch=[P, P, P, C.c_size_t], post_apply=[P, P, P, P], set_filter=[P, I32], shadow=[P, I32, P],
               vtx_partials=[P, P, P, P], flag_vtx=[P, P, I32, I32], arc_round=[P, I32, P, P, P], arc_set_current=[P, P, I64, I32, P], arc_round_local=[P, I32, I32, P, P],
               arc_round_finish=[P, I32, P, P], arc_table=[P, P, P], rep_pos=[P], n_local=[P, P, I64, I32, I32, I32, P],
               branch_pairs=[P, P, P, I64, P, I32, F64, I32, I32, I32, P, P], branch_decide=[P, F64, F64, F64, P, P, P, P], mark_hits=[P, P, P, I64, P, I32],
               download=[P, P], hazards=[P, P])

    def __init__(self, lib, pfx):
        self.pfx, self.shard, self.hook = pfx, "", None
        for k, args in self.SIG.items():
            f = getattr(lib, "%s_%s" % (pfx, k))
            f.restype, f.argtypes = C.c_int, args
            setattr(self, "_" + k, f)
        self.destroy = getattr(lib, pfx + "_destroy")
        self.destroy.restype, self.destroy.argtypes = None, [P]

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


def canon_records(rec, nw):
    """{(sub << 20 | dom): the OR of its sets}, and whether the sets of equal keys were disjoint"""
    out, disjoint = {}, True
    for r in rec.reshape(-1, 1 + nw).tolist():
        key, bits = r[0], r[1:]
        old = out.setdefault(key, [0] * nw)
        disjoint = disjoint and not any(a & b for a, b in zip(old, bits))
        out[key] = [a | b for a, b in zip(old, bits)]
    keys = sorted(out)
    return np.array([[k] + out[k] for k in keys], np.uint64).reshape(len(keys), 1 + nw), disjoint


def run(api, sh, until=99):
    """the script through one backend: {(step, name): array}; until: the last step to run"""
    api.shard = sh.name
    out = {}
    N, Q, S = sh.N, sh.Q, sh.n_seg
    ctx = C.c_void_p()

    def download(step):
        a = {k: np.full(N, -9, np.int32) for k in STATE[1:7]}
        a["flags"], a["flt_x_bits"] = np.full(N, 0xffffffff, np.uint32), np.full((N + 63) // 64, 0xffffffffffffffff, np.uint64)
        st = sr.HitState(**{k: ptr(v) for k, v in a.items()})
        api.download(ctx, C.byref(st))
        a["flags"] = a["flags"] & PUBLIC
        for k in STATE:
            out[step, k] = a[k]

    def hazards(step):
        hz = Hazard()
        api.hazards(ctx, C.byref(hz))
        out[step, "hazards"] = np.array([hz.h1, hz.h2_cm, hz.h2_cs, hz.h3], np.int64)

    def front():  # steps 0 and 2
        api.begin(ctx)
        api.ingest(ctx, None)
        p_max, p_sums, n_pseudo = C.c_void_p(), C.c_void_p(), C.c_int64(-1)
        api.post_partials(ctx, C.byref(p_max), C.byref(p_sums))
        api.post_apply(ctx, ptr(sh.rep), ptr(sh.pj), C.byref(n_pseudo))
        api.set_filter(ctx, FLT_PSEUDO)
        api.shadow(ctx, 1, None)

    def table(step):
        p, n = C.c_void_p(), C.c_int64(-1)
        api.arc_table(ctx, C.byref(p), C.byref(n))
        t = np.zeros(max(0, n.value), ARC)
        if n.value > 0:
            api.fetch(ctx, ptr(t), p, t.nbytes)
        out[step, "n_arc"] = np.array([n.value])
        for k in ARC.names:
            out[step, "arc." + k] = t[k].copy()
        return int(n.value)

    def local_round(step):
        seg_cnt, deg = np.full(2 * S, -1, np.int32), np.full(2 * S, -1, np.int32)
        api.arc_round_local(ctx, sh.use_ori, S, ptr(seg_cnt), ptr(deg))
        out[step, "seg_cnt"], out[step, "deg"] = seg_cnt, deg
        return table(step)

    api.create(C.byref(ctx), C.byref(sh.c), C.byref(sh.par))
    front()
    # 1
    p_cnt, p_rec, n_rec = C.c_void_p(), C.c_void_p(), C.c_int64(-1)
    api.vtx_partials(ctx, C.byref(p_cnt), C.byref(p_rec), C.byref(n_rec))
    nw = (sh.c.n_genome_global + 63) // 64
    cnt, rec = np.full(2 * Q, -1, np.int32), np.zeros(max(0, n_rec.value) * (1 + nw), np.uint64)
    api.fetch(ctx, ptr(cnt), p_cnt, cnt.nbytes)
    if rec.size:
        api.fetch(ctx, ptr(rec), p_rec, rec.nbytes)
    out["1", "vtx_cnt"] = cnt
    out["1", "vtx_rec"], out["1", "vtx_disjoint"] = canon_records(rec, nw)
    # 2
    api.flag_vtx(ctx, ptr(sh.g2s), S, 1)
    download("2")
    if until < 3:
        api.destroy(ctx)
        return out
    # 3
    local_round("3")
    hazards("3")
    download("3")
    # 4
    front()
    api.vtx_partials(ctx, C.byref(p_cnt), C.byref(p_rec), C.byref(n_rec))  # (the vertex step counts the hits the live lists are decided by)
    api.flag_vtx(ctx, ptr(sh.g2s), S, 1)
    api.arc_round_local(ctx, sh.use_ori, S, None, None)
    api.rep_pos(ctx)
    seg_cnt, deg = np.full(2 * S, -1, np.int32), np.full(2 * S, -1, np.int32)
    rc = api._arc_round_finish(ctx, S, ptr(seg_cnt), ptr(deg))
    if rc not in (0, 1):
        fail(sh.name, "%s_arc_round_finish returned %d" % (api.pfx, rc))
    out["4", "status"] = np.array([rc])
    if api.hook:
        out["4", "route"] = api.hook(ctx)
    if rc == 1:  # the repeat is a plain call; what was queued behind the first one is repeated too
        api.arc_round_local(ctx, sh.use_ori, S, ptr(seg_cnt), ptr(deg))
        api.rep_pos(ctx)
    out["4", "seg_cnt"], out["4", "deg"] = seg_cnt, deg
    table("4")
    # 5
    p_sc, p_arcs, n = C.c_void_p(), C.c_void_p(), C.c_int64(-1)
    api.arc_round(ctx, sh.use_ori, C.byref(p_sc), C.byref(p_arcs), C.byref(n))
    seg_cnt, t, deg = np.full(2 * S, -1, np.int32), np.zeros(max(0, n.value), ARC), np.full(2 * S, -1, np.int32)
    api.fetch(ctx, ptr(seg_cnt), p_sc, seg_cnt.nbytes)
    if n.value > 0:
        api.fetch(ctx, ptr(t), p_arcs, t.nbytes)
    api.arc_set_current(ctx, p_arcs, n.value, S, ptr(deg))
    out["5", "seg_cnt"], out["5", "deg"], out["5", "n_arc"] = seg_cnt, deg, np.array([n.value])
    for k in ARC.names:
        out["5", "arc." + k] = t[k].copy()
    n_arc = int(n.value)
    # 6
    api.rep_pos(ctx)
    hazards("6")
    # 7
    pairs = np.ascontiguousarray(sh.pairs, np.int32)
    for k, (ld, lc, fm) in enumerate(sh.nl_settings):
        p_cnt = C.c_void_p()
        api.n_local(ctx, ptr(pairs), len(pairs), ld, lc, fm, C.byref(p_cnt))
        cnt = np.full(len(pairs), -1, np.int32)
        if len(pairs):
            api.fetch(ctx, ptr(cnt), p_cnt, cnt.nbytes)
        out["7.%d" % k, "nl_cnt"] = cnt
        hazards("7.%d" % k)
    # 8
    b = sh.branch
    p_cnt, n_pairs = C.c_void_p(), C.c_int64(-1)
    api.branch_pairs(ctx, None, None, n_arc, ptr(sh.seg_gid), S, b["diff"], b["local_dist"], b["local_count"], b["frag_mode"], C.byref(p_cnt), C.byref(n_pairs))
    weak, ndl, f1, f2 = np.full(max(1, n_arc), 0xff, np.uint8), np.full(2 * S, -1, np.int32), C.c_int64(-1), C.c_int64(-1)
    api.branch_decide(ctx, b["diff"], b["dist"], b["cut"], ptr(weak), ptr(ndl), C.byref(f1), C.byref(f2))
    out["8", "n_pairs"], out["8", "arc_weak"], out["8", "n_dist_loci"], out["8", "n_flt"] = np.array([n_pairs.value]), weak[:n_arc], ndl, np.array([f1.value, f2.value])
    # 9
    n_marked = C.c_int64(-1)
    api.mark_hits(ctx, None, None, n_arc, C.byref(n_marked), 1)
    out["9", "n_marked"] = np.array([n_marked.value])
    download("9")
    # 10
    local_round("10")
    hazards("10")
    download("10a")
    api.set_filter(ctx, FLT_SHADOW)
    download("10b")
    # 11
    if api.hook:
        out["11", "route"] = api.hook(ctx)
    api.destroy(ctx)
    return out


def compare(sh, dev, ora, repeats=False):
    """repeats: a round of the device is repeated on the sort path in this environment (a gene beyond its table)"""
    name = sh.name
    if not dev["1", "vtx_disjoint"]:
        fail(name, "step 1: two of the device's vertex records have one (sub, dom) key and sets that are not disjoint")
    for key, w in ora.items():
        if key[1] in ("vtx_disjoint", "route"):
            continue
        g = dev[key]
        what = "step %s, %s" % key
        if key[1] == "hazards":
            # h2_cm counts an equal-cm adjacency once per walk over it: the oracle walks in every arc round and in mark_hits, the device keeps a walk while
            # nothing changed and walks twice in a round it repeats on the sort path.  Step 3: equal, twice the oracle's in a repeated round; zero together everywhere.
            if (key[0] == "3" and g[1] != (2 if repeats else 1) * w[1]) or (g[1] > 0) != (w[1] > 0):
                fail(name, "%s: h2_cm is %d on the device, %d in the oracle" % (what, g[1], w[1]))
            if name.startswith("reps") and key[0] == "7.0" and not g[2] > dev["6", "hazards"][2]:
                fail(name, "%s: no H2b event on the device (h2_cs %d as after rep_pos)" % (what, g[2]))
            if name.startswith("local") or (key[0] in ("3", "6") and not repeats):  # (a repeated round repeats the rep_pos queued behind it, and its events)
                if g[2] != w[2]:
                    fail(name, "%s: h2_cs is %d on the device, %d in the oracle" % (what, g[2], w[2]))
            elif key[0] in ("3", "6"):  # a repeated round: one rep_pos more on the device
                if (g[2] > 0) != (w[2] > 0) or g[2] < w[2]:
                    fail(name, "%s: h2_cs is %d on the device, %d in the oracle, in a repeated round" % (what, g[2], w[2]))
            elif g[2] - (dev["6", "hazards"][2] - ora["6", "hazards"][2]) > w[2]:  # from step 7 on: the device's n_local stops at the first certain genome
                fail(name, "%s: h2_cs is %d on the device, above the oracle's %d" % (what, g[2], w[2]))
            continue
        if key[1] == "nl_cnt" and not name.startswith("local"):
            g, w = g > 0, w > 0
        if key == ("4", "status"):
            continue  # the oracle never asks for a repeat; the child asserts the device's status by environment
        if len(g) == 0 and len(w) == 0:
            continue
        g2, w2 = g.reshape(len(g), max(1, g.size // max(1, len(g)))), w.reshape(len(w), max(1, w.size // max(1, len(w))))
        if g2.shape != w2.shape:
            fail(name, "%s: %d entries on the device, %d in the oracle" % (what, len(g), len(w)))
        if not np.array_equal(g2, w2):
            bad = np.flatnonzero((g2 != w2).any(axis=1))
            k = int(bad[0])
            fail(name, "%s at %d (of %d; %d differ): device %s, oracle %s" % (what, k, len(g), len(bad), g2[k].tolist(), w2[k].tolist()))
    for step in ("4", "5"):  # the deferred form and the exchange form give what step 3 gave
        for k in ("seg_cnt", "deg", "n_arc") + tuple("arc." + f for f in ARC.names):
            if not np.array_equal(dev[step, k], dev["3", k]):
                fail(name, "step %s, %s: not what step 3 left on the device" % (step, k))


def key_counts(sh, o):
    """distinct (orientation, target) keys per gene, from the arc table: the out-degrees of its two vertices"""
    deg = o["3", "deg"].astype(np.int64)
    k = np.zeros(sh.Q, np.int64)
    k[sh.seg_gid] = deg[0::2] + deg[1::2]
    return k


def member_counts(sh, o, live):
    """entries per gene of the gene-major index: every hit, or the hits without flt when the lists are built (at the first arc round: after step 2)"""
    gid = np.concatenate([g.pid for g in sh.genomes] + [np.zeros(0, np.int64)])
    keep = (o["2", "flags"] & ar.F_FLT) == 0 if live else np.ones(sh.N, bool)
    return np.bincount(gid[keep], minlength=sh.Q)


def check_route(sh, dev, ora, a):
    name = sh.name
    r4, r = dict(zip(ROUTE, dev["4", "route"].tolist())), dict(zip(ROUTE, dev["11", "route"].tolist()))
    status = int(dev["4", "status"][0])
    keys = key_counts(sh, ora)
    cap = 1 << a.table_log2
    bad = []
    live = r["live_on"]
    members = member_counts(sh, ora, live)
    hub = bool((keys > min(cap, ar.GA_CAP)).any())  # a gene that no table holds: the gene path gives up
    if a.live >= 0 and live != a.live:
        bad.append("live_on %d" % live)
    if r["NL"] != (int(((ora["2", "flags"] & ar.F_FLT) == 0).sum()) if live else sh.N):
        bad.append("NL %d" % r["NL"])
    if (r["NL"] or a.walk == 4) and r["walk_ipt"] != a.walk:
        bad.append("walk form %d" % r["walk_ipt"])
    if a.sort_path:
        if status != 0 or r["table_sparse"] or r4["table_sparse"]:
            bad.append("status %d, table_sparse %d / %d on the sort path" % (status, r4["table_sparse"], r["table_sparse"]))
    elif sh.N:
        if status != int(hub):
            bad.append("status %d of arc_round_finish with at most %d keys a gene and tables of %d" % (status, keys.max(), min(cap, ar.GA_CAP)))
        if r4["overflowed"] != int((keys > min(cap, ar.GA_CAP)).sum()):
            bad.append("%d overflowed genes before the repeat" % r4["overflowed"])
        want_big4 = int(((sh.g2s >= 0) & ((members > ar.GA_WAVE_HITS) | (keys > min(cap, ar.GA_CAP_WAVE)))).sum())
        if r4["n_big"] != want_big4:  # the first round: the genes the wave kernel handed on, for their hits or for their keys
            bad.append("n_big %d behind the deferred round, but %d genes have more than %d hits or more than %d keys" % (r4["n_big"], want_big4, ar.GA_WAVE_HITS, min(cap, ar.GA_CAP_WAVE)))
        if r4["table_sparse"] != 1:
            bad.append("table_sparse %d behind the deferred round" % r4["table_sparse"])
        keys2 = np.zeros(sh.Q, np.int64)  # (the last round is the second one)
        d2 = ora["10", "deg"].astype(np.int64)
        keys2[sh.seg_gid] = d2[0::2] + d2[1::2]
        hub2 = bool((keys2 > min(cap, ar.GA_CAP)).any())
        if r["table_sparse"] != (not hub2):
            bad.append("table_sparse %d after the second round" % r["table_sparse"])
        vtx = sh.g2s >= 0
        want_big = int((vtx & ((members > ar.GA_WAVE_HITS) | (keys2 > min(cap, ar.GA_CAP_WAVE)))).sum())
        if r["n_big"] != want_big:
            bad.append("n_big %d, but %d genes have more than %d hits or more than %d keys" % (r["n_big"], want_big, ar.GA_WAVE_HITS, min(cap, ar.GA_CAP_WAVE)))
    if sh.N and r["lds_vtx"] != a.lds_vtx:
        bad.append("lds_vtx_set != 0 is %d" % r["lds_vtx"])
    if r["rp_form"] != {"reps_full": RP_FULL, "reps_wide": RP_WIDE}.get(name, RP_COMPACT):
        bad.append("rp_form %d" % r["rp_form"])
    if bad:
        fail(name, "the route is not the one this environment asks for: %s (hook: step 4 %s, step 11 %s)" % (", ".join(bad), r4, r))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sort-path", action="store_true")
    ap.add_argument("--live", type=int, default=-1)
    ap.add_argument("--walk", type=int, default=1)
    ap.add_argument("--table-log2", type=int, default=9)
    ap.add_argument("--lds-vtx", type=int, default=0)
    ap.add_argument("--lib", default="")
    ap.add_argument("shards", nargs="*")
    a = ap.parse_args()
    from pangene_amd import capi
    hip = C.CDLL(a.lib or capi.LIB_HIP, mode=os.RTLD_LOCAL | os.RTLD_NOW)
    ora = C.CDLL(os.path.join(ROOT, "oracle", "liboracle.so"), mode=os.RTLD_LOCAL | os.RTLD_NOW)
    dev_api, ora_api = Api(hip, "pga"), Api(ora, "pgo")
    hip.pga_selftest_arc_route.restype, hip.pga_selftest_arc_route.argtypes = C.c_int, [C.c_void_p, C.c_void_p]

    def hook(ctx):
        route = np.full(8, -1, np.int32)
        if hip.pga_selftest_arc_route(ctx, route.ctypes.data) != 0:
            fail(dev_api.shard, "pga_selftest_arc_route failed")
        return route
    dev_api.hook = hook
    t_all, t_ora, t_dev = time.time(), 0.0, 0.0
    for name in a.shards or ar.NAMES:
        t0 = time.time()
        sh = ar.make(name)
        t1 = time.time()
        want = run(ora_api, sh)
        t2 = time.time()
        got = run(dev_api, sh)
        t3 = time.time()
        compare(sh, got, want, repeats=not a.sort_path and bool((key_counts(sh, want) > min(1 << a.table_log2, ar.GA_CAP)).any()))
        check_route(sh, got, want, a)
        t_ora, t_dev = t_ora + t2 - t1, t_dev + t3 - t2
        new_flt = int(((want["9", "flags"] & ar.F_FLT) != 0).sum() - ((want["3", "flags"] & ar.F_FLT) != 0).sum())
        print("%s: ok  %d hits, %d arcs, status %d, %d pairs, flt1 / flt2 %s, marked %d, newly filtered %d, route %s  [%.2f s: shard %.2f, oracle %.2f, device %.2f]" % (
            name, sh.N, int(want["3", "n_arc"][0]), int(got["4", "status"][0]), int(want["8", "n_pairs"][0]), want["8", "n_flt"].tolist(), int(want["9", "n_marked"][0]), new_flt,
            got["11", "route"].tolist(), time.time() - t0, t1 - t0, t2 - t1, t3 - t2), flush=True)
    print("%.1f s: oracle %.1f, device %.1f" % (time.time() - t_all, t_ora, t_dev))
    print("ALL OK", flush=True)


if __name__ == "__main__":
    main()
