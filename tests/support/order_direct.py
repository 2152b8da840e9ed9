"""TEST INFRASTRUCTURE: the exact-order overrides of the HIP backend -- pga_override_order, pga_set_head, pga_hazard_segs (pga_host_order.hpp, k_order.hpp,
k_pack_wrec_list / k_walk_list of k_genes.hpp) -- against the plain-C oracle and against the plain restatement of tests/support/order_ref.py, for
tests/test_order_gpu.py, in a child process of its own.  Both libraries are loaded and the same script is driven through pga_* and pgo_* from the same
structs; the overrides stand where graph_driver.cpp has them:

    0  create, begin; set_head where the shard names one; the cs override "0" in front of ingest (nothing stands yet); set_head again where the shard
       says so; ingest, post_partials, post_apply, set_filter(PSEUDO), shadow(1), vtx_partials, flag_vtx(then_filter = 1)
    1  the cm override "1cm"; arc_round_local + arc_table (every field of every record, seg_cnt, deg); the cs override "1cs" behind the round: the
       gene-major index, the walk's records and the half-arcs stand
    2  rep_pos, n_local over the shard's pairs, arc_set_current with the round's table, branch_pairs(NULL) + branch_decide
    3  the cm override "3cm", mark_hits(then_filter = 1): n_marked; the cs override "3cs"
    4  a second arc_round_local + table (its sweep runs behind the cs override); set_filter(SHADOW)
    5  a round (so that everything stands), then the shard's burst of overrides back to back with nothing in between ("5.0", "5.1", ..: by default a
       small one, one of every contig, a small one: both halves of the page-locked area and their events, its regrowth behind a wait); a round + table
    6  an override of no segment ("6a"), one of empty contigs only ("6b"), each with a round + table behind it; every contig in cs order ("6c") and in cm
       order ("6d"); a round + table, rep_pos, n_local

After every override and every step pga_download: all eight state arrays of EVERY hit are equal between the backends, and pos_x / pos_y are what
order_ref.override_restate says.  Tables, seg_cnt, deg, n_pairs, arc_weak, n_dist_loci, n_flt, n_marked: equal; n_local: cnt > 0 element by element (the
ABI specifies no more).  Hazards, after every step: h1 equal; h2_cm zero together (the oracle counts an equal-cm adjacency once per walk over it, the
device keeps a walk that still stands and counts a re-walked adjacency again) and equal behind the first round; h2_cs: rep_pos alone raises it by the
same number on both (steps "2r", "6r", "Tr"), over all the device's <= the oracle's (its n_local stops at the first certain genome) and > 0 behind rep_pos on `strand` (one gene twice in a tie group: the immediate hazard); the device's h3 >= the oracle's; hazard_segs:
the oracle's segments among the device's while both lists are complete and both count the same h2_cs events.

On the device, after every override, the hooks pga_selftest_stage_a + pga_selftest_order are compared with the restatement hit by hit: fidx, gnm, yperm,
inv, headpos; recA {cs, seg, ce} and pm; recB and recC as they stood before the override, moved with their hit; F_CSTIE and F_HEAD in the raw flag words;
where the gene-major index stands zx[zpos[p]] == p for its NL members and zpos == -1 for the others; under live lists lx at every contig's start, ylist =
the members in cm order, cx = the members in X order and cA / cB / cC = the full records of the same members with pm over the members.  The route
record of every override is held against what the step is there for (`want_route`).

Second, on the device alone: a context in which the orders that stand after "3cm" were applied right behind flag_vtx, before anything was built, and one
in which they arrived as in the script give the same round, table, n_local, arc_weak and n_marked (not on `head`: the hit at index 0 keeps the SHADOW
bit of the sweep before it became that, which the two histories set differently).

Prints one line per shard and "ALL OK"; exits 1 at the first difference, naming shard, step, array and first index.

    python tests/support/order_direct.py [--live 0|1] [--sort-path] [--lib PATH] [--until STEP] [shard ...]

--live, --sort-path: what the hook must report for the environment (on the sort path no round leaves half-arcs: no partial walk behind a round); --lib: another build of the HIP library (a scratch build with a deliberately wrong kernel must
fail here); --until: the script ends behind that step (4: no override of every contig), and only the script itself is compared."""
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
import arcs_direct as ad  # noqa: E402
import order_ref as orf  # noqa: E402
from arcs_direct import P, I32, I64, ptr, fail, ARC, STATE, PUBLIC, FLT_PSEUDO, FLT_SHADOW  # noqa: E402

HAZARD_CAP = 4096
ROUTE = ("which", "T", "z_keep", "wrec_ok", "partial", "live", "grew", "ov_seq")


class Api(ad.Api):
    SIG = dict(ad.Api.SIG, override_order=[P, I32, I32, P, P, P, P], set_head=[P, P], hazard_segs=[P, P, I32, P])


class StageA(C.Structure):  # pga_selftest_stage_a_t
    _fields_ = [(k, P) for k in ("recA", "recB", "recC", "flags", "fidx", "gnm", "yperm", "headpos")] + [(k, C.c_uint32) for k in ("f_head", "f_multi", "f_cstie")] + \
               [("route", I32), ("n_unit", I32 * 3), ("n_cu", I32)]


class OrderOut(C.Structure):  # pga_selftest_order_t
    _fields_ = [(k, P) for k in ("inv", "zpos", "zx", "lx", "ylist", "cA", "cB", "cC", "cx")] + \
               [(k, I32) for k in ("NL", "live_on", "z_valid", "inv_valid", "wrec_valid", "ha_valid", "zposy_stale")] + [("route", I32 * 8), ("f_member", C.c_uint32)]


def make_hook(hip):
    hip.pga_selftest_stage_a.restype, hip.pga_selftest_stage_a.argtypes = C.c_int, [P, P]
    hip.pga_selftest_order.restype, hip.pga_selftest_order.argtypes = C.c_int, [P, P]

    def hook(ctx, sh):
        N, G = sh.N, sh.G
        a = {k: np.full((N, 4), -7, np.int32) for k in ("recA", "recB", "recC", "cA", "cB", "cC")}
        a.update({k: np.full(N, -7, np.int32) for k in ("fidx", "gnm", "yperm", "inv", "zpos", "zx", "ylist", "cx")})
        a["flags"], a["headpos"], a["lx"] = np.zeros(N, np.uint32), np.full(G + 1, -7, np.int32), np.full(N + 1, -7, np.int32)
        s = StageA(**{k: ptr(a[k]) for k in ("recA", "recB", "recC", "flags", "fidx", "gnm", "yperm", "headpos")})
        o = OrderOut(**{k: ptr(a[k]) for k in ("inv", "zpos", "zx", "lx", "ylist", "cA", "cB", "cC", "cx")})
        if hip.pga_selftest_stage_a(ctx, C.byref(s)) != 0 or hip.pga_selftest_order(ctx, C.byref(o)) != 0:
            fail(sh.name, "a self-test hook failed")
        a.update(f_head=s.f_head, f_cstie=s.f_cstie, f_member=o.f_member, NL=o.NL, live_on=o.live_on, z_valid=o.z_valid, inv_valid=o.inv_valid, wrec_valid=o.wrec_valid, ha_valid=o.ha_valid,
                 zposy_stale=o.zposy_stale, route=dict(zip(ROUTE, list(o.route))))
        return a
    return hook


def first_bad(got, want):
    got, want = np.asarray(got), np.asarray(want)
    bad = np.flatnonzero((got.reshape(len(got), -1) != want.reshape(len(want), -1)).any(axis=1))
    return (int(bad[0]), len(bad)) if len(bad) else None


def check_device(sh, st, h, before, label, flt0=None):
    """the device's arrays behind an override against the restatement; before: the hook's arrays in front of it; flt0: the flt bit of every hit (file order) as
    pga_download gave it behind pga_flag_vtx -- nothing is filtered between that and the first building of the live lists"""
    name, N = sh.name, sh.N
    d = orf.derived_restate(sh, st)

    def same(what, got, want):
        if len(got) != len(want):
            fail(name, "step %s, %s: %d entries, %d restated" % (label, what, len(got), len(want)))
        k = first_bad(got, want)
        if k:
            fail(name, "step %s, %s at %d (of %d; %d differ): device %s, restated %s" % (label, what, k[0], len(got), k[1], np.asarray(got)[k[0]].tolist(), np.asarray(want)[k[0]].tolist()))
    file = np.array(d["file"], np.int64)
    same("fidx", h["fidx"], file - sh.goff[np.array(d["gnm"], np.int64)] if N else file)
    same("gnm", h["gnm"], d["gnm"])
    same("yperm", h["yperm"], d["yperm"])
    if h["inv_valid"]:
        same("inv", h["inv"], d["inv"])
    live_g = np.flatnonzero(np.diff(sh.goff) > 0)
    same("headpos", h["headpos"][live_g], np.array(d["headpos"], np.int64)[live_g])
    same("recA {cs, seg, ce}", h["recA"][:, :3], np.stack([d["cs"], d["seg"], d["ce"]], axis=1) if N else np.zeros((0, 3)))
    same("pm (recA word 3)", h["recA"][:, 3], d["pm"])
    # the records in front of the override, by hit
    b_file = sh.goff[before["gnm"].astype(np.int64)] + before["fidx"] if N else file
    at = np.zeros(N, np.int64)
    at[b_file] = np.arange(N)
    same("recB (moved with its hit)", h["recB"], before["recB"][at[file]])
    same("recC (moved with its hit)", h["recC"], before["recC"][at[file]])
    rest = ~np.uint32(h["f_head"] | h["f_cstie"])
    same("the flag words but F_HEAD and F_CSTIE (moved with their hit)", h["flags"] & rest, (before["flags"] & rest)[at[file]])
    same("F_CSTIE", (h["flags"] & h["f_cstie"]) != 0, d["cstie"])
    same("F_HEAD", (h["flags"] & h["f_head"]) != 0, d["head"])
    NL = h["NL"]
    if h["z_valid"]:
        member = h["zpos"] >= 0
        if int(member.sum()) != NL or (not h["live_on"] and NL != N):
            fail(name, "step %s: %d hits have a place in the gene-major index, NL = %d, N = %d, live_on %d" % (label, int(member.sum()), NL, N, h["live_on"]))
        m = np.flatnonzero(member)
        if N:
            if h["zpos"][m].max(initial=-1) >= NL or len(np.unique(h["zpos"][m])) != len(m):
                fail(name, "step %s: zpos is not a bijection of the members onto [0, NL)" % label)
            same("zx[zpos[p]] of the members", h["zx"][h["zpos"][m]], m)
        if h["live_on"]:
            # who is a member, not from the index itself: the hits with the member bit; they were without flt when the lists were built (at the first
            # building exactly the hits without flt behind pga_flag_vtx; only -S builds them a second time, from what is without flt then), and every hit
            # without flt now is one (flt is never taken back)
            same("zpos >= 0 exactly on the hits with F_MEMBER", member, (h["flags"] & h["f_member"]) != 0)
            now = (h["flags"] & ar.F_FLT) == 0
            if (now & ~member).any():
                fail(name, "step %s: the hit at %d is without flt and not in the live lists" % (label, int(np.flatnonzero(now & ~member)[0])))
            if flt0 is not None:
                was = ~flt0[file]
                if (member & ~was).any() or (not sh.par.check_strand and (was & ~member).any()):
                    fail(name, "step %s: the members of the live lists are not the hits that were without flt behind pga_flag_vtx, first at %d" % (label, int(np.flatnonzero(member != was)[0])))
            seg = np.array(d["seg"], np.int64)
            starts = np.flatnonzero(np.concatenate([[True], seg[1:] != seg[:-1]])) if N else np.zeros(0, np.int64)
            before_x = np.concatenate([[0], np.cumsum(member)])
            same("lx at the contigs' starts", h["lx"][starts], before_x[starts])
            yp = np.array(d["yperm"], np.int64)
            same("ylist (the members in cm order)", h["ylist"][:NL], yp[member[yp]])
            same("cx (the members in X order)", h["cx"][:NL], m)
            same("cB (the members' records)", h["cB"][:NL], h["recB"][m])
            same("cC (the members' records)", h["cC"][:NL], h["recC"][m])
            same("cA {cs, seg, ce}", h["cA"][:NL, :3], h["recA"][m, :3])
            pm, sg, ce = [0] * len(m), seg[m].tolist(), h["recA"][m, 2].tolist()
            for k in range(len(m)):
                pm[k] = ce[k] if k == 0 or sg[k - 1] != sg[k] else max(pm[k - 1], ce[k])
            same("cA pm (over the members)", h["cA"][:NL, 3], pm)


def want_route(sh, label, seg, r, h, live_env, sort_path=False):
    """what the step is there for; None, or what is wrong.  h: the hook's words in front of the override.  sort_path: the rounds of this environment leave no
    half-arcs (PANGENE_ARC_SORT_PATH=1), so an override behind a round finds none standing: it packs the walk's records again and walks nothing again; rep_pos
    walks for itself, so "3cm" finds half-arcs in every environment"""
    strand, pieced = bool(sh.par.check_strand), bool(len(sh._v))
    small = seg.T * 8 <= sh.N
    bad = []

    def must(k, v):
        if r[k] != int(v):
            bad.append("%s %d, not %d" % (k, r[k], int(v)))
    must("which", seg.which), must("T", seg.T if seg.n else 0)
    keeps = seg.which == 1 or not strand  # -S drops the index with a cs override
    if label == "0":  # nothing stands: no index, no records, no half-arcs
        must("z_keep", 0), must("wrec_ok", 0), must("partial", 0), must("live", 0)
    if label in ("1cs", "5.0") and not sort_path:  # behind a round everything stands
        must("z_keep", keeps), must("wrec_ok", keeps), must("partial", keeps and not pieced and small)
    if label in ("1cs", "5.0") and sort_path:  # a round on the sort path builds nothing of it: what stood in front of the round stands, never the half-arcs
        stands = keeps and h["z_valid"]
        must("z_keep", stands), must("wrec_ok", stands and h["wrec_valid"] and not h["zposy_stale"]), must("partial", 0)
    if label == "3cm" and not strand:  # behind 1cs, which packed the records again, and rep_pos, which walks when no walk stands
        must("z_keep", 1), must("wrec_ok", 1), must("partial", not pieced and small)
    if label in ("1cs", "3cm") and sh.name in orf.PARTIAL + ("eighth1", "pm") and not (sort_path and label == "1cs"):  # what the shard is named for, whatever its sizes have become
        must("wrec_ok", 1), must("partial", sh.name in orf.PARTIAL)
    if label == "3cs":  # mark_hits(then_filter) has dropped the half-arcs
        must("partial", 0), must("z_keep", not strand)
        if not strand:
            must("wrec_ok", 1)
    if label == "6a":  # no segment
        must("T", 0), must("wrec_ok", 0), must("partial", 0)
    if label == "6b":  # empty contigs, behind a round: what stood stands again (a round on the sort path packs no walk records and leaves no half-arcs)
        must("T", 0), must("z_keep", h["z_valid"] if sort_path else 1), must("wrec_ok", not sort_path), must("partial", not pieced and not sort_path)  # (-S on the sort path: no round builds the index a cs override dropped)
    if label == "6c":
        must("T", sh.N), must("partial", 0)
    if label.startswith("5."):
        must("ov_seq", sh.seq0 + int(label[2:]) + 1)
    must("live", h["live_on"] and r["z_keep"])
    if live_env >= 0 and h["z_valid"] and h["live_on"] != live_env:
        bad.append("live_on %d under PANGENE_LIVE_LISTS=%d" % (h["live_on"], live_env))
    if sh.name == "live" and live_env != 0 and not sort_path and label == "1cs" and not h["live_on"]:  # (the lists are built with the index, which a sort-path round does not build)
        bad.append("the live lists are not on though at most three hits in four were left at the vertex step")
    return ", ".join(bad) if bad else None


def run(api, sh, hook=None, ident=False, mode="script", orders=None, live_env=-1, until=9, sort_path=False):
    """the script through one backend: {(step, name): array}.  ident: True: every override hands over the canonical order; "cm" / "cs": those of that kind do.  mode "incr": steps 0 .. "3cm", then the
    tail; "flat": step 0, then `orders` = ({(genome, start): files} of the cs order, of the cm order) at once, then the tail; until: the last step to run"""
    api.shard = sh.name
    out, used = {}, []
    N, S = sh.N, sh.n_seg
    ctx = C.c_void_p()
    st, rng = orf.State(sh), orf.seed(sh)
    sh.seq0 = 0

    def download(step):
        a = {k: np.full(N, -9, np.int32) for k in STATE[1:7]}
        a["flags"], a["flt_x_bits"] = np.full(N, 0xffffffff, np.uint32), np.full((N + 63) // 64, 0xffffffffffffffff, np.uint64)
        s = sr.HitState(**{k: ptr(v) for k, v in a.items()})
        api.download(ctx, C.byref(s))
        a["flags"] = a["flags"] & PUBLIC
        for k in STATE:
            out[step, k] = a[k]
        px, py = orf.positions(sh, st)
        for k, w in (("pos_x", px), ("pos_y", py)):
            bad = first_bad(a[k], w)
            if bad:
                fail(sh.name, "step %s, %s_download %s at %d (%d differ): %d, restated %d" % (step, api.pfx, k, bad[0], bad[1], int(a[k][bad[0]]), int(w[bad[0]])))

    def hazards(step):
        hz, segs, n_tot = ad.Hazard(), np.full(HAZARD_CAP, -1, np.int32), C.c_int64(-1)
        api.hazards(ctx, C.byref(hz))
        api.hazard_segs(ctx, ptr(segs), HAZARD_CAP, C.byref(n_tot))
        out[step, "hazards"] = np.array([hz.h1, hz.h2_cm, hz.h2_cs, hz.h3], np.int64)
        out[step, "hazard_segs"] = (int(n_tot.value), segs[:max(0, min(HAZARD_CAP, int(n_tot.value)))].copy())

    def set_head(hf, label):
        hf = np.ascontiguousarray(hf, np.int32)
        api.set_head(ctx, ptr(hf))
        orf.set_head_restate(st, hf.tolist())
        if hook:
            h = hook(ctx, sh)
            check_device(sh, st, h, h, label)

    def override(label, which, items):
        seg = items if isinstance(items, orf.Seg) else orf.segs(sh, which, items, rng, ident is True or ident == ("cm" if which else "cs"))
        orf.check_contract(sh, seg)
        before = hook(ctx, sh) if hook else None
        api.override_order(ctx, seg.which, seg.n, ptr(seg.genome), ptr(seg.start), ptr(seg.off), ptr(seg.file))
        orf.override_restate(st, seg.which, seg)
        used.append((label, seg))
        if hook:
            h = hook(ctx, sh)
            out[label, "route"] = h["route"]
            bad = want_route(sh, label, seg, h["route"], before, live_env, sort_path)
            if bad:
                fail(sh.name, "step %s: the override did not take the route the step is there for: %s (route %s; before it: z_valid %d, wrec_valid %d, ha_valid %d, zposy_stale %d, live_on %d)" % (
                    label, bad, h["route"], before["z_valid"], before["wrec_valid"], before["ha_valid"], before["zposy_stale"], before["live_on"]))
            if label == "6b" and (h["wrec_valid"] != int(not sort_path) or h["ha_valid"] != int(not len(sh._v) and not sort_path)):
                fail(sh.name, "step 6b: an override of empty contigs must leave the walk's records and the half-arcs standing as they stood: wrec_valid %d, ha_valid %d" % (h["wrec_valid"], h["ha_valid"]))
            check_device(sh, st, h, before, label, (out["0", "flags"] & ar.F_FLT) != 0 if label != "0" else None)
        download(label)
        return seg

    def table(step):
        p, n = C.c_void_p(), C.c_int64(-1)
        api.arc_table(ctx, C.byref(p), C.byref(n))
        t = np.zeros(max(0, n.value), ARC)
        if n.value > 0:
            api.fetch(ctx, ptr(t), p, t.nbytes)
        out[step, "n_arc"] = np.array([n.value])
        for k in ARC.names:
            out[step, "arc." + k] = t[k].copy()
        return int(n.value), p

    def local_round(step):
        seg_cnt, deg = np.full(2 * S, -1, np.int32), np.full(2 * S, -1, np.int32)
        api.arc_round_local(ctx, sh.use_ori, S, ptr(seg_cnt), ptr(deg))
        out[step, "seg_cnt"], out[step, "deg"] = seg_cnt, deg
        n, p = table(step)
        hazards(step)
        download(step)
        return n, p

    def n_local(step):
        pairs = np.ascontiguousarray(sh.pairs, np.int32)
        api.rep_pos(ctx)
        hazards(step + "r")
        for k, (ld, lc, fm) in enumerate(sh.nl_settings):
            p_cnt = C.c_void_p()
            api.n_local(ctx, ptr(pairs), len(pairs), ld, lc, fm, C.byref(p_cnt))
            cnt = np.full(len(pairs), -1, np.int32)
            if len(pairs):
                api.fetch(ctx, ptr(cnt), p_cnt, cnt.nbytes)
            out["%s.%d" % (step, k), "nl_cnt"] = cnt
        hazards(step)

    def branch(step, n_arc, p_table):
        b = sh.branch
        deg = np.full(2 * S, -1, np.int32)
        api.arc_set_current(ctx, p_table, n_arc, S, ptr(deg))  # (arc_weak is defined for the table of arc_set_current: the round's own, as arc_table gave it)
        out[step, "deg_current"] = deg
        p_cnt, n_pairs = C.c_void_p(), C.c_int64(-1)
        api.branch_pairs(ctx, None, None, n_arc, ptr(sh.seg_gid), S, b["diff"], b["local_dist"], b["local_count"], b["frag_mode"], C.byref(p_cnt), C.byref(n_pairs))
        weak, ndl, f1, f2 = np.full(max(1, n_arc), 0xff, np.uint8), np.full(2 * S, -1, np.int32), C.c_int64(-1), C.c_int64(-1)
        api.branch_decide(ctx, b["diff"], b["dist"], b["cut"], ptr(weak), ptr(ndl), C.byref(f1), C.byref(f2))
        out[step, "n_pairs"], out[step, "arc_weak"], out[step, "n_dist_loci"], out[step, "n_flt"] = np.array([n_pairs.value]), weak[:n_arc], ndl, np.array([f1.value, f2.value])

    def marks(step, n_arc, then_filter):
        n_marked = C.c_int64(-1)
        api.mark_hits(ctx, None, None, n_arc, C.byref(n_marked), then_filter)
        out[step, "n_marked"] = np.array([n_marked.value])

    # 0
    api.create(C.byref(ctx), C.byref(sh.c), C.byref(sh.par))
    api.begin(ctx)
    if sh.head1:
        set_head(sh.head1(st), "0.head1")
    old = list(st.head)
    override("0", *sh.ov["0"])
    if sh.head2:
        set_head(sh.head2(st, old), "0.head2")
    api.ingest(ctx, None)
    p_max, p_sums, n_pseudo = C.c_void_p(), C.c_void_p(), C.c_int64(-1)
    api.post_partials(ctx, C.byref(p_max), C.byref(p_sums))
    api.post_apply(ctx, ptr(sh.rep), ptr(sh.pj), C.byref(n_pseudo))
    api.set_filter(ctx, FLT_PSEUDO)
    api.shadow(ctx, 1, None)
    p_cnt, p_rec, n_rec = C.c_void_p(), C.c_void_p(), C.c_int64(-1)
    api.vtx_partials(ctx, C.byref(p_cnt), C.byref(p_rec), C.byref(n_rec))
    api.flag_vtx(ctx, ptr(sh.g2s), S, 1)
    download("0")

    def tail(step):
        n_arc, p_table = local_round(step)
        n_local(step)
        branch(step, n_arc, p_table)
        marks(step, n_arc, 0)
        download(step + "m")

    if mode == "flat":
        cs, cm = orders
        for label, which, o in (("F.cs", 0, cs), ("F.cm", 1, cm)):
            keys = sorted(o)
            override(label, which, orf.Seg(which, [k[0] for k in keys], [k[1] for k in keys], np.concatenate([[0], np.cumsum([len(o[k]) for k in keys])]), [f for k in keys for f in o[k]]))
        tail("T")
        api.destroy(ctx)
        return out, used
    # 1
    override("1cm", *sh.ov["1cm"])
    n_arc, p_table = local_round("1")
    override("1cs", *sh.ov["1cs"])
    # 2
    n_local("2")
    branch("2", n_arc, p_table)
    # 3
    override("3cm", *sh.ov["3cm"])
    if mode == "incr":
        tail("T")
        api.destroy(ctx)
        return out, used
    marks("3", n_arc, 1)
    override("3cs", *sh.ov["3cs"])
    # 4
    local_round("4")
    api.set_filter(ctx, FLT_SHADOW)
    download("4b")
    if until < 5:
        api.destroy(ctx)
        return out, used
    # 5
    local_round("5r")  # (so that the burst's first override finds everything standing)
    if hook:
        sh.seq0 = hook(ctx, sh)["route"]["ov_seq"]
    grew = []
    for k, (which, items) in enumerate(sh.ov["5"]):
        override("5.%d" % k, which, items)
        if hook:
            grew.append(out["5.%d" % k, "route"]["grew"])
    out["5", "grew"] = grew
    local_round("5")
    # 6
    override("6a", 0, [])
    local_round("6a")
    override("6b", 1, [(j, c, "id") for j, g in enumerate(sh.genomes) for c in range(g.n_ctg) if not (g.cid == c).any()])
    local_round("6b")
    every = [(j, c, "perm") for j, g in enumerate(sh.genomes) for c in range(g.n_ctg)]
    override("6c", 0, every)
    override("6d", 1, every)
    local_round("6")
    n_local("6")
    api.destroy(ctx)
    return out, used


def compare(sh, dev, ora):
    name = sh.name
    prev = None
    for key, w in ora.items():
        g = dev[key]
        what = "step %s, %s" % key
        if key[1] == "hazards":
            if key[0] == "1" and (g[1] != w[1] or g[2] != w[2]):  # one walk on either side, no rep_pos yet
                fail(name, "%s: {h2_cm, h2_cs} is %s on the device, %s in the oracle behind the first round" % (what, g[1:3].tolist(), w[1:3].tolist()))
            if key[0].endswith("r") and prev is not None and g[2] - dev[prev][2] != w[2] - ora[prev][2]:  # rep_pos alone: its immediate hazards, one by one
                fail(name, "%s: rep_pos raised h2_cs by %d on the device, by %d in the oracle" % (what, g[2] - dev[prev][2], w[2] - ora[prev][2]))
            prev = key
            if g[0] != w[0] or (g[1] > 0) != (w[1] > 0) or g[2] > w[2] or g[3] < w[3] or (name == "strand" and key[0] == "2" and not g[2] > 0):
                fail(name, "%s: {h1, h2_cm, h2_cs, h3} is %s on the device, %s in the oracle" % (what, g.tolist(), w.tolist()))
            continue
        if key[1] == "hazard_segs":
            if dev[key[0], "hazards"][2] == ora[key[0], "hazards"][2] and g[0] <= HAZARD_CAP and w[0] <= HAZARD_CAP and not set(w[1].tolist()) <= set(g[1].tolist()):
                fail(name, "%s: the oracle's segments %s are not among the device's" % (what, sorted(set(w[1].tolist()) - set(g[1].tolist()))[:10]))
            continue
        if key[1] in ("route", "grew"):
            continue
        if key[1] == "nl_cnt":
            g, w = g > 0, w > 0
        if len(g) == 0 and len(w) == 0:
            continue
        if len(g) != len(w):
            fail(name, "%s: %d entries on the device, %d in the oracle" % (what, len(g), len(w)))
        bad = first_bad(g, w)
        if bad:
            k = bad[0]
            fail(name, "%s at %d (of %d; %d differ): device %s, oracle %s" % (what, k, len(g), bad[1], np.asarray(g)[k].tolist(), np.asarray(w)[k].tolist()))


def final_orders(sh, used):
    """{(genome, start): files} of the last cs and of the last cm override of every contig among `used`"""
    cs, cm = {}, {}
    for label, seg in used:
        if label != "0":
            (cm if seg.which else cs).update({k: v for k, v in orf.seg_orders(seg).items() if v})
    return cs, cm


def same_tail(sh, a, b):
    for key, w in a.items():
        if key[0][0] != "T" or key[1] in ("hazards", "hazard_segs", "route"):
            continue
        g = b[key]
        if len(g) != len(w) or first_bad(g, w):
            k = first_bad(g, w) if len(g) == len(w) else (0, abs(len(g) - len(w)))
            fail(sh.name, "step %s, %s: the orders handed over one by one and the same orders handed over before anything was built leave different results on the device, first at %d (%d differ)" % (key[0], key[1], k[0], k[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--live", type=int, default=-1)
    ap.add_argument("--sort-path", action="store_true")
    ap.add_argument("--lib", default="")
    ap.add_argument("--until", type=int, default=9)
    ap.add_argument("shards", nargs="*")
    a = ap.parse_args()
    from pangene_amd import capi
    hip = C.CDLL(a.lib or capi.LIB_HIP, mode=os.RTLD_LOCAL | os.RTLD_NOW)
    ora = C.CDLL(os.path.join(ROOT, "oracle", "liboracle.so"), mode=os.RTLD_LOCAL | os.RTLD_NOW)
    dev_api, ora_api = Api(hip, "pga"), Api(ora, "pgo")
    hook = make_hook(hip)
    t_all = time.time()
    for name in a.shards or orf.NAMES:
        t0 = time.time()
        sh = orf.make(name)
        t1 = time.time()
        want, _ = run(ora_api, sh, until=a.until)
        t2 = time.time()
        got, used = run(dev_api, sh, hook=hook, live_env=a.live, until=a.until, sort_path=a.sort_path)
        compare(sh, got, want)
        if a.until < 9:
            print("%s: ok  as far as step %d" % (name, a.until), flush=True)
            continue
        grew = [v["grew"] for k, v in got.items() if k[1] == "route"]
        if grew[0] != 1 or got["5", "grew"][-1] != 0 or (name == "grid" and got["5", "grew"].count(1) < 2):  # (grid: T = 1 023 and 4 096 outgrow 1.5 times what came before)
            fail(name, "the page-locked area grew at %s of the script's overrides, at %s of the burst: not at the first, or at the burst's last, or not twice on the way to T = 4 097" % (grew, got["5", "grew"]))
        t3 = time.time()
        if name != "head":
            inc, used_i = run(dev_api, sh, hook=hook, mode="incr", live_env=a.live, sort_path=a.sort_path)
            flat, _ = run(dev_api, sh, hook=hook, mode="flat", orders=final_orders(sh, used_i), live_env=a.live, sort_path=a.sort_path)
            same_tail(sh, inc, flat)
        routes = " ".join("%s:%d%d%d%d" % (k[0], v["z_keep"], v["wrec_ok"], v["partial"], v["live"]) for k, v in got.items() if k[1] == "route")
        print("%s: ok  %d hits, %d overrides, arcs %s, marked %d, routes (z_keep wrec_ok partial live) %s  [%.2f s: shard %.2f, oracle %.2f, device %.2f + %.2f]" % (
            name, sh.N, len(used), [int(want[s, "n_arc"][0]) for s in ("1", "4", "5", "6")], int(want["3", "n_marked"][0]), routes, time.time() - t0, t1 - t0, t2 - t1, t3 - t2,
            time.time() - t3), flush=True)
    print("%.1f s" % (time.time() - t_all))
    print("ALL OK", flush=True)


if __name__ == "__main__":
    main()
