#!/usr/bin/env python3
"""Timing of pangene phylosig on one MI355X ("Phylogenetic signal measured").

    python tests/run_phylosig_timing.py [--no-checker] [--items 100000] [--asm 2000,10000] [--perms 1000] [--reps 3] [--out FILE]

The U-shaped presence model of run_coevo_timing.py (a tenth of the items accessory and lineage-structured, the others core or rare), upgma
over jaccard, g = l = 1, -c 2.  The tree comes from capi.pan_tree and the observed costs from capi.pan_gainloss, once per shape.  Per shape
and for 1, 2 and 4 classes a lane (PANGENE_PHYLOSIG_CLS): the device times of k_ps_ranks, k_ps_cost and k_ps_count from events on the
pool's stream (PANGENE_PHYLOSIG_TIMING: the entry prints them, summed over the batches) and the wall time of pga_pan_phylosig (checks,
packing, upload, the kernels batch by batch, download), each the median of --reps calls after a warm-up; k_ps_cost as ns per replicate
and op, replicates = classes x permutations, ops = 2 A - 1.  Then, with the shipped number of classes a lane, the wall of
capi.pan_phylosig in the product (adds the tree compiler, the packing, the observed costs and the classes) and in the checker build: the
host loops of pan_phylosig.hpp on one core, run on one item of each of --checker-classes classes spread over the sizes with
--checker-perms permutations, less the same call with no permutation, and SCALED by classes x permutations to the full shape, which the
output says."""
import argparse, ctypes as C, json, os, re, sys, tempfile, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
from pangene_amd import capi  # noqa: E402
import pairs_ref as pr  # noqa: E402
import phylosig_ref as ps  # noqa: E402
from phylosig_direct import batch, pga_phylosig_in_t, pga_phylosig_out_t  # noqa: E402
from run_coevo_timing import u_shaped  # noqa: E402


def median(v):
    return sorted(v)[len(v) // 2]


def with_stderr(f):
    """f() with the process's stderr (the library's too) collected: (result, text)"""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            r = f()
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        return r, tmp.read().decode(errors="replace")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-checker", action="store_true")
    ap.add_argument("--items", type=int, default=100000)
    ap.add_argument("--asm", default="2000,10000")
    ap.add_argument("--perms", type=int, default=1000)
    ap.add_argument("--checker-classes", type=int, default=8)
    ap.add_argument("--checker-perms", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs the GPU"
    torch.cuda.init()
    hip = capi.load()
    fn = hip.pga_pan_phylosig
    fn.restype = C.c_int
    res = []
    for A in [int(x) for x in a.asm.split(",")]:
        M, n_perm = a.items, a.perms
        P = u_shaped(M, A, 7)
        t0 = time.perf_counter()
        rec, _ = capi.pan_tree(hip, P, "jaccard", "upgma")
        t_tree = time.perf_counter() - t0
        print("A=%d: tree %.1f s" % (A, t_tree), file=sys.stderr, flush=True)
        kids = pr.tree(rec, A, "upgma")
        op, order, need = pr.program(kids, A)
        obs = capi.pan_gainloss(hip, P, rec, "upgma")
        tested, cls, item_cls = ps.classes(obs["present"], A, 2)
        leaf, cls32, icls32 = np.array(order, dtype=np.int32), cls.astype(np.int32), item_cls.astype(np.int32)
        icost = np.ascontiguousarray(obs["cost"][tested], dtype=np.int32)
        cin = pga_phylosig_in_t(op.ctypes.data, leaf.ctypes.data, A, 1, 1, len(cls32), cls32.ctypes.data, len(icls32), icls32.ctypes.data, icost.ctypes.data, n_perm, 11, None, None)
        cout = pga_phylosig_out_t()

        def call():
            t = time.perf_counter()
            if fn(C.byref(cin), C.byref(cout)) != 0:
                raise RuntimeError("pga_pan_phylosig failed")
            return time.perf_counter() - t
        replicates, n_op = len(cls) * n_perm, 2 * A - 1
        r = {"items": M, "A": A, "tested": int(len(tested)), "classes": int(len(cls)), "perms": n_perm, "stack_need": need, "batch": batch(hip, len(cls)),
             "tree_ms": round(t_tree * 1e3, 3), "replicates": replicates, "ops": n_op, "by_classes_a_lane": {}}
        os.environ["PANGENE_PHYLOSIG_TIMING"] = "1"
        sums = {}
        for k in (1, 2, 4):
            os.environ["PANGENE_PHYLOSIG_CLS"] = str(k)
            call()  # warm-up
            walls, kern = [], {"ranks_ms": [], "cost_ms": [], "count_ms": []}
            for _ in range(a.reps):
                w, text = with_stderr(call)
                walls.append(w)
                line = [ln for ln in text.splitlines() if ln.startswith("[phylosig-kernels]")][-1]
                for name in kern:
                    kern[name].append(float(re.search(name + r"=([0-9.]+)", line).group(1)))
            cost_ms = median(kern["cost_ms"])
            r["by_classes_a_lane"][k] = {"k_ps_ranks_ms": median(kern["ranks_ms"]), "k_ps_cost_ms": cost_ms, "k_ps_count_ms": median(kern["count_ms"]),
                                         "entry_wall_ms": round(median(walls) * 1e3, 3), "k_ps_cost_ns_per_replicate_op": round(cost_ms * 1e6 / (replicates * n_op), 5)}
            print("A=%d: %d classes a lane: %s" % (A, k, r["by_classes_a_lane"][k]), file=sys.stderr, flush=True)
            sums[k] = int(np.ctypeslib.as_array(C.cast(cout.sum, C.POINTER(C.c_int64)), shape=(len(cls),)).sum())
        r["same_sums_for_1_2_4"] = len(set(sums.values())) == 1
        del os.environ["PANGENE_PHYLOSIG_CLS"], os.environ["PANGENE_PHYLOSIG_TIMING"]
        walls = []
        for i in range(a.reps + 1):
            t = time.perf_counter()
            got = capi.pan_phylosig(hip, P, rec, "upgma", 1, 1, n_perm, 11, 2)
            walls.append(time.perf_counter() - t)
        r["product_capi_pan_phylosig_ms"] = round(median(walls[1:]) * 1e3, 3)
        r["sum_n_le"] = int(got["n_le"].sum())
        if not a.no_checker:
            import oracle_host
            ora = oracle_host.load()
            some = cls[np.linspace(0, len(cls) - 1, min(a.checker_classes, len(cls))).astype(np.int64)]  # classes spread over the sizes
            sub = np.array([tested[obs["present"][tested] == n][0] for n in some])  # one item a class: the observed costs take no time beside the replicates
            n_cls_sub = len(np.unique(obs["present"][sub]))
            t = time.perf_counter()
            capi.pan_phylosig(ora, P[sub], rec, "upgma", 1, 1, 0, 11, 2)
            t_none = time.perf_counter() - t
            t = time.perf_counter()
            ref = capi.pan_phylosig(ora, P[sub], rec, "upgma", 1, 1, a.checker_perms, 11, 2)
            t_some = time.perf_counter() - t
            per = (t_some - t_none) / (n_cls_sub * a.checker_perms)
            r["checker_host_loops_ms"] = round(per * replicates * 1e3, 1)
            r["checker_scaled_from"] = "%d classes x %d permutations" % (n_cls_sub, a.checker_perms)
            few = capi.pan_phylosig(hip, P[sub], rec, "upgma", 1, 1, a.checker_perms, 11, 2)
            r["same"] = bool(all(np.array_equal(few[k], ref[k]) for k in ("present", "cost", "tested", "n_le", "n_ge", "sum")))
        print(json.dumps(r), flush=True)
        res.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
