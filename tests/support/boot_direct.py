"""TEST INFRASTRUCTURE: direct pga_pan_boot / pg_pan_boot / pg_pan_boot_records cases for tests/test_boot_gpu.py, run in a child process of
their own so that the test can bound them with a timeout.  The product library (HIP kernels of k_boot.hpp and the batched twins of
k_join.hpp) makes bootstrap replicates no GFA fixture reaches; the numpy restatement (tests/support/boot_ref.py) checks them where that
is affordable, the checker build (host loops of tree.cpp) where it is not.  Prints one line per case and "ALL OK" at the end; exits 1 at
the first difference.

    python tests/support/boot_direct.py {draws|resample|wide|groups|joins|large|chunks|parts|metrics|buffers|counts}"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import boot_ref as br  # noqa: E402
import dist_ref as dr  # noqa: E402
import tree_ref as tr  # noqa: E402

M_EDGES = (1, 31, 32, 33, 257, 5000)  # one item; one bit short of a word, a full word, one bit into the next; 9 and 157 words with a ragged last one


class pga_boot_in_t(C.Structure):
    _fields_ = [("bits", C.c_void_p), ("n_item", C.c_int32), ("n_asm", C.c_int32), ("metric", C.c_int32), ("method", C.c_int32), ("seed", C.c_uint32),
                ("first", C.c_int32), ("n_rep", C.c_int32), ("draws", C.c_void_p)]


class pga_boot_out_t(C.Structure):
    _fields_ = [("rec", C.c_void_p), ("n_rec", C.c_int32)]


def bit_rows(P):
    """(M, A) bool -> uint32 (A, W), bit (m & 31) of word m >> 5 of row a = item m is in assembly a"""
    M, A = P.shape
    W = (M + 31) // 32
    pad = np.zeros((W * 32, A), dtype=np.uint8)
    pad[:M] = P
    return np.ascontiguousarray(np.packbits(np.ascontiguousarray(pad.T).reshape(A, W, 32), axis=2, bitorder="little")).view(np.uint32).reshape(A, W)


def entry(lib, P, metric, method, seed, first, n, want_draws=False):
    """pga_pan_boot itself: (status, records (n, n_rec, 6) or None, draws (n, M) or None)"""
    fn = lib.pga_pan_boot
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(pga_boot_in_t), C.POINTER(pga_boot_out_t)]
    M, A = P.shape
    bits = bit_rows(P)
    dw = np.full((max(n, 1), max(M, 1)), -7, dtype=np.int32) if want_draws else None
    cin = pga_boot_in_t(bits.ctypes.data, M, A, 0 if metric == "jaccard" else 2, tr.METHODS.index(method), seed, first, n, dw.ctypes.data if want_draws else None)
    cout = pga_boot_out_t()
    rc = fn(C.byref(cin), C.byref(cout))
    if rc != 0:
        return rc, None, None
    rec = np.ctypeslib.as_array(C.cast(cout.rec, C.POINTER(C.c_int64)), shape=(n, cout.n_rec, 6)).copy() if n else np.zeros((0, cout.n_rec, 6), dtype=np.int64)
    return 0, rec, dw


def batch(lib, A):
    fn = lib.pga_boot_batch
    fn.restype, fn.argtypes = C.c_int32, [C.c_int32]
    return fn(A)


def report(label, what, ok):
    print("%s %s: %s" % (label, what, "ok" if ok else "DIFFERENT"), flush=True)
    if not ok:
        sys.exit(1)


def main():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    from pangene_amd import capi
    import oracle_host
    hip, ora = capi.load(), oracle_host.load()
    which = sys.argv[1]
    if which == "draws":  # the draws hook against the Python integers, two replicates from first = 3
        for M in M_EDGES:
            P = tr.lineage_presence(M, 4, M)
            rc, _, dw = entry(hip, P, "jaccard", "nj", 9, 3, 2, want_draws=True)
            want = np.stack([br.draws(M, 9, 3), br.draws(M, 9, 4)])
            report("draws", "M=%d" % M, rc == 0 and np.array_equal(dw[:, :M], want) and int(want.min()) >= 0 and int(want.max()) < M)
    elif which == "resample":  # the resampled rows, seen through the records of each replicate
        for M in M_EDGES:
            P = tr.lineage_presence(M, 6, 100 + M, flip=0.2)
            for method in tr.METHODS:
                got = capi.pan_boot_records(hip, P, "diff", method, seed=4, first=1, n=3)
                report("resample", "M=%d %s" % (M, method), np.array_equal(got, br.records(P, "diff", method, 4, 1, 3)))
        P = tr.lineage_presence(1000, 7, 5, flip=0.2)
        want = br.records(P, "jaccard", "nj", 4, 1, 3)
        report("resample", "LDS", np.array_equal(capi.pan_boot_records(hip, P, "jaccard", "nj", seed=4, first=1, n=3), want))
        os.environ["PANGENE_BOOT_LDS_WORDS"] = "8"  # 32 words of row against a window of 8: the rows are read from global memory
        report("resample", "global", np.array_equal(capi.pan_boot_records(hip, P, "jaccard", "nj", seed=4, first=1, n=3), want))
        del os.environ["PANGENE_BOOT_LDS_WORDS"]
        P = tr.lineage_presence(300, 6, 8, flip=0.2)
        P[:, 2] = True  # a row with all bits set: every resampled bit of it is set, and none past M
        for metric in tr.METRICS:
            report("resample", "full row " + metric, np.array_equal(capi.pan_boot_records(hip, P, metric, "upgma", seed=1, first=2, n=2), br.records(P, metric, "upgma", 1, 2, 2)))
    elif which == "wide":  # the resampling with several assemblies per workgroup and several workgroups along a row, against the checker build
        # A workgroup of k_boot_resample takes a_per = min(32, A n n_wc / 2048) assemblies, n_wc = ceil(W / 256) workgroups along a row
        # (pga_host_boot.hpp): 1 everywhere else in these tests.  Here a_per is 4 and 32 -- the row staged in LDS again and again
        # between two barriers, the draws reused from registers -- with a last group of assemblies that is not full (301 = 75 x 4 + 1,
        # 40 = 32 + 8), and rows of 313 and 16 250 words (nearly the whole LDS window): 2 and 64 workgroups along a row, the last one
        # with idle threads (57 and 122 words of 256).  The checker build needs seconds for the 26 replicates of the second shape, so
        # it makes the first two and the last of them; the product makes all 26 in one call, which is what sets a_per.
        for A, M, n, a_per, n_wc, metric, method, check in ((301, 10000, 14, 4, 2, "jaccard", "nj", None), (40, 520000, 26, 32, 64, "diff", "upgma", (0, 1, 25))):
            W = (M + 31) // 32
            assert (W + 255) // 256 == n_wc and min(32, A * n * n_wc // 2048) == a_per and n <= batch(hip, A) and W <= 16384
            P = tr.lineage_presence(M, A, 5, flip=0.1)
            if check is None:
                check, want = tuple(range(n)), capi.pan_boot_records(ora, P, metric, method, seed=8, first=2, n=n)
            else:
                want = np.stack([capi.pan_boot_records(ora, P, metric, method, seed=8, first=2 + k, n=1)[0] for k in check])
            got = capi.pan_boot_records(hip, P, metric, method, seed=8, first=2, n=n)
            report("wide", "A=%d M=%d n=%d: %d assemblies a workgroup, LDS" % (A, M, n, a_per), np.array_equal(got[list(check)], want))
            os.environ["PANGENE_BOOT_LDS_WORDS"] = "8"
            report("wide", "the same, rows read from global memory", np.array_equal(capi.pan_boot_records(hip, P, metric, method, seed=8, first=2, n=n), got))
            del os.environ["PANGENE_BOOT_LDS_WORDS"]
        P = tr.lineage_presence(10000, 4, 10000)  # and the draws of a row of two workgroups of words
        rc, _, dw = entry(hip, P, "jaccard", "nj", 9, 3, 2, want_draws=True)
        report("wide", "draws M=10000", rc == 0 and np.array_equal(dw, np.stack([br.draws(10000, 9, 3), br.draws(10000, 9, 4)])))
    elif which == "groups":  # replicate groups inside one call (PANGENE_BOOT_ROWS_WORDS): the same records and draws as one group
        P = tr.lineage_presence(300, 40, 3)  # a replicate's draws and rows: 300 + 40 x 10 = 700 words
        for metric in tr.METRICS:
            for method in tr.METHODS:
                whole = capi.pan_boot_records(hip, P, metric, method, seed=6, first=1, n=7)
                report("groups", "one group, restatement %s %s" % (metric, method), np.array_equal(whole, br.records(P, metric, method, 6, 1, 7)))
                for words, sizes in (("1500", "2, 2, 2, 1"), ("1", "one by one")):
                    os.environ["PANGENE_BOOT_ROWS_WORDS"] = words
                    report("groups", "groups of %s %s %s" % (sizes, metric, method), np.array_equal(capi.pan_boot_records(hip, P, metric, method, seed=6, first=1, n=7), whole))
                    rc, rec, dw = entry(hip, P, metric, method, 6, 3, 5, want_draws=True)  # replicates 3 .. 7: groups (3, 4), (5, 6), (7)
                    report("groups", "draws and records from first = 3, groups of %s" % sizes,
                           rc == 0 and np.array_equal(rec, whole[2:7]) and np.array_equal(dw, np.stack([br.draws(300, 6, b) for b in range(3, 8)])))
                    del os.environ["PANGENE_BOOT_ROWS_WORDS"]
        # diff: every replicate's own F, with both values inside each group (replicates 1 .. 4 have F = 20, 19, 19, 20)
        P = np.random.default_rng(0).random((950, 6)) < 0.5  # 950 + 6 x 30 = 1 130 words a replicate
        Fs = []
        for b in range(1, 5):
            stats = {}
            br.records(P, "diff", "nj", 3, b, 1, stats)
            Fs.append(min(stats["F"]))
        report("groups", "the replicates' F %s" % Fs, Fs[0] != Fs[1] and Fs[2] != Fs[3])
        os.environ["PANGENE_BOOT_ROWS_WORDS"] = "2500"
        for method in tr.METHODS:
            report("groups", "diff, groups of 2, 2 " + method, np.array_equal(capi.pan_boot_records(hip, P, "diff", method, seed=3, first=1, n=4), br.records(P, "diff", method, 3, 1, 4)))
        del os.environ["PANGENE_BOOT_ROWS_WORDS"]
    elif which == "joins":  # the batched joins against the restatement: ld padding (3, 5), a wave, a tile's rows, the update's workgroup
        for A, M, dup in ((3, 40, 0.5), (4, 40, 0.5), (5, 40, 0.5), (64, 500, 0.15), (65, 500, 0.15), (257, 1000, 0.15)):
            for method in tr.METHODS:
                P = tr.lineage_presence(M, A, 2 if A <= 5 and method == "upgma" else 1, dup=dup)  # seeds whose replicates meet tied minima
                stats = {}
                want = br.records(P, "jaccard" if A % 2 else "diff", method, 7, 1, 3, stats)
                if not (A == 3 and method == "nj") and stats["n_tied"] < 1:
                    report("joins: no tied minimum in the replicates", "A=%d %s" % (A, method), False)
                report("joins", "A=%d %s" % (A, method), np.array_equal(capi.pan_boot_records(hip, P, "jaccard" if A % 2 else "diff", method, seed=7, first=1, n=3), want))
    elif which == "large":  # past one column chunk of 1 024: against the checker build
        P = tr.lineage_presence(600, 1025, 1025)
        for method in tr.METHODS:
            report("large", "A=1025 %s" % method, np.array_equal(capi.pan_boot_records(hip, P, "jaccard", method, seed=2, first=1, n=2),
                                                                 capi.pan_boot_records(ora, P, "jaccard", method, seed=2, first=1, n=2)))
    elif which == "chunks":  # a replicate does not depend on the chunk it is in
        P = tr.lineage_presence(300, 40, 3)
        for method in tr.METHODS:
            whole = capi.pan_boot_records(hip, P, "jaccard", method, seed=6, first=1, n=7)
            report("chunks", "restatement " + method, np.array_equal(whole, br.records(P, "jaccard", method, 6, 1, 7)))
            ref_count = capi.pan_boot(hip, P, "jaccard", method, n_boot=7, seed=6)[2]
            for b in ("3", "1"):
                os.environ["PANGENE_BOOT_BATCH"] = b
                report("chunks", "batch %s %s" % (b, method), batch(hip, 40) == int(b) and
                       np.array_equal(capi.pan_boot_records(hip, P, "jaccard", method, seed=6, first=1, n=7), whole) and
                       np.array_equal(capi.pan_boot(hip, P, "jaccard", method, n_boot=7, seed=6)[2], ref_count))
                rc, _, _ = entry(hip, P, "jaccard", method, 6, 1, int(b) + 1)
                report("chunks", "more than a batch is refused", rc == -3)
                del os.environ["PANGENE_BOOT_BATCH"]
            ones = np.stack([capi.pan_boot_records(hip, P, "jaccard", method, seed=6, first=k, n=1)[0] for k in range(1, 8)])
            report("chunks", "one by one " + method, np.array_equal(ones, whole))
            rc, rec, _ = entry(hip, P, "jaccard", method, 6, 3, 4)
            report("chunks", "entry first=3 " + method, rc == 0 and np.array_equal(rec, whole[2:6]))
        b2k, b10k = batch(hip, 2000), batch(hip, 10000)
        report("chunks", "default batch %d at 2 000, %d at 10 000" % (b2k, b10k), 56 <= b2k <= 72 and b10k == 2)
    elif which == "parts":  # few workgroups in the search: each strides over several tiles, with a batch of 3
        os.environ["PANGENE_JOIN_PARTS"] = "7"
        P = tr.lineage_presence(1500, 600, 1)
        for method in tr.METHODS:
            report("parts", "A=600 " + method, np.array_equal(capi.pan_boot_records(hip, P, "jaccard", method, seed=3, first=1, n=3),
                                                              capi.pan_boot_records(ora, P, "jaccard", method, seed=3, first=1, n=3)))
    elif which == "metrics":  # both metrics and methods; diff with replicates whose F is not the reference's
        P = np.random.default_rng(0).random((950, 6)) < 0.5
        F_ref = tr.fixed(dr.shared(P), "diff")[1]
        for method in tr.METHODS:
            stats = {}
            want = br.records(P, "diff", method, 3, 1, 4, stats)
            report("metrics", "the replicates' F %s, the reference's %d" % (sorted(stats["F"]), F_ref), len(stats["F"] - {F_ref}) >= 1)
            report("metrics", "diff " + method, np.array_equal(capi.pan_boot_records(hip, P, "diff", method, seed=3, first=1, n=4), want))
            report("metrics", "jaccard " + method, np.array_equal(capi.pan_boot_records(hip, P, "jaccard", method, seed=3, first=1, n=4), br.records(P, "jaccard", method, 3, 1, 4)))
        none = P[:0]  # no items: no draws, every replicate is the reference tree
        for metric in tr.METRICS:
            ref0 = capi.pan_tree(hip, none, metric, "nj")[0]
            report("metrics", "no items " + metric, np.array_equal(capi.pan_boot_records(hip, none, metric, "nj", seed=3, first=1, n=2), np.stack([ref0, ref0])))
    elif which == "buffers":  # the cached device buffers: growing, shrinking, given back, and again
        for i, (A, M, n) in enumerate(((40, 300, 2), (300, 900, 5), (3, 20, 1), (130, 2000, 3), (64, 100, 9))):
            P = tr.lineage_presence(M, A, 20 + i)
            for method in tr.METHODS:
                report("buffers", "A=%d n=%d %s" % (A, n, method), np.array_equal(capi.pan_boot_records(hip, P, "jaccard", method, seed=1, first=1, n=n),
                                                                               capi.pan_boot_records(ora, P, "jaccard", method, seed=1, first=1, n=n)))
        hip.pg_trim_host_cache(0)  # gives the buffers back; the next call allocates again
        P = tr.lineage_presence(500, 200, 99)
        report("buffers", "after trim", np.array_equal(capi.pan_boot_records(hip, P, "diff", "nj", seed=1, first=1, n=4), capi.pan_boot_records(ora, P, "diff", "nj", seed=1, first=1, n=4)))
        hip.pg_trim_host_cache(0)
        report("buffers", "and again", np.array_equal(capi.pan_boot_records(hip, P, "diff", "upgma", seed=1, first=5, n=2), capi.pan_boot_records(ora, P, "diff", "upgma", seed=1, first=5, n=2)))
    elif which == "counts":  # pg_pan_boot: the support counts, product = checker = restatement; host arrays and CUDA tensors
        P = tr.lineage_presence(400, 24, 2, flip=0.1)
        for metric in tr.METRICS:
            for method in tr.METHODS:
                rec, F, count = capi.pan_boot(hip, P, metric, method, n_boot=12, seed=5)
                rec_o, F_o, count_o = capi.pan_boot(ora, P, metric, method, n_boot=12, seed=5)
                rec_w, F_w, count_w = br.support(P, metric, method, 12, 5)
                report("counts", "%s %s %s" % (metric, method, count.tolist()), F == F_o == F_w and np.array_equal(rec, rec_o) and np.array_equal(rec, rec_w) and
                       np.array_equal(count, count_o) and np.array_equal(count, count_w) and count[-1] == 12 and 0 < count[:-1].sum() < 12 * (len(count) - 1))
        t = torch.from_numpy(P).cuda()
        rec, F, count = capi.pan_boot(hip, t, "jaccard", "nj", n_boot=12, seed=5)
        report("counts", "torch cuda tensor", np.array_equal(count, br.support(P, "jaccard", "nj", 12, 5)[2]))
        report("counts", "torch cuda tensor, records", np.array_equal(capi.pan_boot_records(hip, t, "jaccard", "nj", seed=5, first=2, n=2), br.records(P, "jaccard", "nj", 5, 2, 2)))
        rc, _, _ = entry(hip, P[:, :2], "jaccard", "nj", 1, 1, 1)
        report("counts", "two assemblies are refused", rc == -3)
        rc, _, _ = entry(hip, P, "jaccard", "nj", 1, 0, 1)
        report("counts", "first = 0 is refused", rc == -3)
    else:
        sys.exit("unknown case " + which)
    print("ALL OK", flush=True)


if __name__ == "__main__":
    main()
