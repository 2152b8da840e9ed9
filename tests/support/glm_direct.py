"""TEST INFRASTRUCTURE: direct pga_pan_glm / pg_pan_glm cases for tests/test_glm_gpu.py, run in a child process of their own so that the
test can bound them with a timeout.  The product library (HIP kernels of k_glm.hpp) runs shapes no GFA fixture reaches; the numpy
restatement (tests/support/glm_ref.py) checks them within the tolerances stated there.  Through the tests-only sums_test pointer of
pga_glm_in_t the product kernel k_glm_sums is reached directly: with columns of small integers every sum is exact in fp64, so the
result must EQUAL numpy's integer product (the f64 result map, the eight steps of a word, the tile edges, the trait tiles and the K
segments are all decided by that), and with normal columns |S - S_ref| <= 4 A 2^-53 sum |cols_i| over the gene's assemblies.
Prints one line per case and "ALL OK" at the end; exits 1 at the first miss.

    python tests/support/glm_direct.py {file:NAME|memory:NAME|maps|sums|stat|collinear|separation|na|twice|range}"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
GOLD = os.path.join(ROOT, "tests", "golden")
HIP = os.path.join(ROOT, "pangene_amd", "bin", "pangene")
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import glm_ref as gr  # noqa: E402

PGA_ERR_RANGE, PGA_ERR_ARG = -2, -3
SIZES_A = (3, 4, 5, 31, 32, 33, 63, 65, 129, 257, 1025)
SIZES_G = (1, 15, 16, 17, 63, 65, 255, 257, 1000)
SIZES_T = (1, 2, 5)


class pga_glm_in_t(C.Structure):
    _fields_ = [("bits", C.c_void_p), ("cols", C.c_void_p), ("chol", C.c_void_p), ("n_gene", C.c_int32), ("n_asm", C.c_int32), ("n_trait", C.c_int32), ("n_cov", C.c_int32),
                ("sums_test", C.c_void_p)]


class pga_glm_out_t(C.Structure):
    _fields_ = [("a", C.POINTER(C.c_int32)), ("u", C.POINTER(C.c_double)), ("v", C.POINTER(C.c_double)), ("sw", C.POINTER(C.c_double))]


def fail(msg):
    print(msg, flush=True)
    sys.exit(1)


def say(label, ok, detail=""):
    print("%s: %s%s" % (label, "ok" if ok else "MISS", (" -- " + detail) if detail else ""), flush=True)
    if not ok:
        sys.exit(1)


def pack(P):
    """gene-major bit rows (G, W) uint32 of P (G, A) bool, bit c & 31 of word c >> 5"""
    G, A = P.shape
    W = (A + 31) // 32
    full = np.zeros((G, W * 32), dtype=np.uint8)
    full[:, :A] = P
    return np.ascontiguousarray(np.packbits(full.reshape(G, W, 32), axis=2, bitorder="little").view("<u4").reshape(G, W))


def direct(lib, P, cols, chol, k, want_sums=True, n_asm=None, n_gene=None):
    """pga_pan_glm itself on P (G, A) bool, cols (T, A, 16), chol (T, k + 1, k + 1): the status when it is not 0, else a dict a, u, v, sw
    (T, G) and sums (T, G, 16)"""
    G, A = P.shape
    cols = np.ascontiguousarray(cols, dtype=np.float64)
    T = cols.shape[0]
    chol = np.ascontiguousarray(chol, dtype=np.float64)
    bits = pack(P)
    s = np.full((T, G, 16), np.nan) if want_sums else None
    arg = pga_glm_in_t(bits.ctypes.data, cols.ctypes.data, chol.ctypes.data, G if n_gene is None else n_gene, A if n_asm is None else n_asm, T, k,
                       s.ctypes.data if want_sums else None)
    out = pga_glm_out_t()
    lib.pga_pan_glm.restype = C.c_int
    rc = lib.pga_pan_glm(C.byref(arg), C.byref(out))
    if rc != 0:
        return rc
    n = T * G
    r = {key: np.ctypeslib.as_array(getattr(out, key), shape=(max(n, 1),))[:n].reshape(T, G).copy() for key in ("a", "u", "v", "sw")}
    r["sums"] = s
    return r


def shapes():
    """every A with two G and every G with two A, the traits in turn"""
    seen, out = set(), []
    for i, A in enumerate(SIZES_A):
        for G in (SIZES_G[i % 9], SIZES_G[(i + 4) % 9]):
            seen.add((A, G))
    for j, G in enumerate(SIZES_G):
        for A in (SIZES_A[j % 11], SIZES_A[(j + 5) % 11]):
            seen.add((A, G))
    for n, (A, G) in enumerate(sorted(seen)):
        out.append((A, G, SIZES_T[n % 3]))
    out.append((1025, 1000, 5))
    return out


def case(A, G, T, integers):
    """a presence matrix, its columns (zero rows for the assemblies without a value) and unit lower-triangular factors of 13 covariates"""
    rng = np.random.default_rng(A * 4096 + G * 8 + T)
    P = rng.random((G, A)) < 0.5
    valid = rng.random((T, A)) < 0.8
    cols = rng.integers(-8, 9, size=(T, A, 16)).astype(np.float64) if integers else rng.standard_normal((T, A, 16))
    cols[:, :, 0] = 1.0
    cols *= valid[:, :, None]
    chol = np.tile(np.eye(14), (T, 1, 1))
    if not integers:
        chol = chol + np.tril(rng.standard_normal((T, 14, 14)) * 0.1, -1)
    return P, valid, cols, chol


def check_shapes(lib, integers):
    for A, G, T in shapes():
        P, valid, cols, chol = case(A, G, T, integers)
        got = direct(lib, P, cols, chol, 13)
        if not isinstance(got, dict):
            fail("A=%d G=%d T=%d: status %d" % (A, G, T, got))
        Pi = P.astype(np.int64)
        ok, detail = True, ""
        for t in range(T):
            pop = Pi @ valid[t].astype(np.int64)
            if integers:
                want = Pi @ cols[t].astype(np.int64)
                y = want[:, 2:16]
                ok = ok and np.array_equal(got["sums"][t], want.astype(np.float64)) and np.array_equal(got["a"][t], pop) and np.array_equal(got["u"][t], want[:, 1]) and \
                    np.array_equal(got["sw"][t], want[:, 2]) and np.array_equal(got["v"][t], (want[:, 2] - (y * y).sum(axis=1)).astype(np.float64))
                if not ok:
                    wrong = np.argwhere(got["sums"][t] != want)
                    detail = "trait %d: %d sums differ, the first at gene %d column %d" % ((t, len(wrong)) + (tuple(wrong[0]) if len(wrong) else (-1, -1)))
                    break
            else:
                want = gr.sums(P, cols[t])
                bound = 4.0 * A * gr.EPS * gr.sums(P, np.abs(cols[t]))
                err = np.abs(got["sums"][t] - want)
                ok = ok and bool(np.all(np.isfinite(got["sums"][t])) and np.all(err <= bound)) and np.array_equal(got["a"][t], pop) and \
                    np.array_equal(got["u"][t], got["sums"][t][:, 1]) and np.array_equal(got["sw"][t], got["sums"][t][:, 2]) and bool(np.all(np.isfinite(got["v"][t])))
                detail = "largest error / bound = %.3g" % float((err / np.maximum(bound, 1e-300)).max())
                if not ok:
                    break
        say("%s A=%d G=%d T=%d" % ("maps" if integers else "sums", A, G, T), ok, detail)


def random_case(seed, G, A, k, na):
    rng = np.random.default_rng(seed)
    P = rng.random((G, A)) < rng.uniform(0.1, 0.9, size=(G, 1))
    cov = rng.standard_normal((A, k))
    lin = 0.3 + (0.8 * cov[:, 0] if k else 0.0)
    yb = (rng.random(A) < 1.0 / (1.0 + np.exp(-lin))).astype(np.float64)
    yq = rng.standard_normal(A) + (0.7 * cov[:, 0] if k else 0.0) + 0.9 * P[3 % G]
    for y in (yb, yq):
        y[rng.choice(A, size=na, replace=False)] = np.nan
    return P, cov, yb, yq


def run_cli(args, env=None):
    r = subprocess.run([HIP] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env)
    return r.returncode, r.stdout, r.stderr


def pafs_of(name):
    d = os.path.join(GOLD, name)
    return sorted(os.path.join(d, f) for f in os.listdir(d) if ".paf" in f)


def main():
    which = sys.argv[1]
    from pangene_amd import capi
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    lib = capi.load()
    if which.startswith("file:"):
        # the product's command line on the GFA fixture, both families, k = 0 and 3, against the restatement
        import test_glm as tg
        name = which[5:]
        for family, folder in tg.FAMILIES:
            for k in (0, 3):
                bad, compared = tg.check_fixture(HIP, name, family, folder, k)
                say("file %s %s k=%d: %d genes compared" % (name, family, k, compared), not bad and (k > 0 or compared > 0), "; ".join(bad[:5]))
    elif which.startswith("memory:"):
        # `pangene --glm=FILE *.paf` equals `pangene glm -t FILE` on the GFA of the same run, byte for byte (the same build, the same code:
        # the determinism rule), and stands within the bounds of the restatement
        import test_glm as tg
        name = which[7:]
        files = pafs_of(name)
        rc, gfa, _ = run_cli(files)
        tmp = os.path.join(os.environ.get("TMPDIR", "/tmp"), "glm_direct_%d.gfa" % os.getpid())
        open(tmp, "wb").write(gfa)
        try:
            for family, folder, k in (("binary", "trait", 3), ("quant", "qtrait", 1)):
                tsv = os.path.join(GOLD, folder, name + ".tsv")
                rc1, a, err = run_cli(["--glm=" + tsv, "--glm-family=" + family, "--glm-axes=%d" % k] + files)
                rc2, b, _ = run_cli(["glm", "-t", tsv, "-y", family, "-k", str(k), tmp])
                bad, compared = tg.check_fixture(HIP, name, family, folder, k, gfa=tmp, text=(a, err)) if rc1 == 0 else (["exit %d" % rc1], 0)
                say("memory %s %s k=%d: %d genes compared" % (name, family, k, compared), rc == 0 and rc1 == 0 and rc2 == 0 and a == b and not bad, "; ".join(bad[:5]))
        finally:
            os.unlink(tmp)
    elif which == "maps":
        check_shapes(lib, True)
    elif which == "sums":
        check_shapes(lib, False)
    elif which == "stat":
        # k = 0, 1 and 13 at A = 129 and G = 257, both families: U, V and s_w against the restatement and against the checker build
        import oracle_host
        ora = oracle_host.load()
        for k in (0, 1, 13):
            P, cov, yb, yq = random_case(100 + k, 257, 129, k, 9)
            for family, y in (("binary", yb), ("quant", yq)):
                ref = gr.one_trait(P, y, cov, family)
                got, other = capi.pan_glm(lib, torch.from_numpy(P).cuda(), y, cov, family), capi.pan_glm(ora, P, y, cov, family)
                bad = gr.check_values(got, 0, ref, against=other)
                say("stat k=%d %s: fit %d, %d iterations, %d tested, tolV %.3g" % (k, family, got["fit"][0], got["iterations"][0], got["tested"][0], ref["tolV"]),
                    not bad and ref["fit"] == 1 and ref["clear"] and got["tested"][0] > 200, "; ".join(bad))
    elif which == "collinear":
        for family in ("binary", "quant"):
            P, cov, yb, yq = random_case(6, 120, 57, 1, 0)
            g = 7
            cov = np.hstack([cov, P[g][:, None].astype(np.float64)])
            y = yb if family == "binary" else yq
            got, ref = capi.pan_glm(lib, P, y, cov, family), gr.one_trait(P, y, cov, family)
            same = np.flatnonzero((P == P[g]).all(axis=1) | (P == ~P[g]).all(axis=1))
            say("collinear %s: V / s_w = %.3g" % (family, got["V"][0][g] / got["s_w"][0][g]), ref["collinear"][g] and bool(ref["margin"].all()) and got["fit"][0] == 1 and
                got["V"][0][g] <= 1e-10 * got["s_w"][0][g] and got["tested"][0] == int(ref["eligible"].sum()) - len(same) and not gr.check_values(got, 0, ref))
    elif which == "separation":
        import test_glm as tg
        import pathlib
        import tempfile
        P, cov, _, _ = random_case(8, 120, 57, 2, 0)
        y = (cov[:, 0] > 0).astype(np.float64)
        ref = gr.one_trait(P, y, cov, "binary")
        got = capi.pan_glm(lib, P, y, cov, "binary")
        say("separation: fit 0, no values", ref["fit"] == 0 and ref["clear"] and got["fit"][0] == 0 and got["tested"][0] == 0 and bool(np.all(got["a"] == -1)) and not got["U"].any())
        with tempfile.TemporaryDirectory() as td:
            tg.check_separation_cli(HIP, pathlib.Path(td))
        say("separation: the command line prints Fit 0, a note and no G lines", True)
    elif which == "na":
        for family in ("binary", "quant"):
            P, cov, yb, yq = random_case(9, 300, 131, 2, 23)
            y = yb if family == "binary" else yq
            v = np.flatnonzero(~np.isnan(y))
            full, cut = capi.pan_glm(lib, P, y, cov, family, 2), capi.pan_glm(lib, P[:, v], y[v], cov[v], family, 2)
            ref, ref2 = gr.one_trait(P, y, cov, family, 2), gr.one_trait(P[:, v], y[v], cov[v], family, 2)
            el = ref["eligible"]
            ok = full["N"][0] == len(v) == cut["N"][0] and np.array_equal(full["a"], cut["a"]) and full["tested"][0] == cut["tested"][0]
            ok = ok and not gr.check_values(full, 0, ref) and not gr.check_values(cut, 0, ref2)
            ok = ok and bool(np.all(np.abs(full["U"][0] - cut["U"][0])[el] <= (ref["eU"] + ref2["eU"])[el]) and np.all(np.abs(full["V"][0] - cut["V"][0])[el] <= (ref["eV"] + ref2["eV"])[el]))
            say("na %s: %d of %d assemblies have a value" % (family, len(v), len(y)), bool(ok))
        few = np.full((2, 131), np.nan)
        few[0, :4] = [0, 1, 0, 1]
        few[1, :30] = 1.0
        got = capi.pan_glm(lib, P, few, cov, "binary")
        say("na: too few values and one value only are no fit", list(got["N"]) == [4, 30] and not got["fit"].any() and bool(np.all(got["a"] == -1)))
    elif which == "twice":
        # the same call twice, and again after a larger and a smaller call in between (the pool's buffers are reused): the same bits
        P, valid, cols, chol = case(257, 255, 2, False)
        big, small = case(1025, 1000, 5, False), case(33, 17, 1, False)
        first = direct(lib, P, cols, chol, 13)
        again = direct(lib, P, cols, chol, 13)
        direct(lib, big[0], big[2], big[3], 13)
        direct(lib, small[0], small[2], small[3], 13)
        third = direct(lib, P, cols, chol, 13)
        lib.pg_trim_host_cache(0)  # gives the buffers back; the next call allocates again
        fourth = direct(lib, P, cols, chol, 13)
        for other, what in ((again, "twice"), (third, "after a larger and a smaller call"), (fourth, "after the buffers were given back")):
            say("twice: %s" % what, all(first[key].tobytes() == other[key].tobytes() for key in ("a", "u", "v", "sw", "sums")))
    elif which == "range":
        P, valid, cols, chol = case(33, 17, 1, True)
        say("range: n_asm = 16 385", direct(lib, P, cols, chol, 13, n_asm=16385) == PGA_ERR_RANGE)
        say("range: n_cov = 14 and -1", direct(lib, P, cols, chol, 14) == PGA_ERR_RANGE and direct(lib, P, cols, chol, -1) == PGA_ERR_ARG)
        say("range: n_gene = 2^24", direct(lib, P, cols, chol, 13, n_gene=1 << 24) == PGA_ERR_RANGE)
        got = direct(lib, np.zeros((0, 33), dtype=bool), cols, chol, 13)
        say("range: no genes", isinstance(got, dict) and got["a"].size == 0)
        got = direct(lib, np.zeros((5, 0), dtype=bool), np.zeros((1, 0, 16)), chol, 13)
        say("range: no assemblies: every sum is zero", isinstance(got, dict) and not got["a"].any() and not got["sums"].any())
        Pq, cov, yb, yq = random_case(10, 40, 30, 1, 0)
        for call, status in ((lambda: capi.pan_glm(lib, np.zeros((1, 16385), dtype=bool), np.zeros(16385), None, "quant"), "-2"),
                             (lambda: capi.pan_glm(lib, Pq, yq, np.zeros((30, 14)), "quant"), "-2"),
                             (lambda: capi.pan_glm(lib, Pq, np.where(np.arange(30) == 5, np.inf, yq), cov, "quant"), "-3")):
            try:
                call()
                say("range: pg_pan_glm refuses", False)
            except RuntimeError as e:
                say("range: pg_pan_glm status " + status, ("status " + status) in str(e))
        got = direct(lib, P, cols, chol, 13)
        say("after the refusals", isinstance(got, dict) and np.array_equal(got["sums"][0], (P.astype(np.int64) @ cols[0].astype(np.int64)).astype(np.float64)))
    else:
        sys.exit("unknown case " + which)
    print("ALL OK", flush=True)


if __name__ == "__main__":
    main()
