"""TEST INFRASTRUCTURE: a numpy / Python-int restatement of pangene permanova (include/pangene_amd.h pg_permanova_opt_t, pg_pan_permanova)
for tests/test_permanova.py, tests/test_permanova_gpu.py and tests/support/permanova_direct.py.  Per trait the compacted submatrix qc, the
shift s, w = (qc >> s)^2 in int64; A of every label row comes from Y @ W in int64 -- exact, every sum is below 2^62 -- and G = N A - 2 n1 B
in Python ints.  The permuted label rows are trait_ref.perm_labels (curves_ref.order).  The printed doubles are exact fractions rounded
once."""
from fractions import Fraction

import numpy as np

import trait_ref

HEADER = "Trait\tN\tn1\tn0\tFbits\tSS_total\tSS_within\tF\tR2\tn_ge\tp_perm"
LIMIT_N = 16384
IN_MAX = (1 << 29) - 1
BLOCK = 1024


def shift_of(m, N):
    """the smallest s >= 0 with (m >> s)^2 N (N - 1) < 2^62"""
    s = 0
    while (int(m) >> s) ** 2 * N * (N - 1) >= 1 << 62:
        s += 1
    return s


def planes_of(w_max):
    """D: the smallest count of balanced base-256 digits (each in [-128, 127]) that holds w_max"""
    D, cap = 1, 127
    while cap < w_max:
        D, cap = D + 1, cap * 256 + 127
    return D


def digits(w, D):
    """w (int64 array, >= 0) -> D signed-byte planes, w = sum d_k 256^k"""
    w = np.asarray(w, dtype=np.int64).copy()
    out = []
    for _ in range(D):
        d = ((w + 128) & 255) - 128
        out.append(d)
        w = (w - d) >> 8
    assert not w.any()
    return out


def weights(qc, s):
    e = np.asarray(qc, dtype=np.int64) >> s
    w = e * e
    np.fill_diagonal(w, 0)
    return w


def sums(w, Y):
    """w (N, N) int64, Y (n, N) 0/1 -> (A (n,), B (n,)) int64"""
    Y = np.asarray(Y, dtype=np.int64)
    return ((Y @ w) * Y).sum(axis=1), Y @ w.sum(axis=1)


def G(N, n1, A, B):
    return N * int(A) - 2 * n1 * int(B)


def direct(qc, y, n_perm=1000, seed=11, rows=0):
    """The backend's step for one compacted matrix and label row: dict s, T, A, B, k[, A_p and B_p of the first `rows` permutations]"""
    qc = np.asarray(qc, dtype=np.int64)
    y = np.asarray(y, dtype=np.uint8)
    N, n1 = len(y), int(y.sum())
    s = shift_of(qc.max(), N)
    w = weights(qc, s)
    A, B = sums(w, y[None, :])
    g_obs = G(N, n1, A[0], B[0])
    k, a_rows, b_rows = 0, [], []
    for p0 in range(0, n_perm, BLOCK):
        Y = trait_ref.perm_labels(y, min(BLOCK, n_perm - p0), seed, 1 + p0)
        Ap, Bp = sums(w, Y)
        k += sum(G(N, n1, a, b) <= g_obs for a, b in zip(Ap.tolist(), Bp.tolist()))
        a_rows.append(Ap), b_rows.append(Bp)
    r = {"s": s, "T": int(w.sum()), "A": int(A[0]), "B": int(B[0]), "k": k}
    if rows:
        r["a_rows"], r["b_rows"] = np.concatenate(a_rows)[:rows], np.concatenate(b_rows)[:rows]
    return r


def one(q, lab, F, n_perm=1000, seed=11):
    """One label row lab (A,) (1, 0, negative = missing) over q (A, A) with F fraction bits: dict N, n1, Fe, T, A, B, k; k = -1 and
    skip = 1 (N < 3 or an empty group) or 2 (no distance above zero) for a trait that is not tested"""
    q = np.asarray(q, dtype=np.int64)
    lab = np.asarray(lab)
    cols = np.nonzero(lab >= 0)[0]
    y = (lab[cols] > 0).astype(np.uint8)
    N, n1 = len(cols), int(y.sum())
    r = {"N": N, "n1": n1, "Fe": 0, "T": 0, "A": 0, "B": 0, "k": -1, "skip": 1}
    if N < 3 or n1 == 0 or n1 == N:
        return r
    qc = q[np.ix_(cols, cols)]
    if not qc.any():
        r["skip"] = 2
        return r
    d = direct(qc, y, n_perm, seed)
    r.update(Fe=F - d["s"], T=d["T"], A=d["A"], B=d["B"], k=d["k"], skip=0)
    return r


def pan_permanova(q, labels, F=20, n_perm=1000, seed=11):
    """What capi.pan_permanova returns: dict of int64 (T,)"""
    L = np.asarray(labels)
    if L.ndim == 1:
        L = L[None, :]
    rs = [one(q, l, F, n_perm, seed) for l in L]
    return {key: np.array([r[key] for r in rs], dtype=np.int64) for key in ("N", "n1", "Fe", "T", "A", "B", "k")}


def same(got, want):
    return all(np.array_equal(np.asarray(got[key], dtype=np.int64), want[key]) for key in ("N", "n1", "Fe", "T", "A", "B", "k"))


def stats(r):
    """(SS_total, SS_within, F, R2) of a tested trait as exact fractions of the integers, each rounded once; F = inf when SSW = 0"""
    N, n1 = r["N"], r["n1"]
    n0 = N - n1
    X = G(N, n1, r["A"], r["B"]) + n1 * r["T"]  # 2 n0 n1 SSW
    tn = r["T"] * n0 * n1
    Y = tn - N * X
    scale = Fraction(4) ** r["Fe"]
    return (float(Fraction(r["T"], 2 * N) / scale), float(Fraction(X, 2 * n0 * n1) / scale), float(Fraction(Y * (N - 2), N * X)) if X else float("inf"),
            float(Fraction(Y, tn)))


def line(name, r, n_perm):
    sst, ssw, f, r2 = stats(r)
    perm = "%d\t%.6f" % (r["k"], (r["k"] + 1.0) / (n_perm + 1.0)) if n_perm else "NA\tNA"
    return "%s\t%d\t%d\t%d\t%d\t%.6f\t%.6f\t%s\t%.4f\t%s" % (name, r["N"], r["n1"], r["N"] - r["n1"], r["Fe"], sst, ssw, "inf" if f == float("inf") else "%.6f" % f, r2, perm)


def text(trait_names, labels, q, F, n_perm=1000, seed=11):
    """What pangene permanova prints"""
    out = [HEADER]
    for name, lab in zip(trait_names, labels):
        r = one(q, lab, F, n_perm, seed)
        if not r["skip"]:
            out.append(line(name, r, n_perm))
    return ("\n".join(out) + "\n").encode()


def parse(b):
    """a printed table -> list of dicts: Trait, SS_total, SS_within, F, R2, p_perm (text), N, n1, n0, Fbits (int), n_ge (int or None)"""
    lines = b.decode().split("\n")
    assert lines[0] == HEADER and lines[-1] == ""
    out = []
    for l in lines[1:-1]:
        f = l.split("\t")
        assert len(f) == 11, l
        out.append({"Trait": f[0], "N": int(f[1]), "n1": int(f[2]), "n0": int(f[3]), "Fbits": int(f[4]), "SS_total": f[5], "SS_within": f[6], "F": f[7], "R2": f[8],
                    "n_ge": None if f[9] == "NA" else int(f[9]), "p_perm": f[10]})
    return out


def float_permanova(d, y):
    """Anderson's two-group PERMANOVA in plain float64 over distances d (N, N): (F, R2) from the sums of squared distances over group sizes"""
    d = np.asarray(d, dtype=np.float64)
    y = np.asarray(y) != 0
    N = len(y)
    iu = np.triu_indices(N, 1)
    sst = (d[iu] ** 2).sum() / N
    ssw = 0.0
    for g in (y, ~y):
        sub = d[np.ix_(g, g)]
        ssw += (sub[np.triu_indices(int(g.sum()), 1)] ** 2).sum() / int(g.sum())
    return (sst - ssw) * (N - 2) / ssw, 1.0 - ssw / sst


def read_traits(path, asm):
    """(trait names, labels (T, A) int8 with -1 = missing) of a trait file"""
    lines = open(path).read().split("\n")
    names = lines[0].split("\t")[1:]
    L = np.full((len(names), len(asm)), -1, dtype=np.int8)
    for l in lines[1:]:
        if not l or l[0] == "#":
            continue
        f = l.split("\t")
        L[:, asm.index(f[0])] = [-1 if v in ("NA", "") else int(v) for v in f[1:]]
    return names, L


# ---- generators -------------------------------------------------------------------------------------------------------------------

def random_matrix(N, seed, hi=1 << 20):
    """symmetric, zero diagonal, entries in [0, hi)"""
    rng = np.random.default_rng(seed)
    q = np.triu(rng.integers(0, hi, size=(N, N), dtype=np.int64), 1)
    return q + q.T


def distinct_matrix(N):
    """every w distinct: e[i][j] = 1 + i N + j for i < j, mirrored (the `maps` case; w = e^2 with s = 0)"""
    i, j = np.triu_indices(N, 1)
    q = np.zeros((N, N), dtype=np.int64)
    q[i, j] = 1 + i * N + j
    return q + q.T


def planted(N, seed, spread=1 << 12, gap=1 << 14):
    """two groups of points on a line, distances |x_i - x_j|; (q, y) with y the planted groups"""
    rng = np.random.default_rng(seed)
    y = (rng.random(N) < 0.5).astype(np.uint8)
    y[0], y[1] = 0, 1
    x = rng.integers(0, spread, size=N, dtype=np.int64) + gap * y.astype(np.int64)
    return np.abs(x[:, None] - x[None, :]), y


def balanced(N, seed):
    rng = np.random.default_rng(seed)
    y = np.zeros(N, dtype=np.uint8)
    y[rng.permutation(N)[:N // 2]] = 1
    return y


def digit_matrix(N, D, seed, zero_plane=None):
    """e in [0, ...) such that w = e^2 needs exactly D planes and, with s = 0, the digits -128 and 127 occur in every plane that is not
    zero_plane; zero_plane: that plane's digit is 0 in every w (entries are picked among squares that have it)"""
    rng = np.random.default_rng(seed)
    cap = (127 * (256 ** D - 1)) // 255
    lo = (127 * (256 ** (D - 1) - 1)) // 255 + 1 if D > 1 else 1
    import math
    e_hi = math.isqrt(min(cap, ((1 << 62) - 1) // (N * (N - 1))))  # (D = 8 leaves room for N <= 8 only)
    assert e_hi * e_hi >= lo and e_hi ** 2 * N * (N - 1) < 1 << 62 and e_hi < 1 << 31
    cand = rng.integers(1, e_hi + 1, size=200000, dtype=np.int64)
    cand[0] = e_hi
    dg = np.stack(digits(cand * cand, D))  # (D, n)
    if zero_plane is not None:
        keep = dg[zero_plane] == 0
        cand, dg = cand[keep], dg[:, keep]
    must = []
    for k in range(D):
        if k == zero_plane:
            continue
        for v in (-128, 127):
            hit = np.nonzero(dg[k] == v)[0]
            if len(hit):
                must.append(int(cand[hit[0]]))
    if zero_plane is None:
        must.append(e_hi)
    n_pair = N * (N - 1) // 2
    vals = np.concatenate([np.array(must, dtype=np.int64), cand[rng.integers(0, len(cand), size=max(n_pair - len(must), 0))]])[:n_pair]
    q = np.zeros((N, N), dtype=np.int64)
    q[np.triu_indices(N, 1)] = rng.permutation(vals)
    return q + q.T
