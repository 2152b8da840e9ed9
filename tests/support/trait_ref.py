"""TEST INFRASTRUCTURE: a plain numpy restatement of pangene trait (include/pangene_amd.h pg_trait_opt_t, pg_pan_trait) for
tests/test_trait.py and tests/test_trait_gpu.py.  The permuted label rows are y[order(N, p, seed)] with curves_ref.order, the counts
s_p = |B_g & y_p| a float32 matrix product over blocks (exact: every count is below 2^24), k_g = #{p : |D_p| >= |D|} in int64.  The
Fisher p is exact (math.comb, fractions.Fraction), Benjamini-Hochberg and phi are double precision."""
import math
from fractions import Fraction

import numpy as np

import curves_ref

HEADER = "Trait\tGene\tN\tnT\tnG\tnTG\tphi\tp_fisher\tq_bh\tn_ge\tp_perm"
INT_COLS = ("N", "nT", "nG", "nTG", "n_ge")
FLOAT_COLS = ("phi", "p_fisher", "q_bh")
BLOCK = 4096
LONG_ROW = 8192  # columns from which the orders come from curves_ref.orders (all of a block at once) instead of curves_ref.order
_long_orders = {}


def long_orders(N, first, n, seed):
    """curves_ref.orders(N, first, n, seed); the last result is kept, so that the checks of one input compute its orders once"""
    key = (N, first, n, seed)
    if key not in _long_orders:
        _long_orders.clear()
        _long_orders[key] = curves_ref.orders(N, first, n, seed)
    return _long_orders[key]


def perm_labels(y, n, seed=11, first=1):
    """(n, N) uint8: row i = the labels under permutation first + i, y_p[r] = y[o_p[r]]"""
    y = np.asarray(y, dtype=np.uint8)
    N = len(y)
    if N >= LONG_ROW and n:
        return y[long_orders(N, first, n, seed)]
    Y = np.empty((n, N), dtype=np.uint8)
    for i in range(n):
        Y[i] = y[np.asarray(curves_ref.order(N, first + i, seed), dtype=np.int64)] if N else y
    return Y


def pack(rows):
    """(n, N) 0/1 -> (n, ceil(N / 32)) uint32 bit rows, bit (c & 31) of word c >> 5"""
    rows = np.asarray(rows, dtype=np.uint8)
    n, N = rows.shape
    W = (N + 31) // 32
    pad = np.zeros((n, W * 32), dtype=np.uint8)
    pad[:, :N] = rows
    return np.packbits(pad.reshape(n, W, 32), axis=2, bitorder="little").view("<u4").reshape(n, W)


def counts(B, y, n_perm=1000, seed=11, min_count=1):
    """B (G, N) bool over the compacted columns, y (N,) 0/1 -> (a, s, k, eligible), int64 and bool; k = 0 where not eligible"""
    B = np.asarray(B) != 0
    y = np.asarray(y).astype(np.int64)
    G, N = B.shape
    t = int(y.sum())
    a = B.sum(axis=1, dtype=np.int64)
    s = (B & (y != 0)[None, :]).sum(axis=1, dtype=np.int64)
    el = np.minimum(a, N - a) >= min_count
    k = np.zeros(G, dtype=np.int64)
    if n_perm and el.any():
        d_abs = np.abs(s * N - a * t)[el]
        at = (a * t)[el]
        Bf = B[el].astype(np.float32)
        ke = np.zeros(int(el.sum()), dtype=np.int64)
        for p0 in range(0, n_perm, BLOCK):
            Y = perm_labels(y, min(BLOCK, n_perm - p0), seed, 1 + p0).astype(np.float32)
            Sp = (Bf @ Y.T).astype(np.int64)  # (E, b)
            ke += (np.abs(Sp * N - at[:, None]) >= d_abs[:, None]).sum(axis=1)
        k[el] = ke
    return a, s, k, el


def pan_trait(P, labels, n_perm=1000, seed=11, min_count=1):
    """What capi.pan_trait returns: dict of int32 (T, G)"""
    P = np.asarray(P) != 0
    L = np.asarray(labels)
    if L.ndim == 1:
        L = L[None, :]
    G, T = P.shape[0], L.shape[0]
    out = {key: np.zeros((T, G), dtype=np.int32) for key in ("N", "t", "a", "s", "k")}
    for ti in range(T):
        cols = np.nonzero(L[ti] >= 0)[0]
        y = (L[ti][cols] > 0).astype(np.int64)
        N, t = len(cols), int(y.sum())
        out["N"][ti], out["t"][ti], out["a"][ti] = N, t, -1
        if t == 0 or t == N:
            continue
        a, s, k, el = counts(P[:, cols], y, n_perm, seed, min_count)
        out["a"][ti] = np.where(el, a, -1)
        out["s"][ti] = np.where(el, s, 0)
        out["k"][ti] = np.where(el, k, 0)
    return out


WIDE_PERM = 70  # two waves' worth of lanes in the permutation kernel


def wide_inputs():
    """[(label, P (130, N) bool, y (N,) int8, {row: k it must get})]: the inputs of the `wide` cases, where the 64-bit products of the
    thresholds lo = floor((a t - |D|) / N), hi = ceil((a t + |D|) / N) pass 2^31.
      N = 70 001 (a prime; 2 188 words, the last partial), t = 35 000: 100 rows of density 0.1 .. 0.9, 26 of density 0.88 .. 0.995 (a t
        and s N above 2^31), an empty row, a full one (not eligible), the label row itself (|D| at its maximum t (N - t), lo = -1)
        and its complement (D = -t (N - t)).
      N = 70 000, t = 35 000: a t - |D| = N min(s, a - s) and a t + |D| = N max(s, a - s), so every row sits on equality on BOTH sides
        (a permutation with s_p = lo exactly is a hit); row 0 has a = 40 000, s = 20 000, D = 0 exactly: every permutation is a hit."""
    out = []
    for N in (70001, 70000):
        rng = np.random.default_rng(N)
        t = 35000
        y = np.zeros(N, dtype=np.int8)
        y[rng.permutation(N)[:t]] = 1
        dens = np.concatenate([np.linspace(0.1, 0.9, 100), np.linspace(0.88, 0.995, 26)])
        P = np.zeros((130, N), dtype=bool)
        P[:126] = rng.random((126, N)) < dens[:, None]
        P[127] = True
        P[128] = y != 0
        P[129] = y == 0
        must = {}
        if N == 70000:
            ones, zeros = np.nonzero(y != 0)[0], np.nonzero(y == 0)[0]
            P[0] = False
            P[0, ones[:20000]] = True
            P[0, zeros[:20000]] = True
            must[0] = WIDE_PERM
        out.append(("wide N=%d" % N, P, y, must))
    return out


_fisher_cache = {}


def fisher(N, t, a, s):
    """two-sided Fisher exact p: the sum of the hypergeometric P(x) over the feasible x with P(x) <= P(s) (1 + 1e-7), capped at 1"""
    key = (N, t, a, s)
    if key not in _fisher_cache:
        w = {x: math.comb(a, x) * math.comb(N - a, t - x) for x in range(max(0, a + t - N), min(a, t) + 1)}
        lim = w[s] * (10 ** 7 + 1)
        tot = sum(v for v in w.values() if v * 10 ** 7 <= lim)
        _fisher_cache[key] = min(1.0, float(Fraction(tot, math.comb(N, t))))
    return _fisher_cache[key]


def bh(p):
    """Benjamini-Hochberg q of p (in row order): sort ascending, ties by row; q_(i) = min over j >= i of p_(j) m / j, capped at 1"""
    m = len(p)
    idx = sorted(range(m), key=lambda i: (p[i], i))
    q, run = [0.0] * m, 1.0
    for j in range(m, 0, -1):
        run = min(run, p[idx[j - 1]] * m / j)
        q[idx[j - 1]] = run
    return q


def table(genes, asm, P, trait_names, labels, n_perm=1000, seed=11, min_count=1, max_p=1.0):
    """rows (trait, gene, N, nT, nG, nTG, phi, p_fisher, q_bh, n_ge, p_perm text) as pangene trait prints them; labels (T, A), -1 = missing"""
    rows = []
    P = np.asarray(P) != 0
    for ti, name in enumerate(trait_names):
        L = np.asarray(labels[ti])
        cols = np.nonzero(L >= 0)[0]
        y = (L[cols] > 0).astype(np.int64)
        N, t = len(cols), int(y.sum())
        if t == 0 or t == N:
            continue
        a, s, k, el = counts(P[:, cols], y, n_perm, seed, min_count)
        gs = np.nonzero(el)[0].tolist()
        pf = [fisher(N, t, int(a[g]), int(s[g])) for g in gs]
        q = bh(pf)
        for e, g in enumerate(gs):
            if not pf[e] <= max_p:
                continue
            ag, sg = int(a[g]), int(s[g])
            D, Vg, Vt = sg * N - ag * t, ag * (N - ag), t * (N - t)
            f = float(D) / math.sqrt(float(Vg) * float(Vt))
            perm = ("%d" % k[g], "%.6f" % ((int(k[g]) + 1.0) / (n_perm + 1.0))) if n_perm else ("NA", "NA")
            rows.append((name, genes[g], N, t, ag, sg, f, pf[e], q[e], perm[0], perm[1]))
    return rows


def text(rows):
    """What pangene trait prints for the rows of table()"""
    out = [HEADER]
    for r in rows:
        out.append("%s\t%s\t%d\t%d\t%d\t%d\t%.4f\t%.3e\t%.3e\t%s\t%s" % r)
    return ("\n".join(out) + "\n").encode()


def parse(b):
    """a printed table -> list of dicts: Trait, Gene (str); N, nT, nG, nTG (int); phi, p_fisher, q_bh (float); n_ge (int or None);
    p_perm (the printed text)"""
    lines = b.decode().split("\n")
    assert lines[0] == HEADER and lines[-1] == ""
    out = []
    for l in lines[1:-1]:
        f = l.split("\t")
        assert len(f) == 11, l
        out.append({"Trait": f[0], "Gene": f[1], "N": int(f[2]), "nT": int(f[3]), "nG": int(f[4]), "nTG": int(f[5]), "phi": float(f[6]),
                    "p_fisher": float(f[7]), "q_bh": float(f[8]), "n_ge": None if f[9] == "NA" else int(f[9]), "p_perm": f[10]})
    return out


def trait_file(asm, trait_names, labels):
    """the text of a trait file: header, then one line per assembly that has a value in some trait (the others are left out)"""
    out = ["assembly\t" + "\t".join(trait_names)]
    L = np.asarray(labels)
    for c, nm in enumerate(asm):
        if (L[:, c] >= 0).any():
            out.append(nm + "\t" + "\t".join("NA" if v < 0 else str(int(v)) for v in L[:, c]))
    return "\n".join(out) + "\n"
