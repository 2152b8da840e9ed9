"""TEST INFRASTRUCTURE: a plain numpy restatement of pangene qtrait (include/pangene_amd.h pg_qtrait_opt_t, pg_pan_qtrait) for
tests/test_qtrait.py, tests/test_qtrait_gpu.py and tests/support/qtrait_direct.py.  Ranks by counting (r2[c] = 2 #{v < v_c} +
#{v == v_c} + 1, c2 = r2 - (N + 1)), D = B @ c2 in int64, the permuted value rows c2[order(N, p, seed)] with curves_ref.order (the
function trait_ref uses), k_g = #{p : |D_p| >= |D|} in int64.  U, auc, z and p_wilcox (math.erfc) are double precision,
Benjamini-Hochberg is trait_ref.bh."""
import math

import numpy as np

import curves_ref
import trait_ref

HEADER = "Trait\tGene\tN\tnG\tU\tauc\tz\tp_wilcox\tq_bh\tn_ge\tp_perm"
BLOCK = 2048


def ranks(v):
    """v (N,) float -> (c2 int64 (N,), T = sum over tie groups of t^3 - t)"""
    v = np.asarray(v, dtype=np.float64)
    N = len(v)
    less = (v[None, :] < v[:, None]).sum(axis=1, dtype=np.int64)
    same = (v[None, :] == v[:, None]).sum(axis=1, dtype=np.int64)
    c2 = 2 * less + same + 1 - (N + 1)
    _, cnt = np.unique(v + 0.0, return_counts=True)  # (-0.0 + 0.0 is 0.0: the two zeros are one group)
    cnt = cnt.astype(np.int64)
    return c2, int((cnt ** 3 - cnt).sum())


def ranks_sorted(v):
    """the c2 of ranks(v) by sorting, for rows too long for its N x N comparisons (tests/test_qtrait.py checks that the two agree)"""
    v = np.asarray(v, dtype=np.float64) + 0.0
    _, inv, cnt = np.unique(v, return_inverse=True, return_counts=True)
    cnt = cnt.astype(np.int64)
    less = np.cumsum(cnt) - cnt
    return 2 * less[inv] + cnt[inv] - len(v)


def digits(c2):
    """(lo, hi) of the count kernel's two signed-byte planes: c2 = 256 hi + lo, lo in [-128, 127]"""
    c2 = np.asarray(c2, dtype=np.int64)
    lo = ((c2 + 128) & 255) - 128
    return lo, (c2 - lo) >> 8


LIMIT_N = 32000   # the largest N: |c2| <= 31 999 fits two signed bytes, |D| <= N^2 / 4 < 2^30
LIMIT_PERM = 130  # a full 128-permutation tile and two rows of a second


def limit_inputs():
    """[(label, B (130, N) bool, c2 (N,) int64)]: the inputs of the `limit` cases.
      N = 32 000 without ties: c2 takes every odd value in +-31 999, so hi reaches +-125 and lo, odd like c2, -127 and 127.  Row 0 holds
        exactly the 16 000 largest values (|D| = 16 000^2 = 2.56e8, the largest the definition allows), row 1 the smallest, row 2 every
        column of even index, row 3 is empty, row 4 full, the others have random densities.
      N = 31 999 without ties: every even value in +-31 998, so lo reaches -128 (and 126), hi +-125 again.
      N = 31 999 with three tie groups of 10 000, 11 000 and 10 999 columns."""
    out = []
    for N, ties in ((LIMIT_N, False), (LIMIT_N - 1, False), (LIMIT_N - 1, True)):
        rng = np.random.default_rng(N + ties)
        if not ties:
            c2 = 2 * rng.permutation(N).astype(np.int64) - (N - 1)
        else:
            c2 = ranks_sorted(rng.permutation(np.repeat([1.0, 2.0, 3.0], [10000, 11000, 10999])))
        B = rng.random((130, N)) < rng.random((130, 1))
        B[0], B[1] = c2 > 0, c2 < 0
        B[2] = np.arange(N) % 2 == 0
        B[3], B[4] = False, True
        out.append(("limit N=%d%s" % (N, ", ties" if ties else ""), B, c2))
    return out


_rows_cache = {}


def perm_rows(c2, n, seed=11, first=1):
    """(n, N) int64: row i = the centred ranks under permutation first + i, c2_p[r] = c2[o_p[r]].  The rows of one (c2, seed) are kept, so
    that the cases of a test which share them compute each order once."""
    c2 = np.asarray(c2, dtype=np.int64)
    N = len(c2)
    if N >= trait_ref.LONG_ROW and n:
        return c2[trait_ref.long_orders(N, first, n, seed)]
    key = (c2.tobytes(), seed)
    have = _rows_cache.get(key, np.empty((0, N), dtype=np.int64))
    need = first - 1 + n
    if len(have) < need:
        more = np.empty((need - len(have), N), dtype=np.int64)
        for i in range(len(more)):
            more[i] = c2[np.asarray(curves_ref.order(N, len(have) + 1 + i, seed), dtype=np.int64)] if N else c2
        have = np.concatenate([have, more])
        if have.size <= 1 << 24:
            _rows_cache[key] = have
    return have[first - 1:need]


def counts(B, c2, n_perm=1000, seed=11, min_count=1, d_rows=0):
    """B (G, N) bool over the compacted columns, c2 (N,) -> (a, D, k, eligible[, D_p of the first d_rows permutations (d_rows, G)]);
    k = 0 where not eligible"""
    B = np.asarray(B) != 0
    c2 = np.asarray(c2, dtype=np.int64)
    G, N = B.shape
    a = B.sum(axis=1, dtype=np.int64)
    Bi = B.astype(np.float64)  # exact: every |sum| is below N (N - 1) / 2 < 2^53
    D = (Bi @ c2.astype(np.float64)).astype(np.int64)
    el = np.minimum(a, N - a) >= min_count
    k = np.zeros(G, dtype=np.int64)
    first = np.zeros((d_rows, G), dtype=np.int64)
    for p0 in range(0, n_perm, BLOCK):
        R = perm_rows(c2, min(BLOCK, n_perm - p0), seed, 1 + p0)
        Dp = (Bi @ R.T.astype(np.float64)).astype(np.int64)  # (G, b)
        k += (np.abs(Dp) >= np.abs(D)[:, None]).sum(axis=1)
        if p0 < d_rows:
            m = min(d_rows, p0 + Dp.shape[1]) - p0
            first[p0:p0 + m] = Dp[:, :m].T
    k[~el] = 0
    return (a, D, k, el, first) if d_rows else (a, D, k, el)


def _columns(vrow):
    v = np.asarray(vrow, dtype=np.float64)
    cols = np.nonzero(~np.isnan(v))[0]
    return cols, v[cols]


def pan_qtrait(P, values, n_perm=1000, seed=11, min_count=1):
    """What capi.pan_qtrait returns: dict of int32 (T, G)"""
    P = np.asarray(P) != 0
    V = np.asarray(values, dtype=np.float64)
    if V.ndim == 1:
        V = V[None, :]
    G, T = P.shape[0], V.shape[0]
    out = {key: np.zeros((T, G), dtype=np.int32) for key in ("N", "a", "D", "k")}
    for ti in range(T):
        cols, v = _columns(V[ti])
        N = len(cols)
        out["N"][ti], out["a"][ti] = N, -1
        if N < 2 or (v == v[0]).all():
            continue
        c2, _ = ranks(v)
        a, D, k, el = counts(P[:, cols], c2, n_perm, seed, min_count)
        out["a"][ti] = np.where(el, a, -1)
        out["D"][ti] = np.where(el, D, 0)
        out["k"][ti] = np.where(el, k, 0)
    return out


def table(genes, asm, P, trait_names, values, n_perm=1000, seed=11, min_count=1, max_p=1.0):
    """rows (trait, gene, N, nG, U text, auc, z, p_wilcox, q_bh, n_ge text, p_perm text) as pangene qtrait prints them; values (T, A),
    NaN = missing"""
    rows = []
    P = np.asarray(P) != 0
    for ti, name in enumerate(trait_names):
        cols, v = _columns(values[ti])
        N = len(cols)
        if N < 2 or (v == v[0]).all():
            continue
        c2, T = ranks(v)
        a, D, k, el = counts(P[:, cols], c2, n_perm, seed, min_count)
        gs = np.nonzero(el)[0].tolist()
        tie = float(N + 1) - float(T) / (float(N) * float(N - 1))
        z = [float(D[g]) / math.sqrt(float(int(a[g]) * (N - int(a[g]))) / 3.0 * tie) for g in gs]
        pw = [math.erfc(abs(x) / math.sqrt(2.0)) for x in z]
        q = trait_ref.bh(pw)
        for e, g in enumerate(gs):
            if not pw[e] <= max_p:
                continue
            ag, Dg = int(a[g]), int(D[g])
            ab = ag * (N - ag)
            U = (Dg + ab) * 0.5
            perm = ("%d" % k[g], "%.6f" % ((int(k[g]) + 1.0) / (n_perm + 1.0))) if n_perm else ("NA", "NA")
            rows.append((name, genes[g], N, ag, "%.1f" % U, U / ab, z[e], pw[e], q[e], perm[0], perm[1]))
    return rows


def text(rows):
    """What pangene qtrait prints for the rows of table()"""
    out = [HEADER]
    for r in rows:
        out.append("%s\t%s\t%d\t%d\t%s\t%.4f\t%.4f\t%.3e\t%.3e\t%s\t%s" % r)
    return ("\n".join(out) + "\n").encode()


def parse(b):
    """a printed table -> list of dicts: Trait, Gene, U, n_ge, p_perm (the printed text; n_ge "NA" or digits); N, nG (int); auc, z,
    p_wilcox, q_bh (float)"""
    lines = b.decode().split("\n")
    assert lines[0] == HEADER and lines[-1] == ""
    out = []
    for l in lines[1:-1]:
        f = l.split("\t")
        assert len(f) == 11, l
        out.append({"Trait": f[0], "Gene": f[1], "N": int(f[2]), "nG": int(f[3]), "U": f[4], "auc": float(f[5]), "z": float(f[6]),
                    "p_wilcox": float(f[7]), "q_bh": float(f[8]), "n_ge": f[9], "p_perm": f[10]})
    return out


def read_file(path, asm):
    """(trait names, values (T, A) float64 with NaN = missing) of a trait file"""
    lines = open(path).read().split("\n")
    names = lines[0].split("\t")[1:]
    V = np.full((len(names), len(asm)), np.nan)
    for l in lines[1:]:
        if not l or l[0] == "#":
            continue
        f = l.split("\t")
        V[:, asm.index(f[0])] = [np.nan if x in ("NA", "") else float(x) for x in f[1:]]
    return names, V


def trait_file(asm, trait_names, fields):
    """the text of a trait file from fields[T][A] of strings ("NA" = missing): header, then one line per assembly that has a value in some
    trait (the others are left out)"""
    out = ["assembly\t" + "\t".join(trait_names)]
    for c, nm in enumerate(asm):
        col = [fields[t][c] for t in range(len(trait_names))]
        if any(x != "NA" for x in col):
            out.append(nm + "\t" + "\t".join(col))
    return "\n".join(out) + "\n"
