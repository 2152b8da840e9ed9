"""TEST INFRASTRUCTURE: a plain numpy restatement of pangene assoc (include/pangene_amd.h pg_assoc_opt_t, pg_pan_assoc) for
tests/test_assoc.py and tests/test_assoc_gpu.py.  It reads the presence matrix of dist_ref.presence(gfa, "gene"), counts
s = |B_g & B_h| with a float32 matrix product over row blocks (exact: every count is below 2^24), decides the selection EXACTLY --
int64 where both sides of 10^6 D^2 >= p^2 V_g V_h fit, Python integers where they might not -- and prints what the command prints."""
import numpy as np

import dist_ref

SIGNS = ("both", "pos", "neg")
BLOCK = 512
MAX_ASM = 16777215


def permille(r):
    return int(np.floor(1000.0 * r + 0.5))


def select(P, min_phi=0.8, min_count=2, sign="both"):
    """(pairs int32 (n, 3) = (g, h, s) ascending, counts int64 (G,)) of a presence matrix (G, A)"""
    P = np.asarray(P) != 0
    G, A = P.shape
    assert A <= MAX_ASM
    p2 = permille(min_phi) ** 2
    cnt = P.sum(axis=1, dtype=np.int64)
    el = np.nonzero(np.minimum(cnt, A - cnt) >= min_count)[0]
    E = len(el)
    B = P[el].astype(np.float32)
    a_all = cnt[el]
    V_all = a_all * (A - a_all)
    # both sides stay below 2^62 when 10^6 (A^2 / 4)^2 does: then int64 decides, otherwise Python integers
    small = 10 ** 6 * (A * A // 4 + 1) ** 2 < 2 ** 62
    out = []
    for i0 in range(0, E, BLOCK):
        S = (B[i0:i0 + BLOCK] @ B.T).astype(np.int64)  # (b, E)
        a = a_all[i0:i0 + BLOCK, None]
        D = S * A - a * a_all[None, :]
        Vg, Vh = V_all[i0:i0 + BLOCK, None], V_all[None, :]
        upper = np.arange(E)[None, :] > np.arange(i0, min(i0 + BLOCK, E))[:, None]
        if sign == "pos":
            upper &= D >= 0
        elif sign == "neg":
            upper &= D < 0
        if small:
            ok = upper & (10 ** 6 * D * D >= p2 * Vg * Vh)
        else:
            # a float64 screen that cannot lose a pair (relative error of either side < 1e-12), then Python integers
            maybe = upper & (1e6 * D.astype(np.float64) ** 2 >= (1.0 - 1e-9) * p2 * Vg.astype(np.float64) * Vh.astype(np.float64))
            ok = np.zeros_like(maybe)
            Vg_b, Vh_b = np.broadcast_to(Vg, D.shape), np.broadcast_to(Vh, D.shape)
            for i, j in zip(*np.nonzero(maybe)):
                ok[i, j] = 10 ** 6 * int(D[i, j]) ** 2 >= p2 * int(Vg_b[i, j]) * int(Vh_b[i, j])
        i, j = np.nonzero(ok)
        out.append(np.stack([el[i0 + i], el[j], S[i, j]], axis=1))
    pairs = np.concatenate(out, axis=0).astype(np.int32) if out else np.zeros((0, 3), dtype=np.int32)
    return pairs.reshape(-1, 3), cnt


def phi(pairs, cnt, A):
    """float64 (n,): (double)D / sqrt((double)V_g * (double)V_h)"""
    a, b, s = cnt[pairs[:, 0]], cnt[pairs[:, 1]], pairs[:, 2].astype(np.int64)
    D, Vg, Vh = s * A - a * b, a * (A - a), b * (A - b)
    return D.astype(np.float64) / np.sqrt(Vg.astype(np.float64) * Vh.astype(np.float64))


def text(genes, P, min_phi=0.8, min_count=2, sign="both"):
    """What pangene assoc prints"""
    pairs, cnt = select(P, min_phi, min_count, sign)
    f = phi(pairs, cnt, np.asarray(P).shape[1])
    out = ["GeneA\tGeneB\tnA\tnB\tnAB\tphi"]
    for (g, h, s), x in zip(pairs.tolist(), f.tolist()):
        out.append("%s\t%s\t%d\t%d\t%d\t%.4f" % (genes[g], genes[h], cnt[g], cnt[h], s, x))
    return ("\n".join(out) + "\n").encode()


def read_gfa(path):
    """(gene names in segment order, presence (G, A) bool) of a GFA, as dist_ref.presence(path, "gene") reads it"""
    seg = {}
    for l in dist_ref._lines(path):
        l = l.rstrip("\r")
        t = l.split("\t")
        if l[:1] == "S" and len(t) >= 3:
            seg.setdefault(t[1], len(seg))
        elif l[:1] == "L" and len(t) >= 5 and t[2] in ("+", "-") and t[4] in ("+", "-"):
            seg.setdefault(t[1], len(seg))
            seg.setdefault(t[3], len(seg))
    _, P = dist_ref.presence(path, "gene")
    assert P.shape[0] == len(seg)
    return list(seg), P


EDGE_ROWS = (1, 127, 128, 129, 257)          # one partial 128-row tile, an exact one, diagonal + off-diagonal tiles, three tile rows
EDGE_COLS = (1, 991, 1024, 1025, 2070)       # rows of 1, 31, 32, 33 and 65 words: a partial 32-word chunk, an exact one, a second chunk of 1 word and a third


def edge_rows(R, C, seed, eligible=False):
    """(R, C) bool for the shapes at the edges of the 128 x 128 bit tile: row r has a density of its own, cycling through all-zero, all-one,
    0.03, 0.3, 0.5 and 0.9.  eligible (C >= 2): every row gets a one and a zero, so that none is constant"""
    rng = np.random.default_rng(seed)
    dens = np.array([0.0, 1.0, 0.03, 0.3, 0.5, 0.9])[(np.arange(R) + seed) % 6]
    P = rng.random((R, C)) < dens[:, None]
    if eligible:
        r = np.arange(R)
        P[r, r % C], P[r, (r + 1) % C] = True, False
    return P


def planted(G, A, seed, n_module=6):
    """(G, A) bool with a U-shaped frequency spectrum (most genes nearly core or rare) and planted modules: groups of genes that copy
    one pattern (correlated) or its complement (anti-correlated), a few of them with one assembly flipped"""
    rng = np.random.default_rng(seed)
    if G == 0 or A == 0:
        return np.zeros((G, A), dtype=bool)
    f = rng.beta(0.15, 0.15, size=G).astype(np.float32)
    P = np.empty((G, A), dtype=bool)
    for g0 in range(0, G, 4096):
        P[g0:g0 + 4096] = rng.random((min(4096, G - g0), A), dtype=np.float32) < f[g0:g0 + 4096, None]
    for m in range(n_module):
        k = int(min(G, rng.integers(2, 7)))
        rows = rng.choice(G, size=k, replace=False)
        pat = rng.random(A) < rng.uniform(0.2, 0.8)
        for n, r in enumerate(rows):
            row = pat.copy() if (n % 3 != 2) else ~pat
            if n % 2 and A > 2:
                row[rng.integers(0, A)] ^= True
            P[r] = row
    return P


def two_rows(A, a, b, s):
    """(2, A) bool: |B_0| = a, |B_1| = b, |B_0 & B_1| = s"""
    assert s <= min(a, b) and a + b - s <= A
    P = np.zeros((2, A), dtype=bool)
    P[0, :a] = True
    P[1, a - s:a - s + b] = True
    return P


def exact_threshold_cases(max_A=40):
    """(A, a, b, s, p) with 10^6 D^2 = p^2 V_g V_h exactly and p not a multiple of 100"""
    from math import isqrt
    out = []
    for A in range(4, max_A + 1):
        for a in range(2, A - 1):
            for b in range(a, A - 1):
                VV = a * (A - a) * b * (A - b)
                for s in range(max(0, a + b - A), min(a, b) + 1):
                    D = s * A - a * b
                    if D == 0:
                        continue
                    n = 10 ** 6 * D * D
                    if n % VV:
                        continue
                    p = isqrt(n // VV)
                    if p * p == n // VV and 0 < p < 1000 and p % 100:
                        out.append((A, a, b, s, p))
    return out


TIE_P = (337, 801)


def tie_tiles():
    """[(label, P (G, 4000) bool, p, side, cross pairs, identical-row pairs)]: matrices whose every cross pair sits EXACTLY on the
    threshold p / 1000.  A = 4000, X and Y rows of 2000 bits with |X & Y| = 1000 + side p: D = side 4000 p, V = 4 10^6, so
    10^6 D^2 = p^2 V^2 for any p.  Off-diagonal tile: G = 256, rows 0 .. 127 = X and 128 .. 255 = Y, so the 128 x 128 cross pairs are
    every (thread, ii, jj) slot of the tile (0, 1).  Diagonal tile: G = 130, rows alternating X, Y (li < lj, a partial tile)."""
    out = []
    for p in TIE_P:
        for side in (1, -1):
            s = 1000 + side * p
            xy = two_rows(4000, 2000, 2000, s)
            off = xy[np.arange(256) // 128]
            dia = xy[np.arange(130) % 2]
            out.append(("ties off-diagonal p=%d side=%+d" % (p, side), off, p, side, 128 * 128, 2 * (128 * 127 // 2)))
            out.append(("ties diagonal p=%d side=%+d" % (p, side), dia, p, side, 65 * 65, 2 * (65 * 64 // 2)))
    return out


def tie_count(p, side, cross, same, at, sign):
    """the pairs select() must give for a matrix of tie_tiles() at the threshold at / 1000: the identical rows (phi = 1) unless the sign
    is neg, the cross pairs when at <= p and the sign admits D = side 4000 p"""
    return (same if sign != "neg" else 0) + (cross if at <= p and sign in ("both", "pos" if side > 0 else "neg") else 0)


BAND = 2 ** 41  # a case is kept when |10^6 D^2 / (p^2 V^2) - 1| < 1 / BAND: strictly inside the kernel's guard band of 2^-40


def band_search(p, A=MAX_ASM, negative=False, lo=2, hi=None):
    """[(a, s, cmp)] at A assemblies: two rows with |X| = |Y| = a, |X & Y| = s, whose 10^6 D^2 is within 2^-41 relative of p^2 V^2;
    cmp = 0 (equal), 1 (above: selected at p) or -1 (below).  With a = b the condition is linear, 1000 |s A - a^2| against
    p a (A - a): for every a in [lo, hi) the s nearest to the threshold is taken in int64 (all terms below 2^58), kept when
    |1000 D - p V| < 16000, and classified in Python integers.  negative: D < 0, s below a^2 / A."""
    from fractions import Fraction
    hi = A // 2 if hi is None else hi
    a = np.arange(lo, hi, dtype=np.int64)
    V = a * (A - a)
    T = 1000 * a * a + (-p if negative else p) * V  # 1000 s A is to be near T
    s = (T + 500 * A) // (1000 * A)
    r = 1000 * s * A - T
    keep = (np.abs(r) < 16000) & (s >= 0) & (s <= a) & (2 * a - s <= A)
    out = []
    for ai, si in zip(a[keep].tolist(), s[keep].tolist()):
        D, Vi = si * A - ai * ai, ai * (A - ai)
        if D == 0 or (D < 0) != negative:
            continue
        L, R = 10 ** 6 * D * D, p * p * Vi * Vi
        if abs(Fraction(L, R) - 1) < Fraction(1, BAND):
            out.append((ai, si, (L > R) - (L < R)))
    return out


def band_cases(p):
    """[(p, a, s, cmp)] at A = 16 777 215, the documented limit, where the double-precision pre-test of the device rounds: the searches
    of band_search for one p (337 or 801), D > 0 over a in [2, A / 2) and D < 0 over a in [2, A - 2)"""
    return [(p,) + c for c in band_search(p) + band_search(p, negative=True, hi=MAX_ASM - 2)]


def band_matrix(a, s, A=MAX_ASM):
    """(4, A) uint8: rows X, Y, Y, X with |X| = |Y| = a and |X & Y| = s"""
    P = np.zeros((4, A), dtype=np.uint8)
    P[0, :a] = P[3, :a] = 1
    P[1, a - s:2 * a - s] = P[2, a - s:2 * a - s] = 1
    return P


def band_expected(a, s, at, sign="both", A=MAX_ASM):
    """(pairs int32 (n, 3), phi) of band_matrix(a, s) at the threshold at / 1000 and min_count <= min(a, A - a), from (a, s) alone in
    Python integers: the identical rows (0, 3) and (1, 2) have D = V > 0, the four cross pairs D = s A - a^2"""
    D, V = s * A - a * a, a * (A - a)
    cross = 10 ** 6 * D * D >= at * at * V * V and (sign == "both" or (sign == "pos") == (D >= 0))
    rows = [(g, h, a if g + h == 3 else s) for g in range(4) for h in range(g + 1, 4) if (sign != "neg" if g + h == 3 else cross)]
    pairs = np.array(rows, dtype=np.int32).reshape(-1, 3)
    return pairs, phi(pairs, np.full(4, a, dtype=np.int64), A)
