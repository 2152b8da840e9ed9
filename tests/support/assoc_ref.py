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
