"""TEST INFRASTRUCTURE: a plain numpy restatement of the bootstrap of pangene tree (DESIGN.md section 8 "Bootstrap"; include/pangene_amd.h
pg_pan_boot, pg_pan_boot_records) for tests/test_boot.py and tests/test_boot_gpu.py: the draws in Python integers, the resampled counts
by np.bincount weights, the distances and joins of tree_ref, the leaf sets below the joins as frozensets (neighbour-joining: the side of
the split without leaf 0), and the Newick line with its support labels."""
import numpy as np

import tree_ref as tr

MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def mix64(z):
    """splitmix64's output function"""
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def draws(M, seed, b):
    """the M items replicate b >= 1 draws, in draw order (int64)"""
    x0 = mix64((((seed & 0xFFFFFFFF) << 32) | b) & MASK)
    return np.array([mix64((x0 + (t + 1) * GOLDEN) & MASK) % M for t in range(M)], dtype=np.int64)


def shared(P, m):
    """S_b (A, A) int64 of a presence matrix P (M, A) and the draws m: item k counts as often as it was drawn"""
    P = np.asarray(P) != 0
    M, A = P.shape
    w = np.bincount(m, minlength=M).astype(np.int64) if M else np.zeros(0, dtype=np.int64)
    Pi = P.astype(np.int64)
    return (Pi * w[:, None]).T @ Pi


def replicate(P, metric, method, seed, b, stats=None):
    """(records, F) of replicate b; tr.RangeError as the definition has it"""
    P = np.asarray(P) != 0
    q, F = tr.fixed(shared(P, draws(P.shape[0], seed, b)), metric)
    return tr.joins(q, method, stats), F


def records(P, metric, method, seed, first, n, stats=None):
    """int64 (n, records, 6) of replicates first .. first + n - 1; stats receives n_tied summed over them and the set of F"""
    out, tied, Fs = [], 0, set()
    for b in range(first, first + n):
        st = {}
        rec, F = replicate(P, metric, method, seed, b, st)
        tied += st["n_tied"]
        Fs.add(F)
        out.append(rec)
    if stats is not None:
        stats["n_tied"], stats["F"] = tied, Fs
    A = np.asarray(P).shape[1]
    return np.array(out, dtype=np.int64).reshape(n, A - 2 if method == "nj" else A - 1, 6)


def clades(rec, A, method):
    """Per join that can be supported (nj: s < A - 3, upgma: s < A - 2) the leaves below its node as a frozenset; nj: the side of the
    split that does not hold leaf 0"""
    below = [frozenset([x]) for x in range(A)]
    full = frozenset(range(A))
    out = []
    for s in range(A - 3 if method == "nj" else A - 2):
        i, j = int(rec[s][0]), int(rec[s][1])
        below[i] = below[i] | below[j]
        out.append(full - below[i] if method == "nj" and 0 in below[i] else below[i])
    return out


def support(P, metric, method, B, seed):
    """(reference records, F, count int32 per record)"""
    P = np.asarray(P) != 0
    A = P.shape[1]
    import dist_ref as dr
    q, F = tr.fixed(dr.shared(P), metric)
    rec = tr.joins(q, method)
    count = np.zeros(len(rec), dtype=np.int32)
    count[-1] = B
    ref = clades(rec, A, method)
    if ref:
        for b in range(1, B + 1):
            have = set(clades(replicate(P, metric, method, seed, b)[0], A, method))
            for s, c in enumerate(ref):
                count[s] += c in have
    return rec, F, count


def percent(count, B):
    """per cent, rounded half up, in integers"""
    return (200 * int(count) + B) // (2 * B)


def newick(names, rec, method, F, count, B):
    """tree_ref.newick with the support behind the node of every join that can be supported"""
    if B == 0:
        return tr.newick(names, rec, method, F)
    sub = [tr.quoted(n) for n in names]
    if method == "nj":
        for s, (i, j, dij, Ri, Rj, r) in enumerate(tuple(int(v) for v in row) for row in rec[:-1]):
            li = (dij + (Ri - Rj) / (r - 2)) / 2
            lj = dij - li
            sub[i] = "(%s%s,%s%s)%d" % (sub[i], tr._len(li, F), sub[j], tr._len(lj, F), percent(count[s], B))
        x, y, z, dxy, dxz, dyz = (int(v) for v in rec[-1])
        return "(%s%s,%s%s,%s%s);\n" % (sub[x], tr._len((dxy + dxz - dyz) / 2, F), sub[y], tr._len((dxy + dyz - dxz) / 2, F), sub[z], tr._len((dxz + dyz - dxy) / 2, F))
    height = [0.0] * len(names)
    root = 0
    for s, (i, j, dij, _, _, _) in enumerate(tuple(int(v) for v in row) for row in rec):
        h = dij / 2
        sub[i] = "(%s%s,%s%s)%s" % (sub[i], tr._len(h - height[i], F), sub[j], tr._len(h - height[j], F), "%d" % percent(count[s], B) if s < len(rec) - 1 else "")
        height[i], root = h, i
    return sub[root] + ";\n"


def text(names, P, metric="jaccard", method="nj", B=0, seed=0):
    """What pangene tree -b B -s seed prints"""
    import dist_ref as dr
    P = np.asarray(P) != 0
    A = len(names)
    if A < 3 or B == 0:
        return tr.text(names, dr.shared(P), metric, method)
    rec, F, count = support(P, metric, method, B, seed)
    return newick(names, rec, method, F, count, B).encode()
