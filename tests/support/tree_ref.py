"""TEST INFRASTRUCTURE: a plain numpy restatement of pangene tree (DESIGN.md section 8 "Trees"; include/pangene_amd.h pg_tree_opt_t,
pg_pan_join, pg_pan_tree) for tests/test_tree.py and tests/test_tree_gpu.py: the fixed-point distances from the shared-item counts of
dist_ref, the neighbour-joining and UPGMA joins in Python integers / int64, and the Newick line the command prints."""
import numpy as np

import dist_ref as dr

METRICS = ("jaccard", "diff")
METHODS = ("nj", "upgma")
LIMIT = 1 << 30


class RangeError(Exception):
    """a distance left the range of the definition (PGA_ERR_RANGE)"""


def fixed(S, metric):
    """(q int64 (A, A), F): distance * 2^F from the shared-item counts"""
    S = np.asarray(S, dtype=np.int64)
    n = np.diag(S)
    if metric == "diff":
        D = n[:, None] + n[None, :] - 2 * S
        F = min(20, 29 - int(D.max() if D.size else 0).bit_length())
        if F < 0:
            raise RangeError("diff")
        return D << F, F
    u = n[:, None] + n[None, :] - S
    q = ((1 << 21) * (u - S) + u) // np.maximum(2 * u, 1)
    return np.where(u == 0, 0, q), 20


def joins(q, method, stats=None):
    """The records (int64, (A - 2, 6) for nj, (A - 1, 6) for upgma) of a symmetric matrix q with a zero diagonal, A >= 3.
    stats, a dict, receives n_tied: the joins whose smallest criterion was reached by more than one live pair, and peak: the largest
    size of a distance, the input's included (set before a RangeError is raised, so that a search can see how far a run went)."""
    d = np.array(q, dtype=np.int64)
    A = d.shape[0]
    live = np.arange(A)
    size = np.ones(A, dtype=np.int64)
    rec, n_tied = [], 0
    peak = int(np.abs(d).max())
    nj = method == "nj"
    while len(live) > (3 if nj else 1):
        r = len(live)
        sub = d[np.ix_(live, live)]
        R = sub.sum(axis=1)
        crit = (r - 2) * sub - R[:, None] - R[None, :] if nj else sub.copy()
        crit[np.tril_indices(r)] = np.iinfo(np.int64).max
        at = int(np.argmin(crit))  # the first smallest in row-major order: the smallest i, then the smallest j
        n_tied += int((crit == crit.flat[at]).sum() > 1)
        a, b = divmod(at, r)
        i, j = int(live[a]), int(live[b])
        dij = int(d[i, j])
        rec.append((i, j, dij, int(R[a]), int(R[b]), r) if nj else (i, j, dij, int(size[i]), int(size[j]), r))
        others = np.delete(live, [a, b])
        if nj:
            new = (d[i, others] + d[j, others] - dij) >> 1
        else:
            new = (size[i] * d[i, others] + size[j] * d[j, others]) // (size[i] + size[j])
        if new.size:
            peak = max(peak, int(np.abs(new).max()))
            if stats is not None:
                stats["peak"] = peak
        if peak >= LIMIT:
            raise RangeError("join")
        d[i, others] = new
        d[others, i] = new
        size[i] += size[j]
        live = np.delete(live, b)
    if nj:
        x, y, z = (int(v) for v in live)
        rec.append((x, y, z, int(d[x, y]), int(d[x, z]), int(d[y, z])))
    if stats is not None:
        stats["n_tied"], stats["peak"] = n_tied, peak
    return np.array(rec, dtype=np.int64).reshape(-1, 6)


def quoted(name):
    if not any(c in name for c in "(),:;[]' \t\n"):
        return name
    return "'" + name.replace("'", "''") + "'"


def _len(x, F):
    return ":%.6f" % (x / float(1 << F))


def newick(names, rec, method, F):
    """The line of A >= 3 leaves from their records"""
    sub = [quoted(n) for n in names]
    if method == "nj":
        for i, j, dij, Ri, Rj, r in (tuple(int(v) for v in row) for row in rec[:-1]):
            li = (dij + (Ri - Rj) / (r - 2)) / 2
            lj = dij - li
            sub[i] = "(%s%s,%s%s)" % (sub[i], _len(li, F), sub[j], _len(lj, F))
        x, y, z, dxy, dxz, dyz = (int(v) for v in rec[-1])
        return "(%s%s,%s%s,%s%s);\n" % (sub[x], _len((dxy + dxz - dyz) / 2, F), sub[y], _len((dxy + dyz - dxz) / 2, F), sub[z], _len((dxz + dyz - dxy) / 2, F))
    height = [0.0] * len(names)
    root = 0
    for i, j, dij, _, _, _ in (tuple(int(v) for v in row) for row in rec):
        h = dij / 2
        sub[i] = "(%s%s,%s%s)" % (sub[i], _len(h - height[i], F), sub[j], _len(h - height[j], F))
        height[i], root = h, i
    return sub[root] + ";\n"


def text(names, S, metric="jaccard", method="nj"):
    """What pangene tree prints"""
    A = len(names)
    if A == 0:
        return b";\n"
    if A == 1:
        return ("(%s);\n" % quoted(names[0])).encode()
    q, F = fixed(S, metric)
    if A == 2:
        h = _len(int(q[0, 1]) / 2, F)
        return ("(%s%s,%s%s);\n" % (quoted(names[0]), h, quoted(names[1]), h)).encode()
    return newick(names, joins(q, method), method, F).encode()


def lineage_presence(M, A, seed, founders=4, flip=0.02, dup=0.15):
    """(M, A) bool: a few founder columns, every assembly a copy of one with `flip` of its bits flipped -- or, with probability `dup`,
    an exact copy of an earlier assembly, which gives zero distances and many exactly tied minima"""
    rng = np.random.default_rng(seed)
    base = rng.random((M, founders)) < 0.5
    P = np.empty((M, A), dtype=bool)
    for a in range(A):
        if a > 0 and rng.random() < dup:
            P[:, a] = P[:, rng.integers(0, a)]
        else:
            P[:, a] = base[:, rng.integers(0, founders)] ^ (rng.random(M) < flip)
    return P


IN_MAX = (1 << 29) - 1  # the largest size of an input entry
SIGNED_SIZES = (3, 4, 5, 63, 65, 129, 257)


def signed_matrix(n, seed):
    """(n, n) int32: symmetric, zero diagonal, entries uniform in [-(2^29 - 1), 2^29 - 1] -- both signs at the full magnitude the
    definition admits, so that floor(x / 2) and the floored division of UPGMA meet negative sums from the first join on"""
    rng = np.random.default_rng(seed)
    a = np.triu(rng.integers(-IN_MAX, IN_MAX + 1, size=(n, n)), 1)
    return (a + a.T).astype(np.int32)


def peak_search(seed=1, steps=400, n=5):
    """(q, peak, leaving): a hill-climb over n x n signed matrices for a neighbour-joining run that comes as near to the range limit
    2^30 as it can WITHOUT leaving the range: one entry (and its mirror) is redrawn or set to +-(2^29 - 1) per step, and the step is
    kept when the run's peak does not fall.  leaving: the first matrix met whose run leaves the range (RangeError), or None."""
    rng = np.random.default_rng(seed)
    q = signed_matrix(n, seed).astype(np.int64)

    def run(m):
        st = {}
        try:
            joins(m, "nj", st)
        except RangeError:
            return None
        return st["peak"]
    best, leaving = run(q), None
    assert best is not None
    for _ in range(steps):
        i, j = sorted(rng.choice(n, size=2, replace=False).tolist())
        c = q.copy()
        c[i, j] = c[j, i] = int(rng.choice([IN_MAX, -IN_MAX, int(rng.integers(-IN_MAX, IN_MAX + 1))]))
        got = run(c)
        if got is None:
            leaving = c.astype(np.int32) if leaving is None else leaving
        elif got >= best:
            q, best = c, got
    return q.astype(np.int32), best, leaving
