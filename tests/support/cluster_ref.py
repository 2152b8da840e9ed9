"""TEST INFRASTRUCTURE: a plain numpy restatement of pangene cluster (DESIGN.md section 8 "Clusters"; include/pangene_amd.h
pg_cluster_opt_t, pg_pan_medoids, pg_pan_cluster) for tests/test_cluster.py and tests/test_cluster_gpu.py: k-medoids over the fixed-point
distances of tree_ref, BUILD and SWAP literally as the definition states them -- every delta is the difference of two TDs, each a
minimum over the whole medoid set --, the labels, sums and silhouettes in the host's operation order, and the three blocks of text."""
import numpy as np

import tree_ref as tr

LIMIT = 1 << 29


def td(q, M):
    """TD(M): the sum over the columns of the distance to the nearest medoid"""
    return int(q[:, M].min(axis=1).sum())


def deltas(q, M):
    """(candidates x ascending, medoids m ascending, delta[x][m] = TD(M - m + x) - TD(M)) by brute force"""
    n = q.shape[0]
    cand = np.array([x for x in range(n) if x not in M], dtype=np.int64)
    ms = sorted(M)
    cur = td(q, M)
    out = np.empty((len(cand), len(ms)), dtype=np.int64)
    for j, m in enumerate(ms):
        rest = q[:, [y for y in M if y != m]].min(axis=1)
        out[:, j] = np.minimum(rest[:, None], q[:, cand]).sum(axis=0) - cur
    return cand, ms, out


def medoids(q, k, max_iter=1000):
    """What capi.pan_medoids returns, for a symmetric int matrix q with a zero diagonal and entries in [0, 2^29)"""
    q = np.asarray(q, dtype=np.int64)
    n = q.shape[0]
    M, rec = [], []
    D = np.full(n, LIMIT, dtype=np.int64)
    for _ in range(k):  # BUILD
        gain = np.maximum(D[None, :] - q, 0).sum(axis=1)
        gain[M] = -1
        x = int(np.argmax(gain))  # the first largest: the smallest x
        rec.append((x, -1, int(gain[x])))
        M.append(x)
        D = np.minimum(D, q[x])
    n_swap = converged = 0
    for _ in range(max_iter):  # SWAP
        cand, ms, dl = deltas(q, M)
        at = int(np.argmin(dl))  # the first smallest in (x, m) order
        a, b = divmod(at, len(ms))
        if int(dl[a, b]) >= 0:
            converged = 1
            break
        x, m = int(cand[a]), ms[b]
        rec.append((x, m, int(dl[a, b])))
        M[M.index(m)] = x
        n_swap += 1
    med = np.array(sorted(M), dtype=np.int64)
    label = np.empty(n, dtype=np.int64)
    for o in range(n):
        own = np.nonzero(med == o)[0]
        label[o] = own[0] if own.size else int(np.argmin(q[o, med]))  # the first smallest: the smallest medoid index
    dist = q[np.arange(n), med[label]]
    size = np.bincount(label, minlength=k)
    sums = np.stack([q[:, label == c].sum(axis=1) for c in range(k)], axis=1)
    return {"medoid": med.astype(np.int32), "label": label.astype(np.int32), "dist": dist.astype(np.int32), "size": size.astype(np.int32),
            "sums": sums.astype(np.int64), "rec": np.array(rec, dtype=np.int64).reshape(-1, 3), "td": int(dist.sum()), "n_swap": n_swap,
            "converged": converged}


def same(got, want):
    """every field of two results"""
    return all(np.array_equal(got[f], want[f]) for f in ("medoid", "label", "dist", "size", "sums", "rec")) and \
        all(int(got[f]) == int(want[f]) for f in ("td", "n_swap", "converged"))


def silhouettes(r):
    """s(o) from sums and size alone, in the host's operation order: Python integers, one float division"""
    n, k = r["sums"].shape
    out = []
    for o in range(n):
        c = int(r["label"][o])
        sc = int(r["size"][c])
        if sc == 1:
            out.append(0.0)
            continue
        B = sb = 0
        for e in range(k):
            if e == c:
                continue
            v, se = int(r["sums"][o, e]), int(r["size"][e])
            if sb == 0 or v * sb < B * se:
                B, sb = v, se
        X, Y = B * (sc - 1), int(r["sums"][o, c]) * sb
        mx = max(X, Y)
        out.append(float(X - Y) / float(mx) if mx else 0.0)
    return out


def mean_sil(r, sil, c=None):
    s, cnt = 0.0, 0
    for o, v in enumerate(sil):
        if c is None or int(r["label"][o]) == c:
            s += v
            cnt += 1
    return s / float(cnt)


def _fixed(v, F):
    return "%.6f" % (int(v) / float(1 << F))


def text(names, S, metric="jaccard", k_lo=2, k_hi=None, max_iter=1000):
    """What pangene cluster prints for at least 3 assemblies and 2 <= k_lo <= k_hi <= assemblies - 1"""
    k_hi = k_lo if k_hi is None else k_hi
    q, F = tr.fixed(S, metric)
    lines = ["#K\tk\tTD\tmean_sil\tswaps\tconverged"]
    best = None
    for k in range(k_lo, k_hi + 1):
        r = medoids(q, k, max_iter)
        sil = silhouettes(r)
        mean = mean_sil(r, sil)
        lines.append("K\t%d\t%s\t%.4f\t%d\t%d" % (k, _fixed(r["td"], F), mean, r["n_swap"], r["converged"]))
        if best is None or mean > best[0]:
            best = (mean, r, sil)
    _, r, sil = best
    lines.append("#C\tcluster\tmedoid\tsize\tmean_sil")
    for c, m in enumerate(r["medoid"]):
        lines.append("C\t%d\t%s\t%d\t%.4f" % (c + 1, names[int(m)], int(r["size"][c]), mean_sil(r, sil, c)))
    lines.append("#A\tassembly\tcluster\tmedoid\tdist\tsil")
    for o, name in enumerate(names):
        c = int(r["label"][o])
        lines.append("A\t%s\t%d\t%s\t%s\t%.4f" % (name, c + 1, names[int(r["medoid"][c])], _fixed(r["dist"][o], F), sil[o]))
    return ("\n".join(lines) + "\n").encode()


def decomposition(q, M, last=False):
    """delta[x][m] in the layout of deltas(), from removal, acc and plus (k_medoids.hpp).  last: a column as near to a second medoid as
    to its nearest takes the LAST of them as its nearest instead of the first -- the identity holds either way."""
    q = np.asarray(q, dtype=np.int64)
    n = q.shape[0]
    ms = sorted(M)
    cand = np.array([x for x in range(n) if x not in M], dtype=np.int64)
    sub = q[:, ms]  # [o][slot]
    nn = (len(ms) - 1 - np.argmin(sub[:, ::-1], axis=1)) if last else np.argmin(sub, axis=1)
    D = sub[np.arange(n), nn]
    masked = sub.copy()
    masked[np.arange(n), nn] = LIMIT
    DS = masked.min(axis=1)
    removal = np.array([int((DS - D)[nn == s].sum()) for s in range(len(ms))], dtype=np.int64)
    d = q[cand]  # [x][o]
    plus = np.where(d < D[None, :], d - D[None, :], 0).sum(axis=1)
    f = np.where(d < D[None, :], (D - DS)[None, :], np.where(d < DS[None, :], d - DS[None, :], 0))
    acc = np.stack([f[:, nn == s].sum(axis=1) for s in range(len(ms))], axis=1)
    return cand, ms, removal[None, :] + acc + plus[:, None]


def planted(n, groups, seed, spread=40, grid=1 << 12):
    """(n, n) int32: L1 distances of points scattered on a coarse integer grid around `groups` centres -- a metric with cluster
    structure, many tied distances and, where two points fall on one grid node, zeros off the diagonal"""
    rng = np.random.default_rng(seed)
    centre = rng.integers(0, 1000, size=(groups, 3))
    pts = centre[rng.integers(0, groups, size=n)] + rng.integers(-spread, spread + 1, size=(n, 3)) // 8 * 8
    q = np.abs(pts[:, None, :] - pts[None, :, :]).sum(axis=2) * grid
    return q.astype(np.int32)


def random_matrix(n, seed, hi=1 << 20):
    """(n, n) int32: symmetric, zero diagonal, entries uniform in [0, hi) -- no structure at all, so BUILD is far from a local optimum
    and SWAP has work to do; a small hi gives many ties"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, hi, size=(n, n))
    q = np.triu(a, 1)
    return (q + q.T).astype(np.int32)


def full_random(n, seed):
    """(n, n) int32: symmetric, zero diagonal, entries uniform in [2^28, 2^29) -- the upper half of the range the definition admits, so
    that every sum over a few columns needs 64 bits"""
    rng = np.random.default_rng(seed)
    q = np.triu(rng.integers(1 << 28, LIMIT, size=(n, n)), 1)
    return (q + q.T).astype(np.int32)


# (n, k) of the uniform matrices against the restatement, the one against the checker build, and (n, k, groups, spread, swaps at the
# least) of the matrices with structure: planted() on a grid of 2^17, entries up to 3 240 << 17 < 2^29
MAGNITUDE_RANDOM = ((257, 2), (257, 17), (513, 3))
MAGNITUDE_CHECKER = (1025, 16)
MAGNITUDE_PLANTED = ((257, 17, 5, 300, 3), (769, 9, 4, 300, 3), (1281, 2, 2, 300, 1))


def magnitude_inputs():
    """[(label, q, k, swaps at the least or None)] of the `magnitude` cases that the restatement checks.  n = 257 and above: the sums
    cross workgroups.  The last one has n = 1 281 columns, five or six a lane in the one-workgroup-a-row kernels, and half of them within
    2^27 of the candidate: a lane's own part of BUILD's first gain passes 2^31 (first_gain_parts)."""
    out = [("uniform", full_random(n, n + k), k, None) for n, k in MAGNITUDE_RANDOM]
    out += [("planted", planted(n, g, 1, spread=spread, grid=1 << 17), k, swaps) for n, k, g, spread, swaps in MAGNITUDE_PLANTED]
    return out


def first_gain_parts(q, lanes=256):
    """the largest sum over the columns o = l (mod lanes) of BUILD's first gain max(0, 2^29 - q[x][o]), x the first medoid"""
    q = np.asarray(q, dtype=np.int64)
    x = int(medoids(q, 2, 0)["rec"][0, 0])
    v = np.maximum(LIMIT - q[x], 0)
    return max(int(v[l::lanes].sum()) for l in range(lanes))
