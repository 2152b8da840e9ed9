"""TEST INFRASTRUCTURE: a plain numpy restatement of pangene phylosig (DESIGN.md section 8 "Phylogenetic signal"; include/pangene_amd.h
pg_pan_phylosig, include/pangene_hip.h pga_pan_phylosig) for tests/test_phylosig.py and tests/test_phylosig_gpu.py.  The pinned
Fisher-Yates orders with splitmix64 (one order in Python integers, a batch of them stepped together in uint64 arrays), the tip sets
o_p[x] < n, the (C0, C1) recurrence over the tree of pairs_ref.tree with every replicate at once as a vector, the counts, the sums,
Benjamini-Hochberg, and the table as the bytes the command prints; the counts by direct loops and every tree shape of a few leaves for
the brute force of tests/test_phylosig.py."""
import numpy as np

import gainloss_ref as gr
import pairs_ref as pr

HEADER = b"Gene\tPresent\tCost\tMaxCost\tExpect\tRI\tn_le\tn_ge\tp_signal\tp_scatter\tq_signal\n"
M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def _mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def fisher_yates_order(A, seed, p):
    """pgx::fisher_yates_order(A, seed, p): from the last column down, j = next() % (i + 1), splitmix64 from mix((seed << 32) | p)"""
    o = list(range(A))
    x = _mix(((seed & 0xFFFFFFFF) << 32) | p)
    for i in range(A - 1, 0, -1):
        x = (x + GOLDEN) & M64
        j = _mix(x) % (i + 1)
        o[i], o[j] = o[j], o[i]
    return o


def _mix_u64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def orders(A, seed, first, n):
    """(A, n) int32, assembly-major: column q = fisher_yates_order(A, seed, first + q), the n generators stepped together"""
    o = np.tile(np.arange(A, dtype=np.int32)[:, None], (1, n))
    cols = np.arange(n)
    with np.errstate(over="ignore"):
        x = _mix_u64(np.uint64((seed & 0xFFFFFFFF) << 32) | np.arange(first, first + n, dtype=np.uint64))
        for i in range(A - 1, 0, -1):
            x = x + np.uint64(GOLDEN)
            j = (_mix_u64(x) % np.uint64(i + 1)).astype(np.int64)
            oi = o[i].copy()
            o[i] = o[j, cols]
            o[j, cols] = oi
    return o


def up_costs(present, kids, g=1, l=1):
    """present (A, R) bool, one column per replicate or item: min(C0, C1) at the root, int64 (R,).  A leaf with bit b has C[b] = 0 and
    C[1 - b] = g + l; a join C[s] = the sum over its children of min(C_c[s], C_c[1 - s] + w(s)), w = (g, l).  An entry is dropped once
    its parent is made, so a large tree holds one level at a time."""
    present = np.asarray(present, dtype=bool)
    A = present.shape[0]
    w = (g, l)
    C = [None] * (A + len(kids))

    def take(v):
        if v < A:
            return np.where(present[v], g + l, 0).astype(np.int32), np.where(present[v], 0, g + l).astype(np.int32)  # (every cost stays below 2^25)
        c, C[v] = C[v], None
        return c

    for t, (a, b) in enumerate(kids):
        ca, cb = take(a), take(b)
        C[A + t] = tuple(np.minimum(ca[s], ca[1 - s] + w[s]) + np.minimum(cb[s], cb[1 - s] + w[s]) for s in (0, 1))
    c0, c1 = take(A + len(kids) - 1)
    return np.minimum(c0, c1).astype(np.int64)


def replicate_costs(kids, A, cls, n_perm, seed, g=1, l=1, first=1, rk=None):
    """int64 (len(cls), n_perm): cost(cls[c], first + q); rk: the orders (A, >= n_perm) when the caller has them already"""
    if rk is None:
        rk = orders(A, seed, first, n_perm)
    rk = rk[:, :n_perm]
    cls = np.asarray(cls, dtype=np.int64)
    if len(cls) == 0 or n_perm == 0:
        return np.zeros((len(cls), n_perm), dtype=np.int64)
    present = (rk[:, None, :] < cls[None, :, None]).reshape(A, len(cls) * n_perm)
    return up_costs(present, kids, g, l).reshape(len(cls), n_perm)


def counts(cost_rows, item_cls, item_cost):
    """(n_le, n_ge) int64 (n_item,) of the rows cost_rows (n_cls, P)"""
    rows = cost_rows[np.asarray(item_cls, dtype=np.int64)]
    obs = np.asarray(item_cost, dtype=np.int64)[:, None]
    return (rows <= obs).sum(axis=1), (rows >= obs).sum(axis=1)


def classes(present_counts, A, min_count=2):
    """(tested items ascending, cls ascending, item_cls per tested item)"""
    n = np.asarray(present_counts, dtype=np.int64)
    tested = np.nonzero(np.minimum(n, A - n) >= min_count)[0]
    cls = np.unique(n[tested])
    return tested, cls, np.searchsorted(cls, n[tested])


def pan_phylosig(P, kids, g=1, l=1, n_perm=1000, seed=11, min_count=2):
    """what capi.pan_phylosig returns: present, cost, tested, n_le, n_ge (int64 (M,)) and sum (int64 (A + 1,)); and cost_rows, cls"""
    P = np.asarray(P) != 0
    M, A = P.shape
    present = P.sum(axis=1).astype(np.int64)
    cost = up_costs(P.T, kids, g, l) if A >= 1 else np.zeros(M, dtype=np.int64)
    tested, cls, item_cls = classes(present, A, min_count)
    rows = replicate_costs(kids, A, cls, n_perm, seed, g, l) if len(tested) else np.zeros((0, n_perm), dtype=np.int64)
    le, ge = counts(rows, item_cls, cost[tested]) if len(tested) else (np.zeros(0, dtype=np.int64),) * 2
    out = {k: np.zeros(M, dtype=np.int64) for k in ("tested", "n_le", "n_ge")}
    out["present"], out["cost"] = present, cost
    out["tested"][tested], out["n_le"][tested], out["n_ge"][tested] = 1, le, ge
    out["sum"] = np.zeros(A + 1, dtype=np.int64)
    out["sum"][cls] = rows.sum(axis=1)
    out["cost_rows"], out["cls"] = rows, cls
    return out


def same(got, want):
    """what capi.pan_phylosig returns against pan_phylosig"""
    return all(np.array_equal(np.asarray(got[k], dtype=np.int64), want[k]) for k in ("present", "cost", "tested", "n_le", "n_ge", "sum"))


def bh(p):
    """Benjamini-Hochberg q of p (in row order): sort ascending, ties by row; q_(i) = min over j >= i of p_(j) m / j, capped at 1"""
    m = len(p)
    idx = sorted(range(m), key=lambda i: (p[i], i))
    q, run = [0.0] * m, 1.0
    for j in range(m, 0, -1):
        run = min(run, p[idx[j - 1]] * m / j)
        q[idx[j - 1]] = run
    return q


def table_of(item_names, A, res, g=1, l=1, n_perm=1000, max_p=1.0):
    """the bytes of the table for the result of pan_phylosig"""
    tested = np.nonzero(res["tested"])[0]
    ps = [(1.0 + int(res["n_le"][i])) / (1.0 + n_perm) for i in tested]
    pc = [(1.0 + int(res["n_ge"][i])) / (1.0 + n_perm) for i in tested]
    q = bh(ps)
    out = [HEADER]
    for k, i in enumerate(tested):
        if n_perm > 0 and min(ps[k], pc[k]) > max_p:
            continue
        n, cost = int(res["present"][i]), int(res["cost"][i])
        max_cost = min(n * g, (A - n) * l)
        den = max_cost - min(g, l)
        ri = "NA" if den == 0 else "%.4f" % (float(max_cost - cost) / float(den))
        if n_perm > 0:
            rest = "%.3f\t%s\t%d\t%d\t%.6f\t%.6f\t%.6f" % (float(int(res["sum"][n])) / float(n_perm), ri, res["n_le"][i], res["n_ge"][i], ps[k], pc[k], q[k])
        else:
            rest = "NA\t%s\tNA\tNA\tNA\tNA\tNA" % ri
        out.append(("%s\t%d\t%d\t%d\t%s\n" % (item_names[i], n, cost, max_cost, rest)).encode())
    return b"".join(out)


def table(gfa, kind="gene", metric="jaccard", method="upgma", g=1, l=1, n_perm=1000, seed=11, min_count=2, max_p=1.0):
    """What `pangene phylosig` prints for a GFA file"""
    names, item_names, P = gr.items(gfa, kind)
    A = len(names)
    if A == 0 or P.shape[0] == 0:
        return HEADER
    kids = pr.tree(gr.records(P, metric, method), A, method)
    return table_of(item_names, A, pan_phylosig(P, kids, g, l, n_perm, seed, min_count), g, l, n_perm, max_p)


def brute_counts(costs_of_class, obs):
    """(n_le, n_ge) of one item by direct loops"""
    le = ge = 0
    for c in costs_of_class:
        if c <= obs:
            le += 1
        if c >= obs:
            ge += 1
    return le, ge


def all_shapes(A):
    """every rooted binary tree shape over the leaves 0 .. A - 1 in this order (the Catalan number of them) as kids lists in the numbering
    of pairs_ref.tree: node x < A = leaf x, node A + t = join t, children before parents, the root last"""
    def build(lo, hi):  # the shapes over leaves lo .. hi - 1 as nested tuples
        if hi - lo == 1:
            return [lo]
        return [(a, b) for m in range(lo + 1, hi) for a in build(lo, m) for b in build(m, hi)]

    out = []
    for shape in build(0, A):
        kids = []

        def number(s):
            if not isinstance(s, tuple):
                return s
            a, b = number(s[0]), number(s[1])
            kids.append((a, b))
            return A + len(kids) - 1
        number(shape)
        out.append(kids)
    return out


def option_args(kind="gene", metric="jaccard", method="upgma", g=1, l=1, n_perm=1000, seed=11, min_count=2, max_p=1.0):
    """the same options as the arguments of `pangene phylosig` and of `pangene --phylosig`"""
    sub = ["-t", kind, "-m", metric, "-a", method, "-g", str(g), "-l", str(l), "-n", str(n_perm), "-s", str(seed), "-c", str(min_count), "-p", repr(float(max_p))]
    long = ["--phylosig=%d" % n_perm, "--phylosig-type=" + kind, "--phylosig-metric=" + metric, "--phylosig-method=" + method, "--phylosig-gain=%d" % g,
            "--phylosig-loss=%d" % l, "--phylosig-seed=%d" % seed, "--phylosig-min=%d" % min_count, "--phylosig-max-p=" + repr(float(max_p))]
    return sub, long


def capi_options(kind="gene", metric="jaccard", method="upgma", g=1, l=1, n_perm=1000, seed=11, min_count=2, max_p=1.0):
    """the same options as the keywords of capi.phylosig_opt"""
    return dict(type=kind, metric=metric, method=method, gain=g, loss=l, n_perm=n_perm, seed=seed, min_count=min_count, max_p=max_p)


# the option sets the fixtures go through: the default; adj/diff/nj; -g 2 -l 1; -c 1 -n 50 -s 7; -n 0
OPTION_SETS = ({}, {"kind": "adj", "metric": "diff", "method": "nj"}, {"g": 2, "l": 1}, {"min_count": 1, "n_perm": 50, "seed": 7}, {"n_perm": 0})
