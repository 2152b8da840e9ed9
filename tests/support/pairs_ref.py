"""TEST INFRASTRUCTURE: a plain Python restatement of the lineage-aware trait test (DESIGN.md section 8 "Lineage-aware trait test";
include/pangene_amd.h pg_pan_pairs, pangene trait -L) for tests/test_pairs.py and tests/test_pairs_gpu.py.  Two things: the dynamic
programme over the records of a tree, with values (pairs, side) compared as tuples and None for infeasible; and a brute force for at
most 8 leaves that enumerates every set of contrasting leaf pairs and keeps those whose tree paths share no vertex.  The binomial p
values are exact big-integer sums."""
import math
from fractions import Fraction

import numpy as np

import dist_ref as dr
import tree_ref as tr

COLUMNS = "pairs\tsupp\topp\tp_pair_best\tp_pair_worst"
SUPPORTING = {(3, 0), (0, 3)}  # type = gene bit * 2 + label; 3-0 supports, 2-1 opposes


def tree(rec, A, method, trifurcation=0):
    """The records as a binary tree: kids, one (a, b) per join, node x < A = leaf x, node A + t = join t (children before parents, the
    root last).  nj's closing record (x, y, z) is read as ((x, y), z); trifurcation = 1, 2 reads it as ((x, z), y), ((y, z), x)."""
    if A < 2:
        return []
    if A == 2:
        return [(0, 1)]
    at = list(range(A))
    kids = []

    def join(i, j):
        kids.append((at[i], at[j]))
        at[i], at[j] = A + len(kids) - 1, None

    rec = np.asarray(rec, dtype=np.int64).reshape(-1, 6)
    n_plain = A - 3 if method == "nj" else A - 1
    for t in range(n_plain):
        join(int(rec[t, 0]), int(rec[t, 1]))
    if method == "nj":
        x, y, z = (int(v) for v in rec[n_plain, :3])
        a, b, c = ((x, y, z), (x, z, y), (y, z, x))[trifurcation]
        join(a, b)
        join(a, c)
    return kids


def types(gene_row, labels):
    """per leaf: gene bit * 2 + label, None for a leaf without a label"""
    return [None if y < 0 else (2 if b else 0) + (1 if y > 0 else 0) for b, y in zip(gene_row, labels)]


def _add(a, b):
    return None if a is None or b is None else (a[0] + b[0], a[1] + b[1])


def _best(*vals):
    vals = [v for v in vals if v is not None]
    return max(vals) if vals else None


def dp(kids, leaf_types, side):
    """(pairs, pairs of `side` among them) of the root: the lexicographic maximum.  side = SUPPORTING or its complement"""
    if not leaf_types:
        return (0, 0)
    N, F = [], []
    for s in leaf_types:
        N.append((0, 0))
        F.append([(0, 0) if s == c else None for c in range(4)])
    for a, b in kids:
        n = _add(N[a], N[b])
        for s in range(4):
            t = 3 - s
            bonus = (1, 1 if ((s, t) in SUPPORTING) == side else 0)
            n = _best(n, _add(_add(F[a][s], F[b][t]), bonus))
        N.append(n)
        F.append([_best(_add(F[a][s], N[b]), _add(N[a], F[b][s])) for s in range(4)])
    return N[-1]


def counts_one(kids, leaf_types):
    """(pairs, supp, opp) of one gene and trait"""
    best, worst = dp(kids, leaf_types, True), dp(kids, leaf_types, False)
    assert best[0] == worst[0]
    return best[0], best[1], worst[1]


def counts(P, labels, rec, method, trifurcation=0):
    """What capi.pan_pairs returns: dict of int32 (T, G).  Genes with the same presence row share one run of the programme"""
    P = np.asarray(P) != 0
    L = np.asarray(labels)
    if L.ndim == 1:
        L = L[None, :]
    G, A = P.shape
    kids = tree(rec, A, method, trifurcation)
    out = np.zeros((3, L.shape[0], G), dtype=np.int32)
    for ti in range(L.shape[0]):
        seen = {}
        for g in range(G):
            key = P[g].tobytes()
            if key not in seen:
                seen[key] = counts_one(kids, types(P[g], L[ti]))
            out[:, ti, g] = seen[key]
    return {"pairs": out[0], "supp": out[1], "opp": out[2]}


def brute(kids, leaf_types):
    """(pairs, supp, opp) by enumeration: every set of contrasting leaf pairs whose tree paths share no vertex; at most 8 leaves"""
    A = len(leaf_types)
    assert A <= 8
    up = {}
    for t, (a, b) in enumerate(kids):
        up[a] = up[b] = A + t

    def path(u, v):
        pu, pv = [u], [v]
        while pu[-1] in up:
            pu.append(up[pu[-1]])
        while pv[-1] in up:
            pv.append(up[pv[-1]])
        common = set(pu) & set(pv)
        top = next(x for x in pu if x in common)  # the lowest common ancestor
        return frozenset(pu[:pu.index(top) + 1]) | frozenset(pv[:pv.index(top)])

    cand = []  # (leaf u, leaf v, supporting?, vertices of the path)
    for u in range(A):
        for v in range(u + 1, A):
            s, t = leaf_types[u], leaf_types[v]
            if s is not None and t is not None and s + t == 3:
                cand.append((u, v, (s, t) in SUPPORTING, path(u, v)))
    best = {}  # size -> (most supporting, most opposing)

    def walk(k, used, n, n_supp):
        m = best.get(n, (-1, -1))
        best[n] = (max(m[0], n_supp), max(m[1], n - n_supp))
        for i in range(k, len(cand)):
            if not (cand[i][3] & used):
                walk(i + 1, used | cand[i][3], n + 1, n_supp + cand[i][2])

    walk(0, frozenset(), 0, 0)
    top = max(best)
    return top, best[top][0], best[top][1]


def p2(k, n):
    """exact two-sided binomial p at 1/2: min(1, 2 P(X >= max(k, n - k))), 1 for n = 0"""
    if n == 0:
        return 1.0
    m = max(k, n - k)
    return min(1.0, float(Fraction(2 * sum(math.comb(n, x) for x in range(m, n + 1)), 1 << n)))


def columns(D, pairs, supp, opp):
    """the five columns pangene trait -L appends to a line whose gene has the association D"""
    n_for, n_against = (supp, opp) if D >= 0 else (opp, supp)
    return "%d\t%d\t%d\t%.3e\t%.3e" % (pairs, supp, opp, p2(n_for, pairs), p2(pairs - n_against, pairs))


def records(P, method):
    """the records of the tree `pangene tree -t gene -m jaccard -a method` builds over all assemblies of P (G, A); None below 3"""
    P = np.asarray(P) != 0
    if P.shape[1] < 3:
        return None
    return tr.joins(tr.fixed(dr.shared(P), "jaccard")[0], method)


def table(genes, P, trait_names, labels, method):
    """{(trait, gene): the five columns} for every gene and every trait that has two values"""
    P = np.asarray(P) != 0
    L = np.asarray(labels)
    keep = [ti for ti in range(len(trait_names)) if (L[ti] == 0).any() and (L[ti] > 0).any()]
    out = {}
    if not keep:
        return out
    c = counts(P, L[keep], records(P, method), method)
    for r, ti in enumerate(keep):
        cols = np.nonzero(L[ti] >= 0)[0]
        y = L[ti][cols] > 0
        N, t = len(cols), int(y.sum())
        for g, name in enumerate(genes):
            a, s = int(P[g, cols].sum()), int((P[g, cols] & y).sum())
            out[(trait_names[ti], name)] = columns(s * N - a * t, int(c["pairs"][r, g]), int(c["supp"][r, g]), int(c["opp"][r, g]))
    return out


def balanced_records(A):
    """upgma-shaped records of a balanced tree of A leaves: neighbours are joined level by level (leaves 2 m and 2 m + 1 first, then
    their parents, ...; an odd one out waits for the next level); the stack need is floor(log2 A) + 1 for A = 2^k and A = 2^k - 1"""
    rec, nodes, size = [], list(range(A)), [1] * A
    while len(nodes) > 1:
        nxt = []
        for k in range(0, len(nodes) - 1, 2):
            i, j = nodes[k], nodes[k + 1]
            rec.append((i, j, 0, size[i], size[j], 0))
            size[i] += size[j]
            nxt.append(i)
        if len(nodes) % 2:
            nxt.append(nodes[-1])
        nodes = nxt
    return np.array(rec, dtype=np.int64).reshape(-1, 6)


def caterpillar_records(A):
    """upgma-shaped records of a caterpillar: ((((0, 1), 2), 3), ...); the stack need is 2"""
    return np.array([(0, j, 0, j, 1, 0) for j in range(1, A)], dtype=np.int64).reshape(-1, 6)


def program(kids, A):
    """The backend's postfix program of a tree: (op uint8 [2 A - 1] with 0 = push the next leaf and 1 = join the top two, the leaves in
    push order, the stack entries it needs).  A join visits the child with the larger need first, ties the first child"""
    if A == 0:
        return np.zeros(0, dtype=np.uint8), [], 0
    need = [1] * A
    for a, b in kids:
        need.append(need[a] + 1 if need[a] == need[b] else max(need[a], need[b]))
    op, order, todo = [], [], [A + len(kids) - 1]
    while todo:
        v = todo.pop()
        if v < 0:
            op.append(1)
        elif v < A:
            op.append(0)
            order.append(v)
        else:
            a, b = kids[v - A]
            first, second = (a, b) if need[a] >= need[b] else (b, a)
            todo += [~v, second, first]
    return np.array(op, dtype=np.uint8), order, need[-1]
