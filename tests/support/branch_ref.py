"""pg_mark_branch_flt_arc (reference branch.c:60-90) restated in plain Python over a GIVEN "is local" relation, and the tables that make the
device see that relation (tests/test_branch_lazy_gpu.py).

A vertex is (s1[n], local) with local a set of frozenset({i, j}) over its arcs; every arc of every vertex gets a gene of its own.  The relation
is encoded in the position records by giving local pair number p of a vertex genome p, in which only those two genes of the vertex are
present, on a contig of the vertex's own and at the same place: pg_n_local of two genes is then > 0 iff the pair is in the relation, however
non-transitive the relation is."""
import numpy as np

WAVE = 64


def decide_ref(s1, local, bd, bdist, bcut):
    """-> (weak_br[n], n_dist_loci, pairs consulted by the rows >= 1 as the lazy form lists them) of one vertex"""
    n = len(s1)
    if n < 2:
        return [0] * n, 0, 0
    loc = lambda i, j: frozenset((i, j)) in local  # noqa: E731
    max_s1 = max(s1)
    best = [i for i in range(n) if s1[i] == max_s1]
    weak = [0] * n
    for i in range(n):  # branch.c:70-79
        r = 1.0 - float(s1[i]) / max_s1
        if r > bd:
            n_local = sum(loc(j, i) for j in best)
            weak[i] = 2 if ((n_local == 0 and r > bdist) or r > bcut) else 1
    tmp, n_group = [0] * n, 0
    residual = 0
    for i in range(n):  # branch.c:83-89
        if tmp[i] == 0:
            n_group += 1
            tmp[i] = n_group
        for j in range(i + 1, n):
            if loc(i, j) and tmp[j] == 0:
                tmp[j] = tmp[i]
        if i == 0:
            residual = sum(j - 1 for j in range(1, n) if tmp[j] == 0)  # every (i, j), 1 <= i < j, for the j row 0 left without a group
    return weak, n_group, residual


def n_pairs(s1, bd, lazy):
    """the length of a vertex's stretch of the main list"""
    n = len(s1)
    if n < 2:
        return 0
    max_s1 = max(s1)
    n_max = sum(1 for v in s1 if v == max_s1)
    n_weak = sum(1 for v in s1 if 1.0 - float(v) / max_s1 > bd)
    return n_max * n_weak + (n - 1 if lazy and n <= WAVE else n * (n - 1) // 2)


def tables(vertices):
    """-> dict(vs, ve, s1, agid, rp[Q, GL, 4], Q, GL) for a list of (s1, local) vertices"""
    vs, ve, s1, off = [], [], [], 0
    for sc, _ in vertices:
        vs.append(off)
        off += len(sc)
        ve.append(off)
        s1 += list(sc)
    Q = max(off, 1)
    GL = max([len(loc) for _, loc in vertices] + [1])
    rp = np.zeros((Q, GL, 4), dtype=np.int32)
    rp[:, :, 0] = -1  # absent
    for v, (sc, loc) in enumerate(vertices):
        for p, pair in enumerate(sorted(tuple(sorted(x)) for x in loc)):
            for k, i in enumerate(pair):
                rp[vs[v] + i, p] = (v, 5 * k, 1000 + 7 * k, 0)  # {contig, rank, cm, interval}: 7 apart on the same contig
    return dict(vs=np.array(vs, dtype=np.int32), ve=np.array(ve, dtype=np.int32), s1=np.array(s1 or [1], dtype=np.int32),
                agid=np.arange(Q, dtype=np.int32), rp=rp, Q=Q, GL=GL)
