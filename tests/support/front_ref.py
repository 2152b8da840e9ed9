"""TEST INFRASTRUCTURE: plain restatement of the host's part of pg_post_process between the protein sums and post_apply
(graph_driver.cpp, post_host_step: pg_cap_score_dom's table, pg_flag_representative's protein part, the joint-pseudo predicate of
hit.c:176-181), for tests/test_front.py and tests/test_front_gpu.py.  Python integers and floats (IEEE doubles, one operation at a time:
what a build with -ffp-contract=off computes); nothing here is vectorised, the instances are a few hundred proteins.

sums: int64 [6, P] as pga_post_partials leaves them -- plane 0 the sum of score_adj, 2 / 3 the rank-0 hits with one / several exons,
4 / 5 their sums of score_ori; plane 1 (the count) is 2 + 3 and is ignored on input."""
import numpy as np

M64 = (1 << 64) - 1


def cvt_i32(v):
    """(int32_t)double as an x86-64 build computes it: truncation, 0x80000000 for what does not fit (and for a NaN)"""
    if v != v or not (-2147483649.0 < v < 2147483648.0):
        return -(1 << 31)
    return int(v)


def i32(x):
    """(int32_t)int64"""
    x &= 0xffffffff
    return x - (1 << 32) if x >= (1 << 31) else x


def keys_of(sums):
    """((uint64_t)sum << 32) + (uint64_t)count, per protein"""
    P = sums.shape[1]
    return [(((int(sums[0, p]) & M64) << 32) + ((int(sums[2, p]) + int(sums[3, p])) & M64)) & M64 for p in range(P)]


def fdiv(a, b):
    """a / b in doubles, with the IEEE results where Python raises: the divisors here are converted integers or a quotient 0 / n, so a
    zero divisor is +0"""
    a, b = float(a), float(b)
    if b == 0.0:
        if a == 0.0 or a != a:
            return float("nan")
        return float("inf") if a > 0 else float("-inf")
    return a / b


def n_and_avg(keys):
    n = [i32(k & 0xffffffff) for k in keys]
    avg = [cvt_i32(fdiv(k >> 32, nn) + .499) if nn else 0 for k, nn in zip(keys, n)]
    return n, avg


def reps_by_order(order, prot_gid, Q):
    """graph_driver.cpp: walking the sorted proteins from the back, the first protein met of a gene is its representative"""
    rep_pid = [-1] * Q
    for pid in reversed(list(order)):
        g = int(prot_gid[pid])
        if rep_pid[g] < 0:
            rep_pid[g] = int(pid)
    return rep_pid


def joint_pseudo(sums, n_genome, min_vertex_ratio, no_joint_pseudo, drop_sgl_exon):
    P = sums.shape[1]
    pj = [0] * P
    if no_joint_pseudo:
        return pj
    thr = n_genome * float(min_vertex_ratio)
    for p in range(P):
        ic0, ic1 = i32(int(sums[2, p])), i32(int(sums[3, p]))
        s0, s1 = int(sums[4, p]), int(sums[5, p])
        a = ic1 > 0 and float(ic1) >= thr and fdiv(fdiv(s1, ic1), fdiv(s0, ic0)) >= 0.99
        b = (ic1 == 0 or float(ic1) <= thr) and bool(drop_sgl_exon)
        pj[p] = int(bool(a or b))
    return pj


def post_rep_ref(sums, prot_gid, Q, n_genome, min_vertex_ratio, no_joint_pseudo=False, drop_sgl_exon=False):
    """-> dict: n, avg (per protein), rep_pid (per gene: the protein with the gene's largest key; among equal keys the smallest id, which
    is a GUESS then), tie (some gene has two proteins at its largest key: only the reference's sort order knows its representative),
    tie_genes, pj (per protein)"""
    keys = keys_of(sums)
    n, avg = n_and_avg(keys)
    best, rep_pid, n_best = [-1] * Q, [-1] * Q, [0] * Q
    for p, k in enumerate(keys):
        g = int(prot_gid[p])
        if k > best[g]:
            best[g], rep_pid[g], n_best[g] = k, p, 1
        elif k == best[g]:
            n_best[g] += 1
    tie_genes = [g for g in range(Q) if n_best[g] > 1]
    return {"keys": keys, "n": n, "avg": avg, "rep_pid": rep_pid, "tie": bool(tie_genes), "tie_genes": tie_genes,
            "pj": joint_pseudo(sums, n_genome, min_vertex_ratio, no_joint_pseudo, drop_sgl_exon)}


def instance(rng, sizes, tie_at_max=(), tie_below=(), zero_key_genes=(), zero_count=0.1, score=1 << 18):
    """sums [6, P] and prot_gid [P] for genes with sizes[g] proteins each, every key different unless asked otherwise; the proteins of a
    gene are scattered over the id range.  tie_at_max / tie_below: genes (of >= 2 / >= 3 proteins) whose two best / two worst proteins
    share a key; zero_key_genes: every protein of the gene has key 0; zero_count: share of the other proteins with no rank-0 hit."""
    Q = len(sizes)
    prot_gid = np.repeat(np.arange(Q, dtype=np.int32), sizes)
    rng.shuffle(prot_gid)
    P = len(prot_gid)
    sums = np.zeros((6, P), dtype=np.int64)
    c0, c1 = rng.integers(0, 40, size=P), rng.integers(0, 40, size=P)
    empty = rng.random(P) < zero_count
    c0[empty], c1[empty] = 0, 0
    sums[2], sums[3] = c0, c1
    sums[0] = rng.permutation(P).astype(np.int64) * 3 + rng.integers(1, score, size=P) * (4 * P)  # all different, so are the keys
    sums[0][rng.random(P) < 0.05] *= -1  # (a negative sum wraps in the key's unsigned arithmetic)
    sums[0] = np.where(sums[0] == 0, 1, sums[0])
    sums[4], sums[5] = rng.integers(0, score, size=P) * c0, rng.integers(0, score, size=P) * c1
    for g in zero_key_genes:
        sums[:, prot_gid == g] = 0
    keys = keys_of(sums)
    for genes, top in ((tie_at_max, True), (tie_below, False)):
        for g in genes:
            members = sorted(np.flatnonzero(prot_gid == g).tolist(), key=lambda p: keys[p])
            a, b = (members[-1], members[-2]) if top else (members[0], members[1])
            sums[0, b], sums[2, b], sums[3, b] = sums[0, a], sums[2, a], sums[3, a]
    return sums, prot_gid
