"""TEST INFRASTRUCTURE: the walk side of `pangene call` (pga_call_bubbles) restated in plain Python with numpy, from the contract in
include/pangene_hip.h (the comment above pga_call_rec_t); no product code.  Checks the HIP kernels of k_call.hpp through
tests/support/call_direct.py, and itself through tests/test_call_ref.py (the records are built in two independent forms).

Input:  step (N,) int32 oriented segments (vertex = segment * 2 + reverse), walk_off (n_walk + 1,) int64, n_seg,
        bub_vs / bub_ve (n_bub,) int32 (bub_vs < 0: no bubble).
Output: walk_side(...) = dict(rec (R, 4) int32 [bo, walk, st_off, en_off], rep (R,) int32, cnt (R,) int32,
        gene_bub (H,) int32, gene_seg (H,) int32, gene_first (H,) int64)."""
import numpy as np

KEYS = ("rec", "rep", "cnt", "gene_bub", "gene_seg", "gene_first")


def _entries(bub_vs, bub_ve):
    """(bo, start vertex, end vertex) of every live (bubble, orientation): + runs vs .. ve, - runs ve^1 .. vs^1"""
    out = []
    for b in range(len(bub_vs)):
        if bub_vs[b] < 0:
            continue
        out.append((2 * b, int(bub_vs[b]), int(bub_ve[b])))
        out.append((2 * b + 1, int(bub_ve[b]) ^ 1, int(bub_vs[b]) ^ 1))
    return out


def _as_rec(rows):
    return np.asarray(rows, dtype=np.int32).reshape(-1, 4)


def records_procedure(step, walk_off, n_seg, bub_vs, bub_ve):
    """One pass over every walk with an open-starts list per end vertex, reset the first time a start for that vertex appears in a new
    walk; at each position the starts at this vertex are registered first, then the ends at this vertex emit one record for EVERY open
    start (ends never close a start); collected per bubble."""
    starts_at = {}
    for bo, u, v in _entries(bub_vs, bub_ve):
        starts_at.setdefault(u, []).append((bo, v))
    open_at, open_walk = {}, {}
    per = [[] for _ in range(len(bub_vs))]
    step = np.asarray(step).tolist()
    for j in range(len(walk_off) - 1):
        a = int(walk_off[j])
        for i in range(int(walk_off[j + 1]) - a):
            x = step[a + i]
            for bo, v in starts_at.get(x, ()):
                if open_walk.get(v) != j:
                    open_walk[v], open_at[v] = j, []
                open_at[v].append((i, bo))
            if open_walk.get(x) == j:
                for st, bo in open_at[x]:
                    per[bo >> 1].append((bo, j, st, i))
    return _as_rec([r for p in per for r in p])


def records_closed_form(step, walk_off, n_seg, bub_vs, bub_ve):
    """For every live (bubble, orientation) with start u and end v: all pairs p < i of one walk with walk[p] == u and walk[i] == v;
    sorted by (bubble, walk, en_off, st_off, orientation)."""
    step = np.asarray(step, dtype=np.int64)
    walk_off = np.asarray(walk_off, dtype=np.int64)
    N = len(step)
    wid = np.searchsorted(walk_off, np.arange(N, dtype=np.int64), side="right") - 1  # the last walk that starts at or before g
    where = {}
    order = np.argsort(step, kind="stable")
    cut = np.searchsorted(step[order], np.arange(2 * n_seg + 1))
    parts = []
    for bo, u, v in _entries(bub_vs, bub_ve):
        for x in (u, v):
            if x not in where:
                where[x] = order[cut[x]:cut[x + 1]]  # ascending positions of vertex x
        P, Q = where[u], where[v]
        if len(P) == 0 or len(Q) == 0:
            continue
        lo = np.searchsorted(P, walk_off[wid[Q]], side="left")  # starts at or after the beginning of the end's walk ...
        hi = np.searchsorted(P, Q, side="left")                 # ... and before the end
        n = hi - lo
        if n.sum() == 0:
            continue
        q = np.repeat(Q, n)
        p = P[np.repeat(lo, n) + (np.arange(n.sum()) - np.repeat(np.cumsum(n) - n, n))]
        w = wid[q]
        parts.append(np.stack([np.full(len(q), bo, dtype=np.int64), w, p - walk_off[w], q - walk_off[w]], axis=1))
    if not parts:
        return _as_rec([])
    r = np.concatenate(parts)
    o = np.lexsort((r[:, 0] & 1, r[:, 2], r[:, 3], r[:, 1], r[:, 0] >> 1))
    return r[o].astype(np.int32)


def path_of(rec_row, step, walk_off):
    """the oriented path of a record, bubble start to bubble end: + is w[st .. en], - is w[en .. st] ^ 1"""
    bo, w, st, en = (int(x) for x in rec_row)
    p = np.asarray(step[int(walk_off[w]) + st:int(walk_off[w]) + en + 1], dtype=np.int32)
    return p if (bo & 1) == 0 else p[::-1] ^ 1


def alleles(rec, step, walk_off):
    """rep[r] = the first record of r's bubble with r's oriented path; cnt = the size of that class, at its representative"""
    R = len(rec)
    rep, cnt = np.zeros(R, dtype=np.int32), np.zeros(R, dtype=np.int32)
    first = {}
    step = np.ascontiguousarray(step, dtype=np.int32)
    for r in range(R):
        f = first.setdefault((int(rec[r, 0]) >> 1, path_of(rec[r], step, walk_off).tobytes()), r)
        rep[r] = f
        cnt[f] += 1
    return rep, cnt


def genes(rec, step, walk_off, n_seg):
    """interior steps st_off + 1 .. en_off - 1 numbered globally in record order; every (bubble, segment) once, with its first
    number, sorted by (bubble, segment)"""
    step = np.asarray(step, dtype=np.int64)
    walk_off = np.asarray(walk_off, dtype=np.int64)
    r = rec.astype(np.int64)
    n_int = np.maximum(r[:, 3] - r[:, 2] - 1, 0)
    n_tot = int(n_int.sum())
    if n_tot == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int64)
    first_in = walk_off[r[:, 1]] + r[:, 2] + 1  # global position of a record's first interior step
    k = np.arange(n_tot, dtype=np.int64) - np.repeat(np.cumsum(n_int) - n_int, n_int)
    seg = step[np.repeat(first_in, n_int) + k] >> 1
    bub = np.repeat(r[:, 0] >> 1, n_int)
    o = np.lexsort((np.arange(n_tot), seg, bub))  # (bubble, segment, number)
    head = np.ones(n_tot, dtype=bool)
    head[1:] = (bub[o][1:] != bub[o][:-1]) | (seg[o][1:] != seg[o][:-1])
    h = o[head]
    return bub[h].astype(np.int32), seg[h].astype(np.int32), h.astype(np.int64)


def walk_side(step, walk_off, n_seg, bub_vs, bub_ve, records=records_closed_form):
    rec = records(step, walk_off, n_seg, bub_vs, bub_ve)
    rep, cnt = alleles(rec, step, walk_off)
    gb, gs, gf = genes(rec, step, walk_off, n_seg)
    return dict(rec=rec, rep=rep, cnt=cnt, gene_bub=gb, gene_seg=gs, gene_first=gf)
