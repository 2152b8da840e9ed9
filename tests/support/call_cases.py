"""TEST INFRASTRUCTURE: seeded inputs of pga_call_bubbles for tests/test_call_ref.py and tests/support/call_direct.py -- walk and bubble
shapes that no graph of the pipeline has.  Every live bubble has vs != ve (the host route never passes another).

    cases(which) -> list of (label, (step, walk_off, n_seg, bub_vs, bub_ve), has_records)

has_records is False for the inputs built to have no record; everything else must have some (tests/test_call_ref.py asserts it)."""
import itertools

import numpy as np

WHICH = ("exhaustive", "edges", "pileup", "graphlike")
SCAN_TILE = 1024      # TILE of dev_prims.hpp (the tiled scan), RS_TILE = 2048 (a radix tile), SCAN_ONE_MAX = 4096 (the one-block scan)


def _pack(walks, n_seg, bubbles):
    """walks: a list of vertex lists; bubbles: a list of (vs, ve)"""
    off = np.zeros(len(walks) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(w) for w in walks])
    step = np.asarray([v for w in walks for v in w], dtype=np.int32)
    b = np.asarray(bubbles, dtype=np.int32).reshape(-1, 2)
    return step, off, int(n_seg), np.ascontiguousarray(b[:, 0]), np.ascontiguousarray(b[:, 1])


def exhaustive():
    """4 vertices, every walk of 1 .. 4 steps (340 walks, 1 252 steps) against all 12 ordered pairs vs != ve -- the hairpins
    ve == vs ^ 1 among them -- two of them twice, and two entries that are no bubble, the first and one in the middle"""
    walks = [list(w) for n in (1, 2, 3, 4) for w in itertools.product(range(4), repeat=n)]
    pairs = [(a, b) for a in range(4) for b in range(4) if a != b]
    bub = [(-1, -1)] + pairs[:6] + [(-1, 3)] + pairs[6:] + [pairs[1], pairs[8]]  # (0, 1) is a hairpin, (2, 3) another
    return [("exhaustive", _pack(walks, 2, bub), True)]


def _lengths(rng, n_walk, N):
    """n_walk lengths that add up to N; with room for it the first walk, the last one and two neighbours in the middle are empty"""
    empty = set()
    if n_walk >= 6:
        empty = {0, n_walk - 1, n_walk // 2, n_walk // 2 + 1}
    elif n_walk >= 2:
        empty = {int(rng.integers(0, 2)) * (n_walk - 1)}
    live = [j for j in range(n_walk) if j not in empty]
    cut = np.sort(rng.integers(0, N + 1, size=len(live) - 1))
    ln = np.zeros(n_walk, dtype=np.int64)
    ln[live] = np.diff(np.concatenate(([0], cut, [N])))
    return ln


def random_case(seed, n_seg, n_walk, N, n_bub):
    """Random walks over a skewed vertex distribution (a few hot vertices recur inside every walk, the highest vertex 2 n_seg - 1 is
    one of them) and bubbles taken from the walks: (w[p], w[i]) with i - p in 1 .. 4; one in eight is no bubble, one in eight is a
    hairpin (u, u ^ 1), one in eight a random pair, and -- with 8 bubbles or more -- 8 share the end vertex of bubble 0, one of
    them twice."""
    rng = np.random.default_rng([seed, n_seg, n_walk, N, n_bub])
    nv = 2 * n_seg
    hot = np.unique(np.concatenate(([nv - 1], rng.integers(0, nv, size=min(nv, 5)))))
    ln = _lengths(rng, n_walk, N)
    p_hot = min(0.5, 12.0 * max(1, int((ln > 0).sum())) / max(1, N))  # a dozen hot steps a walk: records grow with their square
    step = np.where(rng.random(N) < p_hot, rng.choice(hot, size=N), rng.integers(0, nv, size=N)).astype(np.int32)
    off = np.concatenate(([0], np.cumsum(ln))).astype(np.int64)
    wid = np.searchsorted(off, np.arange(N), side="right") - 1

    def other(u):
        return int((u + 1 + rng.integers(0, nv - 1)) % nv)  # any vertex but u

    def from_walk():
        for _ in range(64):
            p = int(rng.integers(0, N))
            i = p + int(rng.integers(1, 5))
            if i < N and wid[i] == wid[p] and step[i] != step[p]:
                return int(step[p]), int(step[i])
        u = int(rng.integers(0, nv))
        return u, other(u)

    bub = []
    for b in range(n_bub):
        kind = int(rng.integers(0, 8)) if b > 0 else 7
        if kind == 0:
            bub.append((-1, int(rng.integers(-1, nv))))
        elif kind == 1:
            u = int(rng.integers(0, nv))
            bub.append((u, u ^ 1))
        elif kind == 2:
            u = int(rng.integers(0, nv))
            bub.append((u, other(u)))
        else:
            bub.append(from_walk())
    if n_bub >= 8:
        ve = bub[0][1]
        slots = rng.choice(np.arange(1, n_bub), size=7, replace=False)
        at = np.flatnonzero(step == ve)
        for s in slots[:6]:
            q = int(rng.choice(at)) if at.size else 0
            before = q > 0 and wid[q - 1] == wid[q] and step[q - 1] != ve  # the step before an occurrence of ve, where there is one
            bub[int(s)] = (int(step[q - 1]) if before else other(ve), ve)
        bub[int(slots[6])] = bub[int(slots[0])]
    return step, off, int(n_seg), np.asarray([x[0] for x in bub], dtype=np.int32), np.asarray([x[1] for x in bub], dtype=np.int32)


# (n_seg, n_walk, N, n_bub): 2 n_seg = 254 / 256 / 258 crosses a step of the vertex bits; N around a radix tile (2 048), the scan
# tile (1 024) and the one-block scan (4 096); N = 1 cannot have a record (a record needs two steps).  The records of a walk grow
# with the square of its length over the vertices it has, and the interior steps with the cube: few segments or many bubbles go
# with many short walks, one or two long walks with many segments and few bubbles.
EDGE_SHAPES = [(1, 1, 1, 1), (1, 257, 2, 2), (2, 256, 2047, 3), (1, 255, 2048, 2), (127, 257, 2049, 256), (128, 256, 4095, 257),
               (129, 255, 4097, 256), (128, 257, 1023, 257), (129, 2, 1024, 3), (127, 1, 2047, 1), (128, 1, 2048, 2),
               (129, 2, 2049, 3), (128, 1, 4096, 3), (127, 2, 1025, 2)]
EDGE_SEEDS = (0, 1, 2)


def edges():
    out = []
    for n_seg, n_walk, N, n_bub in EDGE_SHAPES:
        for seed in EDGE_SEEDS:
            if N == 2:  # the smallest input with a record: one walk of two steps among empty ones
                walks = [[] for _ in range(n_walk)]
                walks[(n_walk // 3) * (seed + 1) % n_walk] = [seed & 1, (seed & 1) ^ 1]
                case = _pack(walks, n_seg, [(0, 1), (1, 0)][:n_bub])
            else:
                case = random_case(seed, n_seg, n_walk, N, n_bub)
            out.append(("edges n_seg=%d n_walk=%d N=%d n_bub=%d seed=%d" % (n_seg, n_walk, N, n_bub, seed), case, N > 1))
    # bubbles, steps, and no record: the vertices of (4, 6) and (6, 4) are in no walk, the end of (4, 0) is but its start is not,
    # and both vertices of (0, 2) are, but every 2 comes before every 0 of its walk
    out.append(("edges no record", _pack([[2, 2, 0, 0], [], [2, 0], [0], [2, 2, 2]], 4, [(4, 6), (6, 4), (4, 0), (0, 2)]), False))
    out.append(("edges no step", _pack([[], [], []], 3, [(0, 2), (3, 1)]), False))
    step, off, n_seg, vs, ve = random_case(5, 7, 9, 300, 12)
    out.append(("edges no live bubble", (step, off, n_seg, np.full_like(vs, -1), ve), False))
    return out


def pileup():
    """one walk u v u v ... (100 times) and its reverse complement, bubbles (u, v) and (v ^ 1, u ^ 1): 5 050 records a walk and
    bubble, 20 200 in all over 400 steps, 1.3 M interior steps, 100 alleles a bubble"""
    u, v = 0, 3
    w = [u, v] * 100
    rc = [x ^ 1 for x in reversed(w)]
    return [("pileup", _pack([w, rc], 3, [(u, v), (v ^ 1, u ^ 1)]), True)]


def graphlike(n_walk=2000, n_seg=5000, n_bub=3000, length=100, seed=1):
    """walks that are noisy copies (deletions, local inversions, tandem repeats) of windows of one base order, a third of them
    reversed and complemented; bubbles (w[p], w[i]) with i - p in 2 .. 12 taken from the walks"""
    rng = np.random.default_rng(seed)
    base = rng.permutation(n_seg) * 2 + (rng.random(n_seg) < 0.3)
    walks = []
    for j in range(n_walk):
        a = int(rng.integers(0, n_seg - length))
        w = base[a:a + length + int(rng.integers(-10, 11))].tolist()
        for _ in range(int(rng.integers(0, 4))):  # deletions
            p, n = int(rng.integers(0, len(w))), int(rng.integers(1, 6))
            del w[p:p + n]
        for _ in range(int(rng.integers(0, 3))):  # local inversions
            p, n = int(rng.integers(0, len(w))), int(rng.integers(2, 8))
            w[p:p + n] = [x ^ 1 for x in reversed(w[p:p + n])]
        for _ in range(int(rng.integers(0, 3))):  # tandem repeats
            p, n = int(rng.integers(0, len(w))), int(rng.integers(1, 5))
            w[p:p] = w[p:p + n] * int(rng.integers(1, 3))
        if j % 3 == 2:
            w = [x ^ 1 for x in reversed(w)]
        walks.append(w)
    bub = []
    while len(bub) < n_bub:
        w = walks[int(rng.integers(0, n_walk))]
        p = int(rng.integers(0, len(w)))
        i = p + int(rng.integers(2, 13))
        if i < len(w) and w[i] != w[p]:
            bub.append((w[p], w[i]))
    return [("graphlike", _pack(walks, n_seg, bub), True)]


def cases(which):
    return {"exhaustive": exhaustive, "edges": edges, "pileup": pileup, "graphlike": graphlike}[which]()
