"""TEST INFRASTRUCTURE: shards for the exact-order overrides (pga_override_order, pga_set_head: pga_host_order.hpp, k_order.hpp, k_walk_list of k_genes.hpp),
the orders handed to them, and a plain restatement of what an override leaves, for tests/test_order.py (oracle against restatement, no GPU) and
tests/support/order_direct.py (the HIP backend against the oracle and against the restatement, step by step).

Built on stage_a_ref.Shard / sweep_ref.XGenome with the builders of arcs_ref (`_Build`, `_G.put(..., tie=True)`): a gene has one protein, three genomes
(37 hits, none, 50 hits) stand in front, so nothing starts on a multiple of 64.  A TIE GROUP here is a run of hits of different genes on one contig
that share their start (cs), their cm, or both; their exon lists share 10 of 110 bp or nothing, so that none shadows another and all of them are walkable.

The contract of an override (pangene_hip.h:239-249): a segment is a whole contig, file_idx lists all its hits, non-decreasing in cs (which = 0) or in cm
(which = 1); only the order inside groups of equal key is free.  `segs` draws it there: "rev" the group reversed, "rot" rotated by one, "perm" a drawn
permutation, "id" the canonical order (by file index for cs, by X position for cm: what pga_begin leaves), "ce_desc" / "ce_asc" by the hits' ends.

`override_restate` / `set_head_restate` are written from the ABI comment alone, as loops over Python lists: per genome x[p] = the file index of the hit
at X position p, y[k] = the X position of the hit at Y position k, head = the X position of "index 0".  `derived_restate` gives what the device must
hold beside them: pm, the (contig, cs) tie marks, one head mark a non-empty genome, inv.

The shards, by what they reach (asserted in tests/test_order.py); BLOCK = 256, a scan tile is 1 024 positions (dev_prims.hpp):
  grid      contigs of 1, 2, 252, 1, 1, 766, 1, 1, 3071, 1 hits: overrides of T = 1, 255, 256, 257, 1 023, 1 024, 1 025, 4 096, 4 097 hits, back to back,
            cs and cm in turn (the page-locked area grows twice on the way); a contig of one hit, one of two hits, swapped
  pm        a contig of 2 500 hits whose hit of maximal ce stands in a cs tie group at the contig's first position -- first there, then second (the first
            hit's pm falls); 4 144 hits in all, so that the override of every contig (more than SCAN_ONE_MAX entries) takes the tiled scan and carries
            that maximum across two tile borders, the smaller overrides across the threads and waves of the one-workgroup scan; two adjacent contigs
            whose last and first hit share cs; a tie group at a contig's end; groups of 2, 3, 64 and 65
  head      three genomes whose first contig begins with a tie group of two hits, both under a longer hit of a gene without a segment: set_head to one
            that is not first, a cs override of that contig, set_head again -- to the hit that now stands where the old mark stood, to another, not at all;
            an empty genome in between; a genome in which only a later contig is overridden
  cmties    cm tie groups of two and three walkable hits of different genes and two of one gene; a group whose middle hit is FLT, one whose middle hit is
            SHADOW; walkable hits whose nearest walkable neighbours along the contig lie 1, 63, 64, 65 and 300 positions away on either side; a contig that
            ends in unwalkable hits in front of one that begins with them; the first and the last walkable hit of the shard
  eighth, eighth1   N = 2 048: overrides of 256 hits (N / 8: the partial walk) and of 257 (the full one), the same orders
  strand    check_strand = 1: one gene twice at one start on opposite strands, swapped; a cs override drops the gene-major index, a cm override keeps it
  pieces    a contig in two virtual pieces (vfirst != NULL): the walk's records stand, the partial walk is off
  live      most of the hits are pseudogene hits, filtered before the vertex step: the live lists come on by themselves; contigs without a member,
            with one, with members only; non-members at both ends of a tie group and inside
  marks     arcs_ref's branch shard with the hub's hit and its target on one cm: after a cm override mark_hits marks other hits"""
import zlib

import numpy as np

import stage_a_ref as sr
import arcs_ref as ar

SCAN_TILE, BLOCK, SCAN_ONE_MAX = 1024, 256, 4096  # dev_prims.hpp:16, 68-69, 164 (a scan of at most SCAN_ONE_MAX entries takes one workgroup and has no tiles)
GRID_SIZES = (1, 2, 252, 1, 1, 766, 1, 1, 3071, 1)
GRID_T = (1, 255, 256, 257, 1023, 1024, 1025, 4096, 4097)
PM_SIZES = (2, 3, 64, 65)
WALK_D = (1, 63, 64, 65, 300)  # k_walk_list looks along the contig one position at a time; k_walk, whose answers it must give, 64 at a time
EIGHTH_N = 2048


# ------------------------------------------------------------------------------------------------
# the orders
# ------------------------------------------------------------------------------------------------
class Seg:
    """the arguments of one override"""

    def __init__(self, which, genome, start, off, file):
        self.which, self.n = int(which), len(genome)
        self.genome, self.start = np.ascontiguousarray(genome, np.int32), np.ascontiguousarray(start, np.int32)
        self.off, self.file = np.ascontiguousarray(off, np.int64), np.ascontiguousarray(file, np.int32)
        self.T = int(self.off[-1])


def contig_start(sh, j, c):
    return int((sh.genomes[j].cid < c).sum())


def canonical(sh, which, j, c):
    """the file indices of contig c of genome j in the order pga_begin leaves, and their keys"""
    g = sh.genomes[j]
    k = np.flatnonzero(g.cid == c)
    k = k[np.lexsort((k, g.cs[k]))]                      # X order: cs, then the file index
    if which == 1:
        k = k[np.argsort(g.cm[k], kind="stable")]        # Y order: cm, then the X position
    return k.tolist(), (g.cm if which else g.cs)[k].tolist()


def reorder(sh, which, j, c, mode, rng):
    fl, key = canonical(sh, which, j, c)
    ce = sh.genomes[j].ce
    out, i = [], 0
    while i < len(fl):
        e = i
        while e < len(fl) and key[e] == key[i]:
            e += 1
        grp = fl[i:e]
        if mode == "rev":
            grp = grp[::-1]
        elif mode == "rot":
            grp = grp[1:] + grp[:1]
        elif mode == "perm":
            grp = [grp[k] for k in rng.permutation(len(grp))]
        elif mode in ("ce_desc", "ce_asc"):
            grp = sorted(grp, key=lambda f: int(ce[f]) * (-1 if mode == "ce_desc" else 1))
        else:
            assert mode == "id", mode
        out += grp
        i = e
    return out


def segs(sh, which, items, rng, ident=False):
    """items: (genome, contig, mode) or (genome, contig, the file indices themselves)"""
    genome, start, off, file = [], [], [0], []
    for j, c, mode in items:
        fl = list(mode) if not isinstance(mode, str) else reorder(sh, which, j, c, "id" if ident else mode, rng)
        genome.append(j), start.append(contig_start(sh, j, c))
        file += fl
        off.append(len(file))
    return Seg(which, genome, start, off, file)


def seg_orders(seg):
    """{(genome, start): file indices} of an override"""
    return {(int(seg.genome[s]), int(seg.start[s])): seg.file[seg.off[s]:seg.off[s + 1]].tolist() for s in range(seg.n)}


def check_contract(sh, seg):
    """what the device relies on: whole contigs, keys that do not decrease"""
    for s in range(seg.n):
        j, st = int(seg.genome[s]), int(seg.start[s])
        g = sh.genomes[j]
        fl = seg.file[seg.off[s]:seg.off[s + 1]]
        if len(fl) == 0:
            continue
        c = int(g.cid[fl[0]])
        assert st == contig_start(sh, j, c) and sorted(fl.tolist()) == np.flatnonzero(g.cid == c).tolist()
        assert (np.diff((g.cm if seg.which else g.cs)[fl]) >= 0).all()


# ------------------------------------------------------------------------------------------------
# the restatement (pangene_hip.h:239-249)
# ------------------------------------------------------------------------------------------------
class State:
    def __init__(self, sh):
        w = sr.restate(sh)
        self.x, self.y, self.head = [], [], []
        for j in range(sh.G):
            a, e = int(sh.goff[j]), int(sh.goff[j + 1])
            self.x.append([int(v) for v in w["fidx"][a:e]])
            self.y.append([int(v) - a for v in w["yperm"][a:e]])
            self.head.append(0)


def override_restate(state, which, seg):
    genome, start, off, file = seg.genome.tolist(), seg.start.tolist(), seg.off.tolist(), seg.file.tolist()
    for s in range(seg.n):
        j, p0, fl = genome[s], start[s], file[off[s]:off[s + 1]]
        x, y = state.x[j], state.y[j]
        where = {}
        for p in range(len(x)):
            where[x[p]] = p
        if which == 1:  # the hits to put at the Y positions of the segment
            for k in range(len(fl)):
                y[p0 + k] = where[fl[k]]
            continue
        new = {}        # X position before -> after, for the hits that move
        for k in range(len(fl)):
            new[where[fl[k]]] = p0 + k
        for k in range(len(fl)):
            x[p0 + k] = fl[k]
        for k in range(len(y)):
            if y[k] in new:
                y[k] = new[y[k]]
        if p0 == 0 and len(fl):  # "index 0 of a genome" is the first hit of the order given
            state.head[j] = 0


def set_head_restate(state, head_file):
    for j in range(len(state.x)):
        state.head[j] = 0
        if head_file[j] >= 0 and head_file[j] in state.x[j]:
            state.head[j] = state.x[j].index(head_file[j])


def positions(sh, state):
    """pos_x / pos_y as pga_download gives them: file order, local to the genome"""
    px, py = np.full(sh.N, -9, np.int32), np.full(sh.N, -9, np.int32)
    for j in range(sh.G):
        a = int(sh.goff[j])
        x, y = state.x[j], state.y[j]
        for p in range(len(x)):
            px[a + x[p]] = p
        for k in range(len(y)):
            py[a + x[y[k]]] = k
    return px, py


def derived_restate(sh, state):
    """in X order: file (global file index), gnm, cs, seg, ce, pm, cstie, head; yperm; inv [file -> X]; headpos [G]"""
    N = sh.N
    file, gnm, cs, seg, ce = ([0] * N for _ in range(5))
    yperm, inv, headpos = [0] * N, [0] * N, [0] * sh.G
    for j, g in enumerate(sh.genomes):
        a = int(sh.goff[j])
        gcs, gce, gcid = g.cs.tolist(), g.ce.tolist(), g.cid.tolist()
        headpos[j] = a + state.head[j]
        for p, f in enumerate(state.x[j]):
            file[a + p], gnm[a + p], cs[a + p], ce[a + p], seg[a + p] = a + f, j, gcs[f], gce[f], int(sh.ctg_base[j]) + gcid[f]
            inv[a + f] = a + p
        for k, p in enumerate(state.y[j]):
            yperm[a + k] = a + p
    pm, cstie, head = [0] * N, [False] * N, [False] * N
    for p in range(N):
        first = p == 0 or seg[p - 1] != seg[p]
        pm[p] = ce[p] if first else max(pm[p - 1], ce[p])
        cstie[p] = (p > 0 and seg[p - 1] == seg[p] and cs[p - 1] == cs[p]) or (p + 1 < N and seg[p + 1] == seg[p] and cs[p + 1] == cs[p])
    for j in range(sh.G):
        if sh.goff[j + 1] > sh.goff[j]:
            head[headpos[j]] = True
    return dict(file=file, gnm=gnm, cs=cs, seg=seg, ce=ce, pm=pm, cstie=cstie, head=head, yperm=yperm, inv=inv, headpos=headpos)


# ------------------------------------------------------------------------------------------------
# the shards
# ------------------------------------------------------------------------------------------------
def group(b, g, genes, cs_tie=True, cm_tie=True, rev=None, flat=False):
    """a tie group of hits of the given genes at the genome's next free place: all walkable.  flat: one exon of 10 bp each, 20 bp apart (cm ties only)"""
    a, out = g.at, []
    for i, gene in enumerate(genes):
        r = int(b.rng.integers(0, 2)) if rev is None else rev[i]
        if flat:
            out.append(g.put(gene, r, cm=a + 300 + (0 if cm_tie else i), cs=a + 20 * i, ex=[(0, 10)]))
        else:
            out.append(g.put(gene, r, cm=a + 5 + (0 if cm_tie else i), cs=a + (0 if cs_tie else 20 * i), ex=[(0, 10), (1000 * (i + 1), 1000 * (i + 1) + 100)], tie=cs_tie and i > 0))
    if flat:
        g.at = max(g.at, a + 1300)
    return out


def groups_of(b, g, n, pool, cycle=(2, 3, 1)):
    """exactly n hits on the current contig: tie groups (cs and cm) of the sizes of `cycle` in turn, genes drawn from pool"""
    k = 0
    while n > 0:
        m = min(n, cycle[k % len(cycle)])
        k += 1
        group(b, g, [pool[int(v)] for v in b.rng.permutation(len(pool))[:m]])
        n -= m


def probe(b, g):
    """five hits of genes that stand nowhere else, as tie groups of two and three 3 000 bp apart: the first of the one and the last of the other are four
    ranks apart, every other pair at most three (local_count) -- so WHICH pair pg_n_local finds apart is the cs order's doing; returns the pairs to ask for"""
    U = b.genes.many(5)
    group(b, g, U[:2])
    group(b, g, U[2:])
    return np.array([(x, y) for x in U for y in U if x != y], np.int32)


def _script(sh, tied, small=None, big=None, part1=None, part3=None, **kw):
    """the default orders of the script's slots (order_direct.py); tied: the contigs that hold tie groups; part1 / part3: those of them that "1cs" and "3cm"
    override, where all of them together are more than an eighth of the shard (the partial walk, k_walk_list)"""
    small = tied[:1] if small is None else small
    part1, part3 = tied if part1 is None else part1, tied if part3 is None else part3
    big = [(j, c) for j, g in enumerate(sh.genomes) for c in range(g.n_ctg)] if big is None else big
    on = lambda cs, mode: [(j, c, mode) for j, c in cs]
    sh.ov = {"0": (0, on(tied, "rev")), "1cm": (1, on(tied, "rev")), "1cs": (0, on(part1, "rot")), "3cm": (1, on(part3, "perm")), "3cs": (0, on(tied, "id")),
             "5": [(0, on(small, "perm")), (1, on(big, "rot")), (0, on(small, "rev"))]}
    sh.tied, sh.head1, sh.head2, sh.kind = tied, None, None, "both"
    sh.ov.update(kw)
    return sh


def grid():
    b = ar._Build("grid", 5)
    pool = b.genes.many(70)
    g = b.g[3]
    for n in GRID_SIZES:
        g.ctg()
        groups_of(b, g, n - 5 if n == 252 else n, pool, cycle=(2, 3, 2))
        if n == 252:
            pairs = probe(b, g)
    b.g[4].filler(20)
    sh = b.finish(pairs=pairs)
    pre = lambda k: [(3, c) for c in range(k)]
    burst = []
    for i, T in enumerate(GRID_T):
        k = int(np.flatnonzero(np.cumsum(GRID_SIZES) == T)[0]) + 1
        burst.append((i & 1, [(j, c, ("rev", "rot", "perm")[i % 3]) for j, c in pre(k)]))
    return _script(sh, [(3, 1), (3, 2)], **{"5": burst})


def pm():
    b = ar._Build("pm", 6)
    pool = b.genes.many(70)
    g = b.g[3]
    g.ctg()
    a = g.at  # the contig's first tie group: its second hit ends behind every other hit of the contig
    far = 12_000_000
    g.put(pool[0], 0, cm=a + 5, cs=a, ex=[(0, 10), (1000, 1100)])
    g.put(pool[1], 0, cm=a + 5, cs=a, ex=[(0, 10), (far, far + 100)], tie=True)
    g.at = a + 3000
    groups_of(b, g, 2500 - 2 - 2, pool)
    group(b, g, [pool[2], pool[3]])  # a tie group at the contig's end ...
    end_cs = g.h[-1][6]
    g.ctg(end_cs)                    # ... and the next contig begins at the same cs
    assert g.at == end_cs
    group(b, g, [pool[4], pool[5], pool[6]])
    g.filler(3)
    pairs = probe(b, g)
    g = b.g[4]
    for n in PM_SIZES:
        g.ctg()
        g.filler(2)
        group(b, g, [pool[int(v)] for v in b.rng.permutation(len(pool))[:n]])
        g.filler(1)
    b.g[5].filler(1400)  # N > 4 096 (dev_prims.hpp: SCAN_ONE_MAX): an override of every contig takes the tiled scan, and two tile borders lie in the long contig
    sh = b.finish(pairs=pairs)
    tied = [(3, 0), (3, 1)] + [(4, c) for c in range(len(PM_SIZES))]
    rest = [(j, c, "perm") for j, c in tied[1:]]
    return _script(sh, tied, **{"0": (0, [(3, 0, "ce_desc")] + rest), "1cs": (0, [(3, 0, "ce_asc")] + [(j, c, "rot") for j, c in tied[1:]]),
                                "3cs": (0, [(3, 0, "ce_desc")] + [(j, c, "id") for j, c in tied[1:]])})


def head():
    b = ar._Build("head", 9)
    pool = b.genes.many(20)
    marks = {}
    for j in (3, 5, 6, 7):  # genome 4 stays empty
        g = b.g[j]
        g.ctg()
        a = g.at  # two hits at one start, and over both a longer, better hit of the gene without a segment: SHADOW until pga_flag_vtx filters that one
        h0 = g.put(pool[0], 0, cm=a + 5, cs=a, ex=[(0, 10), (1000, 1100)])
        h1 = g.put(pool[1], 0, cm=a + 5, cs=a, ex=[(0, 10), (2000, 2100)], tie=True)
        g.put(b.dead, 0, sadj=2000, cm=a + 6, cs=a + 1, ce=a + 2301)
        g.filler(3)
        g.ctg()
        group(b, g, [pool[2], pool[3], pool[4]])
        g.filler(2)
        marks[j] = (h0, h1)
    b.g[8].filler(100)
    b.mark = marks
    sh = b.finish()
    tied = [(3, 0), (5, 0), (6, 0), (7, 1)]  # genome 7: the later contig only
    _script(sh, tied, small=[(3, 0)])
    sh.kind = "cs"
    fo = lambda j, k: int(sh.genomes[j].file_of[k])

    def head1(state):  # a hit of the first tie group that is NOT at X position 0
        hf = [-1] * sh.G
        for j in (3, 5, 6, 7):
            hf[j] = state.x[j][1]
            assert hf[j] in (fo(j, marks[j][0]), fo(j, marks[j][1]))
        return hf

    def head2(state, old):  # genome 3: the hit that stands now where the old mark stood; 5: another hit than the one at index 0; 6: none named; 7: the same again
        hf = [-1] * sh.G
        hf[3], hf[5], hf[7] = state.x[3][old[3]], state.x[5][2], state.x[7][old[7]]
        return hf
    sh.head1, sh.head2 = head1, head2
    return sh


def cmties():
    b = ar._Build("cmties", 6)
    A, B, Cg, D, E, S1, S2, Z = b.genes.many(8)
    g = b.g[3]
    g.ctg()
    g.filler(2)
    group(b, g, [A, B], flat=True)             # two and three walkable hits of different genes on one cm
    g.filler(1)
    group(b, g, [Cg, D, E], flat=True)
    g.filler(1)
    group(b, g, [A, A], flat=True)             # two of one gene (no base of their exons in common)
    g.filler(1)
    group(b, g, [B, b.dead, Cg], flat=True)    # the middle hit FLT
    g.filler(1)
    a = g.at                                   # the middle hit SHADOW: Z ends on top of S1, which has the smaller score
    g.put(D, 0, cm=a + 300, cs=a, ex=[(0, 10)])
    g.put(S1, 0, cm=a + 300, cs=a + 20, ex=[(0, 10)])
    g.put(Z, 0, sadj=2000, cm=a + 300, cs=a + 21, ex=[(0, 10)])
    g.put(E, 0, cm=a + 300, cs=a + 40, ex=[(0, 10)])
    g.at = a + 1300
    g.filler(2)
    for d in WALK_D:  # W, d - 1 unwalkable hits, a cm tie pair, d - 1 unwalkable hits, W
        g.ctg()
        g.put(S2, 0)
        for _ in range(d - 1):
            g.put(b.dead)
        group(b, g, [A, B], flat=True)
        for _ in range(d - 1):
            g.put(b.dead)
        g.put(Cg, 1)
    g.ctg()           # a contig that ends in unwalkable hits ...
    group(b, g, [D, E], flat=True)
    for _ in range(5):
        g.put(b.dead)
    g.ctg()           # ... in front of one that begins with them: D / E and A / B are no neighbours
    for _ in range(5):
        g.put(b.dead)
    group(b, g, [A, B], flat=True)
    b.g[4].filler(4100)  # (so that the contigs of the distances are less than an eighth of the shard: the partial walk)
    g = b.g[5]
    g.ctg()
    g.filler(3)
    group(b, g, [B, Cg], flat=True)  # the last walkable hits of the shard
    for _ in range(3):
        g.put(b.dead)
    b.mark = dict(A=A, B=B, C=Cg, D=D, E=E, S1=S1, Z=Z)
    sh = b.finish()
    tied = [(3, c) for c in range(sh.genomes[3].n_ctg)] + [(5, 0), (0, 0)]  # (genome 0's contig: the first walkable hit of the shard; no tie there)
    far = 1 + WALK_D.index(300)
    _script(sh, tied, small=[(3, 1)], part1=[t for t in tied if t[0] == 3 and t[1] != far], part3=[(3, far), (5, 0), (0, 0)])
    sh.kind = "cm"
    return sh


def eighth(plus=0):
    b = ar._Build("eighth", 5)  # (both draw the same shard)
    pool = b.genes.many(70)
    g = b.g[3]
    g.ctg()
    groups_of(b, g, EIGHTH_N // 8 - 5, pool)
    pairs = probe(b, g)
    g.ctg()
    g.filler(1)
    g.ctg()
    g.filler(EIGHTH_N - ar.PRE - EIGHTH_N // 8 - 1)
    b.name = "eighth1" if plus else "eighth"
    sh = b.finish(pairs=pairs)
    assert sh.N == EIGHTH_N
    more = [(3, 1)] if plus else []
    _script(sh, [(3, 0)] + more)
    return sh


def strand():
    b = ar._Build("strand", 5)
    pool = b.genes.many(20)
    SG = b.genes.new()
    g = b.g[3]
    g.ctg()
    g.filler(2)
    a = g.at  # one gene twice at one start and one cm, on opposite strands: both walkable under -S
    g.put(SG, 0, cm=a + 50, cs=a, ce=a + 100)
    g.put(SG, 1, cm=a + 50, cs=a, ce=a + 100, tie=True)
    g.put(pool[0], 0, gap=3000)
    group(b, g, [pool[1], pool[2], pool[3]])
    g.filler(2)
    g.ctg()
    group(b, g, [pool[4], pool[5]])
    g.filler(40)
    b.g[4].filler(300)
    b.mark = dict(SG=SG)
    sh = b.finish(par=(0.5, 1))
    marked = [SG] + pool[:6]
    sh.pairs = np.array([(x, y) for x in marked for y in marked if x != y], np.int32)
    return _script(sh, [(3, 0), (3, 1)])


def pieces():
    b = ar._Build("pieces", 5)
    pool = b.genes.many(20)
    g = b.g[3]
    g.ctg()
    g.filler(2)
    group(b, g, [pool[0], pool[1]])
    g.filler(1)
    base = 2 ** 32
    g.ctg(g.at, piece_base=base)  # the contig goes on in a second piece
    group(b, g, [pool[2], pool[3], pool[4]])
    pairs = probe(b, g)
    g.filler(2)
    g.ctg()
    g.filler(300)
    b.g[4].filler(40)
    sh = b.finish(pairs=pairs)
    return _script(sh, [(3, 0), (3, 1)])


def live():
    b = ar._Build("live", 6)
    pool = b.genes.many(20)
    PZ = b.genes.many(4)  # pseudogenes: their one-exon hits are filtered before the vertex step
    g = b.g[3]
    pz = lambda: g.put(PZ[int(b.rng.integers(0, 4))], 0)
    g.ctg()               # no member
    for _ in range(40):
        pz()
    a = g.at
    g.put(PZ[0], 0, cm=a + 5, cs=a, ex=[(0, 10)])
    g.put(b.dead, 0, cm=a + 5, cs=a, ex=[(0, 10)], tie=True)
    g.ctg()               # one member, in the middle of a tie group of non-members
    for _ in range(30):
        pz()
    a = g.at
    g.put(PZ[1], 0, sadj=500, cm=a + 5, cs=a, ce=a + 10)
    g.put(pool[0], 0, cm=a + 5, cs=a, ex=[(0, 10), (1000, 1100)], tie=True)
    g.put(PZ[2], 0, sadj=500, cm=a + 5, cs=a, ce=a + 10, tie=True)
    g.at = a + 3000
    for _ in range(30):
        pz()
    g.ctg()               # members only
    groups_of(b, g, 55, pool)
    pairs = probe(b, g)
    g.ctg()               # groups with non-members at both ends and inside, members in between
    for k in range(20):
        a = g.at
        genes = [PZ[0], pool[1 + k % 5], b.dead, pool[7 + k % 5], PZ[3]]
        for i, gene in enumerate(genes):
            one = gene in PZ or gene == b.dead
            g.put(gene, 0, sadj=500 if one else 1000, cm=a + 5, cs=a, ex=[(0, 10)] if one else [(0, 10), (1000 * (i + 1), 1000 * (i + 1) + 100)], tie=i > 0)
        g.at = a + 7000
        for _ in range(4):
            pz()
    g = b.g[4]
    g.filler(300)
    for _ in range(1800):
        g.put(PZ[int(b.rng.integers(0, 4))], 0)
    b.g[5].filler(20)
    b.mark = dict(PZ=PZ)
    sh = b.finish(pairs=pairs)
    sh.pj[PZ] = 1
    return _script(sh, [(3, 0), (3, 1), (3, 2), (3, 3)], small=[(3, 1)], part1=[(3, 1), (3, 2), (3, 3)], part3=[(3, 1), (3, 2), (3, 3)])


def marks():
    sh = ar.branch("marks", cm_tie=True)
    tied = [(3, c) for c in range(sh.genomes[3].n_ctg)]
    _script(sh, tied, small=tied[:2], part1=tied[:20], part3=tied[5:35])  # (5 .. 34: contigs of the hub of 63 arcs, weak ones among them)
    sh.kind = "marks"
    return sh


PARTIAL = ("grid", "head", "cmties", "eighth", "live", "marks")  # "1cs" and "3cm" are there for the partial walk (k_walk_list) on these; on eighth1 and pm for the full one
NAMES = ["grid", "pm", "head", "cmties", "eighth", "eighth1", "strand", "pieces", "live", "marks"]


def make(name):
    if name.startswith("eighth"):
        return eighth(int(name[6:] or 0))
    return {"grid": grid, "pm": pm, "head": head, "cmties": cmties, "strand": strand, "pieces": pieces, "live": live, "marks": marks}[name]()


def seed(sh):
    """the generator of a run's drawn orders: the same for every run over a shard"""
    return np.random.default_rng(zlib.crc32((sh.name + "/orders").encode()))
