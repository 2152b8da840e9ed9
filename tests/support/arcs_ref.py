"""TEST INFRASTRUCTURE: shards for the vertex step and the host-driven arc and branch rounds (k_vertex.hpp, k_genes.hpp, k_arcs.hpp, k_branch.hpp), and a
plain restatement of pg_gen_arc (graph.c:103-169, `arc_restate`) and of pg_gen_rep_pos + pg_n_local (branch.c:6-46, `rep_restate`), for tests/test_arcs.py
(shards and oracle against the restatement, no GPU) and tests/support/arcs_direct.py (the HIP backend against the oracle, step by step).

Built on stage_a_ref.Shard / sweep_ref.XGenome.  A gene has ONE protein here (pid == gid), every hit has one exon of 100 bp [cm - 50, cm + 50) unless
said otherwise, hits are laid down contig by contig in cm order, so that X order == Y order == the order they were put in; the file order is a
drawn permutation.  A hit is made unwalkable either by FLT -- its gene has no segment, pga_flag_vtx(then_filter = 1) filters it -- or by SHADOW: a hit of
another gene with the larger score_adj overlaps it (`_G.shadowed`: one shadower a hit; `_G.cover`: one long hit whose cm lies at its start shadows k small
ones behind it).  As in sweep_ref three genomes stand in front (37 hits, none, 50 hits): nothing starts on a multiple of 64.  Every shard is deterministic,
seeded by its name, and carries g2s / n_seg, the settings it is to be run with (use_ori, nl_settings, branch parameters, pairs) and marks.

The constants are those of k_genes.hpp (lines 282-284: GA_CAP_WAVE = 128, GA_CAP = 512, GA_WAVE_HITS = 512, GA_BIG_STAGE = 2048; line 337: the halo of 32
hits, so the window of k_gene_arcs_big steps by 2048 - 2 * 32 = 1984; k_walk, line 175: a tile of BLOCK * WK_IPT = 256 or 1024 positions, line 195: the
look-back takes 64 positions a step) and of k_branch.hpp (line 238 / 271: sixteen, 32 or 64 genomes a step of k_n_local).

The shards, by what they reach (asserted in tests/test_arcs.py):
  hits      genes with 1, 2, 511, 512, 513, 1983, 1984, 1985, 3969 hits in the gene-major index over 20 genomes: GA_WAVE_HITS and the window step; groups of
            150 .. 240 hits of one gene in one genome (longer than the halo), one across the window border; a group whose first hit is shadowed, one without
            a walkable hit
  keys      genes with 127, 128, 129, 511, 512 distinct (orientation, target) keys: GA_CAP_WAVE and GA_CAP; every hub hit between two different genes
  hub       one gene with 513 keys: the gene path gives up, the round is repeated on the sort path
  dups      the same arc two, three and four times in one genome: means with fractions .5, .333, .667; a leader that is not the first hit of its group; both
            strands in one group; the tandem A+ A+; the inverted A+ A-; zero and negative scores
  walk, walk1, walk255, walk256, walk257   the nearest walkable predecessor 1, 63, 64, 65, 255, 256, 257, 600 positions in front of a tile of k_walk<1>; a tile
            without a walkable hit; nothing walkable in front of the first walkable hit; a genome change at position 256, a contig change at 512; FLT and
            SHADOW; two walkable neighbours with one (contig, cm); the cuts: the first 1, 255, 256, 257 hits
  local17, local33   gene pairs that are local in exactly one genome j = 0, 15, 16, 17, last of 17 / 33 genomes, by distance or by count, d = +-local_dist,
            +-(local_dist + 1), cc = +-local_count, +-(local_count + 1), on one contig and on two
  branch    vertices with 2, 3, 63, 64, 65 arcs, s1 ratios on both sides of branch_diff, branch_diff_dist and branch_diff_cut, targets local and not; hits that
            mark_hits filters and hits that keep weak_br = 1 under a hit of another gene, so that the second round's sweep decides by weak_br (overlap.c:139)
  vtx64, vtx65, vtx130   genes with 7, 8, 9, 20 dominators around VTX_K = 8 (k_vertex.hpp:65), a gene dominant here and subordinate there, a dominator that is
            not dominant where it dominates; n_genome_global 64, 65, 130 with genome_global not the identity: one, two and three bit words
  reps, reps_full, reps_wide   genomes of 1023, 1024, 1025, 2049 hits around RK_T (k_branch.hpp:23); (contig, cs) tie groups of two and three walkable hits of
            different genes (interval records; pairs whose count test differs across the interval, and pairs whose does not), one of two hits of ONE gene on
            opposite strands (the immediate hazard); groups whose last hit is not walkable, or none; genes absent from the first genomes, from the last, from
            all; a genome that declares 4 096 contigs (RP_FULL); a contig in two virtual pieces cut inside an adjacency (RP_WIDE, graph.c:73)
  round500, round1000   arcs whose sum_s1 / n_genome is 980.498 / .500 / .502 over 500 genomes and 980.500 / .501 / .502 over 1 000, beside arcs of s1 = 1 000;
            use_ori 0 and 1; a walkable hit whose dominator has no segment and whose score_dom >= score_ori; the 32- and 64-lane forms of k_n_local by the
            number of genomes, pairs local in one of the last genomes only"""
import zlib

import numpy as np

import stage_a_ref as sr
import sweep_ref as sw

GA_CAP_WAVE, GA_CAP, GA_WAVE_HITS, GA_BIG_STAGE, GA_HALO = 128, 512, 512, 2048, 32  # k_genes.hpp:282-284, 337
GA_STEP = GA_BIG_STAGE - 2 * GA_HALO                                              # k_genes.hpp:345
WK_TILE, WK_LOOK = 256, 64                                                        # k_genes.hpp:175 (BLOCK x WK_IPT = 1), 195
PRE = 87
F_REV, F_FLT, F_SHADOW, WEAK_SHIFT, WEAK_MASK = 1, 2, 0x80, 9, 0x600
N_FILL = 8


class _Genes:
    def __init__(self):
        self.vtx = []

    def new(self, vertex=True):
        self.vtx.append(bool(vertex))
        return len(self.vtx) - 1

    def many(self, n, vertex=True):
        return [self.new(vertex) for _ in range(n)]


class _G:
    """one genome under construction; hits in the order put = contig-major, cm not decreasing inside a contig"""

    def __init__(self, rng, fill):
        self.rng, self.fill, self.h, self.n_ctg, self.at = rng, fill, [], 0, 0
        self.declare, self.vfirst, self.vbase = 0, [], []  # contigs the block declares (0: those it has); per contig: its first piece and its base

    def ctg(self, at=0, piece_base=None):
        """a new contig; piece_base: it is the next virtual piece of the contig before it, its coordinates are relative to that base"""
        self.n_ctg += 1
        self.at = at
        self.vfirst.append(self.n_ctg - 1 if piece_base is None else self.vfirst[-1])
        self.vbase.append(0 if piece_base is None else piece_base)
        return self.n_ctg - 1

    def put(self, gene, rev=0, sori=None, sadj=1000, cm=None, gap=None, cs=None, ce=None, ex=None, tie=False):
        if self.n_ctg == 0:
            self.ctg()
        c = self.n_ctg - 1
        if gap is not None:
            cm = self.h[-1][1] + gap
        if cm is None:
            cm = self.at + 50
        cs = cm - 50 if cs is None else cs
        ce = (cs + ex[-1][1] if ex is not None else cm + 50) if ce is None else ce
        ex = [(0, ce - cs)] if ex is None else ex  # exons relative to cs, from 0 to ce - cs; tie: the hit starts where the one before it starts
        assert cs >= 0 and (not self.h or self.h[-1][0] != c or (self.h[-1][1] <= cm and (self.h[-1][6] < cs or (tie and self.h[-1][6] == cs))))
        sori = int(self.rng.integers(1, 1000)) if sori is None else sori
        self.h.append((c, int(cm), int(gene), int(rev), int(sori), int(sadj), int(cs), int(ce), ex))
        self.at = max(self.at, ce + 900)
        return len(self.h) - 1

    def filler(self, k=1):
        for _ in range(k):
            self.put(self.fill[int(self.rng.integers(0, len(self.fill)))], int(self.rng.integers(0, 2)))

    def shadowed(self, gene, by, rev=0, sori=None, by_sori=None):
        """a hit of `gene` under a hit of `by` with the larger score_adj: 90 of its 100 bp, so SHADOW in every sweep; two positions"""
        k = self.put(gene, rev, sori)
        cm = self.h[k][1]
        self.put(by, rev, by_sori, sadj=2000, cm=cm + 10)
        return k

    def cover(self, k, small, by):
        """one walkable hit of `by` (cm at its start) and, under it, k hits of `small`, all of them shadowed by it; k + 1 positions"""
        a = self.at
        self.put(by, 0, sadj=2000, cm=a + 1, cs=a, ce=a + 100 + 200 * max(k, 1))
        for i in range(k):
            self.put(small, int(self.rng.integers(0, 2)), cm=a + 150 + 200 * i)
        self.at = a + 100 + 200 * max(k, 1) + 900


class _Build:
    def __init__(self, name, n_genome):
        self.name, self.rng, self.genes, self.mark = name, np.random.default_rng(zlib.crc32(name.encode())), _Genes(), {}
        self.dead = self.genes.new(False)  # a gene without a segment: its hits are FLT from pga_flag_vtx on
        self.fill = self.genes.many(N_FILL)
        self.g = [_G(self.rng, self.fill) for _ in range(n_genome)]
        for k in range(3):  # nothing is walkable in front of the first walkable hit
            self.g[0].put(self.dead)
        self.g[0].filler(34)
        self.g[2].filler(50)
        assert len(self.g[0].h) == 37 and sum(len(g.h) for g in self.g[:3]) == PRE

    def pos(self, j):
        """the global position (X order == Y order) of the next hit of genome j, all genomes in front being complete"""
        return sum(len(g.h) for g in self.g[:j + 1])

    def finish(self, cut=None, par=(0.5, 0), **kw):
        rng, gs, left = self.rng, [], cut
        Q = len(self.genes.vtx)
        for g in self.g:
            h = g.h if left is None else g.h[:max(0, left)]
            left = None if left is None else left - len(h)
            n = len(h)
            f = rng.permutation(n)
            col = lambda c: np.array([h[k][c] for k in f], np.int64)
            pid = col(2)
            rank = np.zeros(n, np.int64)
            seen = {}
            for k in range(n):  # the running occurrence number of the protein, in file order: (pid, rank) is unique, as in a parsed PAF
                rank[k] = seen.get(int(pid[k]), 0)
                seen[int(pid[k])] = int(rank[k]) + 1
            x = sw.XGenome(max(1, g.n_ctg, g.declare), col(0), col(6), col(7), col(1), pid, rank, col(4), col(5), col(3), [h[k][8] for k in f])
            x.file_of = np.argsort(f)
            gs.append(x)
        sh = sr.Shard(self.name, gs, rng, prot_gid=np.arange(Q), gene_pref=np.zeros(Q, np.uint8), par=par)
        # virtual contigs (pga_genome_block_t::vfirst / vbase): per contig segment of the shard, the segment of its contig's first piece and its base
        sh.seg_first, sh.seg_base, sh._v = np.arange(int(sh.ctg_base[-1]), dtype=np.int64), np.zeros(int(sh.ctg_base[-1]), np.int64), []
        for k, g in enumerate(self.g):
            if any(g.vbase):
                vf, vb = np.zeros(gs[k].n_ctg, np.int32), np.zeros(gs[k].n_ctg, np.int64)
                vf[:] = np.arange(gs[k].n_ctg)
                vf[:g.n_ctg], vb[:g.n_ctg] = g.vfirst, g.vbase
                sh._v.append((vf, vb))
                sh._blocks[k].vfirst, sh._blocks[k].vbase = vf.ctypes.data, vb.ctypes.data
                sh.seg_first[sh.ctg_base[k]:sh.ctg_base[k + 1]], sh.seg_base[sh.ctg_base[k]:sh.ctg_base[k + 1]] = sh.ctg_base[k] + vf, vb
        keep = np.array(self.genes.vtx)
        sh.g2s, sh.n_seg = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32), int(keep.sum())
        sh.seg_gid = np.flatnonzero(keep).astype(np.int32)
        sh.mark, sh.use_ori, sh.nl_settings, sh.pairs = self.mark, 0, [(2000, 3, 0)], np.zeros((0, 2), np.int32)
        sh.branch = dict(diff=0.02, dist=0.05, cut=0.5, local_dist=2000, local_count=3, frag_mode=0)
        sh.rep, sh.pj = np.ones(sh.P, np.uint8), np.zeros(sh.P, np.uint8)
        for k, v in kw.items():
            setattr(sh, k, v)
        if len(sh.pairs) == 0:  # every ordered pair of the first genes with a segment
            g = sh.seg_gid[:24]
            sh.pairs = np.array([(a, b) for a in g for b in g if a != b], np.int32).reshape(-1, 2)
        return sh


# ------------------------------------------------------------------------------------------------
HIT_COUNTS = (1, 2, 511, 512, 513, 1983, 1984, 1985, 3969)


def hits():
    b = _Build("hits", 20)
    hubs = {}
    for n in HIT_COUNTS:
        H, Z = b.genes.new(), b.genes.new()
        nb = b.genes.many(max(4, -(-n // 250)))
        hubs[n] = H
        big = min(n, 150) if n >= 100 else 0  # the multi-copy group of the first genome; the rest evenly over the others (150 .. 240 each for the large genes)
        share = [big] + [(n - big) // 16 + (k < (n - big) % 16) for k in range(16)]
        for j, m in enumerate(share):
            g = b.g[3 + j]
            if m == 0:
                continue
            g.ctg()
            for i in range(m):
                g.put(nb[int(b.rng.integers(0, len(nb)))], int(b.rng.integers(0, 2)))
                # genome 4: the group's first hit is not walkable; genome 5: none of its hits is
                if n >= 511 and (j == 2 or (j == 1 and i == 0)):
                    g.shadowed(H, Z, int(b.rng.integers(0, 2)))
                else:
                    g.put(H, int(b.rng.integers(0, 2)))
            g.put(nb[0], 0)
    b.mark = hubs
    return b.finish()


def _keyed(name, counts):
    """hub genes with exactly K distinct keys: ceil(K / 2) hits, all '+', each on a contig of its own between two different neighbour genes; the hit's next
    neighbour is a target of the hub's '+' vertex nobody else has, its previous neighbour (flipped) one of the '-' vertex"""
    b = _Build(name, 13)
    nbs = b.genes.many(130)
    vtx = [(m, r) for m in nbs for r in (0, 1)]
    hubs, at = {}, 0
    for K in counts:
        H = b.genes.new()
        hubs[K] = H
        k1, k2 = -(-K // 2), K // 2
        for i in range(k1):
            g = b.g[3 + at % 10]
            at += 1
            nx, pv = vtx[i], vtx[(i + 7) % k2]
            assert nx[0] != pv[0]
            g.ctg()
            g.put(pv[0], pv[1]), g.put(H, 0), g.put(nx[0], nx[1])
    b.mark = hubs
    return b.finish(use_ori=1)


def keys():
    return _keyed("keys", (127, 128, 129, 511, 512))


def hub():
    return _keyed("hub", (513,))


def dups():
    b = _Build("dups", 5)
    G = b.genes
    P, A, B, C, D, E, F, Gg, T, U, Z, W = G.many(12)
    g = b.g[3]

    def run(seq, gaps):
        g.ctg()
        for k, (gene, rev, s) in enumerate(seq):
            g.put(gene, rev, s, gap=gaps[k - 1] if k else None)
    run([(P, 0, 5), (A, 0, 7), (B, 0, 9)], [1000, 1000])  # the first hit of A's group has other neighbours: the leader of A+ -> C+ is the second
    run([(A, 0, 10), (C, 0, 30)], [100])
    run([(A, 0, 20), (C, 0, 25)], [101])                  # A+ -> C+ twice: (100 + 101) / 2 = 100.5 -> 100 with + .499
    run([(A, 1, 11), (C, 0, 12)], [177])                   # both strands of A in one group
    for gap in (110, 110, 111):
        run([(D, 0, 40), (E, 1, 50)], [gap])              # three times: 110.333 -> 110
    for gap in (110, 111, 111):
        run([(F, 1, 40), (Gg, 0, 50)], [gap])             # 110.667 -> 111
    run([(T, 0, 60), (T, 0, 61), (T, 0, 62)], [500, 501])  # the tandem, twice: T+ -> T+ and T- -> T- with 500.5
    run([(U, 0, 70), (U, 1, 71)], [300])                  # the inverted self-adjacency: the forward half-arc of the first hit and the backward one of the
    run([(U, 0, 72), (U, 1, 73)], [301])                  # second are ONE arc U+ -> U-: four items in one genome, 300.5 -> 300
    run([(Z, 0, 0), (W, 0, -5)], [140])                    # zero and negative scores: the running maxima start at 0
    run([(Z, 0, -3), (W, 0, 0)], [141])
    g = b.g[4]
    run([(A, 0, 13), (C, 0, 14)], [200])
    run([(D, 0, 1), (E, 1, 2)], [112])
    run([(U, 0, 5), (U, 1, 6)], [299])
    run([(Z, 0, -1), (W, 0, -1)], [139])
    b.mark = dict(A=A, C=C, D=D, E=E, F=F, G=Gg, T=T, U=U, Z=Z, W=W)
    return b.finish()


WALK_D = ((768, 1, "shadow"), (1024, 63, "shadow"), (1280, 64, "flt"), (1536, 65, "shadow"), (1792, 255, "flt"), (2304, 256, "shadow"), (2816, 257, "shadow"), (3584, 600, "shadow"))
WALK_CUTS = (1, 255, 256, 257)


def walk(cut=None):
    b = _Build("walk", 5)  # (every cut draws what the whole shard draws)
    S, L = b.genes.new(), b.genes.new()
    g = b.g[3]
    g.filler(100)
    k = g.put(b.fill[0], 0)
    g.put(b.fill[1], 1, cm=g.h[k][1], cs=g.h[k][7] + 100, ce=g.h[k][7] + 200)  # two walkable neighbours with one (contig, cm): hazard H2a
    g.filler(WK_TILE - PRE - len(g.h))
    assert b.pos(3) == WK_TILE  # the genome changes at position 256
    g = b.g[4]
    g.filler(WK_TILE)
    g.ctg()
    assert b.pos(4) == 2 * WK_TILE  # a contig changes at position 512
    for t0, d, how in WALK_D:
        g.filler(t0 - d - b.pos(4))
        if how == "shadow":
            g.cover(d - 1, S, L)
        else:
            g.filler(1)
            for _ in range(d - 1):
                g.put(b.dead)
        assert b.pos(4) == t0
    g.filler(90)
    b.name = "walk" if cut is None else "walk%d" % cut
    return b.finish(cut=cut)


LOCAL_CASES = ((0, 1), (1, 0), (1, 1), (0, 0))  # (d - local_dist, cc - local_count): local by distance only, by count only, not at all, by both


def local(n_genome):
    b = _Build("local%d" % n_genome, n_genome)
    ld, lc = 2000, 3
    js = sorted({0, 15, 16, n_genome - 1} | ({17} if n_genome > 18 else set()))
    marks = []
    for j in range(3, n_genome):
        b.g[j].filler(5)
    for j in js:
        g = b.g[j]
        for two in (0, 1):
            for dd, dc in LOCAL_CASES:
                a, c = b.genes.new(), b.genes.new()
                d, cc = ld + dd, lc + dc
                g.ctg(10000)
                g.filler(2)
                ka = g.put(a, int(b.rng.integers(0, 2)))
                cm_a = g.h[ka][1]
                if two:
                    g.ctg(cm_a + d - 150 * cc)
                for i in range(cc - 1):  # cc - 1 walkable hits in between: the ranks differ by cc
                    g.put(b.fill[i % N_FILL], 0, cm=cm_a + d - 150 * (cc - 1 - i))
                g.put(c, int(b.rng.integers(0, 2)), cm=cm_a + d)
                g.filler(1)
                marks.append((j, two, dd, dc, a, c))
    genes = [m[4] for m in marks] + [m[5] for m in marks]
    pairs = np.array([(x, y) for x in genes for y in genes if x != y], np.int32)
    b.mark = marks
    return b.finish(pairs=pairs, nl_settings=[(ld, lc, 0), (ld, lc, 1)])


BRANCH_DEG = (2, 3, 63, 64, 65)
BRANCH_S = (1000, 1000, 981, 980, 979, 951, 950, 949, 501, 500, 499, 100)  # the hub hit's score = the arc's s1: 1 - s1 / 1000 around .02, .05 and .5


def branch(name="branch", cm_tie=False):
    """cm_tie (order_ref's `marks`; it draws what `branch` draws): the hub's hit and its target stand on one cm, 1 000 bp apart, wherever no third hit lies between them"""
    b = _Build("branch", 6)
    b.name = name
    ga, gb = b.g[3], b.g[4]
    Zg = b.genes.new()
    hubs = {}
    for n in BRANCH_DEG:
        V = b.genes.new()
        T = b.genes.many(n)
        hubs[n] = (V, T)
        for k in range(n):
            s = BRANCH_S[k % len(BRANCH_S)] if n > 3 else (1000, 960, 990)[k]
            ga.ctg()
            ga.filler(1)
            if k % 12 in (3, 4) and n > 3:  # a hub hit that will carry weak_br = 1, over a weaker hit of another gene: the second round's sweep shadows the HUB hit
                kk = ga.put(V, 0, s, sadj=2000)
                ga.put(Zg, 0, sadj=1000, cm=ga.h[kk][1] + 10)
                kk = -1
            else:
                kk = ga.put(V, 0, s)
            if cm_tie and kk >= 0:
                ga.put(T[k], int(b.rng.integers(0, 2)), cm=ga.h[kk][1], cs=ga.at, ce=ga.at + 100)
            else:
                ga.put(T[k], int(b.rng.integers(0, 2)))
        # a second genome in which every third target stands next to the best-scoring one: local there, nowhere comparable otherwise
        gb.ctg()
        gb.put(T[0], 0)
        for k in range(2, n, 3):
            gb.put(T[k], 0, gap=150)
    b.mark = hubs
    return b.finish()


VTX_K = 8  # k_vertex.hpp:65: the dominator slots of a gene; a gene with more spills single-genome records
VTX_DOMS = (7, 8, 9, 20)
VTX_GLOBAL = (64, 65, 130)


def vtx(n_global):
    """genes subordinate to 7, 8, 9 and 20 different dominators, one a genome (vertex.c:28-51 keeps one dominator a gene and genome); the first of them is
    dominant itself in one more genome; a gene with three dominators of which one is shadowed in turn, so never dominant THERE, though it is elsewhere: that
    record must not appear.  The 24 genomes stand at drawn places among n_global, the last place and both sides of every word border among them."""
    b = _Build("vtx%d" % n_global, 24)
    subs = {}
    for k in VTX_DOMS:
        S = b.genes.new()
        D = b.genes.many(k)
        subs[k] = (S, D)
        for i in range(k):
            g = b.g[3 + i]
            g.filler(1)
            g.shadowed(S, D[i])
        if k == VTX_DOMS[0]:
            b.g[3 + k + 2].put(S, 0)
    S, D, E = b.genes.new(), b.genes.many(3), b.genes.new()
    for i in range(3):
        g = b.g[5 + i]
        g.filler(1)
        a = g.at
        g.put(S, 0, sadj=1000, cm=a + 1, cs=a, ce=a + 100)
        g.put(D[i], 0, sadj=2000, cm=a + 41, cs=a + 40, ce=a + 240)      # 60 of S's 100 bp
        if i == 1:
            g.put(E, 0, sadj=3000, cm=a + 131, cs=a + 130, ce=a + 330)   # 110 of D's 200 bp, nothing of S
    b.g[20].put(D[1], 0)
    subs["never"] = (S, D, E)
    b.mark = subs
    sh = b.finish()
    forced = list(dict.fromkeys(v for v in (n_global - 1, 0, 63, 64, 127, 128) if v < n_global))
    rest = [int(v) for v in b.rng.permutation(n_global) if v not in forced]
    gg = np.array(forced + rest[:sh.G - len(forced)], np.int64)
    sh._gg = np.ascontiguousarray(b.rng.permutation(gg), np.int32)  # not the identity, not sorted
    sh.c.genome_global, sh.c.n_genome_global = sh._gg.ctypes.data, n_global
    return sh


RK_T = 1024  # k_branch.hpp:23: the hits k_rank_genome ranks a step
REPS_SIZES = (RK_T - 1, RK_T, RK_T + 1, 2 * RK_T + 1)
WIDE_BASE = 2 ** 32  # what the second virtual piece of reps_wide's cut contig subtracted from its coordinates


def reps(kind=""):
    """for k_rank_genome, k_tie_bounds, k_rep_fill and the hazards of k_n_local; check_strand = 1, so that hits on opposite strands may share a start.
    kind "full": one genome declares 4 096 contigs (RP_FULL); "wide": one contig comes as two virtual pieces, cut inside an adjacency (RP_WIDE)"""
    b = _Build("reps" + ("_" + kind if kind else ""), 7)
    G = b.genes
    T2, T3, SG, AFT = G.many(2), G.many(3), G.new(), G.many(8)
    K_last, K_none, only_first, only_last, nowhere, M1 = G.many(6)
    W1, W2 = G.many(2)
    Zs = G.new()
    g = b.g[3]
    g.ctg()
    g.filler(3)
    g.put(M1, 0)
    a = g.at  # two walkable hits of different genes at one (contig, cs), on opposite strands: each carries an interval of one rank
    g.put(T2[0], 0, cm=a + 50, cs=a, ce=a + 100)
    g.put(T2[1], 1, cm=a + 60, cs=a, ce=a + 100, tie=True)
    for k in range(8):  # behind them at the ranks + 1 .. + 8 (or + 2 .. + 9) and 3 000 bp apart: the count test decides, for some of them differently across the interval
        g.put(AFT[k], 0, gap=3000)
    a = g.at  # three: two of them on one strand, with two exons each that share 10 bp only
    g.put(T3[0], 0, cm=a + 5, cs=a, ex=[(0, 10), (1000, 1100)])
    g.put(T3[1], 1, cm=a + 6, cs=a, ce=a + 100, tie=True)
    g.put(T3[2], 0, cm=a + 7, cs=a, ex=[(0, 10), (2000, 2100)], tie=True)
    g.filler(2)
    a = g.at  # one gene twice at one start, on opposite strands: which of them is the representative depends on the tie order -- the immediate hazard
    g.put(SG, 0, cm=a + 50, cs=a, ce=a + 100)
    g.put(SG, 1, cm=a + 60, cs=a, ce=a + 100, tie=True)
    g.filler(2)
    g.put(K_last, 0), g.filler(1), g.shadowed(K_last, Zs)    # a group whose last hit is not walkable
    g.shadowed(K_none, Zs), g.filler(1), g.shadowed(K_none, Zs)  # ... and one without a walkable hit
    g.put(only_first, 0)
    if kind == "wide":
        g.ctg(4950)
        g.put(W1, 0, cm=5000)
        g.ctg(5900, piece_base=WIDE_BASE)  # the cut lies between W1 and the next hit: the distance of that adjacency is 2^32 + 1 000, 1 000 as an int32_t (graph.c:73)
        for cm in (6000, 6150, 6300):
            g.put(b.fill[0], 0, cm=cm)
        g.put(W2, 0, cm=6500)              # cm2 - cm1 = 2^32 + 1 500 and four ranks: not local; 1 500 by the low words alone
        g.ctg()
    g.filler(REPS_SIZES[0] - len(g.h))
    for j, n in ((4, REPS_SIZES[1]), (5, REPS_SIZES[2])):  # a representative at the last rank, on either side of the step
        b.g[j].filler(n - 1)
        b.g[j].put(M1, 0)
    g = b.g[6]
    g.filler(REPS_SIZES[3] - 6)
    g.put(K_last, 0), g.shadowed(K_last, Zs), g.put(only_last, 0), g.filler(1), g.put(M1, 0)
    if kind == "full":
        g.declare = 4096
    assert [len(x.h) for x in b.g[3:]] == list(REPS_SIZES)
    marked = T2 + T3 + [SG] + AFT + [K_last, K_none, only_first, only_last, nowhere, M1] + ([W1, W2] if kind == "wide" else [])
    b.mark = dict(T2=T2, T3=T3, SG=SG, AFT=AFT, K_last=K_last, K_none=K_none, only_first=only_first, only_last=only_last, nowhere=nowhere, M1=M1, W=(W1, W2), Zs=Zs)
    pairs = np.array([(x, y) for x in marked for y in marked if x != y], np.int32)
    return b.finish(par=(0.5, 1), pairs=pairs, nl_settings=[(2000, 3, 0), (2000, 3, 1)])


ROUND_N = (500, 1000)
ROUND_MORE = {500: (250, 251, 249), 1000: (501, 500, 502)}  # genomes in which A, B, C score 981 instead of 980: the means are 980.500 / .502 / .498 and 980.501 / .500 / .502


def round_(n):
    """n genomes of three hits A+ B+ C+ whose scores sum to 980 n + ROUND_MORE: the s1 of A+ -> B+, of B+ -> C+ (and B- -> A-) and of C- -> B- are the means of the
    scores of A, B, C (graph.c:171) -- 980 or 981 by the rounding, and 980 is weak beside a second arc of s1 = 1 000 (1 - 980 / 1000 > branch_diff) where 981 is
    not.  The second arcs, and a hit whose stage-A dominator has no segment (graph.c:82-85 then takes its score_dom), stand in four genomes at the END."""
    b = _Build("round%d" % n, 3 + n + 4)
    A, B, C, X1, X2, X3, Hd = b.genes.many(7)
    more = ROUND_MORE[n]
    for k in range(n):
        g = b.g[3 + k]
        for gene, m in zip((A, B, C), more):
            g.put(gene, 0, 981 if k < m else 980)
    e = b.g[3 + n:]
    e[0].filler(1), e[0].put(A, 0, 1000), e[0].put(X1, 0)
    e[1].filler(1), e[1].put(B, 0, 1000), e[1].put(X2, 0)
    e[2].put(X3, 0), e[2].put(C, 0, 1000), e[2].filler(1)
    e[3].filler(1), e[3].shadowed(Hd, b.dead, 0, 300, 5000), e[3].filler(1)
    b.mark = dict(A=A, B=B, C=C, X=(X1, X2, X3), Hd=Hd)
    return b.finish(use_ori=0 if n == 500 else 1)


NAMES = (["hits", "keys", "hub", "dups", "walk"] + ["walk%d" % c for c in WALK_CUTS] + ["local17", "local33", "branch"] + ["vtx%d" % n for n in VTX_GLOBAL]
         + ["reps", "reps_full", "reps_wide"] + ["round%d" % n for n in ROUND_N])


def make(name):
    if name.startswith("walk"):
        return walk(int(name[4:]) if name[4:] else None)
    if name.startswith("local"):
        return local(int(name[5:]))
    if name.startswith("vtx"):
        return vtx(int(name[3:]))
    if name.startswith("reps"):
        return reps(name[5:])
    if name.startswith("round"):
        return round_(int(name[5:]))
    return {"hits": hits, "keys": keys, "hub": hub, "dups": dups, "branch": branch}[name]()


# ------------------------------------------------------------------------------------------------
# plain restatements, from the reference's source lines; loops and Python integers
# ------------------------------------------------------------------------------------------------
def y_order(sh):
    """the shard's hits in Y (cm) order and in X (cs) order as plain lists; file = index into what pga_download gives"""
    w = sr.restate(sh)
    A, B, Cc = w["recA"], w["recB"], w["recC"]
    fx = (sh.goff[w["gnm"]] + w["fidx"]) if sh.N else np.zeros(0, np.int64)
    cm = np.zeros(sh.N, np.int64)
    for k, g in enumerate(sh.genomes):
        cm[sh.goff[k]:sh.goff[k + 1]] = g.cm
    seg = A[:, 1]  # (a piece of a virtual contig: the contig is its first piece's, the coordinate the piece's plus its base, as the reference has them)
    return dict(yperm=w["yperm"].tolist(), file=fx.tolist(), seg=sh.seg_first[seg].tolist(), gid=B[:, 1].tolist(), sori=Cc[:, 3].tolist(), gnm=w["gnm"].tolist(),
                cm=(cm[fx] + sh.seg_base[seg]).tolist() if sh.N else [])


def get_score(ori, score_ori, score_dom, pid_dom0, g2s):
    """pg_get_score, graph.c:82-85 (pid == gid in these shards)"""
    return score_ori if (ori or score_ori > score_dom or pid_dom0 < 0 or g2s[pid_dom0] >= 0) else score_dom


def arc_restate(sh, st, use_ori):
    """pg_gen_arc, graph.c:103-169, on the flags / score_dom / pid_dom0 (file order) that the round's own pg_shadow left: (seg_cnt[2S], {x: (n_genome, tot_cnt,
    sum_dist, sum_s1, sum_s2)}) -- the sums of 153-169 without the roundings of 170-172, as pga_arc_part_t keeps them"""
    d, S, g2s = y_order(sh), sh.n_seg, sh.g2s.tolist()
    flags, sdom, pd0 = st["flags"].tolist(), st["score_dom"].tolist(), st["pid_dom0"].tolist()
    n_genome, tot_cnt, arc = [0] * S, [0] * S, []
    for j in range(sh.G):
        v, vpos, vcid, si, seg_cnt, arc1 = -1, -1, -1, -1, [0] * S, []
        for y in range(int(sh.goff[j]), int(sh.goff[j + 1])):
            a = d["yperm"][y]
            f = d["file"][a]
            if flags[f] & (F_FLT | F_SHADOW):
                continue
            sid = g2s[d["gid"][a]]
            assert sid >= 0
            w = sid << 1 | (flags[f] & F_REV)
            seg_cnt[sid] += 1
            if d["seg"][a] != vcid:
                v, vpos = -1, -1
            sc = get_score(use_ori, d["sori"][a], sdom[f], pd0[f], g2s)
            if v != -1:
                dist = (d["cm"][a] - vpos + 2 ** 31) % 2 ** 32 - 2 ** 31  # graph.c:73: pg_tmparc_t::dist is an int32_t
                arc1.append((v << 32 | w, dist, si, sc))
                arc1.append(((w ^ 1) << 32 | (v ^ 1), dist, sc, si))
            v, vpos, vcid, si = w, d["cm"][a], d["seg"][a], sc
        for i in range(S):
            n_genome[i] += seg_cnt[i] > 0
            tot_cnt[i] += seg_cnt[i]
        grp = {}
        for x, dist, s1, s2 in arc1:
            grp.setdefault(x, []).append((dist, s1, s2))
        for x, it in grp.items():
            dist, max_s1, max_s2 = 0, 0, 0
            for dd, s1, s2 in it:
                dist += dd
                max_s1, max_s2 = max(max_s1, s1), max(max_s2, s2)
            arc.append((x, len(it), int(float(dist) / len(it) + .499), max_s1, max_s2))  # graph.c:141
    out = {}
    for x, n, dist, s1, s2 in arc:
        o = out.setdefault(x, [0, 0, 0, 0, 0])
        o[0] += 1
        o[1] += n
        o[2] += dist * n
        o[3] += s1
        o[4] += s2
    return n_genome + tot_cnt, {x: tuple(v) for x, v in out.items()}


def final_s1(sum_s1, n_genome):
    return int(float(sum_s1) / n_genome + .499)  # graph.c:171


def rep_restate(sh, st, pairs, local_dist, local_count, frag_mode):
    """pg_gen_rep_pos + pg_n_local, branch.c:6-46, on the flags the last arc round left: n_local per pair"""
    w = sr.restate(sh)
    fx = (sh.goff[w["gnm"]] + w["fidx"]).tolist() if sh.N else []
    gid, seg = w["recB"][:, 1].tolist(), sh.seg_first[w["recA"][:, 1]].tolist()
    cm = np.concatenate([g.cm for g in sh.genomes] + [np.zeros(0, np.int64)])
    if sh.N:
        cm[fx] += sh.seg_base[w["recA"][:, 1]]
    cm = cm.tolist()
    flags = st["flags"].tolist()
    pos = []
    for j in range(sh.G):
        aj, r = {}, 0
        for x in range(int(sh.goff[j]), int(sh.goff[j + 1])):  # array order = cs order
            f = fx[x]
            if not flags[f] & (F_FLT | F_SHADOW):
                aj[gid[x]] = (seg[x], r, cm[f])
                r += 1
        pos.append(aj)
    out = []
    for g1, g2 in np.asarray(pairs).tolist():
        n = 0
        for aj in pos:
            if g1 not in aj or g2 not in aj:
                continue
            a1, a2 = aj[g1], aj[g2]
            if not frag_mode and a1[0] != a2[0]:
                continue
            d, c = a1[2] - a2[2], a1[1] - a2[1]
            if -local_dist <= d <= local_dist or -local_count <= c <= local_count:
                n += 1
        out.append(n)
    return out


def lookbacks(walkable, tile):
    """for every tile of the walk over a list with these walkable marks: how far in front of the tile's first position the nearest walkable one lies (0: none)"""
    out, last = {}, -1
    for i, ok in enumerate(walkable):
        if i % tile == 0 and i:
            out[i] = i - last if last >= 0 else 0
        if ok:
            last = i
    return out
