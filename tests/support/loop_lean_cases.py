"""TEST INFRASTRUCTURE for tests/test_loop_lean_gpu.py: the inputs the lean form of the queued rounds (PANGENE_LOOP_LEAN, pga_host_branch.hpp) is held against.

1. Shards of tests/support/sweep_ref.py's kind (its _Lay / _front / _finish, imported, not edited) at the smallest shapes where the window rule of
   sweep_tile bites -- a hit is `open` when its partners reach beyond its wave's window of 64 own slots and SW_HALO = 32 on either side:
     pile33, pile65, pile97   one pile of that many mutually overlapping hits from the global X position 319 on, the last own hit of a wave (33 = the halo and one:
                              the pile just reaches the window's last slot; 65 = a wave and one; 97 = a window and one)
     straddle                 a pile of 40 over the global X positions 250 .. 289: it straddles the slots 255 | 256, a tile border, and reaches past slot 287 where the window of the wave 192 .. 255 ends
     long                     one hit that spans the starts of the 110 hits behind it (more than the 96 slots a window holds behind its first own slot)
     border                   a pile of 40 from 315 on that ends with its contig: the genome behind it begins in the window of the wave 320 .. 383
   open_hits(sh) restates the kernel's window arithmetic (sweep_ref.reaches does the same for its own tests).
2. PAF sets for whole runs: big_gene(n) -- 64 genomes in one gene order, each with a tandem array of 8 copies of gene XBIG (n = 512), one genome with
   9 (n = 513): the gene keeps its vertex (8 copies a genome, three neighbours), and its stretch of the gene-major index holds n hits; hub_gene() -- a gene
   with more distinct neighbours than the wave kernel's table holds, and a pile of 100 overlapping hits a genome."""
import numpy as np

import sweep_ref as sw

SW_HALO, SW_TILE = sw.SW_HALO, sw.SW_TILE


def _pile_at(m, K):
    """K mutually overlapping one-exon hits (every start lies inside every earlier hit), of proteins of different genes; the first is protein 63's best hit
    (shard() keeps gene 63 a vertex: the hit takes part in the sweep after flag_vtx)"""
    base = m.free()
    for t in range(K):
        m.span(base + 10 * t, 10 * (K - t) + 2000, **(dict(pid=63, sadj=2_000_000) if t == 0 else dict(pid=int(m.rng.integers(0, 63)))))


def shard(name, seed=41):
    rng = np.random.default_rng(seed)
    lays = sw._front(rng, 64, multi=False)
    m = sw._Lay(rng, sw.PRE, 64)
    more = []
    if name.startswith("pile"):
        m.pad_to(319)  # the last own hit of the wave 256 .. 319: its window ends at slot 351, the 33rd hit of a pile that begins here
        _pile_at(m, int(name[4:]))
        m.isolated(150)
    elif name == "straddle":
        m.pad_to(250)
        _pile_at(m, 40)
        m.isolated(150)
    elif name == "long":
        m.pad_to(200)
        base = m.free()
        m.span(base, 1000 * 110 + 50, pid=1)
        for t in range(1, 111):
            m.span(base + 1000 * t, 100, pid=2 * int(rng.integers(0, 32)))
        m.isolated(120)
    elif name == "border":
        m.pad_to(315)
        _pile_at(m, 40)  # the contig (and the genome) ends here ...
        n = sw._Lay(rng, m.pos, 64)  # ... and the next genome begins inside the pile's window
        n.isolated(200)
        more = [n]
    else:
        raise KeyError(name)
    sh = sw._finish("lean_" + name, rng, lays + [m] + more, Q=64)
    sh.g2s_force = {63: True}  # (sweep_direct.drawn: the gene keeps its segment)
    return sh


NAMES = ("pile33", "pile65", "pile97", "straddle", "long", "border")


def open_hits(sh):
    """bool per global X position: sweep_tile's `open` test from the records alone (contig, cs, ce, pm = running maximum of ce inside the contig) -- the
    slot in front of the window of the hit's wave reaches over the hit's start, or the window's last slot starts before the hit ends"""
    d = sw.x_order(sh)
    N, cs, ce, seg, pm = sh.N, d["cs"], d["ce"], d["seg"], d["pm"]
    out = np.zeros(N, bool)
    for h in range(N):
        lo = h // 64 * 64  # the wave's first own hit (tiles are 256 = 4 waves: the same arithmetic)
        w0, w1 = lo - SW_HALO, lo + 64 + SW_HALO - 1
        if w0 >= 0 and seg[w0] == seg[h] and pm[w0] > cs[h]:
            out[h] = True
        if w1 < N and seg[w1] == seg[h] and cs[w1] < ce[h]:
            out[h] = True
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# PAF sets
# ---------------------------------------------------------------------------------------------------------------------------------
def _line(name, L, strand, ctg, ctg_len, cs, ms):
    return "%s\t%d\t0\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t0\tms:i:%d\tcg:Z:%dM\n" % (name, L, L, strand, ctg, ctg_len, cs, cs + 3 * L, 3 * L, 3 * L, ms, L)


def big_gene(n, G=64, n_other=40):
    """(file name, PAF text) per genome: genes A000 .. in one order, one hit each, and the tandem array of XBIG in the middle"""
    assert n in (G * 8, G * 8 + 1)
    for j in range(G):
        lines, at = [], 1000
        copies = 8 + (1 if (n > G * 8 and j == 5) else 0)
        ctg, ctg_len = "g%d#0#chr1" % j, 1000 + 700 * (n_other + copies + 2)
        for k in range(n_other):
            if k == n_other // 2:
                for _ in range(copies):
                    lines.append(_line("XBIG", 200, "+", ctg, ctg_len, at, 900))
                    at += 700
            lines.append(_line("A%03d" % k, 200, "+", ctg, ctg_len, at, 900))
            at += 700
        yield ("g%05d.paf" % j, "".join(lines))


HUB_VARIANT = "-g 100"  # max_degree 100: graph 2's test (twice that) keeps the hub, the tightening tests of the queue's rounds delete it


def hub_gene(G=64, n_flank=140, n_pile=100):
    """(file name, PAF text) per genome: genes F000 .. F139 in one order, one hit each; three copies of gene HUB a genome, each between another pair of
    neighbours (139 places over the 64 genomes: about 278 distinct (orientation, target) keys -- more than the 128 of the wave kernel's table, fewer than
    the 512 of the workgroup kernel's -- in 192 hits, far fewer than the 512 the wave kernel stages); and behind them a pile of 100 mutually overlapping
    hits of genes Q000 .. Q099 (more than a sweep's window of 96 slots: some of them are open wherever the pile falls in the X order)."""
    for j in range(G):
        lines, at = [], 1000
        places = {(3 * j + c) % (n_flank - 1) for c in range(3)}
        ctg, ctg_len = "g%d#0#chr1" % j, 1000 + 700 * (n_flank + 8) + 10 * n_pile + 5000
        for k in range(n_flank):
            lines.append(_line("F%03d" % k, 200, "+", ctg, ctg_len, at, 900))
            at += 700
            if k in places:
                lines.append(_line("HUB", 200, "+", ctg, ctg_len, at, 900))
                at += 700
        at += 1000
        for t in range(n_pile):  # every start inside every earlier hit; the scores differ
            lines.append(_line("Q%03d" % t, 300 + 4 * (n_pile - t), "+", ctg, ctg_len, at + 10 * t, 1500 - t))
        yield ("g%05d.paf" % j, "".join(lines))


def n_lines(files):
    import gzip
    return sum(sum(1 for _ in (gzip.open(f, "rt") if f.endswith(".gz") else open(f))) for f in files)
