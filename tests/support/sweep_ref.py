"""TEST INFRASTRUCTURE: shards for the overlap sweep (k_sweep.hpp: pg_shadow + pg_flt_ov_isoform) and stage A's filters (k_ingest.hpp), what each of
them reaches (`reaches`), and a plain restatement of pg_shadow (`shadow_restate`), for tests/test_sweep.py (oracle against restatement, no GPU) and
tests/support/sweep_direct.py (the HIP backend against the oracle, every route).

Built on stage_a_ref: a genome here (`XGenome`) has EXPLICIT pid, rank, score_ori, score_adj, rev and exon lists.  Every shard is deterministic from
its seed; (pid, rank) is unique inside a genome (rank = the running occurrence number of the protein in a drawn order), as in a parsed PAF.  Tiles
and waves of the sweep are cut over the shard's global X order, so three genomes (37 hits, none, 50 hits) stand in front of the one a shard is about:
its hits start at global X position 87.  A genome under construction (`_Lay`) keeps its hits in X order -- one contig, strictly increasing cs -- and
knows the global X position of the next one; the file order is a drawn permutation.  Every exon list starts at cs and ends at ce, as read.c leaves it
(k_sweep.hpp takes the interval of a one-exon hit for its exon: a list that began behind cs -- stage_a_ref.Genome draws such -- would not be the reference's input).

The shards, by what they reach (asserted in tests/test_sweep.py from `reaches`):
  (halo*, piles, single, odd, head*, sparse: a gene per protein, so that pg_flt_subopt_isoform leaves the sweeps after stage A something to do; the others: four proteins a gene)
  halo, halo1 .. halo513   partners at X distances 31 / 32 / 33 at a wave's edges, a hit with 600 later partners, pairs across 63|64, 255|256, 511|512
  piles                    piles of 20 .. 33 overlapping hits, two and three chunks of the pair list in a 64-span, a pile of 70 (LDS and slow list)
  exons                    lists of 1 .. 300 exons, a window of more than SW_XCAP exons, shared exons, equal ends / starts, a hit in an intron, 2x ~ m
  ratio03, ratio13, ratio_strand   the same under min_ov_ratio 0.3 and 1/3 (x / m below, at, above), and with check_strand
  single                   no multi-exon hit (the STAGE_C = false build), as dense as piles
  odd                      exon lists that are not sorted and disjoint: the literal merge
  round                    isolated pairs whose score_dom has the exact fraction .500 / .501 / .502 before + .499
  filters, filters_neg, filters_big   every branch of pg_flag_pseudo, chains, sub-optimal isoform ties; negative score_adj; score_adj = 2^20
  head, head2              the hit at index 0 of a genome keeps its SHADOW bit (overlap.c:108); head2 names another hit with set_head
  sparse                   multi-exon hits that rarely overlap: the sampled density picks k_sweep_lean"""
from collections import Counter
from fractions import Fraction

import numpy as np

import stage_a_ref as sr

SW_HALO, SW_TILE, SW_WCAP, SW_XCAP, SW_XMAX, SW_LEAN_BELOW = 32, 256, 512, 3584, 255, 1024
F_REV, F_FLT, F_ISO_SUB, F_ISO_OV, F_CHAIN, F_PSEUDO, F_VTX, F_SHADOW, F_REP = 1, 2, 4, 8, 0x10, 0x20, 0x40, 0x80, 0x100
PUBLIC = 0x7ff
PRE = 87  # hits of the three genomes in front


class XGenome(sr.Genome):
    """a genome in file order with everything given; exons: one (k, 2) array per hit, relative to cs"""

    def __init__(self, n_ctg, cid, cs, ce, cm, pid, rank, sori, sadj, rev, exons):
        n = len(cs)
        self.n, self.n_ctg = n, int(n_ctg)
        self.cid, self.cs, self.ce, self.cm, self.pid, self.rank, self.sori, self.sadj = (np.asarray(a, np.int64).reshape(n) for a in (cid, cs, ce, cm, pid, rank, sori, sadj))
        self.rev = np.asarray(rev, np.uint8).reshape(n)
        self.nex = np.array([len(e) for e in exons], np.int64)
        self.offx = np.cumsum(self.nex) - self.nex
        ex = np.concatenate([np.asarray(e, np.int64).reshape(-1, 2) for e in exons]) if n else np.zeros((0, 2), np.int64)
        self.os, self.oe, self.n_exon = ex[:, 0].copy(), ex[:, 1].copy(), len(ex)
        assert n == 0 or ((self.nex >= 1).all() and (self.ce >= self.cs).all() and self.cs.min() >= 0 and self.ce.max() <= sr.I32_MAX)
        # a list starts at cs and ends at ce, as read.c:128-236 leaves it: the kernels take the interval of a one-exon hit for its exon
        assert n == 0 or ((self.os[self.offx] == 0).all() and (np.maximum.reduceat(self.oe, self.offx) == self.ce - self.cs).all())
        key = self.pid << 32 | self.rank
        assert len(np.unique(key)) == n, "(pid, rank) is not unique"


class _Lay:
    """one genome under construction: hits in X order on one contig (strictly increasing cs); pos = global X position of the next hit"""

    def __init__(self, rng, pos0, P):
        self.rng, self.pos0, self.P, self.h, self.maxce, self.mark = rng, pos0, P, [], 0, {}

    @property
    def pos(self):
        return self.pos0 + len(self.h)

    def free(self):
        """a coordinate clear of every hit so far"""
        return self.maxce + 1000

    def put(self, cs, ex, pid=None, sadj=None, sori=None, rev=None):
        r = self.rng
        ex = np.asarray(ex, np.int64).reshape(-1, 2)
        assert not self.h or cs > self.h[-1][0]
        pid = int(r.integers(0, self.P)) if pid is None else pid
        sadj = int(r.integers(1, 1_000_000)) if sadj is None else sadj
        sori = int(r.integers(1, 1000)) if sori is None else sori
        rev = int(r.integers(0, 2)) if rev is None else rev
        ce = int(cs + ex[:, 1].max())
        self.h.append((int(cs), ce, pid, sadj, sori, rev, ex))
        self.maxce = max(self.maxce, ce)
        return self.pos - 1

    def span(self, cs, length, **kw):
        return self.put(cs, [(0, length)], **kw)

    def isolated(self, k, **kw):
        for _ in range(k):  # (of an even protein: those have one-exon hits only, in every shard)
            self.span(self.free(), 100, **dict(dict(pid=2 * int(self.rng.integers(0, self.P // 2))), **kw))

    def pad_to(self, gpos):
        assert gpos >= self.pos
        self.isolated(gpos - self.pos)

    def genome(self, n=None):
        r, h = self.rng, self.h if n is None else self.h[:n]
        n = len(h)
        f = r.permutation(n)  # file index k holds the hit at X position f[k]
        order, seen, rank = r.permutation(n), Counter(), np.zeros(n, np.int64)
        for k in order:
            rank[k] = seen[h[k][2]]
            seen[h[k][2]] += 1
        col = lambda c: np.array([h[k][c] for k in f], np.int64)
        cs, ce = col(0), col(1)
        g = XGenome(1, np.zeros(n, np.int64), cs, ce, (cs + ce) // 2, col(2), rank[f], col(4), col(3), col(5), [h[k][6] for k in f])
        g.file_of = np.argsort(f)  # X position inside the genome -> file index
        return g


def cut_exons(rng, length, k):
    """k sorted, disjoint exons from 0 to length"""
    pts = np.sort(rng.choice(np.arange(1, length), 2 * k - 2, replace=False))
    return np.concatenate([[0], pts, [length]]).reshape(-1, 2)


def odd_list(rng, length):
    """three exons over [0, length), not sorted and disjoint: a zero-length exon touching the one before, or an exon that starts inside the one before"""
    a, b = length // 3, 2 * length // 3
    return [(0, a), (a, a), (b, length)] if rng.random() < 0.5 else [(0, a), (a - 5, b), (b + 7, length)]


def _filler(lay, k, multi=False, overlap=0.3, pid_below=None):
    """k ordinary hits; multi: an odd protein has 3 .. 5 exons in every hit, an even one 1 (pg_flag_pseudo, hit.c:84-92, then marks neither)"""
    r = lay.rng
    for _ in range(k):
        ln = int(r.integers(300, 900))
        cs = lay.free() if not lay.h or r.random() >= overlap else lay.h[-1][0] + 1 + int(r.integers(0, 200))
        pid = int(r.integers(0, lay.P if pid_below is None else pid_below))
        ex = [(0, ln)]
        if multi and pid % 2:
            ex = cut_exons(r, ln, int(r.integers(3, 6)))
        lay.put(cs, ex, pid=pid)


def _pile(lay, K, multi):
    r, base = lay.rng, lay.free()
    for t in range(K):
        ln = 10 * (K - t) + 500 + int(r.integers(0, 50))
        pid = int(r.integers(0, lay.P))
        lay.put(base + 10 * t, cut_exons(r, ln, int(r.integers(3, 6))) if multi and pid % 2 else [(0, ln)], pid=pid)


def _front(rng, P, multi=True):
    a, b = _Lay(rng, 0, P), _Lay(rng, 37, P)
    _filler(a, 37, multi)
    _filler(b, 26, multi)
    c = b.free()
    b.span(c, 1000), b.span(c + 500, 1000)  # the pair across the global X positions 63 | 64
    _filler(b, 22, multi)
    assert a.pos == 37 and b.pos == PRE
    return [a, None, b]


def _finish(name, rng, lays, P=64, Q=16, prot_gid=None, par=(0.5, 0), cut=None):
    gs, left = [], cut
    for lay in lays:
        n = None if lay is None or cut is None else max(0, min(len(lay.h), left))
        gs.append(XGenome(1, *[np.zeros(0, np.int64)] * 9, []) if lay is None else lay.genome(n))
        left = None if cut is None else left - gs[-1].n
    sh = sr.Shard(name, gs, rng, prot_gid=np.arange(P) // (P // Q) if prot_gid is None else prot_gid, gene_pref=rng.random(Q) < 0.3, par=par)
    sh.mark = dict(lays[-1].mark)  # named hits of the last genome: global X position
    return sh


HALO_REACH = {255: 256, 511: 512, 161: 192, 288: 320, 415: 448, 127: 158, 639: 671, 767: 800, 900: 1500}  # hit -> the last hit it overlaps
HALO_N = 1600


def halo(cut=None, seed=21):
    rng = np.random.default_rng(seed)
    lays = _front(rng, 64, multi=False)
    m = _Lay(rng, PRE, 64)
    for g in range(PRE, HALO_N):
        m.span(1000 * g, 1000 * (HALO_REACH[g] - g) + 50 if g in HALO_REACH else 100)
    return _finish("halo" if cut is None else "halo%d" % cut, rng, lays + [m], Q=64, cut=cut)


def _dense(name, multi, seed):
    rng = np.random.default_rng(seed)
    lays = _front(rng, 64, multi)
    m = _Lay(rng, PRE, 64)
    m.pad_to(128), _pile(m, 33, multi), m.pad_to(239)       # one pile of 33 inside the span 128 .. 191: 528 pairs
    _pile(m, 33, multi), _pile(m, 32, multi), _pile(m, 33, multi)  # 239 .. 336: the span 256 .. 319 sees 392 + 496 + 392 pairs
    for _ in range(30):
        _pile(m, int(rng.integers(20, 34)), multi)
        m.isolated(int(rng.integers(0, 4)))
    _pile(m, 70, multi)
    for _ in range(8):
        m.isolated(int(rng.integers(0, 4)))
        _pile(m, int(rng.integers(20, 34)), multi)
    return _finish(name, rng, lays + [m], Q=64)


def piles(seed=22):
    return _dense("piles", True, seed)


def single(seed=23):
    return _dense("single", False, seed)


def _comb(k, step, ln):
    return [(step * i, step * i + ln) for i in range(k)]


X_CASES = [(100, 50), (101, 50), (99, 50)]  # (m, x): the shorter CDS and the intersection of a pair of two genes: 2x = m, m - 1, m + 1
R_CASES = [(1000, 299), (1000, 300), (1000, 301), (999, 332), (999, 333), (999, 334), (1000, 333), (1000, 334), (10, 3)]
LIST_LENGTHS = [1, 2, 8, 9, 255, 256, 300]


def _exons(name, seed, cases, par=(0.5, 0)):
    rng = np.random.default_rng(seed)
    lays = _front(rng, 64)
    m = _Lay(rng, PRE, 64)
    # (the filler keeps to the proteins 0 .. 31; every protein of the constructions has hits of about one length of list: none is a pseudogene of hit.c:84-92)
    _filler(m, 100, True, pid_below=32)
    m.pad_to(300)
    base = m.free()
    for t, k in enumerate(LIST_LENGTHS):  # lists on both sides of the bisection threshold and of SW_XMAX, overlapping one another
        m.put(base + 10 * t, _comb(k, 100, 30), pid=32 + t)
    for at in (20015, 25020, 29025):  # ... and met far inside the long ones
        m.put(base + at, _comb(9, 100, 30), pid=35)
    base = m.free()
    for t in range(16):  # 3840 exons in 16 lists: more than SW_XCAP in one window
        m.put(base + 7 * t, _comb(240, 100, 40), pid=40 + t % 8)
    for E, first in ((np.array([(0, 50), (200, 260), (400, 470), (600, 650)]), 1), (np.array(_comb(12, 150, 60)), 3)):  # isoforms of one gene that share exons exactly
        base = m.free()
        m.put(base, E, pid=47 + first)
        rest = np.delete(E[first:], 1, axis=0)
        m.put(base + int(rest[0, 0]), rest - rest[0, 0], pid=48 + first)
    base = m.free()
    m.put(base, [(0, 30), (100, 130)], pid=52), m.put(base + 5, [(0, 15), (95, 135)], pid=56), m.put(base + 10, [(0, 20), (90, 120)], pid=60)  # equal starts / equal ends
    base = m.free()
    m.put(base, [(0, 30), (100, 130)], pid=53), m.span(base + 40, 50, pid=57)  # a hit inside an intron
    for mm, x in cases:
        base = m.free()
        m.put(base, [(0, 2000), (5000, 7000)], pid=54), m.span(base + 2000 - x, mm, pid=58)
    _filler(m, 60, True, pid_below=32)
    return _finish(name, rng, lays + [m], par=par)


def exons(seed=24):
    return _exons("exons", seed, X_CASES)


def ratio(name, seed=25):
    par = {"ratio03": (0.3, 0), "ratio13": (1 / 3, 0), "ratio_strand": (0.3, 1)}[name]
    return _exons(name, seed, X_CASES + R_CASES, par)


def odd(seed=26):
    rng = np.random.default_rng(seed)
    lays = _front(rng, 64)
    m = _Lay(rng, PRE, 64)
    for _ in range(40):
        base, K = m.free(), int(rng.integers(3, 9))
        for t in range(K):
            ln = 10 * (K - t) + 300 + int(rng.integers(0, 50))
            pid = int(rng.integers(0, 64))
            m.put(base + 10 * t, [(0, ln)] if pid % 2 == 0 else odd_list(rng, ln) if rng.random() < 0.4 else cut_exons(rng, ln, int(rng.integers(3, 6))), pid=pid)
    return _finish("odd", rng, lays + [m], Q=64)


ROUND_OV = (1, 2, 499, 500, 998)
ROUND_FRAC = (500, 501, 502)


def round_cases():
    """(ov, cds_h, cds_w, sori_h, sori_w) with sori_h (1 - ov / cds_h) + sori_w ov / cds_w = an integer + t / 1000 exactly, t in ROUND_FRAC: up to 20 for every (ov, t)"""
    out = []
    sw = np.arange(1, 3000, dtype=np.int64)
    for ov in ROUND_OV:
        for t in ROUND_FRAC:
            got = 0
            for ch in (1000, 2000, 1250, 4000, 5000, 8000):
                for cw in (1000, 2000, 1250, 4000, 5000, 8000):
                    for sh in (1000, 999, 777):
                        if ov >= min(ch, cw) or got >= 20:
                            continue
                        num = (sh * (ch - ov) * cw + sw * ov * ch) % (ch * cw)  # the fraction is num / (ch cw)
                        for s in sw[num * 1000 == t * ch * cw][:2]:
                            out.append((ov, ch, cw, sh, int(s)))
                            got += 1
    return out


def round_(seed=27):
    rng = np.random.default_rng(seed)
    lays = _front(rng, 64)
    m = _Lay(rng, PRE, 64)
    for k, (ov, ch, cw, sh, sw) in enumerate(round_cases()):
        # loser h, then winner w: two proteins of one gene (2 g, 2 g + 1: any overlap makes a pair, and stage A filters h) or, where the overlap is half of the
        # shorter CDS, of two genes (64 ..: a gene each; h stays for the sweeps after stage A).  A protein has one- or two-exon hits, never both.
        base, g = m.free(), int(rng.integers(0, 16))
        p, q = 2 * g + 32 * (k % 2), 2 * g + 32 * (k % 2) + 1
        if 2 * ov >= min(ch, cw) and k % 4 < 2:
            p, q = (96 + g, 112 + int(rng.integers(0, 16))) if k % 2 else (64 + g, 64 + (g + 1 + int(rng.integers(0, 31))) % 32)
        if k % 2:  # a loser of two exons: the exact overlap comes out of a merge
            m.put(base, [(0, 1), (3, ch + 2)], pid=p, sadj=1000, sori=sh)
            m.span(base + ch + 2 - ov, cw, pid=q, sadj=2000, sori=sw)
        else:
            m.span(base, ch, pid=p, sadj=1000, sori=sh)
            m.span(base + ch - ov, cw, pid=q, sadj=2000, sori=sw)
    return _finish("round", rng, lays + [m], P=128, Q=96, prot_gid=np.where(np.arange(128) < 64, np.arange(128) // 2, np.arange(128) - 32))


def filters(name="filters", seed=28):
    """proteins 0 .. 31 (genes 0 .. 7): filler; 32 ..: the constructions.  Four proteins a gene; check_strand = 1."""
    rng = np.random.default_rng(seed)
    P, Q = 96, 24
    top = {"filters": (1 << 20) - 1, "filters_neg": 5000, "filters_big": 1 << 20}[name]
    lays = _front(rng, 32)
    m = _Lay(rng, PRE, 32)
    _filler(m, 300, True, overlap=0.5)
    for rep in range(6):  # pg_flag_pseudo: hits of 1, 2 and 4+ exons of one protein, every mix
        for p, mix in ((32, (1, 4)), (33, (2, 4, 5)), (34, (4, 5)), (35, (1,)), (36, (1, 1, 2)), (37, (1, 2, 4, 8)), (38, (2, 2, 4)), (39, (3, 5, 6))):
            for k in mix:
                m.put(m.free(), cut_exons(rng, 900, k), pid=p)
    for rep in range(5):  # a chain: c loses to x (another gene), x to its isoform y, and x is the only hit of its protein
        base, px = m.free(), 44 + 8 * rep
        m.span(base, 1000, pid=px + 1, sadj=900, rev=0), m.span(base + 500, 1000, pid=px, sadj=800, rev=0), m.span(base + 1100, 600, pid=px + 4, sadj=700, rev=0)
    for rep, g in enumerate((21, 22, 23)):  # candidates of equal score_adj on three proteins of a gene, two of them at one (contig, cs) on opposite strands (no pair under check_strand)
        base, s = m.free(), top if rep == 0 else 5000
        m.span(base, 120, pid=4 * g, sadj=s, rev=0), m.h.append((base, base + 120, 4 * g + 1, s, 500, 1, np.array([(0, 120)])))
        m.span(m.free(), 80, pid=4 * g + 2, sadj=s), m.span(m.free(), 80, pid=4 * g + 3, sadj=s - 1)
    _filler(m, 2100 - len(m.h), True, overlap=0.5)
    if name == "filters_neg":
        for k in rng.choice([k for k, h in enumerate(m.h) if h[2] < 32], 150, replace=False):  # (hits of the filler)
            h = m.h[k]
            m.h[k] = h[:3] + (-int(rng.integers(1, 5000)),) + h[4:]
    return _finish(name, rng, lays + [m], P=P, Q=Q, par=(0.5, 1))


def head(name="head", seed=29):
    """proteins 32 / 36: the genome's first hit loses to the second; 40 / 44: the same elsewhere.  The filler keeps to the proteins 0 .. 31; a gene a protein."""
    rng = np.random.default_rng(seed)
    lays = _front(rng, 32)
    m = _Lay(rng, PRE, 32)
    two = [(0, 300), (400, 700)]
    m.mark["h0"] = m.put(1000, two, pid=32, sadj=100)
    m.mark["w0"] = m.put(1050, two, pid=36, sadj=900)
    m.isolated(1)
    _filler(m, 40, True, pid_below=32)
    base = m.free()
    m.mark["h1"] = m.put(base, two, pid=40, sadj=100)
    m.mark["w1"] = m.put(base + 50, two, pid=44, sadj=900)
    m.isolated(1)
    _filler(m, 40, True, pid_below=32)
    sh = _finish(name, rng, lays + [m], Q=64)
    sh.g2s_force = {32: True, 40: True, 36: False, 44: False}  # gene -> keeps a segment in step 3
    if name == "head2":
        sh.head_file = np.full(sh.G, -1, np.int32)
        sh.head_file[-1] = sh.genomes[-1].file_of[sh.mark["h1"] - PRE]
    return sh


def sparse(seed=30):
    rng = np.random.default_rng(seed)
    lays = _front(rng, 64)
    m = _Lay(rng, PRE, 64)
    _filler(m, 700, True, overlap=0.1)
    return _finish("sparse", rng, lays + [m], Q=64)


HALO_CUTS = (1, 255, 256, 257, 513)
NAMES = ["halo"] + ["halo%d" % n for n in HALO_CUTS] + ["piles", "exons", "ratio03", "ratio13", "ratio_strand", "single", "odd", "round", "filters", "filters_neg", "filters_big",
                                                        "head", "head2", "sparse"]


def make(name):
    if name.startswith("halo"):
        return halo(int(name[4:]) if name[4:] else None)
    if name.startswith("ratio"):
        return ratio(name)
    if name.startswith("filters"):
        return filters(name)
    if name.startswith("head"):
        return head(name)
    return {"piles": piles, "exons": exons, "single": single, "odd": odd, "round": round_, "sparse": sparse}[name]()


# ------------------------------------------------------------------------------------------------
# the restatement of pg_shadow, overlap.c:101-178
# ------------------------------------------------------------------------------------------------
def hash32(key):
    """pg_hash_uint32, pgpriv.h:88-97"""
    m = 0xffffffff
    key = (key + (~(key << 15) & m)) & m
    key ^= key >> 10
    key = (key + (key << 3)) & m
    key ^= key >> 6
    key = (key + (~(key << 11) & m)) & m
    key ^= key >> 16
    return key


def merge(a, ca, b, cb):
    """pg_hit_overlap's two-pointer merge, overlap.c:17-33, literally; a, b: (k, 2) lists relative to ca, cb"""
    ia = ib = inter = 0
    while ia < len(a) and ib < len(b):
        s0, e0, s1, e1 = ca + a[ia][0], ca + a[ia][1], cb + b[ib][0], cb + b[ib][1]
        if s0 < s1:
            if e0 < e1:
                inter += max(0, e0 - s1)
                ia += 1
            else:
                inter += e1 - s1
                ib += 1
        elif e1 < e0:
            inter += max(0, e1 - s0)
            ib += 1
        else:
            inter += e0 - s0
            ia += 1
    return inter


def x_order(sh):
    """the shard in global X order, as plain arrays and lists"""
    w = sr.restate(sh)
    A, B, Cc = w["recA"], w["recB"], w["recC"]
    ex = np.concatenate([np.stack([g.os, g.oe], axis=1) for g in sh.genomes] + [np.zeros((0, 2), np.int64)]).tolist()
    d = dict(cs=A[:, 0], seg=A[:, 1], ce=A[:, 2], pm=A[:, 3], gid=B[:, 1], cds=B[:, 2], pid=B[:, 3], rank=Cc[:, 0], nex=Cc[:, 1], sori=Cc[:, 3], sadj=w["sadj"], pref=w["pref"],
             rev=w["rev"], file=sh.goff[w["gnm"]] + w["fidx"] if sh.N else np.zeros(0, np.int64))
    d["ex"] = [ex[o:o + n] for o, n in zip(Cc[:, 2].tolist(), Cc[:, 1].tolist())]
    return d


def interval_pairs(d, lo, hi):
    """(j, i), j < i inside [lo, hi): one contig and ce[j] > cs[i], found as overlap.c:114-127 finds them"""
    out, i0 = [], lo
    for i in range(lo, hi):
        while i0 < i and not (d["seg"][i0] == d["seg"][i] and d["ce"][i0] > d["cs"][i]):
            i0 += 1
        for j in i0 + np.flatnonzero(d["ce"][i0:i] > d["cs"][i]):
            out.append((int(j), i))
    return out


def shadow_restate(sh, cal_dom_sc):
    """pg_shadow on the fresh shard (nothing filtered, weak_br 0 everywhere): public flag bits, pid_dom, score_dom in FILE order, stats [G, 2] = hits, shadowed"""
    d = x_order(sh)
    N = sh.N
    M = (1 << 64) - 1
    score = [((int(s) & M) << 33 & M) | int(p) << 32 | hash32(int(q)) for s, p, q in zip(d["sadj"], d["pref"], d["pid"])]
    flags, pid_dom, score_dom = d["rev"].copy(), np.full(N, -1, np.int64), np.zeros(N, np.int64)
    best, aid, ovl = [0] * N, [-1] * N, [0] * N
    stats = np.zeros((sh.G, 2), np.int64)
    rank, gid, cds, cs, ce = (d[k].tolist() for k in ("rank", "gid", "cds", "cs", "ce"))
    for g in range(sh.G):
        lo, hi = int(sh.goff[g]), int(sh.goff[g + 1])
        for i in range(lo + 1, hi):  # (overlap.c:108: index 0 of a genome is never reset; nothing is set on a fresh shard)
            flags[i] &= ~F_SHADOW
        for j, i in interval_pairs(d, lo, hi):
            if sh.par.check_strand and (flags[i] ^ flags[j]) & F_REV:
                continue
            x = merge(d["ex"][j], cs[j], d["ex"][i], cs[i]) if cs[j] < ce[i] and ce[j] > cs[i] else 0
            if x == 0:
                continue
            if gid[i] != gid[j] and x / min(cds[i], cds[j]) < sh.par.min_ov_ratio:
                continue
            i_loses = score[i] < score[j] or (score[i] == score[j] and rank[i] > rank[j])
            L, W = (i, j) if i_loses else (j, i)
            flags[L] |= F_SHADOW
            if best[L] < score[W]:  # the best-scoring winner, the first in array order among equals (earlier winners are met first, then later ones)
                best[L], aid[L], ovl[L] = score[W], W, x
        for i in range(lo, hi):
            pid_dom[i] = -1
            if cal_dom_sc:
                score_dom[i] = -1
            if best[i] > 0:
                a = aid[i]
                pid_dom[i] = d["pid"][a]
                if cal_dom_sc:
                    score_dom[i] = int(int(d["sori"][i]) * (1.0 - ovl[i] / cds[i]) + int(d["sori"][a]) * (ovl[i] / cds[a]) + .499)
        stats[g] = hi - lo, int(((flags[lo:hi] & F_SHADOW) != 0).sum())
    out = {}
    for k, v in (("flags", flags), ("pid_dom", pid_dom), ("score_dom", score_dom)):
        out[k] = np.zeros(N, np.int64)
        out[k][d["file"]] = v
    out["stats"] = stats
    return out


# ------------------------------------------------------------------------------------------------
# what a shard reaches, from the shard alone
# ------------------------------------------------------------------------------------------------
def cds_inter_np(a, ca, b, cb):
    """the CDS intersection of two sorted, disjoint exon lists as the sum over all exon pairs (no merge)"""
    a, b = np.asarray(a, np.int64) + ca, np.asarray(b, np.int64) + cb
    return int(np.maximum(0, np.minimum(a[:, None, 1], b[None, :, 1]) - np.maximum(a[:, None, 0], b[None, :, 0])).sum())


def reaches(sh):
    d = x_order(sh)
    N, cs, ce, seg, pm, nex = sh.N, d["cs"], d["ce"], d["seg"], d["pm"], d["nex"]
    irregular = [k for k, e in enumerate(d["ex"]) if any(y < x for x, y in e) or any(e[q + 1][0] < e[q][1] for q in range(len(e) - 1))]
    r = dict(N=N, any_multi=int((nex != 1).any()) if N else 0, n_irregular=len(irregular), nex=set(nex.tolist()), max_genome=max(g.n for g in sh.genomes),
             any_neg=int((d["sadj"] < 0).any()) if N else 0, max_sadj=int(d["sadj"].max()) if N else 0)
    pairs = [p for g in range(sh.G) for p in interval_pairs(d, int(sh.goff[g]), int(sh.goff[g + 1]))]
    r["pairs"] = set(pairs)
    J, I = (np.array([p[k] for p in pairs], np.int64) for k in (0, 1)) if pairs else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    # the hits whose partners reach beyond the window of their wave (sweep_tile: `open`): they go to the slow list
    h = np.arange(N)
    w0, w1 = h // 64 * 64 - SW_HALO, h // 64 * 64 + 64 + SW_HALO - 1
    slow = np.zeros(N, bool)
    ok0, ok1 = w0 >= 0, w1 < N
    slow[ok0] |= (seg[w0[ok0]] == seg[ok0]) & (pm[w0[ok0]] > cs[ok0])
    slow[ok1] |= (seg[w1[ok1]] == seg[ok1]) & (cs[w1[ok1]] < ce[ok1])
    r["n_slow"], r["slow"] = int(slow.sum()), slow
    back, fwd, n_part = np.zeros(N, np.int64), np.zeros(N, np.int64), np.zeros(N, np.int64)
    np.maximum.at(back, I, I - J), np.maximum.at(fwd, J, I - J), np.add.at(n_part, I, 1), np.add.at(n_part, J, 1)
    r["back"], r["fwd"], r["n_partner"] = back, fwd, n_part
    first, last = h % 64 == 0, h % 64 == 63
    r["back_lds"], r["back_slow"] = set(back[first & ~slow].tolist()), set(back[first & slow].tolist())  # the farthest earlier partner of a wave's first hit
    r["fwd_lds"], r["fwd_slow"] = set(fwd[last & ~slow].tolist()), set(fwd[last & slow].tolist())        # the farthest later partner of a wave's last hit
    r["pairs_lds_and_slow"] = int((slow[J] != slow[I]).sum())  # pairs that one member sees in LDS and the other in the slow kernel
    sp = np.zeros(N // 64 + 1, np.int64)
    np.add.at(sp, J // 64, 1), np.add.at(sp, I[I // 64 != J // 64] // 64, 1)
    r["span_pairs"] = sp  # pairs with a member in each aligned span of 64
    near = np.zeros(N, bool)
    near[J], near[I] = True, True
    stage = np.where(near & (nex <= SW_XMAX), nex, 0)
    r["window_exons"] = max([int(stage[max(0, t - SW_HALO):t + SW_TILE + SW_HALO].sum()) for t in range(0, N, SW_TILE)] + [0])
    r["density"] = float(np.where(near, nex, 0).sum()) / max(1, (N + SW_TILE - 1) // SW_TILE)  # (k_list_density's test is a neighbour's, not a partner's: close to this)
    if irregular:
        return r
    # the CDS intersections
    two_x, ratio_cmp, fr, ovs = set(), set(), Counter(), set()
    r["shared_exon_pairs"] = r["eq_end"] = r["eq_start"] = r["intron_pairs"] = r["cds_pairs"] = 0
    r["nex_in_pairs"] = set()
    rmin = sh.par.min_ov_ratio
    for j, i in pairs:
        a, b = d["ex"][j], d["ex"][i]
        x = cds_inter_np(a, int(cs[j]), b, int(cs[i]))
        if x == 0:
            r["intron_pairs"] += 1
            continue
        r["cds_pairs"] += 1
        r["nex_in_pairs"] |= {len(a), len(b)}
        m = int(min(d["cds"][j], d["cds"][i]))
        if d["gid"][j] != d["gid"][i]:
            if abs(2 * x - m) <= 1:
                two_x.add(2 * x - m)
            if abs(Fraction(x, m) - Fraction(rmin)) * m < 1.5:
                ratio_cmp.add("below" if x / m < rmin else "at" if x / m == rmin else "above")
        elif len(a) > 1 or len(b) > 1:
            A = {(int(cs[j]) + s, int(cs[j]) + e) for s, e in a}
            B = {(int(cs[i]) + s, int(cs[i]) + e) for s, e in b}
            r["shared_exon_pairs"] += bool(A & B)
        if len(a) > 1 or len(b) > 1:
            A = [(int(cs[j]) + s, int(cs[j]) + e) for s, e in a]
            B = [(int(cs[i]) + s, int(cs[i]) + e) for s, e in b]
            r["eq_end"] += any(p[1] == q[1] and p[0] != q[0] for p in A for q in B) if len(A) * len(B) <= 64 else 0
            r["eq_start"] += any(p[0] == q[0] and p[1] != q[1] for p in A for q in B) if len(A) * len(B) <= 64 else 0
        if n_part[j] == 1 and n_part[i] == 1 and j >= PRE:  # an isolated pair of the last genome: the loser's score_dom before + .499, exactly
            L, W = (j, i) if d["sadj"][j] < d["sadj"][i] else (i, j)
            v = int(d["sori"][L]) * (1 - Fraction(x, int(d["cds"][L]))) + int(d["sori"][W]) * Fraction(x, int(d["cds"][W]))
            fr[v - v.__floor__()] += 1
            ovs.add(x)
    r["two_x_minus_m"], r["ratio_cmp"], r["fractions"], r["isolated_ov"] = two_x, ratio_cmp, fr, ovs
    # pg_flag_pseudo (hit.c:66-105) per (genome, protein): which branch marks it, and whether the rank promotion moves anything
    ps = Counter()
    for g in sh.genomes:
        for p in np.unique(g.pid):
            ne, rk = g.nex[g.pid == p], g.rank[g.pid == p]
            mx, mn = int(ne.max()), int(ne.min())
            if not (mx > 1 and (mn == 1 or mn * 2 <= mx)):
                ps["none_single" if mx == 1 else "none_multi"] += 1
                continue
            ps["min_is_1" if mn == 1 else "min_half_max"] += 1
            pseudo = (ne == 1) | (ne * 2 <= mx)
            ps["pseudo_1"] += int((ne[pseudo] == 1).sum())
            ps["pseudo_2"] += int((ne[pseudo] == 2).sum())
            ps["pseudo_4+"] += int((ne[pseudo] >= 4).sum())
            r1 = int(rk[~pseudo].min())
            ps["promoted" if r1 > 0 else "first_stays"] += 1
    r["pseudo"] = ps
    # candidates of pg_flt_subopt_isoform (hit.c:107-128) as the file gives them: rank-0 hits of one gene with the same, largest score_adj on several proteins
    ties = ties_cs = 0
    for g in sh.genomes:
        gid = sh.prot_gid[g.pid]
        for q in np.unique(gid[g.rank == 0]):
            k = np.flatnonzero((gid == q) & (g.rank == 0))
            k = k[g.sadj[k] == g.sadj[k].max()]
            if len(set(g.pid[k].tolist())) > 1:
                ties += 1
                ties_cs += len(set(zip(g.cid[k].tolist(), g.cs[k].tolist()))) < len(k)
    r["subopt_ties"], r["subopt_ties_same_cs"] = ties, ties_cs
    return r
