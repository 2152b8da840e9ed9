"""TEST INFRASTRUCTURE: shards for stage A (pga_create + pga_begin) and a plain numpy restatement of what pga_begin leaves, for
tests/test_stage_a.py (the restatement against the plain-C oracle, no GPU) and tests/support/stage_a_direct.py (every route of the
HIP backend against the restatement: the per-genome LDS sort family of k_segsort.hpp in its three instantiations, the same kernels over
contig bins, the transposition fix-up of the cm order, the multi-workgroup radix path).

A shard is built from numpy arrays, deterministic from a seed: `Genome` holds one genome in FILE order, `Shard` packs the
pga_genome_block_t blocks (10 planes of int32, rev bytes padded to 4, exon pairs) and the ctypes pga_shard_t.  `restate(shard)` is the
restatement, in numpy integers:

    X order  = lexsort((file index, cs, contig))            Y order = lexsort((X position, cm, contig))
    seg      = ctg_base[g] + contig                          pm[x]   = max of ce over the same contig at X positions <= x
    cds      = sum of oe - os                                off_exon shifted by the genome's exon base
    gid      = prot_gid[pid]                                 flags   = REV | F_MULTI (n_exon != 1) | F_HEAD (X position 0 of a genome
    yperm[y] = global X position                                       with hits) | F_CSTIE (an X neighbour with the same contig and cs)
    headpos  = goff

The comparison key rk (word 0 of record B) is NOT restated -- that would restate the protein hash -- but checked by its properties:
check_rk()."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PGA_F_REV = 1
I32_MAX = 2 ** 31 - 1
N_PROT, N_GENE = 200, 40
NP_MAX, NP_BIG, NP_WIDE = 10240, 14336, 25600  # what the 10-, 14- and 25-items forms of the LDS sort hold (k_segsort.hpp)


class Block(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("n_hit", "n_exon", "n_ctg", "max_cs", "max_cm", "max_score_adj", "any_neg", "any_multi")] + [("data", C.c_void_p), ("n_words", C.c_size_t), ("vfirst", C.c_void_p), ("vbase", C.c_void_p)]


class CShard(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("n_genome", C.c_int32), ("n_genome_global", C.c_int32), ("genome_global", C.c_void_p), ("n_prot", C.c_int32),
                ("n_gene", C.c_int32), ("n_hit", C.c_int64), ("n_exon", C.c_int64), ("block", C.c_void_p), ("prot_gid", C.c_void_p), ("gene_pref", C.c_void_p)]


class Par(C.Structure):
    _fields_ = [("min_ov_ratio", C.c_double), ("check_strand", C.c_int32), ("drop_sgl_exon", C.c_int32), ("reserved", C.c_int32 * 4)]


class HitState(C.Structure):  # pga_hit_state_t
    _fields_ = [(k, C.c_void_p) for k in ("flags", "rank", "score_dom", "pid_dom", "pid_dom0", "pos_x", "pos_y", "flt_x_bits")]


def abi_version():
    hdr = open(os.path.join(ROOT, "include", "pangene_hip.h")).read()
    return int(re.search(r"#define PGA_ABI_VERSION (\d+)u", hdr).group(1))


def bits_for(v):
    """width of the sort key field that holds values up to v (at least one bit, at most 32)"""
    return max(1, min(32, int(v).bit_length()))


class Genome:
    """one genome in file order: contig, cs, ce, cm [n] (int64 here, int32 in the block), and everything else drawn from rng"""

    def __init__(self, rng, n_ctg, cid, cs, ce, cm):
        n = len(cs)
        self.n, self.n_ctg = n, int(n_ctg)
        self.cid, self.cs, self.ce, self.cm = (np.asarray(a, np.int64) for a in (cid, cs, ce, cm))
        assert n == 0 or (self.cid.min() >= 0 and self.cid.max() < n_ctg and self.cs.min() >= 0 and (self.ce >= self.cs).all() and self.cm.min() >= 0
                          and max(self.ce.max(), self.cm.max()) <= I32_MAX)
        self.pid = rng.integers(0, N_PROT, n)
        self.rank = rng.integers(0, 4, n)
        self.sori = rng.integers(1, 1000, n)
        self.sadj = rng.integers(1, 500, n)  # (never 0: a score key of 0 is a case of its own in both forms of rk)
        self.rev = rng.integers(0, 2, n).astype(np.uint8)
        self.nex = np.where(rng.random(n) < 1 / 3, rng.integers(2, 6, n), 1)  # about a third multi-exon, 2 to 5 exons
        self.offx = np.cumsum(self.nex) - self.nex
        # exons: 2 n_exon cut points inside [0, ce - cs], ascending: sorted, disjoint intervals relative to cs
        ne = int(self.nex.sum())
        owner = np.repeat(np.arange(n), 2 * self.nex)
        pts = (rng.random(2 * ne) * (self.ce - self.cs + 1)[owner]).astype(np.int64)
        pts = pts[np.lexsort((pts, owner))]
        self.os, self.oe = pts[0::2], pts[1::2]
        self.n_exon = ne

    def words(self):
        planes = np.stack([self.pid, self.cid, self.rank, self.sori, self.sadj, self.nex, self.offx, self.cs, self.ce, self.cm]).astype(np.int32)
        rev = np.zeros((self.n + 3) // 4 * 4, np.uint8)
        rev[:self.n] = self.rev
        ex = np.stack([self.os, self.oe], axis=1).astype(np.int32)
        return np.ascontiguousarray(np.concatenate([planes.ravel(), rev.view(np.int32), ex.ravel()]))


class Shard:
    """genomes -> pga_shard_t (self.c); max_cs / max_cm: what every block DECLARES (None: what its hits have); prot_gid / gene_pref: the tables
    (None: drawn, N_PROT proteins of N_GENE genes); par: (min_ov_ratio, check_strand)"""

    def __init__(self, name, genomes, rng, max_cs=None, max_cm=None, prot_gid=None, gene_pref=None, par=(0.5, 0)):
        self.name, self.genomes = name, genomes
        self.prot_gid = rng.integers(0, N_GENE, N_PROT).astype(np.int32) if prot_gid is None else np.ascontiguousarray(prot_gid, np.int32)
        self.gene_pref = (rng.random(N_GENE) < 0.3).astype(np.uint8) if gene_pref is None else np.ascontiguousarray(gene_pref, np.uint8)
        self.P, self.Q = len(self.prot_gid), len(self.gene_pref)
        self.goff = np.concatenate([[0], np.cumsum([g.n for g in genomes])]).astype(np.int64)
        self.eoff = np.concatenate([[0], np.cumsum([g.n_exon for g in genomes])]).astype(np.int64)
        self.ctg_base = np.concatenate([[0], np.cumsum([g.n_ctg for g in genomes])]).astype(np.int64)
        self.N, self.E, self.G = int(self.goff[-1]), int(self.eoff[-1]), len(genomes)
        self._words = [g.words() for g in genomes]
        self._blocks = (Block * max(1, self.G))()
        for k, (g, w) in enumerate(zip(genomes, self._words)):
            assert w.size == 10 * g.n + (g.n + 3) // 4 + 2 * g.n_exon
            d_cs = max_cs if max_cs is not None else (int(g.cs.max()) if g.n else 0)
            d_cm = max_cm if max_cm is not None else (int(g.cm.max()) if g.n else 0)
            assert g.n == 0 or (g.cs.max() <= d_cs and g.cm.max() <= d_cm)
            self._blocks[k] = Block(g.n, g.n_exon, g.n_ctg, d_cs, d_cm, int(g.sadj.max()) if g.n else 0, int((g.sadj < 0).any()) if g.n else 0, int((g.nex != 1).any()) if g.n else 0,
                                    w.ctypes.data, w.size, None, None)
        self._gg = np.arange(self.G, dtype=np.int32)
        self.c = CShard(abi_version(), self.G, self.G, self._gg.ctypes.data, self.P, self.Q, self.N, self.E, C.addressof(self._blocks),
                        self.prot_gid.ctypes.data, self.gene_pref.ctypes.data)
        self.par = Par(par[0], par[1], 0)
        self.key_bits = (bits_for(max(b.max_cs for b in self._blocks)), bits_for(max(b.max_cm for b in self._blocks)), bits_for(max(1, max(g.n_ctg for g in genomes)) - 1))


def restate(sh):
    """what pga_begin leaves, in X order (see the module docstring).  Also pos_x / pos_y in file order (what pga_download gives), and sadj /
    pref in X order for check_rk.  Record B's word 0 (rk) is left 0."""
    N = sh.N
    A, B, Cc = (np.zeros((N, 4), np.int64) for _ in range(3))
    flags, fidx, gnm, yperm, sadj = (np.zeros(N, np.int64) for _ in range(5))
    pos_x, pos_y = np.zeros(N, np.int64), np.zeros(N, np.int64)
    for k, g in enumerate(sh.genomes):
        if g.n == 0:
            continue
        b = int(sh.goff[k])
        sl = slice(b, b + g.n)
        xo = np.lexsort((np.arange(g.n), g.cs, g.cid))                # X order: X position -> file index
        yo = np.lexsort((np.arange(g.n), g.cm[xo], g.cid[xo]))        # Y order: Y position -> X position
        cds = np.add.reduceat(np.concatenate([g.oe - g.os, [0]]), g.offx)  # (every hit has at least one exon)
        A[sl] = np.stack([g.cs[xo], sh.ctg_base[k] + g.cid[xo], g.ce[xo], np.zeros(g.n, np.int64)], axis=1)
        B[sl] = np.stack([np.zeros(g.n, np.int64), sh.prot_gid[g.pid[xo]], cds[xo], g.pid[xo]], axis=1)
        Cc[sl] = np.stack([g.rank[xo], g.nex[xo], sh.eoff[k] + g.offx[xo], g.sori[xo]], axis=1)
        flags[sl] = np.where(g.rev[xo] != 0, PGA_F_REV, 0)
        fidx[sl], gnm[sl], yperm[sl], sadj[sl] = xo, k, b + yo, g.sadj[xo]
        pos_x[b + xo] = np.arange(g.n)
        pos_y[b + xo[yo]] = np.arange(g.n)
    # pm: the running maximum of ce inside a contig.  seg never decreases along the X order, so the running maximum of seg << 32 | ce is
    # (the contig we are in, the largest ce seen in it so far)
    if N:
        A[:, 3] = np.maximum.accumulate(A[:, 1] << 32 | A[:, 2]) & 0xffffffff
    same = (A[1:, 1] == A[:-1, 1]) & (A[1:, 0] == A[:-1, 0]) if N else np.zeros(0, bool)  # X neighbours with the same contig and cs
    cstie = np.zeros(N, bool)
    cstie[1:] |= same
    cstie[:-1] |= same
    head = np.zeros(N, bool)
    head[sh.goff[:-1][np.diff(sh.goff) > 0]] = True
    return dict(recA=A, recB=B, recC=Cc, rev=flags, multi=Cc[:, 1] != 1, head=head, cstie=cstie, fidx=fidx, gnm=gnm, yperm=yperm, headpos=sh.goff.copy(),
                pos_x=pos_x, pos_y=pos_y, sadj=sadj, pref=sh.gene_pref[B[:, 1]].astype(np.int64) if N else np.zeros(0, np.int64))


def check_rk(rk, want, by_sort):
    """the properties of the comparison key rk (record B, word 0) of overlap.c:137's (score_adj, preferred, hash(pid)), without the hash;
    None, or what is wrong.  by_sort: the dense rank over the shard (PANGENE_RANK_BY_SORT=1), else score_adj << s | preferred << (s - 1) | a
    number of the protein, s = bits_for(P) + 1."""
    rk = np.asarray(rk, np.int64)
    sadj, pref, pid = want["sadj"], want["pref"], want["recB"][:, 3]
    if rk.size == 0:
        return None
    if not by_sort:
        s = bits_for(N_PROT) + 1
        low = rk & ((1 << (s - 1)) - 1)
        if not np.array_equal(rk >> s, sadj):
            return "rk >> rk_shift is not score_adj at %d" % int(np.flatnonzero((rk >> s) != sadj)[0])
        if not np.array_equal((rk >> (s - 1)) & 1, pref):
            return "the bit below score_adj is not gene_pref[gid] at %d" % int(np.flatnonzero(((rk >> (s - 1)) & 1) != pref)[0])
        n_pid, n_low, n_pair = len(np.unique(pid)), len(np.unique(low)), len(np.unique(pid << 32 | low))
        if not n_pid == n_low == n_pair:
            return "the low field of rk is not an injective function of pid (%d pids, %d values, %d pairs)" % (n_pid, n_low, n_pair)
        return None
    key = (sadj << 1 | pref) << 32 | pid
    n_key, n_rk, n_pair = len(np.unique(key)), len(np.unique(rk)), len(np.unique(np.stack([key, rk]), axis=1).T)
    if not n_key == n_rk == n_pair:
        return "rk is not equal exactly for equal (score_adj, pref, pid) (%d keys, %d ranks, %d pairs)" % (n_key, n_rk, n_pair)
    if not np.array_equal(np.unique(rk), np.arange(1, n_rk + 1)):
        return "rk is not a dense rank 1 .. %d" % n_rk
    if (np.diff((key >> 32)[np.argsort(rk, kind="stable")]) < 0).any():
        return "rk does not order by (score_adj, pref) first"
    return None


def rk_order(rk):
    """the place of every hit's rk among the distinct values: equal for two forms of rk exactly when they order every pair of hits the same way, ties included"""
    return np.unique(np.asarray(rk, np.int64), return_inverse=True)[1].astype(np.int32)


# ------------------------------------------------------------------------------------------------
# the shards
# ------------------------------------------------------------------------------------------------
def _plain(rng, n, n_ctg, span=5_000_000):
    """an ordinary genome: hits of 100 .. 3000 bp anywhere on its contigs, a tenth of them starting where another hit starts (cs ties), cm near the middle
    with a jitter wide enough to disagree with the cs order, a tenth of them on another hit's cm (cm ties)"""
    cid = rng.integers(0, n_ctg, n)
    cs = rng.integers(0, span, n)
    if n > 1:
        dup = rng.random(n) < 0.1
        src = rng.integers(0, n, n)
        cid, cs = np.where(dup, cid[src], cid), np.where(dup, cs[src], cs)
    ln = rng.integers(100, 3000, n)
    cm = cs + ln // 2 + rng.integers(-40, 41, n) * (rng.random(n) < 0.5)
    if n > 1:
        dup = rng.random(n) < 0.1
        src = rng.integers(0, n, n)
        cm = np.where(dup & (cid == cid[src]), cm[src], cm)
    return Genome(rng, n_ctg, cid, cs, np.maximum(cs + ln, cs), np.maximum(cm, 0))


def _reaching(rng, n, span=5_000_000):
    """single contig; the first hit of the X order ends after every other: pm's carry crosses every wave span of the workgroup"""
    g = _plain(rng, n, 1, span)
    first = np.lexsort((np.arange(n), g.cs))[0]
    ce = g.ce.copy()
    ce[first] = 1 << 30
    return Genome(rng, 1, g.cid, g.cs, ce, g.cm)


def _ctg_per_3(rng, n):
    """a contig per 3 hits: contig heads fall on, before and after the boundaries of the wave spans (multiples of 64)"""
    g = _plain(rng, n, 1, span=100_000)
    cid = rng.permutation(n) // 3
    return Genome(rng, (n + 2) // 3, cid, g.cs, g.ce, g.cm)


def _sized(rng, sizes):
    """one genome whose contig c has sizes[c] hits, in file order interleaved"""
    cid = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
    g = _plain(rng, len(cid), 1)
    return Genome(rng, len(sizes), cid, g.cs, g.ce, g.cm)


def crowd(n_cu, seed=11):
    """k_genome_sort2 over whole genomes (2 n_cu + 8 small ones keep class 0 its own launch) with both other forms, sizes at every band edge.  Coordinates
    below 2^20 and up to 3414 contigs a genome (12 bits): all three forms sort composite keys of exactly 32 bits, as the bacterial sets do"""
    rng = np.random.default_rng(seed)
    span = 1_000_000
    cyc = [0, 1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025]
    n_small = 2 * n_cu + 8
    sizes = cyc + [int(v) for v in rng.integers(0, 201, n_small - len(cyc) - 1)] + [0]
    gs = [_plain(rng, n, int(rng.integers(1, 6)), span) for n in sizes]
    big = [_reaching(rng, 10239, span), _ctg_per_3(rng, 10240), _reaching(rng, 10241, span), _reaching(rng, 14336, span), _reaching(rng, 14337, span), _reaching(rng, 25600, span)]
    for k, g in enumerate(big):  # spread among the small ones; the last genome stays the empty one
        gs.insert(5 + 37 * k, g)
    assert gs[-1].n == 0
    return Shard("crowd", gs, rng)


def few(seed=12):
    rng = np.random.default_rng(seed)
    return Shard("few", [_plain(rng, n, int(rng.integers(1, 6))) for n in (1, 64, 1000, 10240, 14336)], rng)


def fix_cases(n=5000):
    """(cs, cm) in X order of the four genomes of the fix shard, with the property each is there for asserted"""
    i = np.arange(n)
    cs = 100 * i
    out = {}
    out["a"] = cs + 50
    assert (np.diff(out["a"]) > 0).all()  # no inversion: the first double pass moves nothing
    b = np.where(i % 7 == 0, cs + 160, cs + 50)
    yo = np.lexsort((i, b))
    moved = np.flatnonzero(yo != i)
    assert len(moved) >= 2 and len(moved) % 2 == 0 and (moved[1::2] == moved[0::2] + 1).all() and (yo[moved[0::2]] == moved[1::2]).all() and (yo[moved[1::2]] == moved[0::2]).all()
    out["b"] = b  # disjoint adjacent swaps only: settles in the first double pass, the second confirms
    c = b.copy()
    c[0] = 400_000
    assert int(np.flatnonzero(np.lexsort((i, c)) == 0)[0]) >= 64 + 12  # 12 phases moving a hit one place each cannot settle it: the radix passes restart
    out["c"] = c
    d = 100 * (i // 5 * 5) + 50
    assert np.array_equal(np.lexsort((i, d)), i) and (np.diff(d) == 0).sum() == n - n // 5 and (np.diff(cs) > 0).all()  # ties of cm keep the X order
    out["d"] = d
    return cs, out


def fix(seed=13):
    rng = np.random.default_rng(seed)
    cs, cases = fix_cases()
    gs = []
    for k in "abcd":
        f = rng.permutation(len(cs))  # file order: any
        gs.append(Genome(rng, 1, np.zeros(len(cs), np.int64), cs[f], np.maximum(cs + 200, cases[k])[f], cases[k][f]))
    return Shard("fix", gs, rng)


WIDTHS = [(1, 1, 1), (2, 127, 255), (2, 2 ** 15 - 1, 2 ** 16 - 1), (2, I32_MAX, I32_MAX), (3, I32_MAX, 2 ** 30 - 1), (3, 2 ** 30 - 1, I32_MAX), (300, 2 ** 23 - 1, 2 ** 24 - 1)]


def _coords(rng, n, top):
    """half uniform up to top, a quarter within 3 of it, a quarter from 8 values"""
    kind = rng.integers(0, 4, n)
    eight = rng.integers(0, top + 1, 8)
    return np.where(kind < 2, rng.integers(0, top + 1, n), np.where(kind == 2, np.maximum(top - rng.integers(0, 4, n), 0), eight[rng.integers(0, 8, n)]))


def widths(k, seed=14):
    """the key widths set exactly by what the blocks declare; cm drawn independently of cs (adversarial for the fix-up, right either way)"""
    n_ctg, max_cs, max_cm = WIDTHS[k]
    rng = np.random.default_rng(seed + k)
    gs = []
    for n in (1700, 1300):
        cs = _coords(rng, n, max_cs)
        gs.append(Genome(rng, n_ctg, rng.integers(0, n_ctg, n), cs, np.minimum(cs + rng.integers(0, 3000, n), I32_MAX), _coords(rng, n, max_cm)))
    return Shard("widths%d" % k, gs, rng, max_cs=max_cs, max_cm=max_cm)


BIN_SIZES = [0, 6000, 4240, 1, 10240, 10241, 14336, 0, 5]  # lean bins {0, 6000, 4240} {1} {10240} {0, 5}, wide bins {10241} {14336}


def bins(seed=15):
    rng = np.random.default_rng(seed)
    return Shard("bins", [_sized(rng, BIN_SIZES), _plain(rng, 100, 3), _plain(rng, 0, 1)], rng)


def over(seed=16):
    """beyond what one workgroup's LDS holds, and no contig bins either (a contig of 25 601 hits): the multi-workgroup radix path"""
    rng = np.random.default_rng(seed)
    return Shard("over", [_reaching(rng, 25601), _sized(rng, [15000, 15000])], rng)


def manyctg(seed=17):
    """5000 hits over 300 contigs of at most 200 hits, some empty (PANGENE_BIN_CAP=256 cuts it into bins: 200 + 56 fits one exactly, 200 + 57 does not)"""
    rng = np.random.default_rng(seed)
    sizes = [200, 56, 200, 57, 0, 0, 1, 199, 0, 200]
    rest = 5000 - sum(sizes)
    tail = np.bincount(rng.integers(0, 250, rest), minlength=290)  # (the last 40 contigs stay empty)
    assert tail.max() <= 200
    return Shard("manyctg", [_sized(rng, sizes + [int(v) for v in tail])], rng)


NAMES = ["crowd", "few", "fix"] + ["widths%d" % k for k in range(len(WIDTHS))] + ["bins", "over", "manyctg"]


def make(name, n_cu=256):
    if name == "crowd":
        return crowd(n_cu)
    if name.startswith("widths"):
        return widths(int(name[6:]))
    return {"few": few, "fix": fix, "bins": bins, "over": over, "manyctg": manyctg}[name]()


def expected_route(name, n_cu):
    """(route, n_unit) in the default environment; n_unit[0] of crowd is a lower bound"""
    if name == "crowd":
        return 1, (2 * n_cu, 2, 2)
    if name == "bins":
        return 2, (5, 2, 0)
    if name == "over":
        return 0, (0, 0, 0)
    return 1, None
