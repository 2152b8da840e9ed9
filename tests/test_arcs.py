"""The shards of the arc and branch round tests (tests/support/arcs_ref.py) and the plain restatements of pg_gen_arc and pg_gen_rep_pos + pg_n_local against
the plain-C oracle, without a GPU: every shard reaches the boundary of k_genes.hpp / k_branch.hpp it is named for -- asserted from the shard's marks and from
what pgo_* gives when the script of tests/support/arcs_direct.py is driven through the oracle alone --, and on every shard pgo_arc_round_local (both rounds
of the script) and pgo_rep_pos + pgo_n_local give the restatement's counters, arc records and counts exactly.  Guards the oracle that
tests/test_arcs_gpu.py compares the HIP kernels with."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import arcs_ref as ar  # noqa: E402
import arcs_direct as ad  # noqa: E402


@pytest.fixture(scope="module")
def ran(built):
    """name -> (shard, what the script leaves through the oracle); each shard runs once"""
    api = ad.Api(C.CDLL(os.path.join(ROOT, "oracle", "liboracle.so")), "pgo")
    memo = {}

    def get(name):
        if name not in memo:
            sh = ar.make(name)
            memo[name] = (sh, ad.run(api, sh))
        return memo[name]
    return get


def vtx(sh, gene, rev):
    return int(sh.g2s[gene]) << 1 | rev


def table(o, step="3"):
    return {int(x): tuple(int(o[step, "arc." + k][i]) for k in ad.ARC.names[1:]) for i, x in enumerate(o[step, "arc.x"])}


def walkable_y(sh, o, step="3"):
    """the walkable marks of the shard in Y order, and the flags there"""
    d = ar.y_order(sh)
    f = o[step, "flags"][[d["file"][a] for a in d["yperm"]]] if sh.N else np.zeros(0, np.uint32)
    return (f & (ar.F_FLT | ar.F_SHADOW)) == 0, f


def test_shards_are_small_and_deterministic():
    for name in ar.NAMES:
        a, b = ar.make(name), ar.make(name)
        assert a.N <= 25_000 and a.genomes[1].n == 0 and a.name == name and (a.N < ar.PRE or (a.genomes[0].n >= 37 and a.genomes[2].n == 50))  # (local* also uses genome 0)
        assert all(np.array_equal(x.words(), y.words()) for x, y in zip(a.genomes, b.genomes)) and np.array_equal(a.g2s, b.g2s)
    assert sum(ar.make(n).N < 6000 for n in ar.NAMES) >= len(ar.NAMES) - 1  # (hits alone has tens of thousands)


def test_hits(ran):
    sh, o = ran("hits")
    members, keys = ad.member_counts(sh, o, False), ad.key_counts(sh, o)
    assert [int(members[sh.mark[n]]) for n in ar.HIT_COUNTS] == list(ar.HIT_COUNTS)  # on both sides of GA_WAVE_HITS = 512 and of one and two steps of 1984
    assert ar.GA_STEP == 1984 and {511, 512, 513, 1983, 1984, 1985, 2 * 1984 + 1} <= set(ar.HIT_COUNTS)
    assert keys.max() <= ar.GA_CAP_WAVE  # no gene leaves the wave kernel for its keys: n_big counts the genes with more than 512 hits
    assert int((members > ar.GA_WAVE_HITS).sum()) == 5
    assert ad.member_counts(sh, o, True)[[sh.mark[n] for n in ar.HIT_COUNTS]].tolist() == list(ar.HIT_COUNTS)  # no hit of them is FLT: the same under live lists
    # the (gene, genome) groups of the largest gene in the order of the gene-major index (X order): longer than the halo, one across each window border
    w = ar.sr.restate(sh)
    gid, gnm = w["recB"][:, 1], w["gnm"]
    fx = sh.goff[gnm] + w["fidx"]
    H = sh.mark[3969]
    z = np.flatnonzero(gid == H)
    gj = gnm[z]
    cut = np.flatnonzero(np.diff(gj)) + 1
    bounds = np.concatenate([[0], cut, [len(z)]])
    sizes = np.diff(bounds)
    assert sizes.min() >= 150 and sizes.max() <= 240 and sizes.min() > ar.GA_HALO
    for border in (ar.GA_STEP, 2 * ar.GA_STEP):
        k = int(np.searchsorted(bounds, border, side="right")) - 1
        assert bounds[k] < border < bounds[k + 1], "no group lies across the window border %d" % border
    assert bounds[int(np.searchsorted(bounds, ar.GA_STEP, side="right")) - 1] < ar.GA_STEP - ar.GA_HALO  # ... and begins in front of the halo: its neighbours come from global memory
    walk = (o["3", "flags"][fx[z]] & (ar.F_FLT | ar.F_SHADOW)) == 0
    per = {int(j): walk[gj == j] for j in np.unique(gj)}
    assert any(not v[0] and v[1:].all() for v in per.values()), "no group whose first hit alone is not walkable"
    assert any(not v.any() for v in per.values()), "no group without a walkable hit"
    assert int((o["3", "flags"] & ar.F_SHADOW != 0).sum()) > 500 and o["3", "hazards"][1:3].tolist() == [0, 0]


def test_keys_and_hub(ran):
    sh, o = ran("keys")
    keys = ad.key_counts(sh, o)
    assert [int(keys[sh.mark[k]]) for k in (127, 128, 129, 511, 512)] == [127, 128, 129, 511, 512]  # GA_CAP_WAVE = 128 and GA_CAP = 512
    assert keys.max() == ar.GA_CAP and int((keys > ar.GA_CAP_WAVE).sum()) == 3 and ad.member_counts(sh, o, False).max() <= ar.GA_WAVE_HITS
    deg = o["3", "deg"]
    for k in (127, 128, 129, 511, 512):  # both vertices of the hub, half the keys each
        s = int(sh.g2s[sh.mark[k]])
        assert (int(deg[2 * s]), int(deg[2 * s + 1])) == (-(-k // 2), k // 2)
    t = table(o)
    H = sh.mark[512]
    tg = {x & 0xffffffff for x in t if x >> 32 == vtx(sh, H, 0)}
    assert {v & 1 for v in tg} == {0, 1} and len({v >> 1 for v in tg}) == 128  # the neighbours come in both orientations
    for g in sh.genomes:  # every hit of a hub lies between two different genes
        for c in range(g.n_ctg):
            k = np.flatnonzero(g.cid == c)
            p = g.pid[k[np.argsort(g.cm[k])]].tolist()
            assert len(p) != 3 or (p[1] in sh.mark.values() and len({p[0], p[1], p[2]}) == 3)
    sh, o = ran("hub")
    keys, deg = ad.key_counts(sh, o), o["3", "deg"]
    s = int(sh.g2s[sh.mark[513]])
    assert int(keys[sh.mark[513]]) == 513 > ar.GA_CAP and int(deg[2 * s]) + int(deg[2 * s + 1]) >= 513 and np.sort(keys)[-2] <= ar.GA_CAP_WAVE


def test_dups(ran):
    sh, o = ran("dups")
    m, t = sh.mark, table(o)

    def arc(a, ra, b, rb):
        return t[vtx(sh, m[a], ra) << 32 | vtx(sh, m[b], rb)]
    # (n_genome, tot_cnt, sum_dist, sum_s1, sum_s2); a genome's distance is (int32_t)(sum / n + .499), graph.c:141
    assert arc("A", 0, "C", 0) == (2, 3, 2 * 100 + 200, 20 + 13, 30 + 14)        # (100 + 101) / 2 = 100.5 -> 100, not 101; the leader is the group's second hit
    assert arc("C", 1, "A", 1) == (2, 3, 2 * 100 + 200, 30 + 14, 20 + 13)        # ... and its mirror
    assert arc("A", 1, "C", 0)[:3] == (1, 1, 177)                                  # the other strand of A in the same group
    assert arc("D", 0, "E", 1) == (2, 4, 3 * 110 + 112, 40 + 1, 50 + 2)          # 110.333 -> 110
    assert arc("F", 1, "G", 0) == (1, 3, 3 * 111, 40, 50)                        # 110.667 -> 111
    assert arc("T", 0, "T", 0) == (1, 2, 2 * 500, 61, 62) and arc("T", 1, "T", 1) == (1, 2, 2 * 500, 62, 61)  # the tandem: 500.5 -> 500
    assert arc("U", 0, "U", 1) == (2, 6, 4 * 300 + 2 * 299, 73 + 6, 73 + 6)      # the inverted self-adjacency: both half-arcs of an adjacency are the SAME arc
    assert arc("Z", 0, "W", 0) == (2, 3, 2 * 140 + 139, 0, 0)                    # zero and negative scores: the maxima start at 0 (graph.c:133)


def test_walk(ran):
    sh, o = ran("walk")
    ok, f = walkable_y(sh, o)
    look = ar.lookbacks(ok.tolist(), ar.WK_TILE)
    assert {1, 63, 64, 65, 255, 256, 257, 600} <= set(look.values()), sorted(set(look.values()))
    assert [look[t0] for t0, d, how in ar.WALK_D] == [d for t0, d, how in ar.WALK_D]
    assert any(not ok[t:t + ar.WK_TILE].any() for t in range(0, sh.N - ar.WK_TILE, ar.WK_TILE)), "no tile without a walkable hit"
    first = int(np.flatnonzero(ok)[0])
    assert first == 3 and not ok[:first].any()
    assert int(sh.goff[4]) == ar.WK_TILE  # a genome begins at position 256 ...
    d = ar.y_order(sh)
    seg = [d["seg"][a] for a in d["yperm"]]
    assert seg[2 * ar.WK_TILE - 1] != seg[2 * ar.WK_TILE] and d["gnm"][2 * ar.WK_TILE - 1] == d["gnm"][2 * ar.WK_TILE]  # ... and a contig at 512
    dead = f[~ok]
    assert int((dead & ar.F_FLT != 0).sum()) >= 300 and int((dead & ar.F_SHADOW != 0).sum()) >= 1000  # unwalkable by FLT here, by SHADOW there
    assert 4 * int((o["2", "flags"] & ar.F_FLT != 0).sum()) < sh.N  # (fewer than a quarter: no live lists by default, the walk runs over every hit)
    assert o["3", "hazards"][1] > 0  # h2_cm: two walkable neighbours share (contig, cm)
    big = ar.lookbacks(ok.tolist(), 4 * ar.WK_TILE)  # k_walk<4>: tiles of 1 024
    assert set(big) == {1024, 2048, 3072} and big[1024] == 63 and big[3072] > 64
    live = ar.lookbacks(ok[(f & ar.F_FLT) == 0].tolist(), ar.WK_TILE)  # the list of the members (live lists): the FLT stretches are gone, the SHADOW ones stand
    assert {1, 64, 65} <= set(live.values()) and max(live.values()) > ar.WK_TILE  # (there the look-back still crosses a step of 64 and a whole tile)
    for n in ar.WALK_CUTS:
        shc, oc = ran("walk%d" % n)
        assert shc.N == n
        okc, _ = walkable_y(shc, oc)
        assert okc.tolist() == ok[:n].tolist()  # the cut is the shard's beginning


@pytest.mark.parametrize("n_genome", [17, 33])
def test_local(ran, n_genome):
    sh, o = ran("local%d" % n_genome)
    assert sh.G == n_genome and {m[0] for m in sh.mark} == {0, 15, 16, n_genome - 1} | ({17} if n_genome > 18 else set())
    at = {(int(a), int(b)): k for k, (a, b) in enumerate(sh.pairs.tolist())}
    present = np.zeros((sh.G, sh.Q), bool)
    for j, g in enumerate(sh.genomes):
        present[j, g.pid] = True
    for k, (ld, lc, fm) in enumerate(sh.nl_settings):
        cnt = o["7.%d" % k, "nl_cnt"]
        assert (ld, lc) == (2000, 3) and cnt.max() <= 1  # every pair is comparable in one genome at the most
        for j, two, dd, dc, a, c in sh.mark:
            assert present[:, a].sum() == present[:, c].sum() == 1 and present[j, a] and present[j, c]
            want = int((not two or fm) and (dd == 0 or dc == 0))  # d = local_dist + dd, cc = local_count + dc, on one contig or on two
            assert cnt[at[a, c]] == cnt[at[c, a]] == want, (j, two, dd, dc, fm)
    assert {(dd, dc) for _, _, dd, dc, _, _ in sh.mark} == {(0, 1), (1, 0), (1, 1), (0, 0)} and {m[1] for m in sh.mark} == {0, 1}
    assert o["6", "hazards"][2] == 0


def test_branch(ran):
    sh, o = ran("branch")
    f1, f2 = o["8", "n_flt"].tolist()
    assert f1 > 0 and f2 > 0 and o["9", "n_marked"][0] > 0
    newly = (o["9", "flags"] & ar.F_FLT != 0) & (o["3", "flags"] & ar.F_FLT == 0)
    weak = (o["9", "flags"] & ar.WEAK_MASK) >> ar.WEAK_SHIFT
    assert newly.sum() > 0 and (weak[newly] == 2).all() and int((weak == 1).sum()) > 0
    deg, t, b = o["3", "deg"], table(o), sh.branch
    for n in ar.BRANCH_DEG:
        V, T = sh.mark[n]
        v = vtx(sh, V, 0)
        assert int(deg[v]) == n
        s1 = {x & 0xffffffff: ar.final_s1(r[3], r[0]) for x, r in t.items() if x >> 32 == v}
        assert len(s1) == n and max(s1.values()) == 1000
        if n > 3:  # on both sides of the three thresholds
            r = sorted(1.0 - s / 1000 for s in s1.values())
            for thr in (b["diff"], b["dist"], b["cut"]):
                assert any(x <= thr for x in r if x > thr - .002) and any(x > thr for x in r if x < thr + .002), (n, thr)
    ndl = o["8", "n_dist_loci"]
    assert ndl.max() > 3 and ndl[ndl > 0].min() >= 1
    # the second round's sweep decides by weak_br (overlap.c:139): a hit that dominated in the first round is shadowed in the second
    turned = (o["10a", "flags"] & ar.F_SHADOW != 0) & (o["3", "flags"] & (ar.F_SHADOW | ar.F_FLT) == 0) & (o["10a", "flags"] & ar.F_FLT == 0)
    assert turned.sum() > 0 and (weak[turned] == 1).all()
    back = (o["3", "flags"] & ar.F_SHADOW != 0) & (o["10a", "flags"] & (ar.F_SHADOW | ar.F_FLT) == 0)
    assert back.sum() > 0 and int(o["10", "n_arc"][0]) != int(o["3", "n_arc"][0])


@pytest.mark.parametrize("n_global", ar.VTX_GLOBAL)
def test_vtx(ran, n_global):
    sh, o = ran("vtx%d" % n_global)
    nw = (n_global + 63) // 64
    assert nw == {64: 1, 65: 2, 130: 3}[n_global] and sh.c.n_genome_global == n_global
    assert not np.array_equal(sh._gg, np.arange(sh.G)) and (np.diff(sh._gg) < 0).any() and len(set(sh._gg.tolist())) == sh.G and sh._gg.max() == n_global - 1
    rec, cnt = o["1", "vtx_rec"], o["1", "vtx_cnt"]
    assert rec.shape[1] == 1 + nw
    sub_of, dom_of = (rec[:, 0] >> np.uint64(20)).astype(np.int64), (rec[:, 0] & np.uint64(0xfffff)).astype(np.int64)
    bits = lambda r: {64 * w + b for w in range(nw) for b in range(64) if int(r[1 + w]) >> b & 1}
    assert ar.VTX_K == 8
    for k in ar.VTX_DOMS:  # 7, 8, 9, 20 dominators: below, at and beyond the slots of a gene
        S, D = sh.mark[k]
        r = rec[sub_of == S]
        assert len(r) == k and sorted(dom_of[sub_of == S].tolist()) == sorted(D)
        assert [bits(x) for x in r] == [{int(sh._gg[3 + D.index(int(d))])} for d in dom_of[sub_of == S]]  # one genome each, at its global place
        assert cnt[sh.Q + S] == k and cnt[S] == (1 if k == ar.VTX_DOMS[0] else 0)  # the first is dominant in one more genome
    S, D, E = sh.mark["never"]
    assert sorted(dom_of[sub_of == S].tolist()) == [D[0], D[2]] and cnt[sh.Q + S] == 3  # subordinate three times, but D[1] is not dominant where it dominates S ...
    assert cnt[D[1]] == 1 and cnt[sh.Q + D[1]] == 1 and (E in dom_of[sub_of == D[1]])  # ... though it is in another genome
    if nw > 1:
        used = set().union(*[bits(x) for x in rec])
        assert {w for w in range(nw)} == {v // 64 for v in used}, "not every bit word is used"


@pytest.mark.parametrize("kind", ["", "_full", "_wide"])
def test_reps(ran, kind):
    sh, o = ran("reps" + kind)
    m = sh.mark
    assert [g.n for g in sh.genomes[3:]] == [1023, 1024, 1025, 2049] == list(ar.REPS_SIZES) and ar.RK_T == 1024 and sh.par.check_strand == 1
    g3, off = sh.genomes[3], int(sh.goff[3])
    ok = (o["3", "flags"] & (ar.F_FLT | ar.F_SHADOW)) == 0
    ok3 = ok[off:off + g3.n]

    def hits_of(g, gene):
        return np.flatnonzero(g.pid == gene)
    for grp in (m["T2"], m["T3"]):  # walkable hits of different genes at one (contig, cs)
        k = np.concatenate([hits_of(g3, x) for x in grp])
        assert len(k) == len(grp) and ok3[k].all() and len(set(zip(g3.cid[k].tolist(), g3.cs[k].tolist()))) == 1
    k = hits_of(g3, m["SG"])  # two walkable hits of one gene at one start, on opposite strands
    assert len(k) == 2 and ok3[k].all() and g3.cs[k[0]] == g3.cs[k[1]] and set(g3.rev[k].tolist()) == {0, 1}
    assert (g3.nex[np.concatenate([hits_of(g3, m["T3"][0]), hits_of(g3, m["T3"][2])])] == 2).all()
    k = hits_of(g3, m["K_last"])  # the group's last hit in array order is not walkable, an earlier one is
    k = k[np.argsort(g3.cs[k])]
    assert len(k) == 2 and ok3[k[0]] and not ok3[k[1]]
    assert len(hits_of(g3, m["K_none"])) == 2 and not ok3[hits_of(g3, m["K_none"])].any()
    have = np.array([[len(hits_of(g, x)) > 0 for g in sh.genomes] for x in (m["only_first"], m["only_last"], m["nowhere"], m["M1"])])
    assert have[0].tolist() == [0, 0, 0, 1, 0, 0, 0] and have[1].tolist() == [0, 0, 0, 0, 0, 0, 1] and not have[2].any() and have[3, 3:].all()
    for j in (4, 5, 6):  # M1 is the last hit of the genomes of 1024, 1025, 2049 hits: its rank lies on either side of the step
        g = sh.genomes[j]
        assert g.pid[np.lexsort((np.arange(g.n), g.cs, g.cid))[-1]] == m["M1"]
    h6, h7 = int(o["6", "hazards"][2]), int(o["7.0", "hazards"][2])
    assert h6 > 0  # the immediate hazard of rep_pos
    tied = set(m["T2"]) | set(m["T3"])
    n_iv = sum(1 for a, c in sh.pairs.tolist() if (a in tied) != (c in tied) and c in set(m["AFT"]) | tied and a in set(m["AFT"]) | tied)
    assert 0 < h7 - h6 < n_iv  # H2b: the count test differs across the interval for some pairs of a tie member and a gene behind it, not for others
    cnt = o["7.0", "nl_cnt"]
    at = {(int(a), int(c)): k for k, (a, c) in enumerate(sh.pairs.tolist())}
    assert cnt[at[m["T2"][0], m["AFT"][0]]] == 1 and cnt[at[m["T2"][0], m["AFT"][7]]] == 0
    assert (sh.genomes[6].n_ctg == 4096) == (kind == "_full") and max(g.n_ctg for g in sh.genomes[:6]) < 4096
    if kind == "_wide":
        W1, W2 = m["W"]
        k1, k2 = hits_of(g3, W1)[0], hits_of(g3, W2)[0]
        vf, vb = sh._v[0]
        assert vf[g3.cid[k2]] == g3.cid[k1] != g3.cid[k2] and vb[g3.cid[k2]] == 2 ** 32  # two pieces of one contig
        d = int(g3.cm[k2] + vb[g3.cid[k2]] - g3.cm[k1])
        assert d == 2 ** 32 + 1500 and d % 2 ** 32 <= 2000 < d  # not local by the true difference; local by the low words alone
        assert all(o["7.%d" % s, "nl_cnt"][at[W1, W2]] == 0 for s in (0, 1))
        t = table(o)
        x = vtx(sh, W1, 0) << 32 | vtx(sh, sh.seg_gid[0], 0)  # W1+ -> the first filler gene, across the cut: 2^32 + 1 000 as an int32_t (graph.c:73)
        assert t[x][:3] == (1, 1, 1000)
    else:
        assert not sh._v


@pytest.mark.parametrize("n", ar.ROUND_N)
def test_round(ran, n):
    sh, o = ran("round%d" % n)
    m, t = sh.mark, table(o)
    assert sh.G == n + 7 and sh.use_ori == (0 if n == 500 else 1) and all(g.n == 3 for g in sh.genomes[3:3 + n])
    assert (256 < sh.G <= 640) == (n == 500)  # nl_lanes_for (k_branch.hpp:238): 32 lanes up to 640 genomes, 64 beyond
    arcs = {"AB": (vtx(sh, m["A"], 0), vtx(sh, m["B"], 0), 0), "BC": (vtx(sh, m["B"], 0), vtx(sh, m["C"], 0), 1), "CB": (vtx(sh, m["C"], 1), vtx(sh, m["B"], 1), 2),
            "BA": (vtx(sh, m["B"], 1), vtx(sh, m["A"], 1), 1)}
    weak = dict(zip(o["3", "arc.x"].tolist(), o["8", "arc_weak"].tolist()))
    fr = set()
    for v, w, k in arcs.values():
        r = t[v << 32 | w]
        assert r[0] == n and r[3] == 980 * n + ar.ROUND_MORE[n][k]
        f = (r[3] % n) * 1000 // n
        fr.add(f)
        s1 = ar.final_s1(r[3], r[0])
        assert s1 == (981 if f >= 501 else 980)  # .498 and .500 stay, .501 and .502 go up under + .499
        assert (weak[v << 32 | w] != 0) == (s1 == 980)  # beside the arc of s1 = 1 000: 1 - 980 / 1000 > branch_diff, 1 - 981 / 1000 is not
    assert fr == ({498, 500, 502} if n == 500 else {500, 501, 502})
    X1 = m["X"][0]
    assert [j for j, g in enumerate(sh.genomes) if (g.pid == X1).any()] == [3 + n]  # (A, X1) is comparable in one of the last genomes only
    at = {(int(a), int(c)): k for k, (a, c) in enumerate(sh.pairs.tolist())}
    assert o["7.0", "nl_cnt"][at[m["A"], X1]] == 1
    g = sh.genomes[3 + n + 3]  # the hit whose dominator has no segment: walkable, score_dom >= score_ori, so graph.c:82-85 takes score_dom unless use_ori
    k = int(np.flatnonzero(g.pid == m["Hd"])[0]) + int(sh.goff[3 + n + 3])
    assert o["3", "flags"][k] & (ar.F_FLT | ar.F_SHADOW) == 0 and o["3", "score_dom"][k] >= 300 and sh.g2s[o["3", "pid_dom0"][k]] < 0
    sd = int(o["3", "score_dom"][k])
    s = [r for x, r in t.items() if x >> 33 == sh.g2s[m["Hd"]]]
    assert len(s) == 2 and all(r[3] == (300 if sh.use_ori else sd) for r in s) and sd > 4000


@pytest.mark.parametrize("name", ar.NAMES)
def test_oracle_equals_restatement(ran, name):
    """pgo_arc_round_local of both rounds against graph.c:103-169, pgo_rep_pos + pgo_n_local against branch.c:6-46, restated in loops and Python integers"""
    sh, o = ran(name)
    for step, st in (("3", "3"), ("10", "10a")):
        seg_cnt, arcs = ar.arc_restate(sh, {k: o[st, k] for k in ("flags", "score_dom", "pid_dom0")}, sh.use_ori)
        assert seg_cnt == o[step, "seg_cnt"].tolist()
        assert arcs == table(o, step) and list(o[step, "arc.x"]) == sorted(arcs)
        deg = np.bincount(np.array([x >> 32 for x in arcs], np.int64), minlength=2 * sh.n_seg) if arcs else np.zeros(2 * sh.n_seg, np.int64)
        assert deg.tolist() == o[step, "deg"].tolist()
    for k in ("seg_cnt", "deg", "n_arc") + tuple("arc." + f for f in ad.ARC.names):  # the deferred form and the exchange form
        assert np.array_equal(o["4", k], o["3", k]) and np.array_equal(o["5", k], o["3", k])
    for k, (ld, lc, fm) in enumerate(sh.nl_settings):
        assert ar.rep_restate(sh, {"flags": o["3", "flags"]}, sh.pairs, ld, lc, fm) == o["7.%d" % k, "nl_cnt"].tolist()
