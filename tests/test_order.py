"""The shards and orders of the exact-order override tests (tests/support/order_ref.py) against the plain-C oracle, without a GPU.  Three things:
pgo_override_order + pgo_set_head + pgo_download give what the plain restatement of the ABI comment gives, on every shard after every override of the
script of tests/support/order_direct.py (which also holds every listed order against the contract: whole contigs, keys that do not decrease); every
override MATTERS to the oracle -- the same script with the canonical orders in place of the cm overrides gives another arc table, with them in place of
the cs overrides other SHADOW bits, h2_cs events or (what a changed representative or rank shows as) n_local counts, on `marks` another n_marked -- so
that an implementation that does nothing cannot pass tests/test_order_gpu.py; and every shard reaches the boundary it is named for."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import arcs_ref as ar  # noqa: E402
import order_ref as orf  # noqa: E402
import order_direct as od  # noqa: E402

SKIP = ("route", "grew", "hazard_segs", "pos_x", "pos_y")


@pytest.fixture(scope="module")
def ran(built):
    """(name, ident) -> (shard, what the script leaves through the oracle, the overrides it made); each runs once"""
    api = od.Api(C.CDLL(os.path.join(ROOT, "oracle", "liboracle.so")), "pgo")
    memo = {}

    def get(name, ident=False):
        if (name, ident) not in memo:
            sh = orf.make(name)
            memo[name, ident] = (sh,) + od.run(api, sh, ident=ident)  # (run exits at the first pos_x / pos_y that is not the restatement's)
        return memo[name, ident]
    return get


def differing(a, b, only=None):
    return sorted(k for k in a if k[1] not in SKIP and (only is None or k[1] in only) and (len(a[k]) != len(b[k]) or not np.array_equal(a[k], b[k])))


def test_shards_are_small_and_deterministic():
    for name in orf.NAMES:
        a, b = orf.make(name), orf.make(name)
        assert a.N <= 5400 and a.genomes[1].n == 0 and a.genomes[0].n == 37 and a.genomes[2].n == 50 and a.name == name
        assert all(np.array_equal(x.words(), y.words()) for x, y in zip(a.genomes, b.genomes)) and np.array_equal(a.g2s, b.g2s)
    assert np.array_equal(ar.make("branch").genomes[3].words(), ar.branch().genomes[3].words())


@pytest.mark.parametrize("name", orf.NAMES)
def test_oracle_is_the_restatement(ran, name):
    """pos_x / pos_y after every override and step (inside run); every other array of the download is what it was in front of the override; the listed
    orders keep the contract and every kind of order is drawn"""
    sh, o, used = ran(name)
    labels = [l for l, _ in used]
    assert labels[:5] == ["0", "1cm", "1cs", "3cm", "3cs"] and labels[-4:] == ["6a", "6b", "6c", "6d"] and len(labels) >= 12
    for prev, label in (("1", "1cs"), ("5r", "5.0"), ("5.0", "5.1"), ("6b", "6c"), ("6c", "6d")):
        for k in od.STATE:
            if k not in ("pos_x", "pos_y", "flt_x_bits"):
                assert np.array_equal(o[prev, k], o[label, k]), (label, k)
    st = orf.State(sh)
    moved = 0
    for label, seg in used:
        orf.check_contract(sh, seg)
        before = orf.positions(sh, st)
        orf.override_restate(st, seg.which, seg)
        after = orf.positions(sh, st)
        moved += int((before[seg.which] != after[seg.which]).any())
        if seg.which == 1:
            assert np.array_equal(before[0], after[0])  # a cm override leaves the X order alone
    assert moved >= 4
    d = orf.derived_restate(sh, st)
    assert sorted(d["inv"]) == list(range(sh.N)) and sorted(d["yperm"]) == list(range(sh.N))
    u = dict(used)
    assert u["6a"].n == 0 and u["6b"].T == 0 and u["6b"].n >= 1 and u["6c"].T == sh.N and u["6d"].T == sh.N


@pytest.mark.parametrize("name", orf.NAMES)
def test_every_override_matters(ran, name):
    sh, o, _ = ran(name)
    table = {"arc.x", "arc.n_genome", "arc.tot_cnt", "arc.sum_dist", "arc.sum_s1", "arc.sum_s2", "n_arc"}
    if sh.kind in ("cm", "both", "marks"):
        _, i, _ = ran(name, "cm")
        assert any(k[0] == "1" for k in differing(o, i, table)), "the cm overrides change no arc of the first round"
    if sh.kind in ("cs", "both"):
        _, i, _ = ran(name, "cs")
        d = differing(o, i, {"flags", "nl_cnt"}) + [k for k in o if k[1] == "hazards" and o[k][2] != i[k][2]]
        assert d, "the cs overrides change neither a SHADOW bit nor an h2_cs event nor an n_local count"
        if name == "head":
            assert ("1", "flags") in d
    if sh.kind == "marks":
        _, i, _ = ran(name, "cm")
        assert int(o["3", "n_marked"][0]) != int(i["3", "n_marked"][0])


def test_partial_and_full_walks(ran):
    """an override of at most an eighth of the shard walks its contigs again (k_walk_list), a larger one leaves the walk to the next round"""
    for name in orf.NAMES:
        sh, _, used = ran(name)
        small = [dict(used)[l].T * 8 <= sh.N for l in ("1cs", "3cm")]
        assert small == [True, True] if name in orf.PARTIAL else name not in ("eighth1", "pm") or small == [False, False], (name, small)


def x_of(sh, j):
    """the hits of genome j in canonical X order: arrays of file index, contig, cs, ce, cm, gene"""
    g = sh.genomes[j]
    k = np.lexsort((np.arange(g.n), g.cs, g.cid))
    return k, g.cid[k], g.cs[k], g.ce[k], g.cm[k], g.pid[k]


def groups(keys, cid):
    """sizes of the runs of equal (contig, key)"""
    out, i = [], 0
    while i < len(keys):
        e = i
        while e < len(keys) and keys[e] == keys[i] and cid[e] == cid[i]:
            e += 1
        out.append(e - i)
        i = e
    return out


def test_grid(ran):
    sh, o, used = ran("grid")
    g = sh.genomes[3]
    assert np.bincount(g.cid).tolist() == list(orf.GRID_SIZES) and np.cumsum(orf.GRID_SIZES)[[0, 2, 3, 4, 5, 6, 7, 8, 9]].tolist() == list(orf.GRID_T)
    burst = [s for l, s in used if l.startswith("5.")]
    assert [s.T for s in burst] == list(orf.GRID_T) and {s.which for s in burst} == {0, 1}
    assert {255, 256, 257} <= set(orf.GRID_T) and {1023, 1024, 1025} <= set(orf.GRID_T) and orf.BLOCK == 256 and orf.SCAN_TILE == 1024  # a workgroup, a scan tile; 4 097: five tiles
    first = dict(used)["0"]
    two = orf.seg_orders(first)[3, 1]
    assert len(two) == 2 and two == orf.canonical(sh, 0, 3, 1)[0][::-1]  # the contig of two hits, swapped
    assert orf.contig_start(sh, 3, 1) == 1  # behind the contig of one hit
    assert dict(used)["1cs"].T * 8 <= sh.N  # the partial walk


def test_pm(ran):
    sh, o, used = ran("pm")
    k, cid, cs, ce, cm, pid = x_of(sh, 3)
    n0 = int((cid == 0).sum())
    assert n0 == 2500 > 2 * orf.SCAN_TILE
    assert cs[0] == cs[1] and ce[:2].max() > ce[2:n0].max() and cs[2] > cs[0]  # the hit that ends last stands in the first tie group, of two
    st = orf.State(sh)
    a = int(sh.goff[3])
    for label, seg in used[:3]:
        orf.override_restate(st, seg.which, seg)
        d = orf.derived_restate(sh, st)
        top = max(d["ce"][a:a + n0])
        if label == "0":    # first: the maximum is carried over every thread's, wave's and (in the tiled scan, below) tile's border of the contig
            assert d["ce"][a] == top and all(d["pm"][a + p] == top for p in (0, 15, 16, 1023, 1024, 2047, 2048, n0 - 1))
        if label == "1cs":  # second: the first hit's pm falls
            assert d["ce"][a + 1] == top and d["pm"][a] < top and d["pm"][a + 1] == top
    assert cs[n0 - 1] == cs[n0 - 2] == cs[n0] and cid[n0] == 1  # a tie group at the contig's end, and the next contig begins at the same cs ...
    assert d["pm"][a + n0] < top and d["cstie"][a + n0 - 1] and d["cstie"][a + n0]  # ... with its own maximum; both are tied, each in its own contig
    # the override of every contig is longer than the one-workgroup scan takes (dev_prims.hpp: SCAN_ONE_MAX = 4 096): the tiled scan, whose tiles of 1 024 list
    # entries end inside the long contig, twice, with the contig's maximum to carry across (its first tie group holds the hit that ends last)
    every = dict(used)["6c"]
    assert every.which == 0 and every.T == sh.N > orf.SCAN_ONE_MAX and every.genome[:4].tolist() == [0, 1, 2, 3] and every.off[3] == a
    assert a < orf.SCAN_TILE < 2 * orf.SCAN_TILE < a + n0 - 1 and int(sh.genomes[3].ce[every.file[a:a + 2]].max()) == top
    k, cid, cs, ce, cm, pid = x_of(sh, 4)
    assert set(orf.PM_SIZES) <= set(groups(cs.tolist(), cid.tolist())) and max(orf.PM_SIZES) == 65
    walk = (o["1", "flags"] & (ar.F_FLT | ar.F_SHADOW)) == 0
    assert walk[int(sh.goff[4]):int(sh.goff[5])].all()  # every hit of every group is walkable


def test_head(ran):
    sh, o, used = ran("head")
    assert sh.genomes[4].n == 0 and sh.genomes[3].n and sh.genomes[5].n
    st = orf.State(sh)
    h1 = sh.head1(st)
    orf.set_head_restate(st, h1)
    old = list(st.head)
    assert [old[j] for j in (3, 5, 6, 7)] == [1, 1, 1, 1]  # the mark stands on a hit that is not the first
    seg = used[0][1]
    assert used[0][0] == "0" and seg.which == 0 and {(3, 0), (5, 0), (6, 0)} <= set(orf.seg_orders(seg)) and (7, 0) not in orf.seg_orders(seg)
    orf.override_restate(st, 0, seg)
    assert [st.head[j] for j in (3, 5, 6, 7)] == [0, 0, 0, 1]  # the first contig overridden: index 0; a later one: untouched
    h2 = sh.head2(st, old)
    assert h2[3] == st.x[3][1] and h2[5] == st.x[5][2] and h2[6] == -1 and h2[7] == st.x[7][1]
    orf.set_head_restate(st, h2)
    assert [st.head[j] for j in (3, 5, 6, 7)] == [1, 2, 0, 1]
    # what the oracle shows of it: behind the first round exactly the hit at index 0 keeps the SHADOW bit of the sweep before pga_flag_vtx
    f = o["1", "flags"]
    for j in (3, 5, 6, 7):
        a = int(sh.goff[j])
        pair = [a + int(sh.genomes[j].file_of[k]) for k in sh.mark[j]]
        kept = [p for p in pair if f[p] & ar.F_SHADOW]
        want = a + st.x[j][st.head[j]]
        assert kept == ([want] if want in pair else []), (j, kept, want)
    assert sum(len([p for p in (int(sh.goff[j]) + int(sh.genomes[j].file_of[k]) for k in sh.mark[j]) if f[p] & ar.F_SHADOW]) for j in (3, 6, 7)) == 3


def test_cmties(ran):
    sh, o, used = ran("cmties")
    m = sh.mark
    k, cid, cs, ce, cm, pid = x_of(sh, 3)
    f = o["1", "flags"][int(sh.goff[3]) + k]
    walk = ((f & (ar.F_FLT | ar.F_SHADOW)) == 0).tolist()
    sizes, at, seen = groups(cm.tolist(), cid.tolist()), 0, set()
    for n in sizes:
        genes, w = pid[at:at + n].tolist(), walk[at:at + n]
        if n == 2 and all(w):
            seen.add("two of one gene" if genes[0] == genes[1] else "two")
        if n == 3 and all(w):
            seen.add("three")
        if n == 3 and w == [True, False, True] and f[at + 1] & ar.F_FLT:
            seen.add("middle FLT")
        if n == 4 and not w[1] and f[at + 1] & ar.F_SHADOW and not f[at + 1] & ar.F_FLT and genes[1] == m["S1"]:
            seen.add("middle SHADOW")
        at += n
    assert seen == {"two", "two of one gene", "three", "middle FLT", "middle SHADOW"}, seen
    # the contigs of the distances: W, d - 1 unwalkable, a walkable pair on one cm, d - 1 unwalkable, W
    for c, d in enumerate(orf.WALK_D, start=1):
        w = [walk[p] for p in np.flatnonzero(cid == c)]
        assert len(w) == 2 * d + 2 and w[0] and w[-1] and w[d] and w[d + 1] and not any(w[1:d]) and not any(w[d + 2:-1])
        cmc = cm[cid == c]
        assert cmc[d] == cmc[d + 1]
    assert {1, 63, 64, 65, 300} == set(orf.WALK_D)
    c = len(orf.WALK_D) + 1
    w1, w2 = [walk[p] for p in np.flatnonzero(cid == c)], [walk[p] for p in np.flatnonzero(cid == c + 1)]
    assert w1 == [True, True] + [False] * 5 and w2 == [False] * 5 + [True, True]  # neighbours only across the contig border: not neighbours
    every = (o["1", "flags"] & (ar.F_FLT | ar.F_SHADOW)) == 0
    first, last = int(np.flatnonzero(every[sr_file_x(sh)])[0]), int(np.flatnonzero(every[sr_file_x(sh)])[-1])
    segs = set(orf.seg_orders(dict(used)["1cs"])) | set(orf.seg_orders(dict(used)["3cm"]))
    assert first == 3 and (0, 0) in segs and (5, 0) in segs and sh.N - 1 - last == 3  # the first and the last walkable hit of the shard lie in overridden contigs
    assert dict(used)["1cs"].T * 8 <= sh.N and dict(used)["3cm"].T * 8 <= sh.N  # both take the partial walk ...
    starts = {s for j, s in orf.seg_orders(dict(used)["1cs"]) if j == 3} | {s for j, s in orf.seg_orders(dict(used)["3cm"]) if j == 3}
    assert {orf.contig_start(sh, 3, c) for c in range(1, len(orf.WALK_D) + 3)} <= starts  # ... over the contigs of the distances and of the border


def sr_file_x(sh):
    """global file index of every X position (canonical order)"""
    w = ar.sr.restate(sh)
    return (sh.goff[w["gnm"]] + w["fidx"]).astype(np.int64)


def test_eighth(ran):
    sh, _, used = ran("eighth")
    sh1, _, used1 = ran("eighth1")
    assert sh.N == sh1.N == orf.EIGHTH_N and all(np.array_equal(a.words(), b.words()) for a, b in zip(sh.genomes, sh1.genomes))
    T, T1 = dict(used)["1cs"].T, dict(used1)["1cs"].T
    assert T * 8 == sh.N and T1 == T + 1 and T1 * 8 > sh.N
    a, b = orf.seg_orders(dict(used)["1cs"]), orf.seg_orders(dict(used1)["1cs"])
    assert a[3, 0] == b[3, 0] and len(b[3, T]) == 1  # the same orders; the one hit more lies where it lay


def test_strand_pieces(ran):
    sh, o, used = ran("strand")
    assert sh.par.check_strand == 1
    g = sh.genomes[3]
    sg = np.flatnonzero(g.pid == sh.mark["SG"])
    assert len(sg) == 2 and g.cs[sg[0]] == g.cs[sg[1]] and g.cid[sg[0]] == g.cid[sg[1]] and g.rev[sg[0]] != g.rev[sg[1]]
    f = o["1", "flags"][int(sh.goff[3]) + sg]
    assert not (f & (ar.F_FLT | ar.F_SHADOW)).any()  # both walkable
    px = [orf.positions(sh, orf.State(sh))[0][int(sh.goff[3]) + sg].tolist()] + [o[l, "pos_x"][int(sh.goff[3]) + sg].tolist() for l in ("0", "1cs", "3cs")]
    assert px[1] == px[0][::-1] and px[2] == px[1] and px[3] == px[0]  # the overrides swap them, and hand the canonical order back in the end
    assert o["2", "hazards"][2] > 0
    sh, o, used = ran("pieces")
    assert len(sh._v) == 1 and sh.seg_first[int(sh.ctg_base[3]) + 1] == int(sh.ctg_base[3]) and sh.seg_base[int(sh.ctg_base[3]) + 1] == 2 ** 32
    assert {(3, 0), (3, orf.contig_start(sh, 3, 1))} <= set(orf.seg_orders(dict(used)["1cs"])) and dict(used)["1cs"].T * 8 <= sh.N  # small enough: it is vfirst that keeps the partial walk off


def test_live(ran):
    sh, o, used = ran("live")
    f = o["0", "flags"]
    pseudo = (f & 0x20) != 0
    assert int((~pseudo).sum()) * 4 <= 3 * sh.N  # at most three hits in four are left when the vertex step counts them
    assert ((f[pseudo] & ar.F_FLT) != 0).all()
    member = (f & ar.F_FLT) == 0  # the lists are built in the first arc round, from the hits without flt
    g, a = sh.genomes[3], int(sh.goff[3])
    per = [int(member[a + np.flatnonzero(g.cid == c)].sum()) for c in range(4)]
    size = np.bincount(g.cid).tolist()
    assert per[0] == 0 and per[1] == 1 and per[2] == size[2] == 60 and 0 < per[3] < size[3]
    assert {(3, orf.contig_start(sh, 3, c)) for c in range(4)} <= set(orf.seg_orders(dict(used)["3cs"]))       # all of them behind the lists ...
    assert {(3, orf.contig_start(sh, 3, c)) for c in (1, 2, 3)} <= set(orf.seg_orders(dict(used)["1cs"]))      # ... and those with a member in the partial walk
    assert dict(used)["1cs"].T * 8 <= sh.N and dict(used)["3cm"].T * 8 <= sh.N
    k, cid, cs, ce, cm, pid = x_of(sh, 3)
    mem_x = member[a + k].tolist()
    at, ends, inside = 0, 0, 0
    for n in groups(cs.tolist(), cid.tolist()):
        w = mem_x[at:at + n]
        if n == 5 and any(w):
            ends += (not w[0]) and (not w[-1])
            inside += "".join("m" if v else "-" for v in w).strip("-").count("-") > 0
        at += n
    assert ends >= 3 and inside >= 3  # (the canonical order inside a group is the file's) non-members at both ends of a tie group, and between two members
    lost = member & ((o["3cs", "flags"] & ar.F_FLT) != 0)
    segs = orf.seg_orders(dict(used)["3cs"])
    assert any(lost[a + np.array(fl)].any() for (j, s), fl in segs.items() if j == 3)  # a member that mark_hits has filtered since, in an overridden contig
