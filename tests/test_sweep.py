"""The shards of the sweep tests (tests/support/sweep_ref.py) and the plain restatement of pg_shadow against the plain-C oracle, without a GPU:
every shard reaches the boundary of k_sweep.hpp / k_ingest.hpp it was built for (`reaches`, computed from the shard alone), and on every shard
pgo_begin + pgo_shadow(1) give the restatement's SHADOW bits, pid_dom, score_dom and statistics exactly.  Guards the oracle that
tests/test_sweep_gpu.py compares the HIP kernels with."""
import ctypes as C
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import stage_a_ref as sr  # noqa: E402
import sweep_ref as sw  # noqa: E402


@pytest.fixture(scope="module")
def oracle(built):
    lib = C.CDLL(os.path.join(ROOT, "oracle", "liboracle.so"))
    for f in ("create", "begin", "shadow", "ingest", "download"):
        getattr(lib, "pgo_" + f).restype = C.c_int
    lib.pgo_begin.argtypes = [C.c_void_p]
    lib.pgo_shadow.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.pgo_ingest.argtypes = lib.pgo_download.argtypes = [C.c_void_p, C.c_void_p]
    lib.pgo_destroy.restype, lib.pgo_destroy.argtypes = None, [C.c_void_p]
    return lib


@pytest.fixture(scope="module")
def reach():
    memo = {}

    def get(name):
        if name not in memo:
            memo[name] = sw.reaches(sw.make(name))
        return memo[name]
    return get


def test_shards_are_small_and_deterministic():
    for name in sw.NAMES:
        a, b = sw.make(name), sw.make(name)
        assert a.N <= 12_000 and a.G == 4 and a.genomes[1].n == 0
        assert all(np.array_equal(x.words(), y.words()) for x, y in zip(a.genomes, b.genomes)) and np.array_equal(a.gene_pref, b.gene_pref)
    assert sum(sw.make(n).N < 3000 for n in sw.NAMES) >= len(sw.NAMES) - 2


def test_shards_reach_what_they_are_for(reach, oracle):
    # halo: partners 31 / 32 / 33 slots away at the edges of a wave -- 31 stays in the LDS window, 32 and 33 send the hit to the slow list --, a hit with
    # 600 later partners across two tile borders, every one of which goes to the slow list, pairs across 63|64, 255|256, 511|512; the cut variants
    r = reach("halo")
    assert r["N"] == sw.HALO_N and not r["any_multi"] and sw.PRE % 64 != 0
    assert 31 in r["back_lds"] and {32, 33} <= r["back_slow"] and max(r["back_lds"]) == 31
    assert 31 in r["fwd_lds"] and {32, 33} <= r["fwd_slow"] and max(r["fwd_lds"]) == 31
    assert {(63, 64), (255, 256), (511, 512)} <= r["pairs"]
    assert r["fwd"][900] == 600 and 1500 // 256 - 900 // 256 == 2 and r["slow"][900] and r["slow"][960:1501].all() and (r["back"][960:1501] > 32).all()
    assert 0 < r["n_slow"] < r["N"] // 2
    for n in sw.HALO_CUTS:
        assert reach("halo%d" % n)["N"] == n
    assert (255, 256) in reach("halo257")["pairs"] and (511, 512) in reach("halo513")["pairs"] and (63, 64) in reach("halo255")["pairs"]
    # piles / single: piles of 20 .. 33 inside the window, a 64-span with two chunks of SW_WCAP pairs and one with three, a pile of 70 partly in LDS
    for name in ("piles", "single"):
        r = reach(name)
        assert r["any_multi"] == (name == "piles")
        sp = r["span_pairs"]
        assert ((sp > sw.SW_WCAP) & (sp <= 2 * sw.SW_WCAP)).any() and (sp > 2 * sw.SW_WCAP).any()
        inside = ~r["slow"] & (r["n_partner"] >= 19) & (r["n_partner"] <= 32)  # (members of the piles of 20 .. 33)
        assert inside.sum() > 500 and len(set(r["n_partner"][inside].tolist())) >= 10 and 32 in r["n_partner"][inside] and max(r["back"][inside].max(), r["fwd"][inside].max()) <= 32
        assert r["n_partner"].max() == 69 and r["pairs_lds_and_slow"] > 0 and (r["slow"] & (r["n_partner"] == 69)).any() and (~r["slow"] & (r["n_partner"] == 69)).any()
    # exons and the ratio shards: list lengths on both sides of 8 and of SW_XMAX in pairs, a window beyond SW_XCAP, shared exons, equal ends / starts,
    # a hit inside an intron, 2x against m; dense enough for the staging build
    for name in ("exons", "ratio03", "ratio13", "ratio_strand"):
        r = reach(name)
        assert set(sw.LIST_LENGTHS) <= r["nex_in_pairs"] and r["window_exons"] > sw.SW_XCAP and r["density"] >= 1.3 * sw.SW_LEAN_BELOW
        assert r["shared_exon_pairs"] >= 2 and r["eq_end"] >= 1 and r["eq_start"] >= 1 and r["intron_pairs"] >= 1
        assert r["two_x_minus_m"] == {-1, 0, 1} and r["n_irregular"] == 0
        if name != "exons":
            assert r["ratio_cmp"] == {"below", "at", "above"}
    assert sw.make("ratio03").par.min_ov_ratio == 0.3 and sw.make("ratio13").par.min_ov_ratio == 1 / 3 and 333 / 999 == 1 / 3 and 3 / 10 == 0.3
    assert sw.make("ratio_strand").par.check_strand == 1 and sw.make("exons").par.min_ov_ratio == 0.5
    # odd: irregular lists; round: the exact fractions, over every overlap; sparse: the lean build
    assert reach("odd")["n_irregular"] >= 20 and reach("odd")["any_multi"]
    r = reach("round")
    assert set(r["fractions"]) == {Fraction(t, 1000) for t in sw.ROUND_FRAC} and min(r["fractions"].values()) >= 60 and sum(r["fractions"].values()) >= 250
    assert set(sw.ROUND_OV) <= r["isolated_ov"] and r["any_multi"]
    r = reach("sparse")
    assert r["any_multi"] and 0 < r["density"] < 0.5 * sw.SW_LEAN_BELOW
    # filters: every branch of pg_flag_pseudo, ties of pg_flt_subopt_isoform, the two variants; what only a run shows (chains) from the oracle's statistics
    for name in ("filters", "filters_neg", "filters_big"):
        r = reach(name)
        ps = r["pseudo"]
        assert min(ps[k] for k in ("none_single", "none_multi", "min_is_1", "min_half_max", "pseudo_1", "pseudo_2", "pseudo_4+", "promoted", "first_stays")) >= 1
        assert r["subopt_ties"] >= 3 and r["subopt_ties_same_cs"] >= 3 and r["max_genome"] == 2100
        assert r["any_neg"] == (name == "filters_neg") and (name == "filters_neg" or r["max_sadj"] == {"filters": (1 << 20) - 1, "filters_big": 1 << 20}[name])
        assert (sr.bits_for(r["max_sadj"]) + sr.bits_for(r["max_genome"] - 1) <= 32) == (name != "filters_big")  # what the 4-byte `best` entries need
        sh = sw.make(name)
        stats = np.zeros((sh.G, 4), np.int32)
        ctx = C.c_void_p()
        assert oracle.pgo_create(C.byref(ctx), C.byref(sh.c), C.byref(sh.par)) == 0 and oracle.pgo_begin(ctx) == 0 and oracle.pgo_ingest(ctx, stats.ctypes.data) == 0
        oracle.pgo_destroy(ctx)
        assert (stats[-1] >= [20, 20, 5, 50]).all(), stats  # pseudo, overlapping isoforms, chains, sub-optimal isoforms
    # head: the first hit of the last genome and an ordinary one lose to hits of other genes
    for name in ("head", "head2"):
        sh = sw.make(name)
        got = sw.shadow_restate(sh, 1)
        f = lambda k: int(sh.goff[-2] + sh.genomes[-1].file_of[sh.mark[k] - sw.PRE])
        assert sh.mark["h0"] == sw.PRE
        for h, w in (("h0", "w0"), ("h1", "w1")):
            assert got["flags"][f(h)] & sw.F_SHADOW and not got["flags"][f(w)] & sw.F_SHADOW and got["pid_dom"][f(h)] == sh.genomes[-1].pid[f(w) - sh.goff[-2]]
    assert sw.make("head2").head_file[-1] == sw.make("head2").genomes[-1].file_of[sw.make("head2").mark["h1"] - sw.PRE]


@pytest.mark.parametrize("name", sw.NAMES)
def test_oracle_agrees_with_the_restatement(oracle, name):
    sh = sw.make(name)
    want = sw.shadow_restate(sh, 1)
    ctx = C.c_void_p()
    assert oracle.pgo_create(C.byref(ctx), C.byref(sh.c), C.byref(sh.par)) == 0
    try:
        assert oracle.pgo_begin(ctx) == 0
        stats = np.full((sh.G, 2), -1, np.int32)
        assert oracle.pgo_shadow(ctx, 1, stats.ctypes.data) == 0
        flags, pid_dom, score_dom = np.full(sh.N, 0xffffffff, np.uint32), np.full(sh.N, -7, np.int32), np.full(sh.N, -7, np.int32)
        st = sr.HitState(flags=flags.ctypes.data, pid_dom=pid_dom.ctypes.data, score_dom=score_dom.ctypes.data)
        assert oracle.pgo_download(ctx, C.byref(st)) == 0
    finally:
        oracle.pgo_destroy(ctx)
    assert np.array_equal(flags & sw.PUBLIC, want["flags"])
    assert np.array_equal(pid_dom, want["pid_dom"])
    assert np.array_equal(score_dom, want["score_dom"])
    assert np.array_equal(stats, want["stats"])
    if sh.N > 100:
        assert want["stats"][:, 1].sum() > 0
