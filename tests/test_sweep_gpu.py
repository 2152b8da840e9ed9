"""The overlap sweep (k_sweep.hpp: k_sweep<MODE, STAGE_C>, k_sweep_lean, k_sweep_slow -- pg_shadow + pg_flt_ov_isoform) and stage A's filters behind
it (k_ingest.hpp: k_pseudo0..3, k_genome_filters<k32> or k_iso_apply / k_chain / k_subopt1/2) of the HIP backend, every route, directly against the
plain-C oracle, on shards built for the boundaries inside the kernels (tests/support/sweep_ref.py; what each reaches is asserted in
tests/test_sweep.py, where the oracle itself is held against a plain restatement of pg_shadow).  One child process per environment
(tests/support/sweep_direct.py; the switches are read once per process) drives pga_create .. pga_ingest .. pga_post_apply .. pga_shadow ..
pga_flag_vtx .. pga_set_filter and a second pga_begin + pga_ingest(NULL) through both backends and compares, with integer equality and for EVERY
hit, filtered ones included: the public flag bits, rank, score_dom, pid_dom, pid_dom0, pos_x, pos_y, flt_x_bits after every step, the statistics
of pga_ingest and pga_shadow, n_pseudo, max_ori, sums, and the hazard counters and hazard segments.  The hook pga_selftest_sweep_route
(pga_host_selftest.hpp) says which builds ran, and the child asserts that they are the ones its environment asks for.

Not covered here: the sweeps of the arc rounds with weak_br set and over the live lists -- MODE 0 runs with weak_br = 0 and over the full records only --
and everything from pga_vtx_partials on: tests/test_arcs_gpu.py, whose second arc round sweeps with weak_br set, under PANGENE_LIVE_LISTS=1 over the
members' lists.  What is left: the sweeps queued by pga_branch_loop."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRECT = os.path.join(ROOT, "tests", "support", "sweep_direct.py")

pytestmark = pytest.mark.gpu


def child(env, *args):
    e = {k: v for k, v in os.environ.items() if not k.startswith("PANGENE_")}
    e.update(env)
    r = subprocess.run([sys.executable, DIRECT] + list(args), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, cwd=ROOT, env=e)
    out = r.stdout.decode(errors="replace")
    print(out[-6000:])
    assert r.returncode == 0 and out.rstrip().endswith("ALL OK"), out[-6000:]
    return out


def test_default_routes(built):
    """the sampled density picks the sweep build: exons stages its lists, sparse leaves them in global memory; the filters' tables in LDS, 8-byte entries"""
    out = child({}, "--lists", "auto")
    assert "exons: ok" in out and "sparse: ok" in out and "filters_big: ok" in out


def test_exon_lists_in_lds(built):
    child({"PANGENE_SWEEP_LISTS": "lds"}, "--lists", "lds")


def test_exon_lists_in_global_memory(built):
    child({"PANGENE_SWEEP_LISTS": "global"}, "--lists", "global")


def test_literal_merge_on_regular_lists(built):
    child({"PANGENE_MERGE_LITERAL": "1"})


def test_filters_with_global_tables(built):
    child({"PANGENE_FILTERS": "global"}, "--filters", "global")


def test_filters_with_4_byte_entries(built):
    """gf_k32 on every shard that allows it; the negative score_adj and the score_adj of 2^20 in a genome of 2100 hits fall back to 8 bytes"""
    child({"PANGENE_FILTERS": "k32"}, "--filters", "k32")


def test_filters_with_8_byte_entries(built):
    child({"PANGENE_FILTERS": "k64"}, "--filters", "k64")


def test_poisoned_pool(built):
    child({"PANGENE_POISON": "1"})
