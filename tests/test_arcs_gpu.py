"""The vertex step and a host-driven arc and branch round of the HIP backend -- pga_vtx_partials, pga_flag_vtx, pga_arc_round_local in its waiting and its
deferred form, pga_arc_round + pga_arc_set_current, pga_rep_pos, pga_n_local, pga_branch_pairs + pga_branch_decide, pga_mark_hits and a second arc round whose
sweep sees weak_br set (k_vertex.hpp, k_genes.hpp: k_walk, k_gene_arcs_wave_t, k_gene_arcs_big, k_arc_compact; k_arcs.hpp: the sort path; k_branch.hpp:
k_rank_genome, k_rep_fill, k_n_local and the pair kernels) -- directly against the plain-C oracle, step by step, on shards built for the constants inside the
kernels (tests/support/arcs_ref.py; what each reaches is asserted in tests/test_arcs.py, where the oracle itself is held against a plain restatement of
graph.c:103-169 and branch.c:6-46).  One child process per environment (tests/support/arcs_direct.py: the script, what is compared, and the route
assertions from the hook pga_selftest_arc_route of pga_host_selftest.hpp).

Not covered here: the queued loop pga_branch_loop with its riders and k_arc_final (tests/test_loop_tail_gpu.py, tests/test_branch_lazy_gpu.py hold it
against these host-driven rounds), the sharded exchange kernels (k_walk_list / pga_override_order: tests/test_order_gpu.py)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRECT = os.path.join(ROOT, "tests", "support", "arcs_direct.py")

pytestmark = pytest.mark.gpu


def child(env, *args):
    e = {k: v for k, v in os.environ.items() if not k.startswith("PANGENE_")}
    e.update(env)
    r = subprocess.run([sys.executable, DIRECT] + list(args), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, cwd=ROOT, env=e)
    out = r.stdout.decode(errors="replace")
    print(out[-8000:])
    assert r.returncode == 0 and out.rstrip().endswith("ALL OK"), out[-8000:]
    return out


def test_default_routes(built):
    """the gene path; hits: n_big = the genes with more than 512 hits; keys: n_big = the genes with more than 128 keys, nothing overflows; hub: the deferred
    round answers 1 with one overflowed gene and is repeated on the sort path"""
    out = child({})
    assert "hits: ok" in out and "hub: ok" in out and "branch: ok" in out


def test_sort_path(built):
    """k_arc_flag .. k_arc_l2 on every shard"""
    child({"PANGENE_ARC_SORT_PATH": "1"}, "--sort-path")


def test_gene_tables_of_4_keys(built):
    """nearly every gene overflows: status 1 from the deferred round on every shard with a gene of more than 4 keys, the repeat on the sort path"""
    child({"PANGENE_GENE_TABLE_LOG2": "2"}, "--table-log2", "2")


def test_gene_tables_of_128_keys(built):
    """128-key tables in both gene kernels: the gene of 129 keys sends `keys` to the sort path"""
    child({"PANGENE_GENE_TABLE_LOG2": "7"}, "--table-log2", "7")


def test_live_lists(built):
    """the walk, the gene-major index and the second round's sweep over the members' lists, which by then hold hits that mark_hits has filtered"""
    child({"PANGENE_LIVE_LISTS": "1"}, "--live", "1")


def test_no_live_lists(built):
    child({"PANGENE_LIVE_LISTS": "0"}, "--live", "0")


def test_walk_of_four_positions_a_thread(built):
    """k_walk<4>: tiles of 1 024 positions"""
    child({"PANGENE_WALK_IPT": "4"}, "--walk", "4")


@pytest.mark.parametrize("lanes", ["32", "64"])
def test_n_local_lanes(built, lanes):
    """the 32- and 64-lane forms of k_n_local on every shard, those of 17 and 33 genomes among them.  That the switch took is taken on trust here (the hook's eight
    values do not include the lanes); by the number of genomes alone round500 (507 genomes) runs the 32-lane form and round1000 the 64-lane form in every child"""
    child({"PANGENE_NL_LANES": lanes})


def test_lds_vertex_kernel_with_small_spill_area(built):
    """k_vtx1_lds, and the second attempt of the spill area"""
    child({"PANGENE_POST": "lds", "PANGENE_VTX_SPILL_CAP": "3"}, "--lds-vtx", "1")


def test_general_rank_and_pair_scans(built):
    child({"PANGENE_RANK_BY_SORT": "1", "PANGENE_PAIR_SCAN_GENERAL": "1"})


def test_poisoned_pool(built):
    child({"PANGENE_POISON": "1"})
