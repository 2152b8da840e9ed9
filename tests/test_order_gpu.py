"""The exact-order overrides of the HIP backend -- pga_override_order with k_ov_sety, k_ov_gather, k_ov_scatter, k_ov_remap_y, k_cstie_list, the two
SegMax list scans, k_ovl_pos, k_ovl_remap_ylist, k_ovl_records, k_pack_wrec_list, k_walk_list and k_inv_only, pga_set_head and pga_hazard_segs
(pga_host_order.hpp, k_order.hpp, k_genes.hpp) -- directly against the plain-C oracle and against a plain restatement of the ABI comment, step by step,
with the overrides where graph_driver.cpp has them, on shards built for the constants inside the kernels (tests/support/order_ref.py; what each reaches
is asserted in tests/test_order.py, where the oracle itself is held against the restatement and every override is shown to matter to it).  One child
process per environment (tests/support/order_direct.py: the script, what is compared, and the route assertions from the hook pga_selftest_order of
pga_host_selftest.hpp).

Not covered here: the overrides inside the queued loop pga_branch_loop (the driver hands them over between its calls), orders that break the contract
(a segment that is not a whole contig, keys that decrease), set_head to a hit of a later contig in front of an override of the first, the sharded
exchange kernels."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRECT = os.path.join(ROOT, "tests", "support", "order_direct.py")

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
    """the lists come on by themselves on `live` alone; the partial walk on grid, head, cmties, eighth, live, marks, the full one on eighth1 and pm, none on pieces"""
    out = child({})
    assert "grid: ok" in out and "head: ok" in out and "live: ok" in out and "marks: ok" in out


def test_live_lists(built):
    """k_ovl_pos, k_ovl_remap_ylist, k_ovl_records and the members' SegMax scan on every shard; the sweep behind a cs override under -S reads the full records"""
    child({"PANGENE_LIVE_LISTS": "1"}, "--live", "1")


def test_no_live_lists(built):
    child({"PANGENE_LIVE_LISTS": "0"}, "--live", "0")


def test_sort_path(built):
    """the rounds on k_arc_flag .. k_arc_l2: they leave no half-arcs, so an override behind a round packs the walk's records of its contigs again and walks
    nothing (partial = 0 at 1cs, 5.0, 6b); the one behind rep_pos, which walks for itself, takes the partial walk as everywhere"""
    child({"PANGENE_ARC_SORT_PATH": "1"}, "--sort-path")


def test_walk_of_four_positions_a_thread(built):
    """k_walk<4> walks what k_walk_list walks again"""
    child({"PANGENE_WALK_IPT": "4"})


def test_general_rank_and_pair_scans(built):
    child({"PANGENE_RANK_BY_SORT": "1", "PANGENE_PAIR_SCAN_GENERAL": "1"})


def test_poisoned_pool(built):
    """every pool buffer an override takes (S_OVPOS, S_OVFILE, S_PERM, S_TILE, S_HZLIST) comes filled with a pattern"""
    child({"PANGENE_POISON": "1"})
