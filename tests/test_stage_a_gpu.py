"""Stage A (pga_create + pga_begin) of the HIP backend, every route, against the plain restatement of tests/support/stage_a_ref.py: the
per-genome LDS sort family of k_segsort.hpp (k_genome_sort2 / 2d / 2w), the same kernels over contig bins, the transposition fix-up of
the cm order and the multi-workgroup radix path, through the self-test hook pga_selftest_stage_a (pga_host_selftest.hpp), which exports
what pga_download does not show: the records A / B / C with pm and rk, the F_HEAD / F_MULTI / F_CSTIE bits, fidx, gnm, yperm, headpos.
One child process per environment (tests/support/stage_a_direct.py; the switches are read once per process); all integer equality."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRECT = os.path.join(ROOT, "tests", "support", "stage_a_direct.py")

pytestmark = pytest.mark.gpu


def child(env, *args):
    e = {k: v for k, v in os.environ.items() if not k.startswith("PANGENE_")}
    e.update(env)
    r = subprocess.run([sys.executable, DIRECT] + list(args), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, cwd=ROOT, env=e)
    out = r.stdout.decode(errors="replace")
    print(out[-3000:])
    assert r.returncode == 0 and out.rstrip().endswith("ALL OK"), out[-3000:]
    return out


@pytest.fixture(scope="module")
def default_run(built, tmp_path_factory):
    """the child in the default environment, once: (its output, the file with the order of rk of every shard)"""
    dump = str(tmp_path_factory.mktemp("stage_a") / "packed.npz")
    return child({}, "--routes", "default", "--dump", dump), dump


def test_default_routes(default_run):
    """crowd: route 1 with all three forms launched (k_genome_sort2 over >= 2 n_cu whole genomes); few: the small genomes in the 14-items
    form; bins: 5 lean + 2 wide contig bins; over: the radix path"""
    assert "crowd: ok" in default_run[0] and "route 2, units (5, 2, 0)" in default_run[0]


def test_cm_order_by_radix_passes(built):
    child({"PANGENE_Y_FIXUP": "0"})


def test_global_radix_path_gives_the_same_arrays(built):
    child({"PANGENE_GLOBAL_SORT": "1"}, "--routes", "global")


def test_contig_bins_of_256(built):
    child({"PANGENE_BIN_CAP": "256"}, "--routes", "bincap")


def test_contig_bins_of_2048(built):
    child({"PANGENE_BIN_CAP": "2048", "PANGENE_BINS": "1"})


def test_without_contig_bins(built):
    child({"PANGENE_BINS": "0"}, "--routes", "bins0")


def test_poisoned_pool(built):
    child({"PANGENE_POISON": "1"})


def test_rank_by_sort_orders_every_pair_as_the_packed_key(default_run, tmp_path):
    """rk as the dense rank over the shard (PANGENE_RANK_BY_SORT=1) and rk as score_adj | preferred | rank of the hash in 32 bits: each with its
    own properties (stage_a_ref.check_rk), and both order every pair of hits of a shard the same way, ties included"""
    a, b = default_run[1], str(tmp_path / "sorted.npz")
    child({"PANGENE_RANK_BY_SORT": "1"}, "--dump", b)
    ra, rb = np.load(a), np.load(b)
    assert sorted(ra.files) == sorted(rb.files) and len(ra.files) >= 13
    for k in ra.files:
        assert np.array_equal(ra[k], rb[k]), k
