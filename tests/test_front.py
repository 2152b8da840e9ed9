"""The plain restatement the device's representative kernel is tested against (tests/support/front_ref.py) is itself right: on instances
without ties its representatives are those the host driver's order-exact route finds -- the proteins sorted by ksort_exact (the replay of
the reference's unstable sort, pangene_amd/csrc/host/ksort_exact.hpp), walked from the back.  And where two proteins of a gene share
the gene's largest key it says so, which is what sends the driver back to that route.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import front_ref as fr  # noqa: E402


@pytest.fixture(scope="module")
def ksort(tmp_path_factory):
    td = tmp_path_factory.mktemp("front_ksort")
    exe = str(td / "front_ksort")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "pangene_amd", "csrc", "host"),
                    os.path.join(ROOT, "tests", "support", "front_ksort.cpp"), "-o", exe], check=True)

    def order(keys):
        fi, fo = str(td / "keys.bin"), str(td / "order.bin")
        np.array(keys, dtype=np.uint64).tofile(fi)
        subprocess.run([exe, fi, fo], check=True)
        return np.fromfile(fo, dtype=np.int32)
    return order


def _sizes(rng, Q):
    return rng.choice([1, 1, 1, 2, 5], size=Q).tolist()


@pytest.mark.parametrize("seed", range(6))
def test_restatement_against_the_exact_sort_order(ksort, seed):
    rng = np.random.default_rng(seed)
    sizes = _sizes(rng, 120)
    three = [g for g, s in enumerate(sizes) if s >= 3]
    sums, gid = fr.instance(rng, sizes, tie_below=three[:4])  # a tie BELOW the largest key decides nothing
    ref = fr.post_rep_ref(sums, gid, len(sizes), 100, 0.05)
    assert not ref["tie"]
    order = ksort(ref["keys"])
    assert sorted(order.tolist()) == list(range(len(gid)))
    assert [ref["keys"][i] for i in order] == sorted(ref["keys"])
    assert fr.reps_by_order(order, gid, len(sizes)) == ref["rep_pid"]


def test_restatement_reports_a_tie_at_the_maximum_only():
    rng = np.random.default_rng(11)
    sizes = [1, 2, 5, 2, 5, 1, 3]
    sums, gid = fr.instance(rng, sizes, tie_at_max=[3], tie_below=[4])
    ref = fr.post_rep_ref(sums, gid, len(sizes), 100, 0.05)
    assert ref["tie"] and ref["tie_genes"] == [3]
    sums, gid = fr.instance(rng, sizes, zero_key_genes=[0, 5])  # all-zero keys of single-protein genes: nothing to decide
    assert not fr.post_rep_ref(sums, gid, len(sizes), 100, 0.05)["tie"]
    sums, gid = fr.instance(rng, sizes, zero_key_genes=[1])
    assert fr.post_rep_ref(sums, gid, len(sizes), 100, 0.05)["tie_genes"] == [1]


def test_restatement_arithmetic_edges():
    """count == 0 skips the division; the key's unsigned arithmetic; a zero c0 makes the predicate's quotient inf or NaN, which compare false"""
    sums = np.zeros((6, 6), dtype=np.int64)
    sums[0] = [7, 0, -1, 10, 1 << 31, 5]
    sums[2] = [0, 0, 1, 2, 1, 0]
    sums[3] = [0, 0, 0, 1, 0, 4]
    sums[4] = [0, 0, 5, 9, 1, 0]
    sums[5] = [0, 0, 0, 9, 0, 40]
    ref = fr.post_rep_ref(sums, np.arange(6, dtype=np.int32), 6, 10, 0.3)
    assert ref["n"] == [0, 0, 1, 3, 1, 4]
    assert ref["avg"] == [0, 0, -(1 << 31), 3, -(1 << 31), 1]  # 0xffffffff / 1 and 2^31 / 1 do not fit an int32: the x86 conversion's answer
    assert ref["keys"][2] == ((1 << 64) - (1 << 32)) + 1
    # protein 3: c1 = 1 < 3; protein 5: c1 = 4 >= 3 but c0 = 0: (s1 / c1) / (0 / 0) is NaN -> false
    assert ref["pj"] == [0, 0, 0, 0, 0, 0]
    assert fr.joint_pseudo(sums, 10, 0.3, False, True) == [1, 1, 1, 1, 1, 0]  # drop_sgl_exon: c1 == 0 or c1 <= 3
    sums[2, 5], sums[4, 5] = 2, 0  # (s1 / c1) / (0 / 2) = inf >= 0.99
    assert fr.joint_pseudo(sums, 10, 0.3, False, False)[5] == 1
    assert fr.joint_pseudo(sums, 10, 0.3, True, True) == [0] * 6
