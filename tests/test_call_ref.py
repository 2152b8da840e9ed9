"""The restatement of the walk side of `pangene call` (tests/support/call_ref.py) checked against itself, without a GPU: the records
built by the procedure of the contract (one pass, open starts per end vertex) must equal the records of the closed form (all pairs
p < i of one walk) on every input that tests/support/call_direct.py gives the HIP kernels, and the alleles must be a partition of the
records by oriented path."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import call_cases as cc  # noqa: E402
import call_ref as cr  # noqa: E402

_MADE = {}


def made(which):
    """[(label, input, has_records, restatement)] of one generator, computed once"""
    if which not in _MADE:
        _MADE[which] = [(label, case, has, cr.walk_side(*case)) for label, case, has in cc.cases(which)]
    return _MADE[which]


def test_hand_example():
    """worked by hand from the contract: walk 0 2 0 2 and its reverse complement 3 1 3 1, one bubble 0 -> 2"""
    step = np.array([0, 2, 0, 2, 3, 1, 3, 1], dtype=np.int32)
    off = np.array([0, 4, 8], dtype=np.int64)
    got = cr.walk_side(step, off, 2, np.array([0], dtype=np.int32), np.array([2], dtype=np.int32))
    assert got["rec"].tolist() == [[0, 0, 0, 1], [0, 0, 0, 3], [0, 0, 2, 3], [1, 1, 0, 1], [1, 1, 0, 3], [1, 1, 2, 3]]
    assert got["rep"].tolist() == [0, 1, 0, 0, 1, 0] and got["cnt"].tolist() == [4, 2, 0, 0, 0, 0]
    assert got["gene_bub"].tolist() == [0, 0] and got["gene_seg"].tolist() == [0, 1] and got["gene_first"].tolist() == [1, 0]
    # a hairpin 0 -> 1: both orientations start at 0 and end at 1, + before - at the same st_off
    got = cr.walk_side(np.array([0, 0, 1], dtype=np.int32), np.array([0, 3], dtype=np.int64), 1, np.array([0], dtype=np.int32), np.array([1], dtype=np.int32))
    assert got["rec"].tolist() == [[0, 0, 0, 2], [1, 0, 0, 2], [0, 0, 1, 2], [1, 0, 1, 2]]
    assert got["rep"].tolist() == [0, 1, 2, 2] and got["gene_first"].tolist() == [0]  # paths 0 0 1, 0 1 1, 0 1, 0 1


@pytest.mark.parametrize("which", cc.WHICH)
def test_procedure_equals_closed_form(which):
    for label, case, has, want in made(which):
        a = cr.records_procedure(*case)
        assert a.shape == want["rec"].shape and np.array_equal(a, want["rec"]), label
        assert (len(a) > 0) == has, "%s: %d records" % (label, len(a))


@pytest.mark.parametrize("which", cc.WHICH)
def test_alleles_partition_the_records(which):
    for label, case, has, want in made(which):
        rec, rep, cnt = want["rec"], want["rep"], want["cnt"]
        R = len(rec)
        r = np.arange(R)
        assert (rep <= r).all() and np.array_equal(rep[rep], rep) and int(cnt.sum()) == R, label
        assert np.array_equal(cnt > 0, rep == r) and np.array_equal(cnt, np.bincount(rep, minlength=R)), label
        assert np.array_equal(rec[rep, 0] >> 1, rec[:, 0] >> 1), label
        seen = set()
        for f in np.flatnonzero(rep == r):  # the representatives of one bubble have different paths
            key = (int(rec[f, 0]) >> 1, cr.path_of(rec[f], case[0], case[1]).tobytes())
            assert key not in seen, label
            seen.add(key)
        gb, gs, gf = want["gene_bub"], want["gene_seg"], want["gene_first"]
        k = gb.astype(np.int64) * max(1, case[2]) + gs
        assert (np.diff(k) > 0).all() and len(set(gf.tolist())) == len(gf), label


def test_shapes_are_what_they_are_for():
    (_, ex, _, ex_want), = made("exhaustive")
    assert len(ex[1]) - 1 == 340 and len(ex[0]) == 1252 and len(ex[3]) == 16 and int((ex[3] < 0).sum()) == 2
    hair = {b for b in range(16) if ex[3][b] >= 0 and ex[4][b] == ex[3][b] ^ 1}
    assert len(hair) == 5 and hair <= set((ex_want["rec"][:, 0] >> 1).tolist())  # (0, 1), (1, 0), (2, 3) twice, (3, 2)
    (_, pl, _, pl_want), = made("pileup")
    n_int = int(np.maximum(pl_want["rec"][:, 3] - pl_want["rec"][:, 2] - 1, 0).sum())
    assert n_int > len(pl_want["rec"]) > len(pl[0]) == 400  # I > R > N: the sort buffers grow twice
    assert int((pl_want["cnt"] > 0).sum()) == 200  # 100 alleles a bubble
    (_, gl, _, gl_want), = made("graphlike")
    assert len(gl[0]) > 150000 and len(gl_want["rec"]) > 2048 * 8
    seen_empty = 0
    for label, case, has, want in made("edges"):
        step, off, n_seg, vs, ve = case
        ln = np.diff(off)
        if len(ln) >= 6 and len(step) > 2:
            assert ln[0] == 0 and ln[-1] == 0 and ((ln[1:] == 0) & (ln[:-1] == 0)).any(), label
        if len(vs) >= 8 and has:
            ends = np.concatenate((ve[vs >= 0], vs[vs >= 0] ^ 1))
            assert np.bincount(ends).max() >= 8, label
        seen_empty += not has
    assert seen_empty == 3 + len(cc.EDGE_SEEDS)  # no record, no step, no live bubble, and the N = 1 shape once a seed
