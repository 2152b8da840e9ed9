"""The plain restatement of stage A's orders (tests/support/stage_a_ref.py) against the plain-C oracle: for every shard the GPU test
(tests/test_stage_a_gpu.py) runs, pgo_create + pgo_begin + pgo_download give the restatement's pos_x, pos_y and REV bits.  Guards the
reference the HIP kernels are compared with, on a machine without a GPU; the fix shard's four constructions are asserted on the way
(stage_a_ref.fix_cases)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import stage_a_ref as sr  # noqa: E402


@pytest.fixture(scope="module")
def oracle(built):
    lib = C.CDLL(os.path.join(ROOT, "oracle", "liboracle.so"))
    lib.pgo_create.restype = lib.pgo_begin.restype = lib.pgo_download.restype = C.c_int
    lib.pgo_begin.argtypes = [C.c_void_p]
    lib.pgo_download.argtypes = [C.c_void_p, C.c_void_p]
    lib.pgo_destroy.restype, lib.pgo_destroy.argtypes = None, [C.c_void_p]
    return lib


@pytest.mark.parametrize("name", sr.NAMES)
def test_restatement_agrees_with_the_oracle(oracle, name):
    sh = sr.make(name, n_cu=256)
    want = sr.restate(sh)
    assert sh.N <= 145_000
    ctx = C.c_void_p()
    assert oracle.pgo_create(C.byref(ctx), C.byref(sh.c), C.byref(sh.par)) == 0
    try:
        assert oracle.pgo_begin(ctx) == 0
        flags, pos_x, pos_y = np.full(sh.N, 0xffffffff, np.uint32), np.full(sh.N, -1, np.int32), np.full(sh.N, -1, np.int32)
        st = sr.HitState(flags=flags.ctypes.data, pos_x=pos_x.ctypes.data, pos_y=pos_y.ctypes.data)
        assert oracle.pgo_download(ctx, C.byref(st)) == 0
    finally:
        oracle.pgo_destroy(ctx)
    assert np.array_equal(pos_x, want["pos_x"])
    assert np.array_equal(pos_y, want["pos_y"])
    rev = np.zeros(sh.N, np.int64)
    rev[sh.goff[want["gnm"]] + want["fidx"]] = want["rev"]  # (the restatement keeps X order, pgo_download gives file order)
    assert np.array_equal(flags & sr.PGA_F_REV, rev)


def test_shards_reach_what_they_are_for():
    """the sizes, key widths and bin cuts the shards exist for, from the shards themselves"""
    sizes = sorted(g.n for g in sr.make("crowd", n_cu=256).genomes)
    for n in (0, 1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 10239, 10240, 10241, 14336, 14337, 25600):
        assert n in sizes
    assert sum(n <= sr.NP_MAX for n in sizes) >= 2 * 256 + 8 and len(sizes) == 2 * 256 + 8 + 6
    assert [g.n for g in sr.make("few").genomes] == [1, 64, 1000, 10240, 14336]
    # (cs, cm, contig) bits: a composite key of exactly 32 bits, the first split key at 33, X split with Y composite and the reverse
    assert [sr.make("widths%d" % k).key_bits for k in range(7)] == [(1, 1, 1), (7, 8, 1), (15, 16, 1), (31, 31, 1), (31, 30, 2), (30, 31, 2), (23, 24, 9)]
    for k in range(7):  # the declared maxima are reached to within 3, and both ends of the contig range are used
        sh = sr.make("widths%d" % k)
        n_ctg, max_cs, max_cm = sr.WIDTHS[k]
        for g in sh.genomes:
            assert g.cs.max() >= max_cs - 3 and g.cm.max() >= max_cm - 3 and g.cid.min() == 0 and g.cid.max() == n_ctg - 1 and (g.ce >= g.cs).all()
    b = sr.make("bins")
    assert np.bincount(b.genomes[0].cid, minlength=9).tolist() == sr.BIN_SIZES and [g.n for g in b.genomes[1:]] == [100, 0]
    o = sr.make("over")
    assert [g.n for g in o.genomes] == [25601, 30000] and np.bincount(o.genomes[1].cid).tolist() == [15000, 15000]
    m = sr.make("manyctg").genomes[0]
    per = np.bincount(m.cid, minlength=m.n_ctg)
    assert m.n == 5000 and m.n_ctg == 300 and per.max() == 200 and (per == 0).sum() >= 40
