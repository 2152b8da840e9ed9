"""Pins the oracle (and the host driver, reader and writers around it) to the reference.

Every (fixture set, option variant) in tests/golden/expected.json holds the md5 of what the untouched
reference prints (tests/golden/make_golden.py).  The host driver + plain-C oracle backend must print the
same bytes.  With PANGENE_EXACT=all the reference's unstable-sort order is replayed for every contig, so
even --bed line order is identical; the default (auto) only replays the index-0 channel and must still give
identical GFA on every non-adversarial set.
"""
import ctypes as C
import hashlib
import os
import subprocess

import pytest

from conftest import ROOT, all_cases, golden_files, reference_output
import oracle_host  # tests/oracle_host.py: the checker build of the host driver
from pangene_amd import capi, synth


@pytest.fixture(scope="module")
def ora(built):
    lib = oracle_host.load()
    C.c_int.in_dll(lib, "pg_verbose").value = 0
    return lib


def _md5(b):
    return hashlib.md5(b).hexdigest()


@pytest.mark.parametrize("name,variant", all_cases())
def test_exact_mode_all_is_byte_identical(ora, expected, name, variant):
    ora.pg_set_exact_mode(2)
    out = capi.run(ora, golden_files(name), variant.split())
    assert len(out) == expected[name][variant]["bytes"]
    assert _md5(out) == expected[name][variant]["md5"]



@pytest.mark.parametrize("name,variant", all_cases())
def test_default_mode_auto(ora, expected, name, variant):
    ora.pg_set_exact_mode(1)
    out = capi.run(ora, golden_files(name), variant.split())
    e = expected[name][variant]
    # tie channels other than array index 0 are detected on the backend and make the driver repeat
    # the run in mode 'all' (e.g. fuzz4 -S), so the default mode is byte-identical on the adversarial sets too
    if "md5_sorted" in e:  # --bed: line order is the unstable sort's; compare as a set of lines
        assert hashlib.md5(b"\n".join(sorted(out.split(b"\n")))).hexdigest() == e["md5_sorted"]
    else:
        assert _md5(out) == e["md5"]


def test_c4_md5_is_the_surveyed_one(expected):
    assert expected["C4"][""]["md5"] == "518822a3debc3e12a4f908cfc123c9e5"


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_live_against_reference_binary(ora, tmp_path, seed):
    """Fresh seeds against the reference's output (recorded in tests/golden/reference_outputs.json; oracle/_ref runs too where built)."""
    files = synth.write_files(synth.bact(12, 400, seed=seed), str(tmp_path / "b"))
    files2 = synth.write_files(synth.fuzz(seed, harsh=bool(seed & 1)), str(tmp_path / "f"))
    for tag, fs in (("b", files), ("f", files2)):
        for mode, args in ((2, []), (2, ["--bed=flag"]), (1, []), (1, ["-S"])):
            ora.pg_set_exact_mode(mode)
            mine = capi.run(ora, fs, args)
            want = reference_output("live:%s%d|%s" % (tag, seed, " ".join(args)), args, fs)
            assert (_md5(mine), len(mine)) == (want["md5"], want["bytes"])


@pytest.mark.parametrize("first,n,shapes,variants", [
    (7000, 150, (False, True), "dc"),   # the seeds and -D/-C variants of the round-1 review: 147 of these 1200 default-mode runs differed then
    (9000, 160, (False,), "all"), (9160, 160, (True,), "all"),  # fresh seeds, every variant of the sweep
])
def test_fuzz_sweep_default_mode_against_reference_binary(built, first, n, shapes, variants):
    """tests/fuzz_oracle_vs_ref.py as a test: the DEFAULT tie-order mode (auto) must print the reference's bytes on > 300 fresh fuzz
    seeds, including the variants that put pg_n_local's local_dist / local_count boundary inside the fuzz shapes (H2b)."""
    import fuzz_oracle_vs_ref as fz
    vs = [v for v in fz.VARIANTS if "-D" in v] if variants == "dc" else fz.VARIANTS
    tot, bad = fz.sweep(first, n, modes=(1,), variants=vs, shapes=shapes, verbose=False, reference=reference_output)
    assert tot == n * len(shapes) * len(vs) and not bad, bad[:10]


def test_dense_shape_against_reference_binary(ora, tmp_path):
    """giant spanning hit + pile-ups (the shape the GPU sweep sends through its slow list), host driver + oracle vs the reference's output"""
    for tag, fs in (("dense3", synth.write_files(synth.dense(3), str(tmp_path / "d"))), ("manydoms2", synth.write_files(synth.many_doms(2), str(tmp_path / "m")))):
        for mode, args in ((2, []), (2, ["-p0", "-a1"]), (1, []), (1, ["-S"]), (1, ["-G"])):
            ora.pg_set_exact_mode(mode)
            mine = capi.run(ora, fs, args)
            want = reference_output("%s|%s" % (tag, " ".join(args)), args, fs)
            assert (_md5(mine), len(mine)) == (want["md5"], want["bytes"]) and want["bytes"] > 1000


@pytest.mark.parametrize("name", ["C4", "bact20", "human8f", "fuzz3"])
def test_batch_reader_equals_sequential_reader(built, name):
    """pg_read_paf_batch (threads + ordered commit) numbers genes/proteins exactly like per-file pg_read_paf calls."""
    ora = oracle_host.load()
    fs = golden_files(name)
    for args in ([], ["-w"], ["--bed=flag"]):
        assert capi.run(ora, fs, args, batch=True) == capi.run(ora, fs, args, batch=False)


def test_ksort_exact_reproduces_the_reference_radix_sort(tmp_path):
    """pangene_amd/csrc/host/ksort_exact.hpp against the reference's own KRADIX_SORT_INIT instance: the same permutation, ties
    included, on ~1000 random arrays of 1 .. 100 k elements -- against digests of the reference's permutations
    (tests/golden/ksort_reference_digests.txt, `ksort_check record`), and directly where the reference's header is present."""
    sup = os.path.join(ROOT, "tests", "support")
    host = "-I" + os.path.join(ROOT, "pangene_amd", "csrc", "host")
    exe = str(tmp_path / "ksort_check")
    subprocess.run(["g++", "-std=c++17", "-O2", host, os.path.join(sup, "ksort_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, "check", os.path.join(ROOT, "tests", "golden", "ksort_reference_digests.txt")], stdout=subprocess.PIPE)
    assert r.returncode == 0, r.stdout.decode()[-1000:]
    assert b" 0 mismatches" in r.stdout
    import re
    ref_dir = re.search(r"^REF\s*\?=\s*(\S+)", open(os.path.join(ROOT, "oracle", "Makefile")).read(), re.M).group(1)  # where oracle/Makefile finds the reference
    if os.path.exists(os.path.join(ref_dir, "ksort.h")):
        obj, exe = str(tmp_path / "stub.o"), str(tmp_path / "ksort_check_ref")
        subprocess.run(["gcc", "-std=c99", "-O2", "-I" + ref_dir, "-c", os.path.join(sup, "ksort_ref_stub.c"), "-o", obj], check=True)
        subprocess.run(["g++", "-std=c++17", "-O2", "-DKSORT_REF", host, os.path.join(sup, "ksort_check.cpp"), obj, "-o", exe], check=True)
        r = subprocess.run([exe], stdout=subprocess.PIPE)
        assert r.returncode == 0, r.stdout.decode()[-1000:]
        assert b" 0 mismatches" in r.stdout
