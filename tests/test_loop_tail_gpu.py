"""The end of a run whose branch rounds were queued to the end (pga_branch_loop with final_on): PG_SET_FILTER(shadow) and the written
graph's arc table in its final form are queued behind the last arc round, in front of the loop's one wait (k_arc_final, pga_final_arcs).
Every route must give the reference's bytes, the fallbacks must be taken when they should, and the table the device writes must be
the table the host driver's own conversion writes, byte for byte."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden_files
from pangene_amd import capi

pytestmark = pytest.mark.gpu

_RUN = os.path.join(ROOT, "tests", "support", "loop_tail_run.py")


_LANDED = b"[fetch_arcs] the loop left the final table"  # (PANGENE_TIMING=1: the driver says when it took the table pga_final_arcs handed out)


def _run(tmp_path, tag, env, variant, files, exact=2):
    """-> (info, gfa bytes, arc bytes, seg bytes) of one run in a process of its own; info["landed"]: the short route was taken"""
    prefix = str(tmp_path / tag)
    r = subprocess.run([sys.executable, _RUN, prefix, variant] + files, env=dict(os.environ, PANGENE_TIMING="1", LOOP_TAIL_EXACT=str(exact), **env),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    info = json.loads(r.stdout.decode().strip().splitlines()[-1])
    info["landed"] = _LANDED in r.stderr
    return info, open(prefix + ".gfa", "rb").read(), open(prefix + ".arc", "rb").read(), open(prefix + ".seg", "rb").read()


_CASES = [("bact20", ""), ("bact20", "-a2"), ("bact20", "-T 3"), ("bact20", "-G"), ("bact20", "-c 3 -g 6"), ("human8f", "-p0 -a1"), ("fuzz3", "-S"), ("manydoms", "-G"),
          ("fuzz7126", "-D 300 -C 2"), ("wide0", ""), ("wide1", ""), ("wide2", ""), ("wide3", "")]
_ROUTES = [{"PANGENE_LOOP": "notail"}, {"PANGENE_LOOP_RIDE": "0"}, {"PANGENE_LOOP_RIDE": "1"}, {}]


@pytest.mark.parametrize("env", _ROUTES, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()) or "default")
@pytest.mark.parametrize("name,variant", _CASES)
def test_both_routes_give_the_reference_bytes(built, expected, tmp_path, name, variant, env):
    """The tail queued inside the loop (default) and behind it (PANGENE_LOOP=notail), nothing / the ranks / the ranks and the records of the next
    pg_gen_rep_pos riding with the arc rounds (PANGENE_LOOP_RIDE=0 / 1 / default), exact mode 2, against the recorded md5 of the reference.
    The wide fixtures hold arcs whose averaged distance does not fit 32 bits: the edge of the device's avg_dist conversion; with -c 3 -g 6
    bact20 loses 210 of its 490 segments inside the rounds, so the table's segments are renumbered."""
    info, gfa, _, _ = _run(tmp_path, "r", env, variant, golden_files(name))
    assert hashlib.md5(gfa).hexdigest() == expected[name][variant]["md5"]


@pytest.mark.parametrize("env", [{"PANGENE_FINAL_ARCS_CAP": "4"}, {"PANGENE_LOOP_PAIR_CAP": "8"}, {"PANGENE_GENE_TABLE_LOG2": "2"}, {"PANGENE_LOOP": "noskip"},
                                 {"PANGENE_LIVE_LISTS": "2"}, {"PANGENE_RANK": "scan"}], ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
@pytest.mark.parametrize("name,variant", [("bact20", ""), ("human8f", "-p0 -a1")])
def test_fallbacks_and_repeats(built, expected, tmp_path, name, variant, env):
    """A landing area of four records (the table never fits: the general route); a pair list beyond its room (status 4: the queue runs twice,
    and so does its tail); a four-entry gene table (RC_REDO after the tail was queued: the repeated run is host-driven); every round run in
    full; lists rebuilt inside the loop; the ranks by the general scan."""
    info, gfa, _, _ = _run(tmp_path, "f", env, variant, golden_files(name))
    assert hashlib.md5(gfa).hexdigest() == expected[name][variant]["md5"]


def test_capacity_at_and_around_the_table_size(built, expected, tmp_path):
    """bact20 with a landing area of exactly n_arc, n_arc + 1 and n_arc - 1 records, in exact mode 2 (against the reference's md5) and in mode 1 (where
    the rounds of this set are queued to the end whenever the tie orders allow it).  Where the default run takes the short route, a table that
    fits lands -- two host waits fewer than the general route: arc_table's and the copy's -- and one record too few leaves only the size and
    the general route runs; the bytes are the same every time."""
    files, want = golden_files("bact20"), expected["bact20"][""]["md5"]
    can_land = 0
    for exact in (2, 1):
        base, gfa0, arc0, seg0 = _run(tmp_path, "n%d" % exact, {"PANGENE_LOOP": "notail"}, "", files, exact)
        assert not base["landed"]
        if exact == 2:
            assert hashlib.md5(gfa0).hexdigest() == want
        probe, _, _, _ = _run(tmp_path, "p%d" % exact, {}, "", files, exact)
        can_land += probe["landed"]
        n_arc = base["n_arc"]
        assert n_arc > 8
        for cap in (n_arc, n_arc + 1, n_arc - 1):
            info, gfa, arc, seg = _run(tmp_path, "c%d_%d" % (exact, cap), {"PANGENE_FINAL_ARCS_CAP": str(cap)}, "", files, exact)
            print("exact", exact, "cap", cap, info, "base", base)
            assert gfa == gfa0 and arc == arc0 and seg == seg0, (exact, cap)
            assert info["landed"] == (probe["landed"] and cap >= n_arc), (exact, cap, info)
            assert info["waits"] == base["waits"] - (2 if info["landed"] else 0), (exact, cap, info, base)
    assert can_land >= 1  # otherwise nothing above was about the landing area


def test_the_table_itself(built, expected, tmp_path):
    """q->arc[0..n_arc) and q->seg[0..n_seg) through the C ABI: the default route against PANGENE_LOOP=notail, byte for byte, on bact20 and
    human8f (exact mode 2 and mode 1, with the default limits and with limits under which pg_flt_high_occ deletes segments in the rounds) and
    on a small synthetic bacterial set.  Where the default run takes the short route it has two host waits fewer.  On at least one set
    that takes it the loop must delete a segment -- n_seg below the number of vertices the loop was entered with, which a run with limits
    nothing reaches shows (bact20 -c 3 -g 6: 280 of 490 left) -- so that the renumbering on the device is not the identity."""
    from pangene_amd import synth
    bact, human = golden_files("bact20"), golden_files("human8f")
    sets = [("bact20", bact, "", 1), ("bact20", bact, "-c 3 -g 6", 2), ("bact20", bact, "-c 3 -g 6", 1), ("human8f", human, "", 2), ("human8f", human, "-c 2 -g 4 -r 1", 1),
            ("synth", synth.write_files(synth.bact(8, 300, seed=7), str(tmp_path / "synth")), "", 1)]
    arc_dt = np.dtype([("x", "<u8"), ("n_genome", "<i4"), ("tot_cnt", "<i4"), ("avg_dist", "<i4"), ("s1", "<i4"), ("s2", "<i4"), ("bits", "<u4")])
    landed = shrinks = 0
    for k, (name, files, variant, exact) in enumerate(sets):
        a, gfa_a, arc_a, seg_a = _run(tmp_path, "a%d" % k, {}, variant, files, exact)
        b, gfa_b, arc_b, seg_b = _run(tmp_path, "b%d" % k, {"PANGENE_LOOP": "notail"}, variant, files, exact)
        full, _, _, _ = _run(tmp_path, "v%d" % k, {"PANGENE_LOOP": "notail"}, "-c 100000 -g 100000 -r 100000", files, exact)
        print(name, repr(variant), "exact", exact, "default", a, "notail", b, "vertices", full["n_seg"])
        assert not b["landed"]
        if exact == 2 and variant in expected[name]:
            assert hashlib.md5(gfa_a).hexdigest() == expected[name][variant]["md5"]
        assert a["n_arc"] == b["n_arc"] > 0 and a["n_seg"] == b["n_seg"] > 0
        assert len(arc_a) == 32 * a["n_arc"] and arc_a == arc_b, (name, variant)
        assert seg_a == seg_b and gfa_a == gfa_b, (name, variant)
        assert a["waits"] == b["waits"] - (2 if a["landed"] else 0), (name, variant, exact, a, b)
        arc = np.frombuffer(arc_a, dtype=arc_dt)
        assert int((arc["x"] >> np.uint64(33)).max()) < a["n_seg"] and int(((arc["x"] & np.uint64(0xffffffff)) >> np.uint64(1)).max()) < a["n_seg"]
        assert not arc["bits"].any()
        landed += a["landed"]
        shrinks += a["landed"] and full["n_seg"] > a["n_seg"]
    assert landed >= 1 and shrinks >= 1


def _host_avg_dist(sum_dist, tot_cnt):
    """(int32_t)(int64_t)((double)(int64_t)sum_dist / tot_cnt + .499) as an x86-64 build computes it: the 64-bit conversion truncates and
    gives 0x8000000000000000 for whatever does not fit, the narrowing keeps the low word"""
    sd = sum_dist - (1 << 64) if sum_dist >= (1 << 63) else sum_dist
    v = float(sd) / tot_cnt + .499
    i = int(v) if -2.0 ** 63 <= v < 2.0 ** 63 else -(1 << 63)
    lo = i & 0xffffffff
    return lo - (1 << 32) if lo >= (1 << 31) else lo


def _host_i32(v):
    """(int32_t)double as an x86-64 build computes it"""
    return int(v) if -2147483649.0 < v < 2147483648.0 else -(1 << 31)


def _compiled_host_expression(tmp_path, cases):
    """the same from the host driver's own C expression, compiled here; None where there is no compiler or the machine is not x86-64"""
    import platform
    import shutil
    if platform.machine() not in ("x86_64", "AMD64") or shutil.which("gcc") is None:
        return None
    src = ("#include <stdio.h>\n#include <stdint.h>\nint main(void){unsigned long long sd; int tc;\n"
           "while (scanf(\"%llu %d\", &sd, &tc) == 2) { volatile double q = (double)(int64_t)(uint64_t)sd / tc + .499; printf(\"%d\\n\", (int32_t)(int64_t)q); }\nreturn 0;}\n")
    c, exe = str(tmp_path / "h.c"), str(tmp_path / "h")
    open(c, "w").write(src)
    subprocess.run(["gcc", "-O0", "-ffp-contract=off", c, "-o", exe], check=True)
    out = subprocess.run([exe], input="".join("%d %d\n" % sc for sc in cases).encode(), stdout=subprocess.PIPE, check=True).stdout
    return [int(x) for x in out.split()]


def test_the_conversions_on_the_device(built, tmp_path):
    """cvt_i64lo_x86 / cvt_i32_x86 as k_arc_final applies them (pga_selftest_arc_final) against the host expression: quotients at +-2^31
    and +-2^63 and just inside them, tot_cnt = 1, negative sums (the sum is a uint64_t that holds sign-extended distances), values whose
    fraction sits on either side of the .499 that is added, and a few thousand random sums."""
    rng = np.random.default_rng(5)
    cases = []
    for q in (1 << 31, (1 << 31) - 1, (1 << 31) + 1, 1 << 32, (1 << 32) - 1, (1 << 62), (1 << 63) - 1, (1 << 63) - 1024, (1 << 63) - 1025, (1 << 63) - 512, 0, 1, 7):
        for tc in (1, 2, 3, 7, 1000):
            for sgn in (1, -1):
                sd = sgn * q if q * tc >= (1 << 63) else sgn * q * tc
                cases.append((sd & ((1 << 64) - 1), tc))
    cases += [((1 << 63), 1), ((1 << 63), 2), ((1 << 64) - 1, 1), (((-(1 << 31)) * 3) & ((1 << 64) - 1), 3), (((-(1 << 31)) * 3 - 1) & ((1 << 64) - 1), 3)]
    for tc in (2, 1000, 1002, 499, 998, 2000):  # fractions k / tc around .501: q + .499 crosses the next integer between them
        for k in range(max(0, tc // 2 - 2), min(tc, tc // 2 + 4)):
            for base in (0, 5, (1 << 31) - 1, -(1 << 31) - 1, -7):
                cases.append(((base * tc + k) & ((1 << 64) - 1), tc))
                cases.append(((base * tc - k) & ((1 << 64) - 1), tc))
    for tc in (1, 3, 20, 100):
        cases += [(int(v), tc) for v in rng.integers(0, 1 << 63, size=500, dtype=np.uint64) * np.uint64(2) + np.uint64(1)]
        cases += [(int(v) & ((1 << 64) - 1), tc) for v in rng.integers(-(1 << 40), 1 << 40, size=500)]
    n = len(cases)
    rec = np.zeros(n, dtype=np.dtype([("x", "<u8"), ("n_genome", "<i4"), ("tot_cnt", "<i4"), ("sum_dist", "<u8"), ("sum_s1", "<i8"), ("sum_s2", "<i8")]))
    assert rec.dtype.itemsize == 40
    rec["sum_dist"] = np.array([c[0] for c in cases], dtype=np.uint64)
    rec["tot_cnt"] = [c[1] for c in cases]
    rec["n_genome"] = [c[1] for c in cases]
    s1 = rng.integers(-(1 << 40), 1 << 40, size=n)
    s1[:6] = [(1 << 31) * 3, (1 << 31) * 3 - 2, -(1 << 31) * 3, -(1 << 31) * 3 - 3, 0, 1]
    rec["sum_s1"], rec["sum_s2"] = s1, s1[::-1]
    rec["n_genome"][:6] = 3
    out = np.zeros((n, 4), dtype=np.int32)
    raw = C.CDLL(capi.LIB_HIP)
    assert raw.pga_selftest_arc_final(rec.ctypes.data_as(C.c_void_p), C.c_int64(n), out.ctypes.data_as(C.c_void_p)) == 0
    want = [_host_avg_dist(sd, tc) for sd, tc in cases]
    compiled = _compiled_host_expression(tmp_path, cases)
    if compiled is not None:
        assert compiled == want  # the restatement above is what the compiler makes of the driver's expression
    bad = [(cases[i], int(out[i, 0]), want[i]) for i in range(n) if int(out[i, 0]) != want[i]]
    assert not bad, bad[:5]
    for col, key in ((1, "sum_s1"), (2, "sum_s2")):
        w = [_host_i32(float(int(rec[key][i])) / int(rec["n_genome"][i]) + .499) for i in range(n)]
        assert out[:, col].tolist() == w
    assert not out[:, 3].any()
