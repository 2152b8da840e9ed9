"""`pangene call` / `pangene --call` on the MI355X: the walk side runs as the HIP kernels of k_call.hpp (pga_call_bubbles).  The product
command line must print what pangene.js printed (tests/golden/call/outputs.json), the in-memory route what the file route prints, and
on inputs too large for the script the product must print what the checker build prints (oracle backend: no call_bubbles entry, so
the host loops of call.cpp -- a second implementation)."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HIP = os.path.join(ROOT, "pangene_amd", "bin", "pangene")
ORA = os.path.join(ROOT, "tests", "_build", "pangene_oraclehost")
DIRECT = os.path.join(ROOT, "tests", "support", "call_direct.py")
sys.path.insert(0, GOLD)
sys.path.insert(0, ROOT)
import make_call_outputs as mco  # noqa: E402

pytestmark = pytest.mark.gpu
with open(os.path.join(GOLD, "call", "outputs.json")) as _f:
    REC = json.load(_f)
CALL_CASES = [c for c in mco.cases() if c[1] == "call"]


def run(exe, args, env=None, timeout=900):
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=timeout)
    if r.returncode < 0 or r.stderr.strip():
        sys.stderr.write("%s: exit %d, stderr: %s\n" % (" ".join(args[:4]), r.returncode, r.stderr.decode(errors="replace")[-2000:]))
    return r.returncode, r.stdout


def check(key, rc, out):
    want = REC[key]
    assert (0 if rc == 0 else 1) == want["rc"], "%s: exit %d" % (key, rc)
    assert len(out) == want["bytes"] and hashlib.md5(out).hexdigest() == want["md5"], key


@pytest.mark.parametrize("key,cmd,fixture,opts", CALL_CASES, ids=[c[0] for c in CALL_CASES])
def test_call_equals_script(built, key, cmd, fixture, opts):
    rc, out = run(HIP, ["call"] + mco.abs_args(opts) + [os.path.join(GOLD, fixture)])
    check(key, rc, out)


@pytest.mark.parametrize("fixture", ["C4.gfa.gz", "human8.gfa.gz", "bact20.gfa.gz", "call/nested.gfa", "call/equal.gfa"])
@pytest.mark.parametrize("opts", ["", "-p"])
def test_forced_hash_collisions_keep_alleles_apart(built, fixture, opts):
    """PANGENE_CALL_HASH_BITS=1: the allele hash keeps one bit, so nearly every two paths of a bubble collide; the element-by-element
    comparison must still keep them apart"""
    rc, out = run(HIP, ["call"] + opts.split() + [os.path.join(GOLD, fixture)], env={"PANGENE_CALL_HASH_BITS": "1"})
    check("call:%s|%s" % (fixture, opts), rc, out)


def _paf_dir(name):
    d = os.path.join(GOLD, name)
    return sorted(os.path.join(d, f) for f in os.listdir(d))


@pytest.mark.parametrize("name", ["C4", "bact20", "human8f"])
def test_in_memory_route(built, tmp_path, name):
    files = _paf_dir(name)
    rc, gfa = run(HIP, files)
    assert rc == 0
    (tmp_path / "g.gfa").write_bytes(gfa)
    rc1, a = run(HIP, ["--call"] + files)
    rc2, b = run(HIP, ["call", str(tmp_path / "g.gfa")])
    assert rc1 == 0 and rc2 == 0 and a == b and a.startswith(b"CC\t")
    rc3, c = run(ORA, ["--call"] + files)
    assert rc3 == 0 and c == a


def test_configs1(built, tmp_path):
    from pangene_amd import synth
    files = synth.write_files(synth.bact(100, 5000, seed=1), str(tmp_path / "c1"))
    rc, gfa = run(HIP, files)
    check("configs1:gfa", rc, gfa)
    (tmp_path / "c1.gfa").write_bytes(gfa)
    for o in ("", "-p", "-w"):
        rc, out = run(HIP, ["call"] + o.split() + [str(tmp_path / "c1.gfa")])
        check("call:configs1|%s" % o, rc, out)
    rc, out = run(HIP, ["--call"] + files)
    check("call:configs1|", rc, out)


def _device_vs_host(tmp_path, files, opts_list=("", "-p", "-m 1000 -p")):
    rc, gfa = run(HIP, files)
    assert rc == 0 and gfa.count(b"\nW\t") > 0
    g = tmp_path / "g.gfa"
    g.write_bytes(gfa)
    for o in opts_list:
        rc1, a = run(HIP, ["call"] + o.split() + [str(g)])
        rc2, b = run(ORA, ["call"] + o.split() + [str(g)])
        assert rc1 == 0 and rc2 == 0 and a == b, o
    rc1, a = run(HIP, ["--call"] + files)
    rc2, b = run(ORA, ["call", str(g)])
    assert rc1 == 0 and a == b


def test_device_equals_host_configs3_shard(built, tmp_path):
    """1 250 bacterial genomes x 5 000 proteins: the per-GPU shard of configs[3] (about 5.8 M walk steps)"""
    from pangene_amd import synth
    files = synth.write_files(synth.bact(1250, 5000, seed=1), str(tmp_path / "big"))
    _device_vs_host(tmp_path, files, ("", "-p"))


def test_device_equals_host_human(built, tmp_path):
    from pangene_amd import synth
    files = synth.write_files(synth.human(47, 20000, seed=1), str(tmp_path / "h"))
    _device_vs_host(tmp_path, files)


@pytest.mark.parametrize("seed", [3, 8, 21])
def test_device_equals_host_fuzz(built, tmp_path, seed):
    from pangene_amd import synth
    files = synth.write_files(synth.fuzz(seed, harsh=bool(seed & 1)), str(tmp_path / "f"))
    _device_vs_host(tmp_path, files)


@pytest.mark.parametrize("seed", [1, 2])
def test_device_equals_host_mutated(built, tmp_path, seed):
    from pangene_amd import synth
    files = synth.write_files(synth.mutate(synth.bact(16, 500, seed=seed), seed=seed), str(tmp_path / "m"))
    _device_vs_host(tmp_path, files)


@pytest.mark.parametrize("hash_bits", [None, "1", "8"], ids=["hash32", "hash1", "hash8"])
@pytest.mark.parametrize("which", ["exhaustive", "edges", "pileup", "graphlike"])
def test_direct_cases(built, which, hash_bits):
    """pga_call_bubbles on walks and bubbles no GFA reaches, all six output arrays equal to the plain restatement
    (tests/support/call_direct.py, call_cases.py, call_ref.py): every walk of 1 .. 4 steps over 4 vertices against every bubble,
    hairpins (ve == vs ^ 1), duplicated and skipped bubbles among them (exhaustive); 2 n_seg, n_walk, N and n_bub around the steps of
    the key widths, a radix tile and the scans, empty walks first, last and in the middle, 8 bubbles on one end vertex, inputs
    without a record, a step or a live bubble (edges); 20 200 records and 1.3 M interior steps from 400 steps, so that the sort
    buffers grow twice, and 100 alleles a bubble behind a hash of 1 or 8 bits (pileup); 2 000 noisy walks, 3 000 bubbles (graphlike).
    The expected arrays do not depend on PANGENE_CALL_HASH_BITS."""
    env = {k: v for k, v in os.environ.items() if k != "PANGENE_CALL_HASH_BITS"}
    if hash_bits is not None:
        env["PANGENE_CALL_HASH_BITS"] = hash_bits
    r = subprocess.run([sys.executable, DIRECT, which], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600, cwd=ROOT, env=env)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and out.rstrip().endswith("ALL OK"), out[-3000:]


def test_direct_refusals(built):
    """a step or a bubble vertex outside [0, 2 n_seg) is PGA_ERR_ARG, a negative n_walk PGA_ERR_RANGE, each found before any device
    work, and the good call straight afterwards is still right (tests/support/call_direct.py refusals)"""
    r = subprocess.run([sys.executable, DIRECT, "refusals"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600, cwd=ROOT)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and out.rstrip().endswith("ALL OK"), out[-3000:]
