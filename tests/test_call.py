"""`pangene call` (pangene.js call, version 1.1-r231) through the checker build: the host driver linked against the oracle backend, whose
table has no call_bubbles entry, so the walk side runs as the plain host loops of call.cpp.  Every fixture x option set must print the
bytes pangene.js printed when tests/golden/make_call_outputs.py recorded it (tests/golden/call/outputs.json)."""
import hashlib
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CLI = os.path.join(ROOT, "tests", "_build", "pangene_oraclehost")
SHIM = os.path.join(ROOT, "tests", "support", "k8_shim.js")
sys.path.insert(0, os.path.join(GOLD))
import make_call_outputs as mco  # noqa: E402

with open(os.path.join(GOLD, "call", "outputs.json")) as _f:
    REC = json.load(_f)
CALL_CASES = [c for c in mco.cases() if c[1] == "call"]


def run_cli(exe, args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)
    return r.returncode, r.stdout, r.stderr


def check(key, rc, out):
    want = REC[key]
    assert (0 if rc == 0 else 1) == want["rc"], key
    assert len(out) == want["bytes"] and hashlib.md5(out).hexdigest() == want["md5"], key


@pytest.mark.parametrize("key,cmd,fixture,opts", CALL_CASES, ids=[c[0] for c in CALL_CASES])
def test_call_equals_script(built, key, cmd, fixture, opts):
    rc, out, _ = run_cli(CLI, ["call"] + mco.abs_args(opts) + [os.path.join(GOLD, fixture)])
    check(key, rc, out)


def test_links_listed_one_way_fail_like_the_script(built):
    """pangene.js follows links forward only when it groups segment ends, and throws "Wrong!" on such a GFA (the reference's own
    test/bubble graphs): a non-zero exit, one line on stderr, nothing on stdout"""
    rc, out, err = run_cli(CLI, ["call", os.path.join(GOLD, "bubble", "t2-1.gfa")])
    assert rc != 0 and out == b"" and err.decode().count("\n") == 1 and "Wrong!" in err.decode()


def test_missing_file_is_an_error(built, tmp_path):
    rc, out, err = run_cli(CLI, ["call", str(tmp_path / "none.gfa")])
    assert rc != 0 and out == b""


def test_usage(built):
    rc, out, _ = run_cli(CLI, ["call"])
    assert rc == 0 and out.startswith(b"Usage: pangene call [options] <in.gfa>\n") and b"-m INT" in out


def test_configs1_graph(built, tmp_path):
    """BASELINE configs[1] (synth.bact(100, 5000), seed 1): the checker writes the graph the reference writes, and `call` on it prints
    what the script printed (default, -p, -w)"""
    sys.path.insert(0, ROOT)
    from pangene_amd import synth
    files = synth.write_files(synth.bact(100, 5000, seed=1), str(tmp_path / "c1"))
    gfa = tmp_path / "c1.gfa"
    rc, out, _ = run_cli(CLI, files)
    assert rc == 0
    check("configs1:gfa", 0, out)
    gfa.write_bytes(out)
    for o in ("", "-p", "-w"):
        rc, out, _ = run_cli(CLI, ["call"] + o.split() + [str(gfa)])
        check("call:configs1|%s" % o, rc, out)


def test_in_memory_route_equals_file_route(built, tmp_path):
    """`pangene --call *.paf` (pg_write_call on the graph in memory) prints what `pangene *.paf > g.gfa; pangene call g.gfa` prints"""
    c4 = sorted(os.path.join(GOLD, "C4", f) for f in os.listdir(os.path.join(GOLD, "C4")))
    rc, gfa, _ = run_cli(CLI, c4)
    assert rc == 0
    (tmp_path / "g.gfa").write_bytes(gfa)
    rc1, a, _ = run_cli(CLI, ["--call"] + c4)
    rc2, b, _ = run_cli(CLI, ["call", str(tmp_path / "g.gfa")])
    assert rc1 == 0 and rc2 == 0 and a == b and b.count(b"\nAL\t") == 9


JS = os.environ.get("PANGENE_JS")  # path of pangene.js (version 1.1-r231) to check the recording against, when node is there too


@pytest.mark.skipif(not (JS and os.path.exists(JS) and shutil.which("node")), reason="PANGENE_JS and node are needed to re-run the script")
@pytest.mark.parametrize("case", [c for c in mco.cases() if "/" in c[2] or c[2].startswith("C4")], ids=lambda c: c[0])
def test_recording_still_holds(case):
    key, cmd, fixture, opts = case
    rc, out = mco.run_script(JS, cmd, os.path.join(GOLD, fixture), opts)
    check(key, rc, out)
