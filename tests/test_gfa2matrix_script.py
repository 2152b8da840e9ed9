"""f4 `gfa2matrix` against pangene.js itself (pangene.js:1168-1247, run under node through tests/support/k8_shim.js and recorded by
tests/golden/make_call_outputs.py): pg_gfa2matrix_file of the checker build must print the script's bytes."""
import ctypes as C
import hashlib
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLD)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_call_outputs as mco  # noqa: E402
import oracle_host  # noqa: E402

with open(os.path.join(GOLD, "call", "outputs.json")) as _f:
    REC = json.load(_f)
CASES = [c for c in mco.cases() if c[1] == "gfa2matrix"]


@pytest.fixture(scope="module")
def lib(built):
    lib = oracle_host.load()
    C.c_int.in_dll(lib, "pg_verbose").value = 0
    return lib


@pytest.mark.parametrize("key,cmd,fixture,opts", CASES, ids=[c[0] for c in CASES])
def test_gfa2matrix_equals_script(lib, tmp_path, key, cmd, fixture, opts):
    it = iter(mco.abs_args(opts))
    cn, clstr, print_cd = 0, None, 0
    for a in it:
        if a == "-c": cn = 1
        elif a == "-p": print_cd = 1
        elif a == "-d": clstr = next(it).encode()
    out = tmp_path / "m.txt"
    lib.pg_set_output(str(out).encode())
    rc = lib.pg_gfa2matrix_file(os.path.join(GOLD, fixture).encode(), cn, clstr, print_cd)
    lib.pg_set_output(None)
    got = out.read_bytes() if out.exists() else b""
    want = REC[key]
    assert rc == 0 and want["rc"] == 0
    assert hashlib.md5(got).hexdigest() == want["md5"] and len(got) == want["bytes"]
