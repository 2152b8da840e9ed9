#!/usr/bin/env python3
"""Records tests/golden/call/outputs.json: what pangene.js itself (version 1.1-r231, run under node through tests/support/k8_shim.js)
prints for `call` on every fixture x option set, and for `gfa2matrix` on the gfa2matrix fixtures.  Keys are "<command>:<fixture>|<options>";
values {"rc": 0 or 1, "md5", "bytes"} of stdout.  tests/test_call.py, tests/test_call_gpu.py and tests/test_gfa2matrix_script.py compare
against it, so the script is needed only to record (and, where it is present, to check that the recording still holds).

    python3 tests/golden/make_call_outputs.py /path/to/pangene.js [/path/to/pangene_ref]

The configs[1] graph (synth.bact(100, 5000), seed 1) is written by the reference binary when its path is given, else by the
`pangene` command line of this repository (byte-identical to the reference's)."""
import glob, gzip, hashlib, json, os, subprocess, sys, tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SHIM = os.path.join(ROOT, "tests", "support", "k8_shim.js")
OUT = os.path.join(HERE, "call", "outputs.json")

# option sets of `call`: the default report, the PST route, walks ignored, the super node, the -m cut-off, the debugging outputs
CALL_OPTS = ["", "-p", "-w", "-p -s", "-m 1", "-m 3 -p", "-b", "-e", "-d", "-p -s -w"]
HAND_OPTS = CALL_OPTS + ["-p -s -r A#1", "-m 2 -p"]
MATRIX = [("bubble/t1-8c.walks.gfa", ""), ("bubble/t1-8c.walks.gfa", "-c"), ("bubble/t1-8c.walks.gfa", "-d bubble/t1-8c.clstr"),
          ("bubble/t1-8c.walks.gfa", "-c -d bubble/t1-8c.clstr"), ("bubble/t1-8c.walks.gfa", "-p -d bubble/t1-8c.clstr"),
          ("C4.gfa.gz", ""), ("C4.gfa.gz", "-c"), ("bubble/t1-1.gfa", ""), ("bubble/intkeys.gfa", "-c -d bubble/intkeys.clstr")]


def pangene_fixtures():
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(HERE, "*.gfa.gz")))


def hand_fixtures():
    return ["call/" + os.path.basename(p) for p in sorted(glob.glob(os.path.join(HERE, "call", "*.gfa")))]


def cases():
    """(key, command, fixture path relative to tests/golden, option list)"""
    out = []
    for f in pangene_fixtures():
        for o in CALL_OPTS:
            out.append(("call:%s|%s" % (f, o), "call", f, o.split()))
    for f in hand_fixtures():
        for o in HAND_OPTS:
            out.append(("call:%s|%s" % (f, o), "call", f, o.split()))
    out.append(("call:bubble/t2-1.gfa|", "call", "bubble/t2-1.gfa", []))  # links listed one way only: the script stops with "Wrong!"
    for f, o in MATRIX:
        out.append(("gfa2matrix:%s|%s" % (f, o), "gfa2matrix", f, o.split()))
    return out


def abs_args(opts):
    return [os.path.join(HERE, a) if a.startswith("bubble/") else a for a in opts]


def run_script(js, cmd, path, opts):
    r = subprocess.run(["node", SHIM, js, cmd] + abs_args(opts) + [path], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return (0 if r.returncode == 0 else 1), r.stdout


def entry(rc, out):
    return {"rc": rc, "md5": hashlib.md5(out).hexdigest(), "bytes": len(out)}


def configs1_gfa(td, ref_bin):
    sys.path.insert(0, ROOT)
    from pangene_amd import synth
    files = synth.write_files(synth.bact(100, 5000, seed=1), os.path.join(td, "c1"))
    exe = ref_bin or os.path.join(ROOT, "pangene_amd", "bin", "pangene")
    gfa = os.path.join(td, "configs1.gfa")
    with open(gfa, "wb") as f:
        subprocess.run([exe] + files, stdout=f, stderr=subprocess.DEVNULL, check=True)
    return gfa


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    js = sys.argv[1]
    ref_bin = sys.argv[2] if len(sys.argv) > 2 else None
    rec = {}
    for key, cmd, f, opts in cases():
        rc, out = run_script(js, cmd, os.path.join(HERE, f), opts)
        rec[key] = entry(rc, out)
    with tempfile.TemporaryDirectory() as td:
        gfa = configs1_gfa(td, ref_bin)
        rec["configs1:gfa"] = entry(0, open(gfa, "rb").read())
        for o in ("", "-p", "-w"):
            rc, out = run_script(js, "call", gfa, o.split())
            rec["call:configs1|%s" % o] = entry(rc, out)
    with open(OUT, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d recordings -> %s" % (len(rec), OUT))


if __name__ == "__main__":
    main()
