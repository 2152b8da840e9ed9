"""Writes tests/golden/cli_transcript.json: what the command line of the analyses (curves, dist, assoc, trait, tree, qtrait, cluster,
permanova, mantel, gainloss, coevo; --matrix and --call beside them) prints, refuses and returns for the command lines listed below, and
what capi.run() gives for the long-option ones.  tests/test_cli_transcript.py replays the same list and compares everything.

    python tests/golden/make_cli_transcript.py            (from a build of the commit whose behaviour is to be kept)

The list is written out by hand on purpose: it is the record of how the options behave, their oddities included, and must not be derived
from the tables of pangene_amd/csrc/cli/main.cpp or pangene_amd/capi.py, which it checks.

Every line runs from the repository root with the checker build (tests/_build/pangene_oraclehost).  In a line, @G is the GFA fixture,
@P the PAF files of tests/golden/C4, @T / @Q the binary / quantitative trait files, @N a file that does not exist.  Recorded per line:
exit status, md5 and length of stdout, stderr without its `[M::` lines (they carry wall times).  Long-option lines (those with @P) also
go through capi.run() on the checker library: the md5 of what it returns, or the exception's type and message."""
import hashlib
import itertools
import json
import os
import shlex
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "cli_transcript.json")
CLI = os.path.join("tests", "_build", "pangene_oraclehost")
G = "tests/golden/C4.gfa.gz"
T = "tests/golden/trait/C4.tsv"
Q = "tests/golden/qtrait/C4.tsv"
N = "tests/golden/trait/no_such_file"

# the thirteen head options, in the order the refusals name them
HEADS = ["--matrix", "--call", "--curves", "--dist", "--assoc", "--trait=@T", "--tree", "--qtrait=@Q", "--cluster=2", "--permanova=@T", "--mantel",
         "--gainloss", "--coevo"]

SUB = """
curves
curves @G
curves -n 3 @G
curves -n 1 @G
curves -n 0 @G
curves -n -2 @G
curves -n x @G
curves -n 3x @G
curves -s 5 @G
curves -s x @G
curves -s -1 @G
curves -n 3 -s 5 @G
curves -z @G
curves -n
dist
dist @G
dist -t adj @G
dist -t gene @G
dist -t x @G
dist -m shared @G
dist -m diff @G
dist -m x @G
dist -p @G
dist -t adj -m diff -p @G
dist -z @G
assoc
assoc @G
assoc -r 0.5 @G
assoc -r 0 @G
assoc -r 1.5 @G
assoc -r -0.1 @G
assoc -r x @G
assoc -r 0.5x @G
assoc -c 1 @G
assoc -c 0 @G
assoc -c x @G
assoc -c 3x @G
assoc -s pos @G
assoc -s neg @G
assoc -s both @G
assoc -s x @G
assoc -x 5 @G
assoc -x 0 @G
assoc -x -1 @G
assoc -x x @G
assoc -r 0.3 -x 2 @G
trait
trait @G
trait -t @T
trait -t @T @G
trait -t @N @G
trait -t @T -n 10 @G
trait -t @T -n 0 @G
trait -t @T -n -1 @G
trait -t @T -n x @G
trait -t @T -n 2147483646x @G
trait -t @T -n 2147483647 @G
trait -t @T -n 10 -s 5 @G
trait -t @T -n 10 -s x @G
trait -t @T -n 10 -c 2 @G
trait -t @T -n 10 -c 0 @G
trait -t @T -n 10 -c x @G
trait -t @T -n 10 -p 0.5 @G
trait -t @T -n 10 -p 0 @G
trait -t @T -n 10 -p -1 @G
trait -t @T -n 10 -p x @G
trait -t @T -n 10 -p nan @G
trait -t @T -n 10 -L nj @G
trait -t @T -n 10 -L upgma @G
trait -t @T -n 10 -L x @G
trait -n 10 -L nj @G
qtrait
qtrait @G
qtrait -t @Q
qtrait -t @Q @G
qtrait -t @N @G
qtrait -t @Q -n 10 @G
qtrait -t @Q -n 0 @G
qtrait -t @Q -n -1 @G
qtrait -t @Q -n x @G
qtrait -t @Q -n 2147483647 @G
qtrait -t @Q -n 10 -s 5 @G
qtrait -t @Q -n 10 -s x @G
qtrait -t @Q -n 10 -c 2 @G
qtrait -t @Q -n 10 -c 0 @G
qtrait -t @Q -n 10 -p 0.5 @G
qtrait -t @Q -n 10 -p -1 @G
qtrait -t @Q -n 10 -p x @G
qtrait -t @Q -L nj @G
tree
tree @G
tree -t adj @G
tree -t x @G
tree -m diff @G
tree -m shared @G
tree -m x @G
tree -a upgma @G
tree -a nj @G
tree -a x @G
tree -b 3 @G
tree -b 0 @G
tree -b -1 @G
tree -b x @G
tree -b 3x @G
tree -b 2147483648 @G
tree -b 3 -s 7 @G
tree -s 7 @G
tree -s -1 @G
tree -s x @G
tree -s 7x @G
tree -s 4294967295 @G
tree -s 4294967296 @G
tree -s 00000000007 @G
cluster
cluster @G
cluster -k 2
cluster -k 2 @G
cluster -k 2-3 @G
cluster -k 3-3 @G
cluster -k 1 @G
cluster -k x @G
cluster -k 3-2 @G
cluster -k 2- @G
cluster -k 2-x @G
cluster -k -2 @G
cluster -k 2-2147483648 @G
cluster -k 40 @G
cluster -k 2 -t adj @G
cluster -k 2 -t x @G
cluster -t x @G
cluster -k 2 -m diff @G
cluster -k 2 -m shared @G
cluster -k 2 -i 5 @G
cluster -k 2 -i 0 @G
cluster -k 2 -i -1 @G
cluster -k 2 -i x @G
cluster -i 5 @G
permanova
permanova @G
permanova -t @T
permanova -t @T @G
permanova -t @N @G
permanova -t @T -T adj @G
permanova -t @T -T x @G
permanova -t @T -m diff @G
permanova -t @T -m shared @G
permanova -t @T -n 10 @G
permanova -t @T -n 0 @G
permanova -t @T -n -1 @G
permanova -t @T -n x @G
permanova -t @T -n 2147483647 @G
permanova -t @T -n 10 -s 5 @G
permanova -t @T -n 10 -s x @G
permanova -T adj @G
mantel
mantel @G
mantel -n 10 @G
mantel -x adj:diff -n 10 @G
mantel -x gene -n 10 @G
mantel -x x:y -n 10 @G
mantel -x gene:shared -n 10 @G
mantel -y gene:diff -n 10 @G
mantel -y x -n 10 @G
mantel -f @T -n 10 @G
mantel -f @N -n 10 @G
mantel -y gene:diff -f @N @G
mantel -f @N -y gene:diff @G
mantel -y x -f @N @G
mantel -n 0 @G
mantel -n -1 @G
mantel -n x @G
mantel -n 2147483647 @G
mantel -n 10 -s 5 @G
mantel -n 10 -s x @G
gainloss
gainloss @G
gainloss -t adj @G
gainloss -t x @G
gainloss -m diff @G
gainloss -m shared @G
gainloss -a nj @G
gainloss -a upgma @G
gainloss -a x @G
gainloss -g 2 @G
gainloss -g 255 @G
gainloss -g 0 @G
gainloss -g 256 @G
gainloss -g x @G
gainloss -l 2 @G
gainloss -l 0 @G
gainloss -l x @G
gainloss -r early @G
gainloss -r late @G
gainloss -r x @G
gainloss -e early @G
gainloss -o node @G
gainloss -o gene @G
gainloss -o x @G
gainloss -c 1 @G
gainloss -c -1 @G
gainloss -c x @G
gainloss -c 2147483648 @G
coevo
coevo @G
coevo -t adj @G
coevo -t x @G
coevo -m diff @G
coevo -m shared @G
coevo -a nj @G
coevo -a x @G
coevo -g 2 @G
coevo -g 0 @G
coevo -g 256 @G
coevo -g x @G
coevo -l 2 @G
coevo -l 0 @G
coevo -l x @G
coevo -e early @G
coevo -e x @G
coevo -r 0.5 @G
coevo -r 1.5 @G
coevo -r x @G
coevo -c 1 @G
coevo -c 0 @G
coevo -c x @G
coevo -c 2147483648 @G
coevo -s pos @G
coevo -s neg @G
coevo -s x @G
coevo -x 5 @G
coevo -x 0 @G
coevo -x -1 @G
coevo -x x @G
coevo -o node @G
"""

LONG = """
@P
-w @P
--matrix @P
--matrix=count @P
--call @P
--call --matrix=count @P
--curves @P
--curves=3 @P
--curves=1 @P
--curves=0 @P
--curves=-2 @P
--curves=x @P
--curves=3x @P
--curves --curves-seed=5 @P
--curves --curves-seed=x @P
--curves --curves-seed=-1 @P
--curves-seed=5 @P
--curves=0 --dist @P
--curves --curves-foo=1 @P
--dist @P
--dist=adj @P
--dist=gene @P
--dist=x @P
--dist=x --dist=adj @P
--dist --dist-metric=shared @P
--dist --dist-metric=diff @P
--dist --dist-metric=x @P
--dist-metric=diff @P
--dist-metric=x @P
--assoc @P
--assoc=0.5 @P
--assoc=0 @P
--assoc=1.5 @P
--assoc=-0.1 @P
--assoc=x @P
--assoc=0.5x @P
--assoc --assoc-min-count=1 @P
--assoc --assoc-min-count=0 @P
--assoc --assoc-min-count=x @P
--assoc --assoc-sign=pos @P
--assoc --assoc-sign=neg @P
--assoc --assoc-sign=x @P
--assoc-min-count=3 @P
--assoc-min-count=0 @P
--assoc-sign=pos @P
--assoc-sign=x @P
--trait=@T @P
--trait=@N @P
--trait @P
--trait=@T --trait-perm=10 @P
--trait=@T --trait-perm=0 @P
--trait=@T --trait-perm=-1 @P
--trait=@T --trait-perm=x @P
--trait=@T --trait-perm=2147483647 @P
--trait=@T --trait-perm=10 --trait-seed=5 @P
--trait=@T --trait-perm=10 --trait-seed=x @P
--trait=@T --trait-perm=10 --trait-lineage=nj @P
--trait=@T --trait-perm=10 --trait-lineage=upgma @P
--trait=@T --trait-perm=10 --trait-lineage=x @P
--trait-perm=10 @P
--trait-perm=-1 @P
--trait-seed=5 @P
--trait-lineage=nj @P
--trait-lineage=x @P
--tree @P
--tree=adj @P
--tree=gene @P
--tree=x @P
--tree --tree-metric=diff @P
--tree --tree-metric=shared @P
--tree --tree-metric=x @P
--tree --tree-method=upgma @P
--tree --tree-method=nj @P
--tree --tree-method=x @P
--tree --tree-boot=3 @P
--tree --tree-boot=0 @P
--tree --tree-boot=-1 @P
--tree --tree-boot=x @P
--tree --tree-boot=2147483648 @P
--tree --tree-boot=3 --tree-seed=7 @P
--tree --tree-seed=7 @P
--tree --tree-seed=-1 @P
--tree --tree-seed=x @P
--tree --tree-seed=7x @P
--tree --tree-seed=4294967295 @P
--tree --tree-seed=4294967296 @P
--tree --tree-seed= @P
--tree-metric=diff @P
--tree-metric=x @P
--tree-method=upgma @P
--tree-method=x @P
--tree-boot=3 @P
--tree-boot=x @P
--tree-seed=7 @P
--tree-seed=x @P
--tree --tree-boot=x --tree-metric=shared @P
--tree --tree-seed=x --tree-boot=x @P
--qtrait=@Q @P
--qtrait=@N @P
--qtrait @P
--qtrait=@Q --qtrait-perm=10 @P
--qtrait=@Q --qtrait-perm=0 @P
--qtrait=@Q --qtrait-perm=-1 @P
--qtrait=@Q --qtrait-perm=x @P
--qtrait=@Q --qtrait-perm=2147483647 @P
--qtrait=@Q --qtrait-perm=10 --qtrait-seed=5 @P
--qtrait=@Q --qtrait-perm=10 --qtrait-seed=x @P
--qtrait-perm=10 @P
--qtrait-perm=-1 @P
--qtrait-seed=5 @P
--cluster=2 @P
--cluster=2-3 @P
--cluster=3-3 @P
--cluster=1 @P
--cluster=x @P
--cluster=3-2 @P
--cluster=2- @P
--cluster=2-x @P
--cluster=-2 @P
--cluster=2-2147483648 @P
--cluster=40 @P
--cluster @P
--cluster=2 --cluster-type=adj @P
--cluster=2 --cluster-type=x @P
--cluster=2 --cluster-metric=diff @P
--cluster=2 --cluster-metric=shared @P
--cluster=2 --cluster-iter=5 @P
--cluster=2 --cluster-iter=0 @P
--cluster=2 --cluster-iter=-1 @P
--cluster=2 --cluster-iter=x @P
--cluster=2 --cluster-foo=1 @P
--cluster-type=adj @P
--cluster-type=x @P
--cluster-metric=diff @P
--cluster-iter=5 @P
--cluster-iter=x @P
--permanova=@T @P
--permanova=@N @P
--permanova @P
--permanova=@T --permanova-type=adj @P
--permanova=@T --permanova-type=x @P
--permanova=@T --permanova-metric=diff @P
--permanova=@T --permanova-metric=shared @P
--permanova=@T --permanova-perm=10 @P
--permanova=@T --permanova-perm=0 @P
--permanova=@T --permanova-perm=-1 @P
--permanova=@T --permanova-perm=x @P
--permanova=@T --permanova-perm=2147483647 @P
--permanova=@T --permanova-perm=10 --permanova-seed=5 @P
--permanova=@T --permanova-perm=10 --permanova-seed=x @P
--permanova=@T --permanova-foo=1 @P
--permanova-type=adj @P
--permanova-type=x @P
--permanova-metric=diff @P
--permanova-perm=10 @P
--permanova-perm=x @P
--permanova-seed=5 @P
--mantel @P
--mantel --mantel-perm=10 @P
--mantel=@T --mantel-perm=10 @P
--mantel=@N --mantel-perm=10 @P
--mantel --mantel-perm=10 --mantel-x=adj:diff @P
--mantel --mantel-x=gene @P
--mantel --mantel-x=x:y @P
--mantel --mantel-x=gene:shared @P
--mantel --mantel-perm=10 --mantel-y=gene:diff @P
--mantel --mantel-y=x @P
--mantel=@N --mantel-y=gene:diff @P
--mantel-y=gene:diff --mantel=@N @P
--mantel=@N --mantel-y=x @P
--mantel --mantel-perm=0 @P
--mantel --mantel-perm=-1 @P
--mantel --mantel-perm=x @P
--mantel --mantel-perm=2147483647 @P
--mantel --mantel-perm=10 --mantel-seed=5 @P
--mantel --mantel-perm=10 --mantel-seed=x @P
--mantel --mantel-foo=1 @P
--mantel-x=adj:diff @P
--mantel-x=x @P
--mantel-y=gene:diff @P
--mantel-perm=10 @P
--mantel-perm=x @P
--mantel-seed=5 @P
--gainloss @P
--gainloss=node @P
--gainloss=gene @P
--gainloss=x @P
--gainloss --gainloss-type=adj @P
--gainloss --gainloss-type=x @P
--gainloss --gainloss-metric=diff @P
--gainloss --gainloss-metric=shared @P
--gainloss --gainloss-method=nj @P
--gainloss --gainloss-method=x @P
--gainloss --gainloss-gain=2 @P
--gainloss --gainloss-gain=0 @P
--gainloss --gainloss-gain=256 @P
--gainloss --gainloss-gain=x @P
--gainloss --gainloss-loss=2 @P
--gainloss --gainloss-loss=0 @P
--gainloss --gainloss-loss=x @P
--gainloss --gainloss-resolve=early @P
--gainloss --gainloss-resolve=x @P
--gainloss --gainloss-min=1 @P
--gainloss --gainloss-min=-1 @P
--gainloss --gainloss-min=x @P
--gainloss --gainloss-min=2147483648 @P
--gainloss --gainloss-foo=1 @P
--gainloss-type=adj @P
--gainloss-type=x @P
--gainloss-metric=diff @P
--gainloss-method=nj @P
--gainloss-gain=2 @P
--gainloss-gain=x @P
--gainloss-loss=2 @P
--gainloss-resolve=early @P
--gainloss-min=1 @P
--coevo @P
--coevo=0.5 @P
--coevo=0 @P
--coevo=1.5 @P
--coevo=x @P
--coevo --coevo-type=adj @P
--coevo --coevo-type=x @P
--coevo --coevo-metric=diff @P
--coevo --coevo-metric=shared @P
--coevo --coevo-method=nj @P
--coevo --coevo-method=x @P
--coevo --coevo-gain=2 @P
--coevo --coevo-gain=0 @P
--coevo --coevo-gain=x @P
--coevo --coevo-loss=2 @P
--coevo --coevo-loss=256 @P
--coevo --coevo-loss=x @P
--coevo --coevo-resolve=early @P
--coevo --coevo-resolve=x @P
--coevo --coevo-min=1 @P
--coevo --coevo-min=0 @P
--coevo --coevo-min=x @P
--coevo --coevo-min=2147483648 @P
--coevo --coevo-sign=pos @P
--coevo --coevo-sign=neg @P
--coevo --coevo-sign=x @P
--coevo --coevo-max=5 @P
--coevo --coevo-max=0 @P
--coevo --coevo-max=-1 @P
--coevo --coevo-max=x @P
--coevo --coevo-foo=1 @P
--coevo-type=adj @P
--coevo-type=x @P
--coevo-metric=diff @P
--coevo-method=nj @P
--coevo-gain=2 @P
--coevo-loss=2 @P
--coevo-resolve=early @P
--coevo-min=1 @P
--coevo-min=0 @P
--coevo-sign=pos @P
--coevo-max=5 @P
--coevo-max=x @P
--curves=3 --curves @P
--curves --curves=3 @P
--dist=adj --dist @P
--dist --dist=adj @P
--tree=adj --tree @P
--tree --tree=adj @P
--assoc=0.5 --assoc @P
--assoc --assoc=0.5 @P
--gainloss=node --gainloss @P
--gainloss --gainloss=node @P
--coevo=0.1 --coevo @P
--coevo --coevo=0.1 @P
--mantel=@N --mantel --mantel-perm=10 @P
--mantel --mantel=@N --mantel-perm=10 @P
--mantel=@N --mantel --mantel-y=gene:diff --mantel-perm=10 @P
--trait=@N --trait=@T --trait-perm=10 @P
--cluster=3 --cluster=2 @P
--curves --dist --qtrait-perm=5 @P
--cluster-iter=3 --coevo-min=0 @P
--coevo-min=1 --cluster-iter=3 @P
--trait-lineage=nj --matrix --curves @P
--mantel-y=gene:diff --mantel=@N --gainloss-min=2 @P
--qtrait-seed=1 --cluster-type=adj @P
--dist --tree --qtrait-perm=5 --coevo @P
--gainloss --coevo --gainloss-gain=0 @P
--tree --gainloss --coevo-min=3 @P
--permanova-perm=x --dist=x @P
--tr @P
--c @P
--coevo-m=2 --coevo @P
--curves-s=5 --curves=2 @P
--tree-b=2 --tree @P
--version
--curves
--coevo --coevo-min=0
"""


def lines():
    """every command line of the transcript, as written (placeholders in place), in the order they run"""
    ls = [s for s in SUB.strip().split("\n")] + [s for s in LONG.strip().split("\n")]
    ls += [a + " " + b + " @P" for a, b in itertools.combinations(HEADS, 2)]  # every unordered pair of the head options
    ls += [b + " " + a + " @P" for a, b in itertools.combinations(HEADS[::3], 2)]  # some of them the other way round
    ls += ["--gpus 2 " + h + " @P" for h in HEADS] + ["--gpus=2 @P", "--procs 2 --dist @P"]
    assert len(set(ls)) == len(ls)
    return ls


def paf_files():
    d = os.path.join(ROOT, "tests", "golden", "C4")
    return sorted("tests/golden/C4/" + f for f in os.listdir(d) if ".paf" in f)


def expand(line):
    """(argv, the long-option words for capi.run or None)"""
    words = [w.replace("@G", G).replace("@T", T).replace("@Q", Q).replace("@N", N) for w in shlex.split(line)]
    if "@P" not in words:
        return words, None
    opts = [w for w in words if w != "@P"]
    return opts + paf_files(), opts


def record(line, lib):
    """one entry of the transcript: run from the repository root"""
    from pangene_amd import capi
    argv, opts = expand(line)
    r = subprocess.run([CLI] + argv, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    err = "".join(s for s in r.stderr.decode("utf-8", "replace").splitlines(True) if not s.startswith("[M::"))
    e = {"line": line, "status": r.returncode, "stdout_md5": hashlib.md5(r.stdout).hexdigest(), "stdout_len": len(r.stdout), "stderr": err}
    if opts is not None:
        cwd = os.getcwd()
        os.chdir(ROOT)
        try:
            e["capi"] = hashlib.md5(capi.run(lib, paf_files(), opts)).hexdigest()
        except Exception as x:  # recorded, type and text: the refusals are part of the behaviour
            e["capi"] = "%s: %s" % (type(x).__name__, x)
        finally:
            os.chdir(cwd)
    return e


def load_checker():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ctypes
    import oracle_host
    lib = oracle_host.load()
    ctypes.c_int.in_dll(lib, "pg_verbose").value = 1  # (capi.run in this process: no progress lines)
    return lib


def main():
    lib = load_checker()
    out = [record(s, lib) for s in lines()]
    with open(sys.argv[1] if len(sys.argv) > 1 else OUT, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d lines" % len(out))


if __name__ == "__main__":
    main()
