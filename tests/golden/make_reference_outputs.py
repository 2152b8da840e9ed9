#!/usr/bin/env python3
"""Records tests/golden/reference_outputs.json: {"md5", "bytes"} of what the UNTOUCHED reference (oracle/_ref/pangene_ref, built by
oracle/Makefile) prints for the seeded inputs of the tests that compare against it (tests/conftest.py: reference_output), so that
they run wherever the reference binary is absent.  Keys name the input and the options: "<input>|<options>"."""
import gzip, hashlib, json, os, subprocess, sys, tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
from pangene_amd import synth  # noqa: E402
import fuzz_oracle_vs_ref as fz  # noqa: E402
from test_reader import _adversarial_lines  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "pangene_ref")
OUT = {}


def rec(key, argv, files):
    out = subprocess.run([REF] + list(argv) + list(files), stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True).stdout
    OUT[key] = {"md5": hashlib.md5(out).hexdigest(), "bytes": len(out)}


def main():
    if not os.path.exists(REF):
        sys.exit("%s is missing: build it first (make -C oracle ref)" % REF)
    with tempfile.TemporaryDirectory() as td:
        for seed in (11, 12, 13):  # test_oracle_vs_ref.py::test_live_against_reference_binary
            fb = synth.write_files(synth.bact(12, 400, seed=seed), os.path.join(td, "b%d" % seed))
            ff = synth.write_files(synth.fuzz(seed, harsh=bool(seed & 1)), os.path.join(td, "f%d" % seed))
            for tag, fs in (("b", fb), ("f", ff)):
                for args in ([], ["--bed=flag"], ["-S"]):
                    rec("live:%s%d|%s" % (tag, seed, " ".join(args)), args, fs)
        # test_oracle_vs_ref.py::test_fuzz_sweep_default_mode_against_reference_binary
        for first, n, shapes, variants in ((7000, 150, (False, True), "dc"), (9000, 160, (False,), "all"), (9160, 160, (True,), "all")):
            vs = [v for v in fz.VARIANTS if "-D" in v] if variants == "dc" else fz.VARIANTS
            for s in range(first, first + n):
                for harsh in shapes:
                    fs = synth.write_files(synth.fuzz(s, harsh=harsh), os.path.join(td, "z%d_%d" % (s, harsh)))
                    for v in vs:
                        rec(fz.fuzz_key(s, harsh, v), v, fs)
        # test_oracle_vs_ref.py::test_dense_shape_against_reference_binary
        for tag, fs in (("dense3", synth.write_files(synth.dense(3), os.path.join(td, "d"))), ("manydoms2", synth.write_files(synth.many_doms(2), os.path.join(td, "m")))):
            for args in ([], ["-p0", "-a1"], ["-S"], ["-G"]):
                rec("%s|%s" % (tag, " ".join(args)), args, fs)
        # test_reader.py::test_adversarial_paf_lines_against_the_reference_binary (same file names as the test)
        ad = os.path.join(td, "adv"); os.makedirs(ad)
        files = []
        for j in range(4):
            text = _adversarial_lines(np.random.default_rng(100 + j) if j % 2 else None)
            p = os.path.join(ad, "a%d.paf" % j)
            with open(p, "w", newline="") as f:
                f.write(text)
            files.append(p)
            if j == 3:
                with gzip.open(p + ".gz", "wt", newline="") as f:
                    f.write(text)
                files[-1] = p + ".gz"
        for args in ([], ["-S"], ["-p0", "-a1"], ["--bed=raw"], ["-e", "0.3", "-l", "0.2"]):
            rec("adversarial|%s" % " ".join(args), args, files)
        # test_hip_parity.py::test_config1_full_size_against_reference (BASELINE configs[1])
        rec("config1|", [], synth.write_files_parallel("bact", os.path.join(td, "c2"), G=100, P=5000, seed=1))
    with open(os.path.join(HERE, "reference_outputs.json"), "w") as f:
        json.dump(OUT, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d reference outputs recorded" % len(OUT))


if __name__ == "__main__":
    main()
