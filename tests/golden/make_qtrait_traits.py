"""Writes tests/golden/qtrait/{C4,bact20,human8}.tsv, the quantitative-trait fixtures of tests/test_qtrait.py and
tests/test_qtrait_gpu.py, from the GFA fixtures beside it.  Seeded: running it again writes the same bytes.

    python tests/golden/make_qtrait_traits.py

Three traits per file: `planted`, a continuous trait that follows the presence of the gene closest to half of the assemblies (shifted
by 2, normal noise, so negatives occur; every other value in exponent notation); `ties`, small integers with heavy ties, written
as 2 or 2.0 by turns, with some NA; `binary`, 0 / 1 only with both values present."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "support"))
import assoc_ref as ar  # noqa: E402
import dist_ref  # noqa: E402
import qtrait_ref as qr  # noqa: E402

NAMES = ["C4", "bact20", "human8"]
TRAITS = ["planted", "ties", "binary"]


def fields(P, A, seed):
    rng = np.random.default_rng(seed)
    cnt = P.sum(axis=1)
    g = int(np.argmin(np.abs(cnt - A / 2.0)))
    v = 2.0 * P[g] - 1.0 + rng.normal(0.0, 0.4, size=A)
    planted = [("%.3e" if c % 2 else "%.4f") % v[c] for c in range(A)]
    t = rng.integers(1, 4, size=A)
    ties = [("%d" if c % 2 else "%d.0") % t[c] for c in range(A)]
    for c in np.nonzero(rng.random(A) < 0.2)[0][: max(A - 3, 0)]:
        ties[c] = "NA"
    b = rng.integers(0, 2, size=A)
    b[0], b[-1] = 1, 0
    return [planted, ties, [str(int(x)) for x in b]]


def main():
    os.makedirs(os.path.join(HERE, "qtrait"), exist_ok=True)
    for i, name in enumerate(NAMES):
        gfa = os.path.join(HERE, name + ".gfa.gz")
        _, P = ar.read_gfa(gfa)
        asm = list(dist_ref.presence(gfa, "gene")[0])
        with open(os.path.join(HERE, "qtrait", name + ".tsv"), "w") as f:
            f.write(qr.trait_file(asm, TRAITS, fields(P, len(asm), 100 + i)))


if __name__ == "__main__":
    main()
