"""TEST INFRASTRUCTURE: a numpy / Python-int restatement of pangene mantel (include/pangene_amd.h pg_mantel_opt_t, pg_pan_mantel) for
tests/test_mantel.py, tests/test_mantel_gpu.py and tests/support/mantel_direct.py.  Per matrix the shift s, a = qx >> sx, b = qy >> sy;
the sums in Python ints; Z of an order o as (a * b[np.ix_(o, o)]).sum() in int64 -- exact, every sum is below 2^62; the orders are
curves_ref.orders.  r comes from `decimal` at 50 digits and is formatted %.4f; r_text asserts that r 10^4 is not within 1e-9 of a rounding
boundary, so that the three long double roundings of the library (two square roots and two divisions of 64-bit mantissas, each below
1e-18 relative) cannot show in the fourth decimal."""
import decimal
import math

import numpy as np

import curves_ref

HEADER = "X\tY\tN\tr\tn_ge\tn_le\tp_greater\tp_less"
LIMIT_N = 16384
IN_MAX = (1 << 29) - 1
BLOCK = 256


def shift_of(m, N):
    """the smallest s >= 0 with (m >> s)^2 N (N - 1) < 2^62"""
    s = 0
    while (int(m) >> s) ** 2 * N * (N - 1) >= 1 << 62:
        s += 1
    return s


def z_of(a, b, o):
    """Z of order o: the sum over ordered pairs of a[i][j] b[o[i]][o[j]] (the diagonals are zero)"""
    o = np.asarray(o, dtype=np.int64)
    return int((a * b[np.ix_(o, o)]).sum())


def direct(a, b, n_perm=1000, seed=11, rows=0):
    """The backend's step for two shifted matrices: dict Z, n_ge, n_le[, z_rows (rows,) int64 and ord_rows (rows, N) of the first `rows`
    permutations]"""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    N = a.shape[0]
    Z = z_of(a, b, np.arange(N))
    n_ge = n_le = 0
    zs, os_ = [], []
    for p0 in range(0, n_perm, BLOCK):
        O = curves_ref.orders(N, 1 + p0, min(BLOCK, n_perm - p0), seed)
        for o in O:
            zp = z_of(a, b, o)
            n_ge += zp >= Z
            n_le += zp <= Z
            if len(zs) < rows:
                zs.append(zp), os_.append(o)
    r = {"Z": Z, "n_ge": n_ge, "n_le": n_le}
    if rows:
        r["z_rows"], r["ord_rows"] = np.array(zs, dtype=np.int64), np.array(os_, dtype=np.int64).reshape(len(os_), N)
    return r


def pan_mantel(qx, qy, n_perm=1000, seed=11):
    """What capi.pan_mantel returns, and skip: 0 = tested, 1 = N < 3, 2 = a matrix with one value only"""
    qx, qy = np.asarray(qx, dtype=np.int64), np.asarray(qy, dtype=np.int64)
    N = qx.shape[0]
    sx, sy = shift_of(qx.max() if N else 0, N), shift_of(qy.max() if N else 0, N)
    a, b = qx >> sx, qy >> sy
    r = {"N": N, "sx": sx, "sy": sy, "Sa": int(a.sum()), "Sb": int(b.sum()), "Saa": int((a * a).sum()), "Sbb": int((b * b).sum()), "Z": 0, "n_ge": -1, "n_le": -1, "skip": 1}
    if N < 3:
        return r
    M = N * (N - 1)
    if M * r["Saa"] - r["Sa"] ** 2 == 0 or M * r["Sbb"] - r["Sb"] ** 2 == 0:
        r["skip"] = 2
        return r
    r.update(direct(a, b, n_perm, seed), skip=0)
    return r


def same(got, want):
    return all(int(got[k]) == int(want[k]) for k in ("N", "sx", "sy", "Sa", "Sb", "Saa", "Sbb", "Z", "n_ge", "n_le"))


def r_exact(r):
    """Mantel's r of a tested pair as a Decimal at 50 digits"""
    with decimal.localcontext() as ctx:
        ctx.prec = 50
        M = r["N"] * (r["N"] - 1)
        num = decimal.Decimal(M * r["Z"] - r["Sa"] * r["Sb"])
        va, vb = decimal.Decimal(M * r["Saa"] - r["Sa"] ** 2), decimal.Decimal(M * r["Sbb"] - r["Sb"] ** 2)
        return num / va.sqrt() / vb.sqrt()


def r_text(r):
    """r as %.4f; the fixture must keep r 10^4 away from a rounding boundary (see the head of this file)"""
    with decimal.localcontext() as ctx:
        ctx.prec = 50
        x = r_exact(r) * 10000
        frac = x - x.to_integral_value(rounding=decimal.ROUND_FLOOR)
        assert abs(frac - decimal.Decimal("0.5")) > decimal.Decimal("1e-9"), "r is on a rounding boundary of %.4f: choose another fixture"
        return format(x.to_integral_value(rounding=decimal.ROUND_HALF_EVEN) / 10000, ".4f")  # (Decimal keeps the sign of -0.0000, as printf does)


def line(x_name, y_name, r, n_perm):
    p = "%.6f\t%.6f" % ((r["n_ge"] + 1.0) / (n_perm + 1.0), (r["n_le"] + 1.0) / (n_perm + 1.0)) if n_perm else "NA\tNA"
    return "%s\t%s\t%d\t%s\t%d\t%d\t%s" % (x_name, y_name, r["N"], r_text(r), r["n_ge"], r["n_le"], p)


def text(x_name, y_name, qx, qy, n_perm=1000, seed=11):
    """What pangene mantel prints for two matrices over the same assemblies"""
    r = pan_mantel(qx, qy, n_perm, seed)
    return ((HEADER + "\n") if r["skip"] else (HEADER + "\n" + line(x_name, y_name, r, n_perm) + "\n")).encode()


def parse(b):
    """a printed table -> None (the header only) or a dict: X, Y, r, p_greater, p_less (text), N, n_ge, n_le (int)"""
    lines = b.decode().split("\n")
    assert lines[0] == HEADER and lines[-1] == "" and len(lines) in (2, 3)
    if len(lines) == 2:
        return None
    f = lines[1].split("\t")
    assert len(f) == 8, lines[1]
    return {"X": f[0], "Y": f[1], "N": int(f[2]), "r": f[3], "n_ge": int(f[4]), "n_le": int(f[5]), "p_greater": f[6], "p_less": f[7]}


# ---- the external matrix ------------------------------------------------------------------------------------------------------------

def read_matrix(path):
    """(names, q int64 (n, n), F) of a matrix file in the table form or in relaxed PHYLIP: values by float(), F the largest F in [0, 20]
    with floor(vmax 2^F + 0.5) < 2^29, q = floor(v 2^F + 0.5) in float64 -- the library's arithmetic, operation by operation"""
    rows = [l.split() for l in open(path).read().split("\n") if l.split()]
    if rows[0][0] == "Asm":
        names = rows[0][1:]
        assert [r[0] for r in rows[1:]] == names
    else:
        assert len(rows[0]) == 1 and int(rows[0][0]) == len(rows) - 1
        names = [r[0] for r in rows[1:]]
    v = np.array([[float(x) for x in r[1:]] for r in rows[1:]], dtype=np.float64).reshape(len(names), len(names))
    vmax = float(v.max()) if v.size else 0.0
    F = max(F for F in range(21) if math.floor(math.ldexp(vmax, F) + 0.5) < 1 << 29)
    return names, np.floor(np.ldexp(v, F) + 0.5).astype(np.int64), F


def matched(x_names, qx, y_names, qy):
    """the assemblies both sides name, in X's order: (qx, qy) over them"""
    at = {n: k for k, n in enumerate(y_names)}
    ix = [i for i, n in enumerate(x_names) if n in at]
    iy = [at[x_names[i]] for i in ix]
    return np.asarray(qx)[np.ix_(ix, ix)], np.asarray(qy)[np.ix_(iy, iy)]


def matrix_text(names, d, phylip=False, fmt="%.6f"):
    """a matrix file as pangene dist prints it"""
    out = [str(len(names))] if phylip else ["\t".join(["Asm"] + list(names))]
    for nm, row in zip(names, d):
        out.append(("  " if phylip else "\t").join([nm] + [fmt % x for x in row]))
    return "\n".join(out) + "\n"


# ---- generators -------------------------------------------------------------------------------------------------------------------

def random_matrix(N, seed, hi=1 << 20):
    """symmetric, zero diagonal, entries in [0, hi)"""
    rng = np.random.default_rng(seed)
    q = np.triu(rng.integers(0, hi, size=(N, N), dtype=np.int64), 1)
    return q + q.T


def distinct_matrix(N, mul=1, add=1):
    """every entry above the diagonal distinct: add + mul (i N + j) for i < j, mirrored"""
    i, j = np.triu_indices(N, 1)
    q = np.zeros((N, N), dtype=np.int64)
    q[i, j] = add + mul * (i * N + j)
    return q + q.T


def noisy_copy(q, seed, noise):
    """q with symmetric noise in [0, noise) added off the diagonal: a second matrix that tells much the same story"""
    e = random_matrix(q.shape[0], seed, hi=noise)
    return np.asarray(q, dtype=np.int64) + e
