"""TEST INFRASTRUCTURE: direct pga_pan_pcoa / pg_pan_pcoa cases for tests/test_pcoa_gpu.py, run in a child process of their own so that
the test can bound them with a timeout.  The product library (HIP kernels of k_pcoa.hpp) runs matrices no GFA fixture reaches; the
numpy restatement (tests/support/pcoa_ref.py) checks them within the tolerances stated there.  Through the tests-only x_test / y_test
pointers of pga_pcoa_in_t the product kernel k_pcoa_mult is reached directly:
    |Y - Y_ref|_i <= 4 N 2^-53 ((|A| |X|)_i + mean(|A| |X|)),
the standard bound of a dot product with a factor 4 for the squaring and the different order of the sum, and the same for the mean.
Prints one line per case and "ALL OK" at the end; exits 1 at the first miss.

    python tests/support/pcoa_direct.py {file:NAME|memory:NAME|maps|negative|rank|multiple|slow|cap|magnitude|twice|range}"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
GOLD = os.path.join(ROOT, "tests", "golden")
HIP = os.path.join(ROOT, "pangene_amd", "bin", "pangene")
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dist_ref as dr  # noqa: E402
import pcoa_ref as pc  # noqa: E402
import tree_ref as tr  # noqa: E402

PGA_ERR_RANGE = -2
SPECS = [("gene", "jaccard"), ("gene", "diff"), ("adj", "jaccard"), ("adj", "diff")]


class pga_pcoa_in_t(C.Structure):
    _fields_ = [("q", C.c_void_p), ("n", C.c_int32), ("fbits", C.c_int32), ("n_axis", C.c_int32), ("seed", C.c_uint32), ("max_step", C.c_int32),
                ("x_test", C.c_void_p), ("y_test", C.c_void_p), ("n_test", C.c_int32)]


class pga_pcoa_out_t(C.Structure):
    _fields_ = [("eig", C.POINTER(C.c_double)), ("resid", C.POINTER(C.c_double)), ("vec", C.POINTER(C.c_double)), ("n_axis", C.c_int32), ("n_step", C.c_int32),
                ("n_restart", C.c_int32), ("converged", C.c_int32)]


def fail(msg):
    print(msg, flush=True)
    sys.exit(1)


def say(label, ok, detail=""):
    print("%s: %s%s" % (label, "ok" if ok else "MISS", (" -- " + detail) if detail else ""), flush=True)
    if not ok:
        sys.exit(1)


def direct(lib, q, F, k, seed=0, max_step=0, x=None, n=None):
    """pga_pan_pcoa itself: the status when it is not 0, else a dict eig, resid, vec (N, axes) -- unit columns, no sign rule --, axes, steps,
    restarts, converged and, with x (N, b), y (N, b)"""
    q = np.ascontiguousarray(q, dtype=np.int32)
    N = q.shape[0] if n is None else n
    y = None
    if x is not None:
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(N, -1)
        y = np.full(x.shape, np.nan)
    arg = pga_pcoa_in_t(q.ctypes.data, N, F, k, seed, max_step, x.ctypes.data if x is not None else None, y.ctypes.data if x is not None else None,
                        x.shape[1] if x is not None else 0)
    out = pga_pcoa_out_t()
    lib.pga_pan_pcoa.restype = C.c_int
    rc = lib.pga_pan_pcoa(C.byref(arg), C.byref(out))
    if rc != 0:
        return rc
    a = out.n_axis
    r = {"axes": a, "steps": out.n_step, "restarts": out.n_restart, "converged": out.converged, "eig": np.array([out.eig[i] for i in range(a)]),
         "resid": np.array([out.resid[i] for i in range(a)]), "vec": np.ctypeslib.as_array(out.vec, shape=(N * max(a, 1),))[:N * a].reshape(N, a).copy()}
    if y is not None:
        r["y"] = y
    return r


def check_mult(lib, q, F, b, label):
    """Y = B X of b columns through x_test against numpy"""
    N = len(q)
    rng = np.random.default_rng(N * 16 + b)
    X = rng.standard_normal((N, b))
    got = direct(lib, q, F, 1, x=X)
    if not isinstance(got, dict):
        fail("%s: status %d" % (label, got))
    d = np.asarray(q, dtype=np.float64) * 2.0 ** -F
    A = -0.5 * (d * d)
    Y = A @ X
    want = Y - Y.mean(axis=0)
    bound = np.abs(A) @ np.abs(X)
    bound = 4 * N * 2.0 ** -53 * (bound + bound.mean(axis=0))
    err = np.abs(got["y"] - want)
    say("%s mult N=%d b=%d" % (label, N, b), bool(np.all(np.isfinite(got["y"])) and np.all(err <= bound)), "largest error / bound = %.3g" % float((err / np.maximum(bound, 1e-300)).max()))


def check_full(lib, q, F, k, label, coords=True, seed=0, want_axes=None):
    """capi.pan_pcoa in the product against the reference; returns (the result, the reference, the axes whose coordinates were compared)"""
    from pangene_amd import capi
    ref = pc.reference(q, F)
    got = capi.pan_pcoa(lib, np.asarray(q, dtype=np.int32), F, k, seed)
    bad, compared = pc.check(q, F, got, k, coords=coords, ref=ref)
    ok = not bad and got["converged"] == 1 and (want_axes is None or got["axes"] == want_axes)
    say("%s N=%d k=%d: axes %d, steps %d, restarts %d, converged %d, coordinates compared on axes %s" % (
        label, len(q), k, got["axes"], got["steps"], got["restarts"], got["converged"], [a + 1 for a in compared]), ok, "; ".join(bad))
    return got, ref, compared


def fixture(name, kind, metric):
    asm, P = dr.presence(os.path.join(GOLD, name + ".gfa.gz"), kind)
    q, F = tr.fixed(dr.shared(P), metric)
    return list(asm), P, q, F


def run_cli(args, env=None):
    r = subprocess.run([HIP] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env)
    return r.returncode, r.stdout, r.stderr


def pafs_of(name):
    d = os.path.join(GOLD, name)
    return sorted(os.path.join(d, f) for f in os.listdir(d) if ".paf" in f)


def slow_matrix():
    """random Jaccard of 200 x 400 presence bits at density 0.3, seed 21: its top three lie within 4 per cent, and axes 2 and 3 stand
    0.0065 l_1 apart, under the gap rule (most seeds leave every gap just above 0.01 l_1)"""
    P = np.random.default_rng(21).random((200, 400)) < 0.3
    return pc.jaccard(P)


def main():
    which = sys.argv[1]
    from pangene_amd import capi
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    lib = capi.load()
    if which.startswith("file:"):
        # the product's command line on the GFA fixture, the four option sets with -k 3, against the reference; and pg_pan_pcoa / presence
        name = which[5:]
        for kind, metric in SPECS:
            asm, P, q, F = fixture(name, kind, metric)
            rc, out, err = run_cli(["pcoa", "-t", kind, "-m", metric, "-k", "3", os.path.join(GOLD, name + ".gfa.gz")])
            if rc != 0:
                fail("pangene pcoa: exit %d: %s" % (rc, err.decode(errors="replace")[-500:]))
            got = pc.of_text(out)
            ref = pc.reference(q, F)
            bad, compared = pc.check(q, F, got, 3, text=True, ref=ref)
            say("file %s %s:%s: axes %d, steps %d, restarts %d, compared %s" % (name, kind, metric, got["axes"], got["steps"], got["restarts"], [a + 1 for a in compared]),
                not bad and got["names"] == asm and got["converged"] == 1, "; ".join(bad))
            check_full(lib, q, F, 3, "pg_pan_pcoa %s %s:%s" % (name, kind, metric))
        asm, P, q, F = fixture(name, "gene", "jaccard")
        got, F2 = capi.pan_pcoa_presence(lib, torch.from_numpy(np.asarray(P) != 0).cuda(), "jaccard", 3)
        bad, _ = pc.check(q, F, got, 3)
        say("pg_pan_pcoa_presence %s" % name, not bad and F2 == F, "; ".join(bad))
    elif which.startswith("memory:"):
        # `pangene --pcoa *.paf` equals `pangene pcoa` on the GFA of the same run, byte for byte (the same build, the same code: the
        # determinism rule), and stands within the bounds
        name = which[7:]
        files = pafs_of(name)
        rc, gfa, _ = run_cli(files)
        tmp = os.path.join(os.environ.get("TMPDIR", "/tmp"), "pcoa_direct_%d.gfa" % os.getpid())
        open(tmp, "wb").write(gfa)
        try:
            for mem, fil, kind, metric, k in ((["--pcoa"], [], "gene", "jaccard", 3),
                                              (["--pcoa=2", "--pcoa-type=adj", "--pcoa-metric=diff", "--pcoa-seed=5"], ["-k", "2", "-t", "adj", "-m", "diff", "-s", "5"], "adj", "diff", 2)):
                rc1, a, _ = run_cli(mem + files)
                rc2, b, _ = run_cli(["pcoa"] + fil + [tmp])
                q, F = tr.fixed(dr.shared(dr.presence(tmp, kind)[1]), metric)  # (of the GFA of this run)
                bad, _ = pc.check(q, F, pc.of_text(a), k, text=True) if rc1 == 0 else (["exit %d" % rc1], [])
                say("memory %s %s" % (name, " ".join(mem)), rc == 0 and rc1 == 0 and rc2 == 0 and a == b and not bad, "; ".join(bad))
        finally:
            os.unlink(tmp)
    elif which == "maps":
        # points in R^3: three axes stand out (the rounding of the distances leaves the rest below 1e-5 l_1).  The tile and lane edges of
        # k_pcoa_mult (four columns a lane, 1 024 a pass of the workgroup, four rows a workgroup) and of the Gram-Schmidt reductions
        for N in (3, 4, 63, 64, 65, 127, 129, 257, 513, 1025):
            q = pc.points(np.random.default_rng(N).random((N, 3)))
            for b in (1, 3, 8):
                check_mult(lib, q, 20, b, "maps")
            got, (B, w, v), compared = check_full(lib, q, 20, 3, "maps", want_axes=min(3, N - 1))
            if N >= 63 and not (w[3] < 1e-4 * w[0] and len(compared) >= 1):  # (two of the three may lie within 0.01 l_1 of each other, as at N = 513)
                fail("maps: the three axes of points in R^3 must stand out")
    elif which == "negative":
        # Twelve points on a line with the SQUARED distance used as the distance: far from Euclidean, l_min = -0.316 l_1.  A solver that
        # ranks by size returns the negative value among its first three.  q = floor(((i - j) / 12)^2 2^20 + 1/2) as the issue states
        # it: the rounding leaves l_2 = 3.7e-7 l_1, ABOVE the cut 1e-9 l_1, so by the definition three axes come back for this matrix,
        # not one (the issue's l_2 = 0 holds for the unrounded distances).  The second matrix has distances ((i - j) / 16)^2, exact in
        # fixed point: there l_2 = 0 up to rounding and exactly one axis must come back.
        i = np.arange(12)
        q = np.floor(((i[:, None] - i[None, :]) / 12.0) ** 2 * 2 ** 20 + 0.5).astype(np.int64)
        B, w, v = pc.reference(q, 20)
        if not (w[-1] < -w[1] - 0.05 * w[0] and abs(w[-1] / w[0] + 0.316) < 1e-3):
            fail("negative: the reference must have l_min < -l_2 - 0.05 l_1")
        got, _, _ = check_full(lib, q, 20, 3, "negative, as stated")
        if not np.all(got["eig"] > 0):
            fail("negative: an axis with an eigenvalue below zero")
        q = ((i[:, None] - i[None, :]) ** 2).astype(np.int64) << 12  # ((i - j) / 16)^2 2^20
        B, w, v = pc.reference(q, 20)
        if not (w[-1] < -w[1] - 0.05 * w[0] and abs(w[1]) < 1e-12 * w[0]):
            fail("negative: the exact matrix must have l_2 = 0 and l_min < -0.05 l_1")
        check_full(lib, q, 20, 3, "negative, exact in fixed point", want_axes=1)
    elif which == "rank":
        # two groups of identical points: B has rank 1.  Without the breakdown rule the second step divides by zero
        g = np.array([0] * 4 + [1] * 6)
        q = (g[:, None] != g[None, :]).astype(np.int64) << 20
        got, _, _ = check_full(lib, q, 20, 3, "rank 1", want_axes=1)
        say("rank 1: at least one restart, finite numbers", got["restarts"] >= 1 and bool(np.all(np.isfinite(got["coord"]))))
        for n, note in ((10, b"no distance above zero"), (1, b"fewer than 3"), (2, b"fewer than 3")):
            z = np.zeros((n, n), dtype=np.int32) if n == 10 else ((1 - np.eye(n, dtype=np.int32)) << 20)
            got = capi.pan_pcoa(lib, z, 20, 3)
            say("rank: N=%d, %s" % (n, note.decode()), got["axes"] == 0 and got["eig"].size == 0)
        # (the notes themselves: tests/test_pcoa_gpu.py test_notes)  A zero matrix below the host's check: nothing divides by zero
        got = direct(lib, np.zeros((2, 2), dtype=np.int32), 20, 1)
        say("rank: pga_pan_pcoa on two identical assemblies", isinstance(got, dict) and got["axes"] == 1 and got["eig"][0] == 0.0)
    elif which == "multiple":
        # a regular simplex: N - 1 equal eigenvalues d^2 / 2.  Without the lock-and-restart rule one axis comes back
        q = (1 - np.eye(6, dtype=np.int64)) << 20
        got, (B, w, v), compared = check_full(lib, q, 20, 3, "multiple", want_axes=3)
        say("multiple: three eigenvalues d^2 / 2, no coordinates compared", bool(np.all(np.abs(got["eig"] - 0.5) <= 1e-9 * 0.5)) and compared == [] and got["restarts"] >= 2)
        x = got["coord"]
        say("multiple: the axes are orthogonal within the shared eigenspace too", bool(np.abs(x.T @ x - 0.5 * np.eye(3)).max() <= 1e-9 * 0.5))
    elif which == "slow":
        q = slow_matrix()
        got, (B, w, v), compared = check_full(lib, q, 20, 3, "slow")
        gaps = [min(w[a - 1] - w[a] if a else np.inf, w[a] - w[a + 1]) for a in range(3)]
        dropped = [a for a in range(3) if a not in compared]
        say("slow: top three within 6 per cent, dropped axes %s have reference gaps below 0.01 l_1, %d steps below the cap" % ([a + 1 for a in dropped], got["steps"]),
            w[2] > 0.94 * w[0] and len(dropped) >= 1 and all(gaps[a] < pc.GAP * w[0] for a in dropped) and got["steps"] < 256 and got["axes"] == 3)
    elif which == "cap":
        assert os.environ.get("PANGENE_PCOA_STEPS") == "6", "run with PANGENE_PCOA_STEPS=6"
        q = slow_matrix()
        B, w, v = pc.reference(q, 20)
        got = capi.pan_pcoa(lib, np.asarray(q, dtype=np.int32), 20, 3)
        ok = got["converged"] == 0 and got["steps"] == 6 and got["axes"] == 3
        for a in range(got["axes"]):
            vec = got["coord"][:, a] / np.sqrt(got["eig"][a])
            true = np.linalg.norm(B @ vec - got["eig"][a] * vec)
            ok = ok and abs(true - got["resid"][a]) <= 1e-9 * w[0] and got["resid"][a] > 1e-6 * w[0]
        say("cap: converged 0 after 6 vectors, every residual is |B v - theta v| of the returned vector", ok, "residuals %s" % got["resid"])
    elif which == "magnitude":
        # entries up to 2^29 - 1: q^2 reaches 2^58, beyond the 53 bits of a double -- the squares are rounded as numpy rounds them
        N = 129
        rng = np.random.default_rng(129)
        q = np.triu(rng.integers(1 << 28, 1 << 29, size=(N, N), dtype=np.int64), 1)
        q = q + q.T
        q[0, 1] = q[1, 0] = (1 << 29) - 1
        for b in (1, 8):
            check_mult(lib, q, 20, b, "magnitude")
        check_full(lib, q, 20, 3, "magnitude")
        check_full(lib, q, 0, 3, "magnitude, F = 0")
    elif which == "twice":
        # the same call twice, and again after a larger and a smaller call in between (the pool's buffers are reused): the same bits
        q, big, small = slow_matrix(), pc.points(np.random.default_rng(7).random((700, 4))), pc.points(np.random.default_rng(8).random((40, 2)))
        first = direct(lib, q, 20, 3, seed=3)
        again = direct(lib, q, 20, 3, seed=3)
        direct(lib, big, 20, 5)
        direct(lib, small, 20, 2)
        third = direct(lib, q, 20, 3, seed=3)
        lib.pg_trim_host_cache(0)  # gives the buffers back; the next call allocates again
        fourth = direct(lib, q, 20, 3, seed=3)
        for other, what in ((again, "twice"), (third, "after a larger and a smaller call"), (fourth, "after the buffers were given back")):
            same = all(np.array_equal(first[key], other[key]) for key in ("eig", "resid", "vec")) and all(first[key] == other[key] for key in ("axes", "steps", "restarts", "converged"))
            say("twice: %s" % what, same and first["vec"].tobytes() == other["vec"].tobytes())
        other = direct(lib, q, 20, 3, seed=4)
        say("twice: another seed takes another start vector and meets the same bounds", not np.array_equal(first["vec"], other["vec"]) and
            bool(np.all(np.abs(first["eig"] - other["eig"]) <= 2e-9 * first["eig"][0])))
    elif which == "range":
        one = np.zeros((1, 1), dtype=np.int32)  # (the refusal comes before the matrix is looked at: one entry does)
        say("range: n = 16 385", direct(lib, one, 20, 3, n=16385) == PGA_ERR_RANGE)
        q = pc.points(np.random.default_rng(5).random((30, 3)))
        say("range: k = 17", direct(lib, q, 20, 17) == PGA_ERR_RANGE and direct(lib, q, 20, 0) == PGA_ERR_RANGE)
        q5 = pc.points(np.random.default_rng(6).random((5, 4)))
        got = direct(lib, q5, 20, 5)  # k = N: clamped to N - 1
        say("range: k = N is clamped to N - 1", isinstance(got, dict) and got["axes"] == 4)
        check_full(lib, q, 20, 3, "after the refusals")
    else:
        sys.exit("unknown case " + which)
    print("ALL OK", flush=True)


if __name__ == "__main__":
    main()
