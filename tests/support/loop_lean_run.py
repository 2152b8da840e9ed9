"""TEST INFRASTRUCTURE for tests/test_loop_lean_gpu.py: runs of the product library in a process of its own (PANGENE_LOOP_LEAN and its
companions are part of the child's environment), with what the lean form of the queued rounds (pga_branch_loop, pga_host_branch.hpp) must leave alone
kept for the caller and the route hook pga_selftest_loop_route read after every pass.

    python loop_lean_run.py OUT_PREFIX "VARIANT" N_PASS FILE...        (LOOP_LEAN_EXACT=1 in the environment: exact mode 1, auto)

N_PASS passes over ONE upload (the second and later ones through pg_rerun_resident, as bench.py's steps).  After the last pass: OUT_PREFIX.gfa (graph
and W lines), OUT_PREFIX.bed (pg_write_bed of EVERY hit, filtered ones included: the per-hit flag words as the formats print them), OUT_PREFIX.arc /
OUT_PREFIX.seg (q->arc and q->seg as bytes: a segment record carries its n_dist_loci and its `del` bit).  Prints one JSON line: n_seg, n_arc, hits, and
route = the hook's ten words after every pass (c == NULL: the last pga_branch_loop of the process)."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from pangene_amd import capi  # noqa: E402


class Graph(C.Structure):  # include/pangene_amd.h: pg_graph_t
    _fields_ = [("d", C.c_void_p), ("g2s", C.c_void_p), ("n_seg", C.c_int32), ("m_seg", C.c_int32), ("seg", C.c_void_p),
                ("n_arc", C.c_int32), ("m_arc", C.c_int32), ("arc", C.c_void_p), ("idx", C.c_void_p)]


def main():
    prefix, variant, n_pass, files = sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4:]
    lib = capi.load()
    raw = C.CDLL(capi.LIB_HIP)
    raw.pga_selftest_loop_route.restype, raw.pga_selftest_loop_route.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
    C.c_int.in_dll(lib, "pg_verbose").value = 0
    lib.pg_set_exact_mode(int(os.environ.get("LOOP_LEAN_EXACT", "2")))
    opt = capi.parse_args(lib, variant.split())
    d = lib.pg_data_init()
    routes = []
    try:
        capi.read_files(lib, opt, d, files)
        for k in range(n_pass):
            if k and lib.pg_rerun_resident(d) != 0:
                raise RuntimeError("pg_rerun_resident failed")
            lib.pg_post_process(C.byref(opt), d)
            assert lib.pg_last_error() == 0, lib.pg_last_error_str()
            g = lib.pg_graph_init(d)
            lib.pg_graph_gen(C.byref(opt), g)
            assert lib.pg_last_error() == 0, lib.pg_last_error_str()
            route = np.full(10, -7, np.int32)
            assert raw.pga_selftest_loop_route(None, route.ctypes.data) == 0
            routes.append(route.tolist())
            if k + 1 < n_pass:
                lib.pg_graph_destroy(g)
        q = C.cast(g, C.POINTER(Graph)).contents
        for name, ptr, n in (("arc", q.arc, q.n_arc), ("seg", q.seg, q.n_seg)):
            with open(prefix + "." + name, "wb") as f:
                if n > 0 and ptr:
                    f.write(bytes((C.c_uint8 * (n * 32)).from_address(ptr)))
        info = {"n_seg": q.n_seg, "n_arc": q.n_arc, "hits": int(lib.pg_last_path_hits()), "route": routes}
        lib.pg_set_output((prefix + ".gfa").encode())
        lib.pg_write_graph(g)
        if not (opt.flag & capi.PG_F_WRITE_NO_WALK):
            lib.pg_write_walk(g)
        lib.pg_set_output((prefix + ".bed").encode())
        lib.pg_write_bed(d, 0)
        lib.pg_set_output(None)
        lib.pg_graph_destroy(g)
    finally:
        lib.pg_data_destroy(d)
        lib.pg_set_output(None)
    print(json.dumps(info))


if __name__ == "__main__":
    main()
