"""One run of the product library in a process of its own (the PANGENE_* switches are read once): main.c's steps through the C ABI
in exact mode 2 (or 1), with what pg_graph_gen leaves behind kept for the caller.

    python loop_tail_run.py OUT_PREFIX "VARIANT" FILE...        (LOOP_TAIL_EXACT=1 in the environment: exact mode 1, auto)

writes OUT_PREFIX.gfa (what the command line would print), OUT_PREFIX.arc / OUT_PREFIX.seg (q->arc[0..n_arc) and q->seg[0..n_seg)
as bytes, pg_graph_t laid out as in bench.py) and prints one JSON line: n_seg, n_arc, and waits = the number of times the host
waited for the backend's stream inside pg_graph_gen (pg_kernel_timing, class 4)."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from pangene_amd import capi  # noqa: E402


class Graph(C.Structure):  # include/pangene_amd.h: pg_graph_t
    _fields_ = [("d", C.c_void_p), ("g2s", C.c_void_p), ("n_seg", C.c_int32), ("m_seg", C.c_int32), ("seg", C.c_void_p),
                ("n_arc", C.c_int32), ("m_arc", C.c_int32), ("arc", C.c_void_p), ("idx", C.c_void_p)]


def main():
    prefix, variant, files = sys.argv[1], sys.argv[2], sys.argv[3:]
    lib = capi.load()
    C.c_int.in_dll(lib, "pg_verbose").value = 0
    lib.pg_set_exact_mode(int(os.environ.get("LOOP_TAIL_EXACT", "2")))
    opt = capi.parse_args(lib, variant.split())
    lib.pg_set_output((prefix + ".gfa").encode())
    d = lib.pg_data_init()
    try:
        capi.read_files(lib, opt, d, files)
        lib.pg_post_process(C.byref(opt), d)
        assert lib.pg_last_error() == 0, lib.pg_last_error_str()
        g = lib.pg_graph_init(d)
        lib.pg_kernel_timing_reset(d)
        lib.pg_graph_gen(C.byref(opt), g)
        assert lib.pg_last_error() == 0, lib.pg_last_error_str()
        ms, n_wait, units = C.c_double(), C.c_int64(), C.c_int64()
        lib.pg_kernel_timing(d, 4, C.byref(ms), C.byref(n_wait), C.byref(units))
        q = C.cast(g, C.POINTER(Graph)).contents
        for name, ptr, n in (("arc", q.arc, q.n_arc), ("seg", q.seg, q.n_seg)):
            with open(prefix + "." + name, "wb") as f:
                if n > 0 and ptr:
                    f.write(bytes((C.c_uint8 * (n * 32)).from_address(ptr)))
        info = {"n_seg": q.n_seg, "n_arc": q.n_arc, "waits": n_wait.value}
        lib.pg_write_graph(g)
        if not (opt.flag & capi.PG_F_WRITE_NO_WALK):
            lib.pg_write_walk(g)
        lib.pg_graph_destroy(g)
    finally:
        lib.pg_data_destroy(d)
        lib.pg_set_output(None)
    print(json.dumps(info))


if __name__ == "__main__":
    main()
