"""TEST INFRASTRUCTURE: two passes of the product library over one data set in a process of its own (PANGENE_FRONT and the other
switches are read once), for tests/test_front_gpu.py: main.c's steps through the C ABI, then pg_rerun_resident and the same again.

    python front_run.py OUT_PREFIX "VARIANT" FILE...        (FRONT_EXACT in the environment: the exact mode, default 1 = auto;
                                                             FRONT_RUN_VERBOSE_FIRST=1: the first pass at pg_verbose = 3, which keeps the host route)

writes OUT_PREFIX.gfa / .arc / .seg of the first pass and OUT_PREFIX.2.gfa / .2.arc / .2.seg of the second (what the command line would
print; q->arc[0..n_arc) and q->seg[0..n_seg) as bytes), prints "[front_run] pass 2" on stderr between the passes and one JSON line:
n_seg, n_arc, and for the second pass waits_post / waits_gen = the times the host waited for the backend's stream inside pg_post_process /
inside pg_graph_gen (pg_kernel_timing, class 4)."""
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
    lib.pg_set_exact_mode(int(os.environ.get("FRONT_EXACT", "1")))
    opt = capi.parse_args(lib, variant.split())
    d = lib.pg_data_init()
    info = {}

    def waits():
        ms, n_wait, units = C.c_double(), C.c_int64(), C.c_int64()
        lib.pg_kernel_timing(d, 4, C.byref(ms), C.byref(n_wait), C.byref(units))
        return n_wait.value

    try:
        capi.read_files(lib, opt, d, files)
        for tag in ("", ".2"):
            lib.pg_set_output((prefix + tag + ".gfa").encode())
            C.c_int.in_dll(lib, "pg_verbose").value = 3 if not tag and os.environ.get("FRONT_RUN_VERBOSE_FIRST") == "1" else 0
            if tag:
                sys.stderr.write("[front_run] pass 2\n")
                sys.stderr.flush()
                assert lib.pg_rerun_resident(d) == 0
                lib.pg_kernel_timing_reset(d)
            lib.pg_post_process(C.byref(opt), d)
            assert lib.pg_last_error() == 0, lib.pg_last_error_str()
            w0 = waits() if tag else 0
            g = lib.pg_graph_init(d)
            lib.pg_graph_gen(C.byref(opt), g)
            assert lib.pg_last_error() == 0, lib.pg_last_error_str()
            if tag:
                info["waits_post"], info["waits_gen"] = w0, waits() - w0
            q = C.cast(g, C.POINTER(Graph)).contents
            for name, ptr, n in (("arc", q.arc, q.n_arc), ("seg", q.seg, q.n_seg)):
                with open(prefix + tag + "." + name, "wb") as f:
                    if n > 0 and ptr:
                        f.write(bytes((C.c_uint8 * (n * 32)).from_address(ptr)))
            info["n_seg"], info["n_arc"] = q.n_seg, q.n_arc
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
