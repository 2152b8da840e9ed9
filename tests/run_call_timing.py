#!/usr/bin/env python3
"""Timing of `pangene call` (file route) and `pangene --call` (in-memory route) on the GPU, against pangene.js on the same GFA where
node and the script are available (PANGENE_JS=/path/to/pangene.js).  Not a test: prints one JSON line per input.

    python3 tests/run_call_timing.py [--full] [--out FILE]

Inputs: BASELINE configs[1] (100 x 5 000 bacterial), the 1 250 x 5 000 per-GPU shard of configs[3], and with --full configs[3] at
its full size (10 000 x 5 000).  Per route: wall time of the command (best of three), and from PANGENE_CALL_TIMING=1 the time of
the call step itself (call_ms: bubbles + walk side + output) and of its walk side (walk_side_ms: the kernels of k_call.hpp with their
copies).  graph_ms: stages A+B+C of the same pass (pg_last_path_seconds), what the in-memory route adds to."""
import argparse, json, os, re, shutil, subprocess, sys, tempfile, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pangene_amd import synth  # noqa: E402

HIP = os.path.join(ROOT, "pangene_amd", "bin", "pangene")
SHIM = os.path.join(ROOT, "tests", "support", "k8_shim.js")


def timed(argv, env=None, reps=3, timeout=1800):
    e = dict(os.environ, PANGENE_CALL_TIMING="1", **(env or {}))
    best, line, out = None, "", b""
    for _ in range(reps):
        t = time.perf_counter()
        r = subprocess.run(argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=timeout)
        dt = time.perf_counter() - t
        if r.returncode != 0:
            raise RuntimeError("%s: exit %d\n%s" % (" ".join(argv[:3]), r.returncode, r.stderr.decode()[-2000:]))
        m = [l for l in r.stderr.decode().split("\n") if l.startswith("[call-timing]")]
        if best is None or dt < best:
            best, line, out = dt, (m[-1] if m else ""), r.stdout
    kv = dict(re.findall(r"(\w+)=(\S+)", line))
    return best, kv, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--full", action="store_true", help="also configs[3] at its full size (10 000 genomes)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    js = os.environ.get("PANGENE_JS")
    sets = [("configs1", 100), ("configs3_shard", 1250)] + ([("configs3", 10000)] if a.full else [])
    res = []
    with tempfile.TemporaryDirectory() as td:
        for name, G in sets:
            files = synth.write_files(synth.bact(G, 5000, seed=1), os.path.join(td, name))
            gfa = os.path.join(td, name + ".gfa")
            t_graph, _, g = timed([HIP] + files, reps=1)
            with open(gfa, "wb") as f:
                f.write(g)
            t_file, kv_file, out_file = timed([HIP, "call", gfa])
            t_mem, kv_mem, out_mem = timed([HIP, "--call"] + files)
            t_plain, _, _ = timed([HIP, "-w"] + files)
            r = {"input": name, "genomes": G, "walk_steps": int(kv_file.get("steps", 0)), "segments": int(kv_file.get("segments", 0)),
                 "file_route_wall_s": round(t_file, 4), "file_call_ms": float(kv_file.get("call_ms", "nan")),
                 "file_walk_side_ms": float(kv_file.get("walk_side_ms", "nan")),
                 "memory_route_wall_s": round(t_mem, 4), "memory_call_ms": float(kv_mem.get("call_ms", "nan")),
                 "memory_collect_ms": float(kv_mem.get("collect_ms", "nan")), "memory_walk_side_ms": float(kv_mem.get("walk_side_ms", "nan")),
                 "graph_only_wall_s": round(t_plain, 4), "same_bytes": out_file == out_mem}
            if js and os.path.exists(js) and shutil.which("node"):
                t = time.perf_counter()
                s = subprocess.run(["node", SHIM, js, "call", gfa], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=3600)
                r["script_s"] = round(time.perf_counter() - t, 3)
                r["script_same_bytes"] = s.stdout == out_file
            print(json.dumps(r), flush=True)
            res.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
