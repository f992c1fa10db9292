#!/usr/bin/env python
"""The kernels search_topk (csrc/search.hip) really launches, per shape class, from a rocprofv3 kernel trace: the record
tests/test_search_plan.py holds pfann_search_plan (csrc/search_plan.h) against.  profiles/search_plan/parent_launches.json
was written by this script on the commit BEFORE the plan existed, so "the refactor launches what the old dispatch launched"
is pinned to that commit and not to the code under test; the same two commands on a later tree must reproduce the file.

    rocprofv3 --kernel-trace -d DIR -o t -- timeout -k 10 600 python tools/search_plan_trace.py --run CALLS.json
    python tools/search_plan_trace.py --collect DIR CALLS.json OUT.json

One process, no other tracing.  --run makes one DeviceIndex.search call (or a search_bound + search_bounded pair) per row
of ROWS, each API call between two pfann_bench_region_marker launches (pfann_prof_marker), and writes the calls' shapes;
--collect cuts the trace at the markers.  Per launch: the kernel's name without return type, namespace and parameter list,
the grid in workgroups, the workgroup size and the DYNAMIC LDS bytes of the dispatch (its group segment minus the kernel's
static one).  The runtime's own fill kernels (hipMemsetAsync) are not launches of the library and are left out.
Rows: random unit rows, k = 100 unless stated, the smallest shapes that still reach the branch; DESIGN.md §4."""
import glob
import json
import os
import re
import sqlite3
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

F32, F32_COPY, F16 = 0, 1, 2          # the `storage` argument of pfann_search_plan
N_MAX, D_MAX = 1000050, 128


def _rows():
    rows = []

    def add(name, storage, n, d, nq, k=100, op="search"):
        rows.append({"row": name, "storage": storage, "n": n, "d": d, "nq": nq, "k": k, "op": op})
    add("empty", F32_COPY, 0, 128, 5)
    add("empty_phase1", F32_COPY, 0, 128, 5, op="bound")
    for nq in (1, 32):
        for d in (128, 64):
            add("small_f16_n5000_d%d_nq%d" % (d, nq), F16, 5000, d, nq)
            add("small_f16_n8193_d%d_nq%d" % (d, nq), F16, 8193, d, nq)
        for n in (4096, 4097, 8192, 8193):
            add("small_copy_n%d_d128_nq%d" % (n, nq), F32_COPY, n, 128, nq)
        add("small_copy_n8193_d64_nq%d" % nq, F32_COPY, 8193, 64, nq)
        for d in (128, 64):
            add("small_f32_n5000_d%d_nq%d" % (d, nq), F32, 5000, d, nq)
            add("small_f32_n20000_d%d_nq%d" % (d, nq), F32, 20000, d, nq)
        add("small_d96_n20000_nq%d" % nq, F32_COPY, 20000, 96, nq)
    add("small_phase1", F32_COPY, 20000, 128, 19, op="bound")
    for n in (9000, 60001, 1000050):
        add("batched_nq33_n%d" % n, F32_COPY, n, 128, 33)
    add("batched_nq2100_n60001", F32_COPY, 60001, 128, 2100)
    add("batched_nq1000_d64_n120000", F32_COPY, 120000, 64, 1000)
    add("batched_nq10000_n1000050", F32_COPY, 1000050, 128, 10000)
    add("batched_k300_nq1000_n300000", F32_COPY, 300000, 128, 1000, k=300)
    add("batched_d96_nq1000_n300000", F32_COPY, 300000, 96, 1000)
    add("batched_nq40_n1500", F32_COPY, 1500, 128, 40)
    add("batched_f16_nq4085_n120000", F16, 120000, 128, 4085)
    for nq in (40, 64, 65, 1000):
        add("f32_d96_nq%d_n300000" % nq, F32, 300000, 96, nq)
    add("f32_d100_nq1000_n600000", F32, 600000, 100, 1000)
    add("sharded_nq1000_n125000", F32_COPY, 125000, 128, 1000, op="sharded")
    add("sharded_other_q_nq1000_n125000", F32_COPY, 125000, 128, 1000, op="sharded_other_q")
    add("gselect_G512_nq14600_n20000", F32_COPY, 20000, 128, 14600)
    add("gselect_G1024_nq8000_n40000", F32_COPY, 40000, 128, 8000)
    add("gselect_G4096_nq200_n200000", F32_COPY, 200000, 128, 200)
    return rows


ROWS = _rows()
MTOP = 33          # dist.py's 2 k / G + 8 at k = 100 on 8 shards


def run(calls_path):
    import numpy as np
    import torch
    from pfann_amd import lib as _l
    from pfann_amd.database import DeviceIndex
    lib = _l.load()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    base = torch.randn((N_MAX, D_MAX), device=dev, dtype=torch.float32)
    qbase = torch.randn((16384, D_MAX), device=dev, dtype=torch.float32)
    calls = []
    loaded = {}

    def index_for(r):
        key = (r["storage"], r["n"], r["d"])
        if loaded.get("key") != key:
            loaded.clear()
            idx = DeviceIndex(r["d"], 0, "f16" if r["storage"] == F16 else "f32")
            x = torch.nn.functional.normalize(base[:r["n"], :r["d"]], dim=1).contiguous()
            idx.load(x, np.array([0, r["n"]], np.int64), 0)
            has_copy = idx.set_prefilter(r["storage"] != F32)
            assert r["n"] == 0 or r["storage"] == F16 or has_copy == (r["storage"] == F32_COPY), r
            loaded.update(key=key, idx=idx)
        return loaded["idx"]

    def bracket(r, phase, resume, fn):
        stream = _l.current_stream_ptr(dev)
        torch.cuda.synchronize()
        lib.pfann_prof_marker(stream)
        out = fn()
        lib.pfann_prof_marker(stream)
        torch.cuda.synchronize()
        calls.append({"row": r["row"], "n": r["n"], "d": r["d"], "nq": r["nq"], "k": r["k"], "storage": r["storage"],
                      "phase": phase, "resume": resume, "mtop": MTOP if phase == 1 else 1})
        return out

    for r in ROWS:
        idx = index_for(r)
        q = torch.nn.functional.normalize(qbase[:r["nq"], :r["d"]], dim=1).contiguous()
        if r["op"] == "search":
            bracket(r, 0, 0, lambda: idx.search(q, r["k"]))
        elif r["op"] == "bound":
            bracket(r, 1, 0, lambda: idx.search_bound(q, r["k"], MTOP))
        else:
            bracket(r, 1, 0, lambda: idx.search_bound(q, r["k"], MTOP))
            lb = torch.full((r["nq"],), -1.0, device=dev, dtype=torch.float32)
            q2 = q if r["op"] == "sharded" else q.clone()
            bracket(r, 2, 1 if q2 is q else 0, lambda: idx.search_bounded(q2, r["k"], lb))
    torch.cuda.synchronize()
    with open(calls_path, "w") as f:
        json.dump(calls, f)
    print("%d calls of %d rows" % (len(calls), len(ROWS)))


def short_name(name):
    """`void pfann::scan_small_kernel<128, 2, 1>(pfann::ScanParams) [clone .kd]` -> `scan_small_kernel<128, 2, 1>`"""
    name = re.sub(r"\s*\[clone[^\]]*\]$", "", name.strip())
    m = re.match(r"_ZN(\d+)pfann(\d+)", name)      # left mangled by the tracer's demangler (_Float16 parameters): N5pfann<len><name>E
    if m:
        return name[m.end():m.end() + int(m.group(2))]
    name = re.sub(r"\.kd$", "", name)
    if name.endswith(")"):                       # the parameter list: the last balanced group
        depth = 0
        for i in range(len(name) - 1, -1, -1):
            depth += (name[i] == ")") - (name[i] == "(")
            if depth == 0:
                name = name[:i]
                break
    name = re.sub(r"^void\s+", "", name)
    return name.replace("pfann::", "").strip()


def collect(trace_dir, calls_path, out_path):
    calls = json.load(open(calls_path))
    dbs = sorted(glob.glob(os.path.join(trace_dir, "**", "*_results.db"), recursive=True))
    assert dbs, "no rocpd database under %s" % trace_dir
    c = sqlite3.connect(max(dbs, key=os.path.getsize))        # (the wrapper processes leave empty ones)
    rows = c.execute("select name, grid_x, grid_y, grid_z, workgroup_x, workgroup_y, workgroup_z, lds_size, static_lds_size "
                     "from kernels order by start").fetchall()
    marks = [i for i, r in enumerate(rows) if "pfann_bench_region_marker" in r[0]]
    assert len(marks) == 2 * len(calls), "%d markers for %d calls" % (len(marks), len(calls))
    out = []
    for j, call in enumerate(calls):
        launches = []
        for name, gx, gy, gz, wx, wy, wz, lds, lds_static in rows[marks[2 * j] + 1:marks[2 * j + 1]]:
            if name.startswith("__amd_rocclr_"):
                continue
            assert gy == gz == wy == wz == 1, (name, gy, gz, wy, wz)
            launches.append({"name": short_name(name), "grid": gx // wx, "block": wx, "lds": (lds or 0) - (lds_static or 0)})
        out.append(dict(call, launches=launches))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(e) for e in out) + "\n]\n")
    names = sorted({l["name"] for e in out for l in e["launches"]})
    print("%d calls, %d launches, %d different kernels:" % (len(out), sum(len(e["launches"]) for e in out), len(names)))
    for nm in names:
        print("  " + nm)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--run":
        run(sys.argv[2])
    elif len(sys.argv) == 5 and sys.argv[1] == "--collect":
        collect(sys.argv[2], sys.argv[3], sys.argv[4])
    else:
        sys.exit(__doc__)
