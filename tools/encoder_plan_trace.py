#!/usr/bin/env python
"""The kernels a pfann_encode call really launches, per case of tests/encoder_tap_cases.py, from a rocprofv3 kernel trace:
the record tests/test_encoder_plan.py holds pfann_encode_plan (csrc/encoder_plan.h) against.
profiles/encoder_plan/parent_launches.json was written by this script with the library of the commit BEFORE the plan
existed, so "the launchers launch what the old dispatch launched" is pinned to that commit and not to the code under test;
the same two commands on a later tree must reproduce the file.

    rocprofv3 --kernel-trace -d DIR -o t -- timeout -k 10 900 python tools/encoder_plan_trace.py --run CALLS.json
    python tools/encoder_plan_trace.py --collect DIR CALLS.json OUT.json

One process, no counters, no other tracing.  --run makes, for every case, one Engine.encode call without taps and one with
pfann_debug_keep(ctx, 1) (taps mode 1; mode 2 did not exist on that commit), each between two pfann_bench_region_marker
launches (pfann_prof_marker), and writes the calls with a SHA-256 of their embeddings (normalised and raw, taps off).
--collect cuts the trace at the markers.  Per launch: the kernel's name without return type, namespace and parameter list,
the grid in workgroups, the workgroup size and the DYNAMIC LDS bytes (group segment minus the kernel's static one), stored
as [index into "kernels", grid, block, lds].  The runtime's own copy / fill kernels are not launches of the library and are
left out."""
import glob
import hashlib
import json
import os
import sqlite3
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# PYTHONPATH=<a tree with another commit's pfann_amd and its built library> traces that commit with this tree's cases
_front = [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]
sys.path[:0] = _front + [REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "tests", "golden"), os.path.dirname(os.path.abspath(__file__))]


def run(calls_path):
    import numpy as np
    import torch
    import encoder_tap_cases as tc
    from pfann_amd import lib as _l
    from pfann_amd import synth
    from pfann_amd.engine import Engine
    lib = _l.load()
    dev = torch.device("cuda", 0)
    calls = []
    state = {}

    def engine_for(model):
        if state.get("model") != model:
            state.clear()
            params = tc.model_params(model)
            eng = Engine(params, 0, max_batch=tc.MAX_BATCH)
            eng.load_state_dict(synth.make_state_dict(params, seed=123))
            state.update(model=model, eng=eng, default_fused=eng.set_fused_layernorm(True), pool=torch.as_tensor(tc.pool(params)).to(dev))
            eng.set_fused_layernorm(state["default_fused"])
        return state["eng"]

    def bracket(fn):
        stream = _l.current_stream_ptr(dev)
        torch.cuda.synchronize()
        lib.pfann_prof_marker(stream)
        out = fn()
        lib.pfann_prof_marker(stream)
        torch.cuda.synchronize()
        return out

    def sha(t):
        return hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()

    for case in tc.CASES:
        model, pb, B, prec, fused = case
        eng = engine_for(model)
        # the context's default path is "fused wherever the model allows it": set_fused_layernorm(True) reports which
        want = state["default_fused"] if fused < 0 else bool(fused)
        assert eng.set_fused_layernorm(want) == want, case
        assert eng.set_encoder_precision(prec) == (prec if want else 0), case
        assert eng.set_plan_batch(pb) == pb
        x = state["pool"][torch.as_tensor(tc.batch_rows(B), device=dev)].contiguous()
        for taps in (0, 1):
            eng.debug_keep(bool(taps))
            emb = bracket(lambda: eng.encode(x, norm=True))
            entry = {"case": tc.case_id(case), "model": model, "plan_batch": pb, "B": B, "precision": prec, "fused": fused, "taps": taps}
            if taps == 0:
                entry.update(emb_sha256=sha(emb), raw_sha256=sha(eng.encode(x, norm=False)))
            calls.append(entry)
        eng.debug_keep(False)
    torch.cuda.synchronize()
    with open(calls_path, "w") as f:
        json.dump(calls, f, indent=0)
    print("%d calls of %d cases" % (len(calls), len(tc.CASES)))


def collect(trace_dir, calls_path, out_path):
    from search_plan_trace import short_name
    calls = json.load(open(calls_path))
    dbs = sorted(glob.glob(os.path.join(trace_dir, "**", "*_results.db"), recursive=True))
    assert dbs, "no rocpd database under %s" % trace_dir
    c = sqlite3.connect(max(dbs, key=os.path.getsize))        # (the wrapper processes leave empty ones)
    rows = c.execute("select name, grid_x, grid_y, grid_z, workgroup_x, workgroup_y, workgroup_z, lds_size, static_lds_size "
                     "from kernels order by start").fetchall()
    marks = [i for i, r in enumerate(rows) if "pfann_bench_region_marker" in r[0]]
    # (the raw embedding of a taps-off call is encoded after its closing marker: outside every bracket)
    assert len(marks) == 2 * len(calls), "%d markers for %d calls" % (len(marks), len(calls))
    kernels, out = [], []
    for j, call in enumerate(calls):
        launches = []
        for name, gx, gy, gz, wx, wy, wz, lds, lds_static in rows[marks[2 * j] + 1:marks[2 * j + 1]]:
            if name.startswith("__amd_rocclr_"):
                continue
            assert gy == gz == wy == wz == 1, (name, gy, gz, wy, wz)
            nm = short_name(name)
            if nm not in kernels:
                kernels.append(nm)
            launches.append([kernels.index(nm), gx // wx, wx, (lds or 0) - (lds_static or 0)])
        out.append(dict({k: v for k, v in call.items() if not k.endswith("sha256")}, launches=launches))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write('{"kernels": %s,\n"calls": [\n' % json.dumps(kernels) + ",\n".join(json.dumps(e, separators=(",", ":")) for e in out) + "\n]}\n")
    print("%d calls, %d launches, %d different kernels:" % (len(out), sum(len(e["launches"]) for e in out), len(kernels)))
    for nm in sorted(kernels):
        print("  " + nm)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--run":
        run(sys.argv[2])
    elif len(sys.argv) == 5 and sys.argv[1] == "--collect":
        collect(sys.argv[2], sys.argv[3], sys.argv[4])
    else:
        sys.exit(__doc__)
