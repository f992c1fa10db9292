"""The launch plan of the search (csrc/search_plan.h, exported as pfann_search_plan) on the CPU.

The expected plans do not come from the code under test: profiles/search_plan/parent_launches.json is a rocprofv3 kernel
trace (tools/search_plan_trace.py) of the commit BEFORE the plan existed, one entry per API call -- the kernels the old
dispatch launched, with grid, workgroup size and dynamic LDS bytes.  The plan must print exactly that list for every
entry.  Every kernel of the UNMASKED search (the first three lists of search_plan.h) is launched in at least one entry;
the one class no machine can run (a sampling stride beyond the 2 GB tile window, shards of ~268 M rows and more) is
checked here from the plan alone.  This covers launches only: that every instantiation, the masked twins included, also
has a case that checks what it COMPUTES against an exact reference is tests/test_search_kernel_coverage.py's to prove."""
import json
import os
import subprocess
import sys

import pytest

import score_bits
from pfann_amd.database import search_plan

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = json.load(open(os.path.join(REPO, "profiles", "search_plan", "parent_launches.json")))
F32, F32_COPY, F16 = 0, 1, 2


def _call_id(c):
    return "%s-phase%d" % (c["row"], c["phase"])


@pytest.mark.parametrize("call", CALLS, ids=_call_id)
def test_plan_prints_the_launches_of_the_old_dispatch(call):
    stages, flags = search_plan(call["n"], call["d"], call["nq"], call["k"], call["storage"], call["phase"], call["resume"],
                                call["mtop"])
    want = [(l["name"], l["grid"], l["block"], l["lds"]) for l in call["launches"]]
    assert stages == want
    assert flags["error"] == "none"


def test_the_trace_covers_every_kernel_the_search_can_launch():
    """The kernels of csrc/search_plan.h's three lists, spelled as the trace prints them."""
    src = open(os.path.join(REPO, "pfann_amd", "csrc", "search_plan.h")).read()
    names = set()
    for line in src.splitlines():
        line = line.strip().rstrip("\\").strip()
        if line.startswith("X(") and line.endswith(")") and "#" not in line:
            names.add(" ".join(line[2:-1].split(",", 1)[1].split()))
    assert len(names) == 46
    traced = {l["name"] for c in CALLS for l in c["launches"]}
    assert names - traced == set()
    assert traced - names == set()


def test_same_shape_same_bytes():
    a = search_plan(1000050, 128, 10000, 100, F32_COPY)
    for _ in range(3):
        assert search_plan(1000050, 128, 10000, 100, F32_COPY) == a
    assert a[1]["path"] == "gmax" and a[1]["canonical_scores"] == "1"


@pytest.mark.parametrize("shape,error", [
    (dict(n=1000, d=128, nq=5, k=0), "k"),
    (dict(n=1000, d=128, nq=5, k=1025), "k"),
    (dict(n=1000, d=126, nq=5, k=10), "d%4"),
    (dict(n=1 << 32, d=128, nq=5, k=10), "n>=2^32"),
    (dict(n=1000, d=1028, nq=5, k=10), "d>1024"),
    # fp32 rows only, ladder with R = 16: 300 M rows put the coarsest level at stride 16^5, and 32 rows of a sub-tile at that
    # stride span more than the 2 GB a buffer offset addresses
    (dict(n=300 * 1000 * 1000, d=128, nq=100, k=100, storage=F32), "stride_window"),
])
def test_error_exits(shape, error):
    stages, flags = search_plan(storage=shape.pop("storage", F32_COPY), **shape)
    assert stages == [] and flags["error"] == error


def test_the_dense_level_never_exceeds_the_survivor_slots():
    """The `dense level above CAP` exit guards an invariant of the ladder (the coarsest level holds <= 4096 <= CAP rows):
    no shape reaches it."""
    for n in (4096, 4097, 8193, 65537, 10 ** 6, 10 ** 9, (1 << 32) - 1):
        for k in (1, 128, 129, 512, 513, 1024):
            for storage, d in ((F32, 96), (F32_COPY, 96), (F16, 96)):
                assert search_plan(n, d, 100, k, storage)[1]["error"] in ("none", "stride_window")


def test_strides_beyond_the_tile_window_plan_the_generic_kernels():
    """k = 300 (ladder, R = 4) on 1.2 G rows: the first thresholded level samples every 4^9-th row, more than the
    query-stationary kernel's 2 GB tile window spans (127 * stride * 2 d + 2 d <= 0x7FFFFFF0: stride <= 66051 at d = 128)."""
    stages, flags = search_plan(1200 * 1000 * 1000, 128, 1000, 300, F32_COPY)
    assert flags["path"] == "ladder_f16" and flags["error"] == "none"
    scans = [s[0] for s in stages if s[0].startswith("scan_")]
    assert len(scans) == 11                                         # strides 4^10 (dense), 4^9, ..., 4, 1
    assert scans[0].startswith("scan_f16_kernel<") and scans[1].startswith("scan_f16_kernel<")
    assert all(s == "scan_f16_qres_kernel<8, false, 128, 2>" for s in scans[2:-1])
    assert scans[-1].startswith("scan_f16_qres_kernel<8, false, 64, ")


def _child(env, code):
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n" % (
        REPO, os.path.join(REPO, "tests")) + code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_scan_s_is_clamped_to_the_sub_list_counters():
    """PFANN_SCAN_S=100 used to give 400 private lists per row where cnt and the selects' s_off hold 256 (4 S <= NSUB_MAX)."""
    code = ("import json\nfrom pfann_amd.database import search_plan\n"
            "print(json.dumps([search_plan(1000050, 128, nq, 100, 1)[0] for nq in (33, 1000, 10000)]))")
    for plans in (_child({"PFANN_SCAN_S": "100"}, code), _child({"PFANN_SCAN_S": "64"}, code)):
        for nq, stages in zip((33, 1000, 10000), plans):
            full = [s for s in stages if s[0].startswith("scan_f16_qres_kernel<8, false")]
            assert len(full) == 1 and full[0][1] == -(-nq // 128) * 64
    stages = _child({"PFANN_SCAN_S": "7"}, code)[1]
    assert [s[1] for s in stages if s[0].startswith("scan_f16_qres_kernel<8, false")] == [8 * 7]


SWEEP_NQ = (1, 32, 33, 64, 65, 1000)
SWEEP_D = (16, 64, 96, 128, 256)
SWEEP_N = (0, 100, 8192, 8193, 60001, 1000050)


def _sweep(no_copy=False):
    """[(case, rescoring_path's answer, the plan's canonical_scores)] over the sweep, for shards of unit rows."""
    out = []
    for n in SWEEP_N:
        for d in SWEEP_D:
            for nq in SWEEP_NQ:
                for storage in ("f32", "f16"):
                    for prefilter in (True, False):
                        # what pfann_db_load / pfann_db_set_prefilter hand to the search (csrc/api.hip)
                        has_copy = storage == "f32" and d % 8 == 0 and not no_copy and n > 0
                        st = F16 if storage == "f16" else (F32_COPY if has_copy and prefilter else F32)
                        flags = search_plan(n, d, nq, 100, st)[1]
                        out.append(((n, d, nq, storage, prefilter), score_bits.rescoring_path_of_shape(n, d, nq, 1.0, prefilter, storage),
                                    flags["canonical_scores"] == "1"))
    return out


def test_rescoring_path_is_the_plans_canonical_scores(monkeypatch):
    monkeypatch.delenv("PFANN_NO_F16_PREFILTER", raising=False)
    monkeypatch.delenv("PFANN_SMALL_F32", raising=False)
    bad = [c for c, a, b in _sweep() if a != b]
    assert bad == []
    monkeypatch.setenv("PFANN_NO_F16_PREFILTER", "1")
    res = _sweep(no_copy=True)
    assert [c for c, a, b in res if a != b] == [] and not any(a for _, a, _ in res)


def test_rescoring_path_is_the_plans_canonical_scores_with_small_f32():
    res = _child({"PFANN_SMALL_F32": "1"},
                 "import json, test_search_plan as t\nprint(json.dumps([[c, a, b] for c, a, b in t._sweep()]))")
    assert [c for c, a, b in res if a != b] == []
    flipped = [c for c, a, b in res if not a and c[3] == "f32" and c[4] and c[2] <= 32 and c[1] in (64, 128) and c[0] > 8192]
    assert len(flipped) == 3 * 2 * 2          # n in (8193, 60001, 1000050), d in (64, 128), nq in (1, 32)
