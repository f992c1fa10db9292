"""Every kernel instantiation the search can launch (the six lists of csrc/search_plan.h) is reached by a shape that a GPU
test holds against an exact reference: the registry of those shapes, tests/search_kernel_cases.py, put through the launch
plan on the CPU, under default tuning.  tests/test_search_plan.py proves that the plan PRINTS each launch; this proves that
each kernel has a case that checks what it COMPUTES."""
import json
import os
import subprocess
import sys

import pytest

import search_kernel_cases as skc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LISTS = ("PF_SCAN_KERNELS", "PF_SCAN_F16_KERNELS", "PF_AUX_KERNELS", "PF_SCAN_EXCL_KERNELS", "PF_SCAN_F16_EXCL_KERNELS",
         "PF_AUX_EXCL_KERNELS")
# the A/B switches of the search (search_plan.h SearchTuning, api.hip's fp16 copy): read once per process by the library
SWITCHES = ("PFANN_SMALL_F32", "PFANN_NO_FOLDED_SMALL", "PFANN_NO_GMAX", "PFANN_QRES_MIN_NQ", "PFANN_GMAX_S", "PFANN_NO_QRES",
            "PFANN_SCAN_DBR128", "PFANN_SCAN_S", "PFANN_SCAN_NBUF3", "PFANN_NO_WAVE_SELECT", "PFANN_NO_WAVE_GROUP_SELECT",
            "PFANN_NO_F16_PREFILTER")

# The cases added for a kernel no older test held against an exact answer -> that kernel.  Stated here a second time on
# purpose: a case that leaves the registry takes its own `kernels` with it, and this table still names what it was for.
ADDED_FOR = {
    "small64_f32": ["scan_small_kernel<64, 4, 1>", "scan_small_kernel<64, 4, 0>", "topk_fallback_kernel<4>"],
    "small64_f32_excl": ["scan_small_kernel<64, 4, 1, true>", "scan_small_kernel<64, 4, 0, true>", "topk_fallback_kernel<4, true>"],
    "emit32_f32": ["scan_emit_kernel<32, 128, 32, 32, 1>"],
    "small64_f16_dense": ["scan_small_kernel<64, 2, 2>"],
    "small64_f16_dense_excl": ["scan_small_kernel<64, 2, 2, true>"],
    "small64_f16_dense_n8192": ["scan_small_kernel<64, 2, 2>"],
    "small64_f16_dense_n8192_excl": ["scan_small_kernel<64, 2, 2, true>"],
    "emit_qt4": ["scan_emit_kernel<128, 128, 64, 64, 4>"],
    "emit_qt4_excl": ["scan_emit_kernel<128, 128, 64, 64, 4, true>"],
    "emit_qt4_d36": ["scan_emit_kernel<128, 128, 64, 64, 4>"],
    "f16_qt4": ["scan_f16_kernel<4>"],
    "f16_qt4_excl": ["scan_f16_kernel<4, true>"],
    "f16_qt4_half": ["scan_f16_kernel<4>"],
    "dbr64_nbuf2_excl": ["scan_f16_qres_kernel<8, false, 64, 2, true>"],
    "wave16_full": ["group_max_select_wave_kernel<16>"],
    "wave16_full_excl": ["group_max_select_wave_kernel<16>"],
    "wave16_bench_d128_copy": ["group_max_select_wave_kernel<16>"],
    "wave16_bench_d128_f16": ["group_max_select_wave_kernel<16>"],
    "wave16_bench_d64_copy": ["group_max_select_wave_kernel<16>"],
    "wave16_bench_d64_f16": ["group_max_select_wave_kernel<16>"],
    "wave_topm_copy_shard0_bound": ["group_max_select_wave_kernel<16>"],
    "wave_topm_copy_shard1_bound": ["group_max_select_wave_kernel<16>"],
    "wave_topm_copy_shard2_bound": ["group_max_select_wave_kernel<16>"],
    "wave_topm_f16_shard0_bound": ["group_max_select_wave_kernel<16>"],
    "wave_topm_f16_shard1_bound": ["group_max_select_wave_kernel<16>"],
    "wave_topm_f16_shard2_bound": ["group_max_select_wave_kernel<16>"],
    "wave8_topm_shard0_bound": ["group_max_select_wave_kernel<8>"],
    "bound_none_20000_19_100_copy": ["bound_none_kernel"],
    "bound_none_20000_130_200_copy": ["bound_none_kernel"],
    "bound_none_20000_130_100_f32": ["bound_none_kernel"],
    "bound_none_0_130_100_copy": ["bound_none_kernel"],
}
# the group counts the wave16 cases were sized for: all 16 values of every lane, and the benchmark's launch group (13)
GROUPS = {"wave16_full": 1024, "wave16_full_excl": 1024, "wave16_bench_d128_copy": 832, "wave16_bench_d128_f16": 832,
          "wave16_bench_d64_copy": 832, "wave16_bench_d64_f16": 832}


def listed_kernels():
    """{list name: [kernel as a trace prints it]} of search_plan.h"""
    out, cur = {}, None
    for line in open(os.path.join(REPO, "pfann_amd", "csrc", "search_plan.h")).read().splitlines():
        line = line.strip().rstrip("\\").strip()
        if line.startswith("#define PF_") and "_KERNELS(" in line:
            cur = line.split()[1].split("(")[0]
            out[cur] = []
        elif cur and line[:2] in ("X(", "Y(") and line.endswith(")") and "#" not in line:
            out[cur].append(" ".join(line[2:-1].split(",", 1)[1].split()))
        elif not line.startswith("//"):
            cur = None
    return {name: v for name, v in out.items() if v}            # (PF_ALL_SEARCH_KERNELS joins the six: no entries of its own)


def plans_of(c, search_plan):
    """the launch plans of the case's call, one per chunk of query rows: [(kernel names, flags)]"""
    out = []
    for lo in range(0, c.nq, skc.CHUNK):
        nq = min(skc.CHUNK, c.nq - lo)
        st = skc.plan_storage(c)
        if c.phase == 0:
            stages, flags = search_plan(c.n, c.d, nq, c.k, st, excl=c.excl)
        elif c.phase == 1:
            stages, flags = search_plan(c.n, c.d, nq, c.k, st, phase=1, mtop=c.mtop)
        else:       # the bounded pass resumes only behind a bound that was left (search.hip: ws.bound_valid)
            left = search_plan(c.n, c.d, nq, c.k, st, phase=1, mtop=c.mtop)[1].get("leaves_bound") == "1"
            stages, flags = search_plan(c.n, c.d, nq, c.k, st, phase=2, resume_with_lb=left)
        assert flags["error"] == "none", (c, flags)
        out.append(([s[0] for s in stages], flags))
    return out


def _all_plans():
    from pfann_amd.database import search_plan
    return {c.name: plans_of(c, search_plan) for c in skc.CASES}


@pytest.fixture(scope="module")
def plans():
    """{case name: plans} under default tuning: a switch in the environment may already have been read by this process, so
    with one set the plans come from a child without it"""
    if not [v for v in SWITCHES if v in os.environ]:
        return _all_plans()
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\nimport json, test_search_kernel_coverage as t\n"
            "print(json.dumps(t._all_plans()))" % (REPO, os.path.join(REPO, "tests")))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return {k: [(names, flags) for names, flags in v] for k, v in json.loads(r.stdout.strip().splitlines()[-1]).items()}


def reached(plans, without=()):
    return {kn for name, pl in plans.items() if name not in without for names, _ in pl for kn in names}


def test_the_six_lists_name_76_kernels():
    lists = listed_kernels()
    assert tuple(lists) == LISTS
    names = [kn for v in lists.values() for kn in v]
    assert len(names) == len(set(names)) == 76
    assert sum(len(lists[l]) for l in LISTS[:3]) == 46 and sum(len(lists[l]) for l in LISTS[3:]) == 30


def test_every_kernel_has_an_exact_answer_case(plans):
    names = {kn for v in listed_kernels().values() for kn in v}
    got = reached(plans)
    assert sorted(names - got) == [], "no registry case reaches %s" % sorted(names - got)
    assert sorted(got - names) == [], "the plan names kernels outside the lists of search_plan.h: %s" % sorted(got - names)


def test_every_case_reaches_the_kernels_it_names(plans):
    for c in skc.CASES:
        for kn in c.kernels:
            missing = [i for i, (names, _) in enumerate(plans[c.name]) if kn not in names]
            # (a ragged last chunk of query rows may be a smaller shape: the first chunk is the case)
            assert 0 not in missing, "%s no longer launches %s: %s" % (c.name, kn, plans[c.name][0][0])


def test_the_added_cases_are_in_the_registry_with_their_kernels():
    have = {c.name: c for c in skc.CASES}
    gone = {nm: kns for nm, kns in ADDED_FOR.items() if nm not in have}
    assert not gone, "cases left the registry; the kernels they were added for: %s" % gone
    short = {nm: [kn for kn in kns if kn not in have[nm].kernels] for nm, kns in ADDED_FOR.items()}
    assert not {nm: v for nm, v in short.items() if v}, "cases that no longer name the kernel they were added for: %s" % short


def test_the_wave_group_selects_run_with_topm(plans):
    """phase 1 of a sharded search (the group select writes the m best group maxima): both wave forms"""
    topm = {kn for c in skc.CASES if c.phase == 1 for names, fl in plans[c.name] if fl.get("leaves_bound") == "1" for kn in names}
    assert {"group_max_select_wave_kernel<8>", "group_max_select_wave_kernel<16>"} <= topm, sorted(topm)


def test_the_wave16_cases_have_the_group_counts_they_were_sized_for(plans):
    for nm, G in GROUPS.items():
        for names, flags in plans[nm]:
            assert flags["path"] == "gmax" and int(flags["groups"]) == G, (nm, flags)
    # masked rows: the wave select reads -inf group maxima with between 513 and 1024 groups
    assert skc.case("wave16_full_excl").excl


def test_every_case_belongs_to_a_test_that_exists():
    for mod in sorted({c.test.split("::")[0] for c in skc.CASES}):
        src = open(os.path.join(REPO, "tests", mod + ".py")).read()
        assert "search_kernel_cases" in src, "%s does not read the registry" % mod
        for fn in sorted({c.test.split("::")[1] for c in skc.CASES if c.test.startswith(mod + "::")}):
            assert "\ndef %s(" % fn in src, "%s::%s" % (mod, fn)
