"""The launch plan of the encoder (csrc/encoder_plan.h, exported as pfann_encode_plan) on the CPU.

The expected plans do not come from the code under test: profiles/encoder_plan/parent_launches.json is a rocprofv3 kernel
trace (tools/encoder_plan_trace.py) of the commit BEFORE the plan existed, one entry per pfann_encode call -- the kernels
the old dispatch launched for every case of tests/encoder_tap_cases.py, without taps and in taps mode 1, with grid, workgroup
size and dynamic LDS bytes.  The plan must print exactly that list for every entry.  The invariants below are written out
here and not read from the plan."""
import json
import os

import numpy as np
import pytest

import encoder_tap_cases as tc
from pfann_amd import synth
from pfann_amd.engine import encode_plan

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACE = json.load(open(os.path.join(REPO, "profiles", "encoder_plan", "parent_launches.json")))
KERNELS, CALLS = TRACE["kernels"], TRACE["calls"]
T, F = "true", "false"

# every kernel instantiation launch_conv_gemm_ln, launch_myg_ln, encode_chunk_fused and the unfused launchers can name
GEMM_LN = (["conv_gemm_ln_w22_kernel<%s, %s>" % (a, b) for a in (T, F) for b in (T, F)] +
           ["conv_gemm_ln_kernel<128, 128, 64, 32, %s, %s, true, 32, false, false>" % (a, b) for a in (T, F) for b in (T, F)] +
           ["conv_gemm_ln_kernel<128, 128, 64, 32, true, %s, true, 32, true, false>" % b for b in (T, F)] +
           ["conv_gemm_ln_kernel<64, 64, 32, 32, %s, false, true, 32, false, true>" % a for a in (T, F)] +
           ["conv_gemm_ln_kernel<64, 64, 32, 32, %s, %s, %s, 32, false, false>" % (a, b, c) for a in (T, F) for b in (T, F) for c in (T, F)])
OTHER = ["conv_first_stats_kernel", "conv_first_gram_stats_kernel", "conv_dw_ln_kernel<true>", "conv_dw_ln_kernel<false>", "ln_finalize_kernel",
         "splitk_reduce_ln_kernel", "ln_apply_kernel", "myg_ln_small_kernel", "myg_ln_kernel<4, 8>", "myg_ln_kernel<1, 32>",
         "conv_first_kernel", "conv_dw_kernel", "conv_gemm_kernel<128, 128, 64, 64>", "conv_gemm_kernel<64, 64, 32, 32>", "ln_act_kernel<256>",
         "ln_act_kernel<1024>", "myg_kernel"]
NOT_TRACED = {
    # ReLU after LayerNorm, first conv folded in, 128-row tiles, neither the five-block kernel nor the fp16 split: the
    # five-block kernel takes every such layer of the golden configs at precision 0 and the split takes it at precision 1;
    # only PFANN_NO_W22 / PFANN_NO_W22_FIRST lead here (checked from the plan in a child process below)
    "conv_gemm_ln_kernel<128, 128, 64, 32, true, true, true, 32, false, false>",
}
PLAN_BATCHES = (0, 65, 256, 304, 9728)


def _plan_list(call):
    launches, flags = encode_plan(tc.model_cfg(call["model"]), call["B"], call["plan_batch"], call["precision"], call["fused"], call["taps"])
    return [(l["name"], l["grid"], l["block"], l["lds"]) for l in launches], flags


@pytest.mark.parametrize("call", CALLS, ids=lambda c: "%s-taps%d" % (c["case"], c["taps"]))
def test_plan_prints_the_launches_of_the_old_dispatch(call):
    got, flags = _plan_list(call)
    assert got == [(KERNELS[k], g, b, l) for k, g, b, l in call["launches"]]
    assert flags["chunks"] == 1


def test_the_trace_holds_every_case_in_both_taps_modes():
    assert [(c["case"], c["taps"]) for c in CALLS] == [(tc.case_id(case), taps) for case in tc.CASES for taps in (0, 1)]
    for c, case in zip(CALLS[::2], tc.CASES):
        assert (c["model"], c["plan_batch"], c["B"], c["precision"], c["fused"]) == case


def test_the_trace_covers_every_kernel_the_encoder_can_launch():
    assert len(set(GEMM_LN)) == 20 and len(set(OTHER)) == 17
    assert set(GEMM_LN + OTHER) - set(KERNELS) == NOT_TRACED
    assert set(KERNELS) - set(GEMM_LN + OTHER) == set()


def test_the_untraced_instantiation_is_what_the_switch_selects():
    import subprocess
    import sys
    code = ("import sys; sys.path[:0] = [%r, %r, %r]\nimport encoder_tap_cases as tc\nfrom pfann_amd.engine import encode_plan\n"
            "print([l['name'] for l in encode_plan(tc.model_cfg('default'), 19, 9728)[0] if l['layer'] == 1][-1])"
            % (REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "tests", "golden")))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PFANN_NO_W22_FIRST="1"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] in NOT_TRACED


@pytest.mark.parametrize("case", tc.CASES, ids=tc.case_id)
def test_every_case_names_the_variant_the_plan_and_the_trace_show(case):
    want = tc.VARIANT[tc.case_id(case)]
    assert tc.signature(tc.case_plan(case)[0]) == want
    call = CALLS[2 * tc.CASES.index(case)]
    assert tc.signature([{"name": KERNELS[k]} for k, _, _, _ in call["launches"]]) == want


def test_the_case_list_stands_on_each_side_of_every_seam():
    """The issue's seam batches of the default model came from a restatement of the predicates; the plan, which the trace
    above pins, shows the same 30 (none had to be corrected).  The other models' tables are held against their plans too."""
    default_B = [c[2] for c in tc.CASES if c[:2] == ("default", 0) and c[3:] == (0, 1)]
    assert default_B[0] == 1 and default_B[1:] == tc.seams("default", 1, 1100, 0, 1)
    for model in tc.GOLDEN_MODELS:
        if model != "default":
            assert list(tc.OTHER_SEAMS[model]) == tc.seams(model), model


def _shapes(params):
    """(rows per sample, C_out) of the 16 sub-layers and the partial slots pfann_create allocates per sample."""
    rps = tc.rows_per_sample(params)
    co = [c for L in synth.layer_plan(params) for c in (L["co"], L["co"])]
    slots = max((r // 64 if r >= 64 else 1) * -(-c // 64) for r, c in zip(rps, co))
    return rps, co, slots


@pytest.mark.parametrize("model", tc.GOLDEN_MODELS)
def test_plan_invariants_over_every_batch(model):
    params = tc.model_params(model)
    cfg = tc.model_cfg(model, 1100)
    rps, co, slots = _shapes(params)
    for pb in PLAN_BATCHES:
        pinned = None
        for B in range(1, 1101):
            launches, flags = encode_plan(cfg, B, pb)
            assert flags["part_slots"] == slots and flags["chunks"] == 1
            choice = []
            for l in launches:
                i = l["layer"]
                if l["tile"] == 0:
                    assert l["out_P"] <= slots
                    if l["name"] not in ("ln_finalize_kernel", "splitk_reduce_ln_kernel"):
                        choice.append((i, l["name"]))
                    continue
                M, N, t = B * rps[i], co[i], l["tile"]
                assert l["grid"] == -(-M // t) * -(-N // t) * max(l["n_splits"], 1), (pb, B, l)
                assert (1 <= l["out_P"] <= slots) if flags["fused"] else l["out_P"] == 0, (pb, B, l)        # (unfused: no partials)
                if l["n_splits"]:
                    assert l["n_splits"] > 1 and flags["fused"] == 1
                    assert l["n_splits"] * M * N * 4 <= flags["splitk_bytes"] <= 256 << 20, (pb, B, l)
                choice.append((i, l["name"], t, l["n_splits"], l["first"], l["out_P"]))
            if pb and B <= max(pb, 65):
                pinned = pinned or choice
                assert choice == pinned, "plan %d: the kernel choice at B = %d differs from B = 1" % (pb, B)


def test_stream_chunks_run_the_calls_kernels_on_disjoint_scratch():
    """The stream count never changes a kernel choice: every chunk launches the kernel variants of the single-stream call,
    with the grids of its own share, and its split layers' partials fit a slice of the scratch no other chunk touches.
    385 samples under plan 304 is the batch ABOVE the plan, which the single-stream call does not split."""
    params = tc.model_params("default")
    cfg = tc.model_cfg("default")
    rps, co, _ = _shapes(params)
    for pb, B, ns, sizes in ((304, 304, 2, [152, 152]), (304, 385, 3, [129, 128, 128]), (9728, 385, 3, [129, 128, 128]), (0, 385, 3, [129, 128, 128]),
                             (0, 304, 2, [152, 152]), (304, 255, 2, [255]), (0, 1024, 8, [128] * 8)):
        launches, flags = encode_plan(cfg, B, pb, streams=ns)
        one = encode_plan(cfg, B, pb)[0]
        info = flags["chunk_info"]
        assert [c["B"] for c in info] == sizes and [c["b0"] for c in info] == [int(v) for v in np.cumsum([0] + sizes[:-1])]
        end = 0
        for k, c in enumerate(info):
            mine = [l for l in launches if l["chunk"] == k]
            pick = lambda ls: [(l["name"], l["block"], l["lds"], l["layer"], l["tile"], l["n_splits"], l["first"], l["out_P"]) for l in ls]
            assert pick(mine) == pick(one), (pb, B, k)
            need = 0
            for l in mine:
                if l["tile"]:
                    M, N, t = c["B"] * rps[l["layer"]], co[l["layer"]], l["tile"]
                    assert l["grid"] == -(-M // t) * -(-N // t) * max(l["n_splits"], 1)
                    need = max(need, l["n_splits"] * M * N * 4)
            assert c["splitk_bytes"] == need and c["splitk_offset"] >= end and c["splitk_offset"] % 256 == 0
            end = c["splitk_offset"] + c["splitk_bytes"]
        assert end <= flags["splitk_bytes"]
    split = lambda pb, B, ns: any(l["n_splits"] > 1 for l in encode_plan(cfg, B, pb, streams=ns)[0])
    assert split(304, 304, 2) and not split(304, 385, 3) and not split(9728, 385, 3) and split(0, 385, 3)


def test_taps_mode_2_leaves_the_production_plan_alone():
    for case in tc.CASES:
        off = [l for l in tc.case_plan(case, taps=0)[0]]
        on = [l for l in tc.case_plan(case, taps=2)[0] if l["name"] != "ln_apply_kernel"]
        assert on == off, case
        kept = [l["layer"] for l in tc.case_plan(case, taps=2)[0] if l["name"] == "ln_apply_kernel"]
        assert kept in ([], list(range(1, 16)))          # (the unfused path copies its taps: no kernel)


def test_the_plan_text_of_eight_streams_with_taps_fits():
    launches, flags = encode_plan(tc.model_cfg("default"), 1024, 304, taps=2, streams=8)
    assert flags["chunks"] == 8 and len({l["chunk"] for l in launches}) == 8


def test_taps_mode_2_keeps_tap_0_where_the_first_conv_is_not_folded():
    import subprocess
    import sys
    code = ("import sys; sys.path[:0] = [%r, %r, %r]\nimport encoder_tap_cases as tc\nfrom pfann_amd.engine import encode_plan\n"
            "ls, fl = encode_plan(tc.model_cfg('default'), 19, 9728, taps=2)\n"
            "print(fl['fold_first'], [l['layer'] for l in ls if l['name'] == 'ln_apply_kernel'])"
            % (REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "tests", "golden")))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PFANN_NO_FOLD_FIRST="1"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == "0 %r" % list(range(16))
