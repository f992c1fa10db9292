"""Float64 differential tests of the encoder (csrc/encoder_fused.hip, csrc/encoder.hip) on every kernel variant, at each
seam of the launch plan.  Cases, inputs, oracle and measurement: tests/encoder_tap_cases.py.

Every case first asserts, through pfann_encode_plan, the kernel variant it is there for (tests/test_encoder_plan.py pins
that plan to a kernel trace of the commit before it existed), then compares on the GPU
  * all B embeddings, normalised and raw,
  * taps 1..15 in taps mode 2 -- the production plan, first conv folded -- at three windows of 8 samples: the first 8, the
    last 8, and the 8 that straddle the first 128-row tile boundary of the deepest 128-tile layer,
  * all 16 taps in mode 1 for the first 8 samples
with the float64 evaluation of the same op sequence (oracle/encoder.py, on the host).

Bars.  The yardstick is the reference itself: the fp32 oracle's own distance from float64 at that tap (max-abs error over
max(1, max |tap|), per sample) or at the embedding (max-abs), taken as the maximum over the 13 pool windows.  The GPU may be
FACTOR = 4 times as far: the project's 2x (test_gpu_error_budget.py, over 5,000 windows) doubled because a maximum over 13
windows is a noisier yardstick; it is the allowance for two fp32 evaluations that differ in summation order and in the form
of the LayerNorm statistics.  One tap has a stated factor of its own, 8: sub-layer 13 (K = 3072) of the unfused path, measured
5.67x on the half-silent window (what is and is not known of the cause: encoder_tap_cases.UNFUSED_TAP13_FACTOR).
No bar goes above 2e-5 on a tap or 5e-6 on an embedding, normalised or raw.  Measured ratios of every
case: profiles/encoder_taps/ratios.json (tools/encoder_tap_ratios.py), summarised in DESIGN.md."""
import numpy as np
import pytest

import encoder_tap_cases as tc

pytestmark = pytest.mark.gpu

_state = {}


def _model(model):
    """One engine and one oracle at a time (the cases are grouped by model)."""
    import torch
    from pfann_amd.engine import Engine
    if _state.get("model") != model:
        _state.clear()
        assert torch.cuda.is_available(), "GPU tests need an MI355X"
        orc = tc.Oracle(model)
        eng = Engine(orc.params, 0, max_batch=tc.MAX_BATCH)
        eng.load_state_dict(orc.sd)
        default_fused = eng.set_fused_layernorm(True)
        _state.update(model=model, orc=orc, eng=eng, default_fused=default_fused, x=torch.as_tensor(orc.x).cuda())
    return _state["eng"], _state["orc"], _state["x"], _state["default_fused"]


def _bars(orc, is_fused=True):
    factors = tc.tap_factors(orc.params, is_fused)
    return ([min(f * r, tc.TAP_CAP) for f, r in zip(factors, orc.ref_tap)], min(tc.FACTOR * orc.ref_emb, tc.EMB_CAP), min(tc.FACTOR * orc.ref_raw, tc.EMB_CAP))


@pytest.mark.parametrize("case", tc.CASES, ids=tc.case_id)
def test_encoder_case_vs_float64(case):
    eng, orc, x, default_fused = _model(case[0])
    launches, flags = tc.case_plan(case)
    assert tc.signature(launches) == tc.VARIANT[tc.case_id(case)]
    assert flags["fused"] == (default_fused if case[4] < 0 else case[4])
    m = tc.measure_case(eng, orc, case, x, default_fused)
    tap_bar, emb_bar, raw_bar = _bars(orc, bool(flags["fused"]))
    worst2 = max(max(v) for v in m["mode2_ratio"].values())
    print("%s [%s]: emb %.2fx (%.2e) raw %.2fx (%.2e) taps mode 2 %.2fx mode 1 %.2fx of the fp32 oracle's distance from float64"
          % (m["case"], tc.VARIANT[m["case"]], m["emb_ratio"], m["emb_err"], m["raw_ratio"], m["raw_err"], worst2, max(m["mode1_ratio"])))
    assert m["emb_err"] <= emb_bar, "normalised embeddings: %.3e > %.3e" % (m["emb_err"], emb_bar)
    assert m["raw_err"] <= raw_bar, "raw embeddings: %.3e > %.3e" % (m["raw_err"], raw_bar)
    assert m["mode2_same_bits"], "taps mode 2 changed the embeddings' bits"
    if flags["fused"]:
        assert "tap 0 is absent" in m["tap0_absent"], m["tap0_absent"]
    for first, errs in m["mode2"].items():
        for i, e in enumerate(errs, 1):
            assert e <= tap_bar[i], "mode 2, samples from %d, tap %d: %.3e > %.3e" % (first, i, e, tap_bar[i])
    for i, e in enumerate(m["mode1"]):
        assert e <= tap_bar[i], "mode 1, tap %d: %.3e > %.3e" % (i, e, tap_bar[i])


# ----------------------------------------------------------------------------------------------------------- streams
def _encode_streams(eng, x, n):
    assert eng.set_streams(n) == n
    out = eng.encode(x, norm=True).cpu().numpy()
    eng.set_streams(1)
    return out


@pytest.mark.parametrize("plan", [304, 9728])
def test_streams_keep_the_pinned_plans_bits(plan):
    """The stream count changes no kernel choice (include/pfann_amd.h): 304 samples on 2 streams (152 + 152) and 385 on 3
    (129 + 128 + 128) against the single-stream call.  Plan 304 splits K on the deep layers of the 304-sample call -- which
    the parent of this test ran unsplit on more than one stream, other bits -- and, like the single-stream call, not of the
    385-sample one (a batch above the plan); plan 9728 splits nothing."""
    import torch
    eng, orc, x, default_fused = _model("default")
    tc.setup_engine(eng, ("default", plan, 1, 0, 1), default_fused)
    eng.debug_keep_at(0)
    assert any(l["n_splits"] > 1 for l in eng.encode_plan(304, plan, streams=2)[0]) == (plan == 304)
    assert not any(l["n_splits"] > 1 for l in eng.encode_plan(385, plan, streams=3)[0])
    for B, n in ((304, 2), (385, 3)):
        assert len(eng.encode_plan(B, plan, streams=n)[1]["chunk_info"]) == n
        xb = x[torch.as_tensor(tc.batch_rows(B), device=x.device)].contiguous()
        one = _encode_streams(eng, xb, 1)
        many = _encode_streams(eng, xb, n)
        assert np.array_equal(one, many), "%d samples on %d streams: %d rows differ from the single-stream call, max %.3e" % (
            B, n, int((one != many).any(axis=1).sum()), np.abs(one - many).max())
    eng.set_plan_batch(0)


def test_streams_unpinned_stay_within_the_bar():
    """Unpinned, every chunk runs the variants of the whole call's own plan (both calls split K on sub-layers 9..15): each row
    within the embedding bar of the cases above, and the single-stream call's bits."""
    import torch
    eng, orc, x, default_fused = _model("default")
    tc.setup_engine(eng, ("default", 0, 1, 0, 1), default_fused)
    eng.debug_keep_at(0)
    _, emb_bar, _ = _bars(orc)
    for B, n in ((304, 2), (385, 3)):
        rows = tc.batch_rows(B)
        xb = x[torch.as_tensor(rows, device=x.device)].contiguous()
        assert any(l["n_splits"] > 1 for l in eng.encode_plan(B, 0, streams=n)[0])
        many = _encode_streams(eng, xb, n)
        err = np.abs(many - orc.emb[rows]).max(axis=1)
        print("unpinned, %d samples on %d streams: worst row %.2fx of the fp32 oracle's distance from float64" % (B, n, err.max() / orc.ref_emb))
        assert err.max() <= emb_bar, "row %d: %.3e > %.3e" % (int(err.argmax()), err.max(), emb_bar)
        assert np.array_equal(many, _encode_streams(eng, xb, 1))
