"""Cases, inputs and plan helpers shared by tests/test_gpu_encoder_taps.py (float64 differential tests of the encoder on
the GPU), tests/test_encoder_plan.py (the launch plan on the CPU) and tools/encoder_plan_trace.py / tools/encoder_tap_ratios.py.

A case is (model, plan_batch, B, precision, fused): one pfann_encode call shape.  VARIANT[case_id] is the kernel-variant
signature the case is there for -- one letter per sub-layer and one for the head (signature() below) -- which the GPU test
asserts of pfann_encode_plan before it runs, and which tests/test_encoder_plan.py derives a second time from the kernel
trace of the commit before the plan existed.  Nothing here needs a GPU."""
import json
import os

import numpy as np

from pfann_amd import synth
from pfann_amd.config import config_from_params

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLDEN_MODELS = ("tiny", "nafstyle", "n640d64", "seg", "default", "elu_full", "strides_pow2", "strides_np2")
MAX_BATCH = 1024
POOL = 13          # no two equal windows of a batch sit a power of two apart (where tile or slot aliasing would put them)


def model_params(model):
    """The configs of test_encoder_vs_reference_golden, and "elu_pre_ln": the default model with ELU before LayerNorm."""
    if model == "elu_pre_ln":
        params = model_params("default")
        params["model"].update(conv_activation="ELU", relu_after_bn=False)
        return params
    return json.loads(str(np.load(os.path.join(HERE, "golden", "encoder_%s.npz" % model))["params"]))


def model_cfg(model, max_batch=MAX_BATCH):
    return config_from_params(model_params(model), max_batch)


def silence_floor(params):
    cfg = config_from_params(params, 8)
    return float({0: cfg.log_eps, 1: np.log(cfg.log_eps), 2: np.log10(cfg.log_eps)}[cfg.log_mode])


def pool(params):
    """The 13 windows every batch is drawn from (batch row b is pool[b % 13]): eight of normal * 3 - 6 noise, the silence
    floor, the floor + 0.01 * noise, a constant window at the floor, a window whose left half is the floor, and one window
    of the golden inputs."""
    import make_golden as mg
    _, _, _, F, T = synth.model_dims(params)
    floor = silence_floor(params)
    x = np.empty((POOL, F, T), np.float32)
    x[:8] = synth.normal(91, "t/taps/pool", 8 * F * T).reshape(8, F, T) * 3.0 - 6.0
    x[8] = floor
    x[9] = floor + 0.01 * synth.normal(92, "t/taps/near_floor", F * T).reshape(F, T)
    x[10] = np.float32(floor)                   # constant (x[8] and x[10]: equal windows 2 apart -- and 11, 15, 24 ... apart)
    x[11] = synth.normal(93, "t/taps/half", F * T).reshape(F, T) * 3.0 - 6.0
    x[11, :, :T // 2] = floor
    x[12] = mg.encoder_inputs(F, T)[0]
    return x


def batch_rows(B):
    return np.arange(B) % POOL


_LETTER = {"conv_first_gram_stats_kernel": "g", "conv_first_stats_kernel": "c", "conv_first_kernel": "c", "conv_dw_kernel": "d",
           "conv_dw_ln_kernel<false>": "d", "conv_dw_ln_kernel<true>": "d*", "myg_ln_small_kernel": "S", "myg_ln_kernel<4, 8>": "4",
           "myg_ln_kernel<1, 32>": "1", "myg_kernel": "m", "conv_gemm_kernel<128, 128, 64, 64>": "G", "conv_gemm_kernel<64, 64, 32, 32>": "s"}
_SKIP = ("ln_finalize_kernel", "ln_apply_kernel", "splitk_reduce_ln_kernel", "ln_act_kernel<256>", "ln_act_kernel<1024>")


def signature(launches):
    """One letter per sub-layer, then the head.  g / c: the first conv's statistics in Gram form / computed with the conv
    (unfused: the conv itself); W: five-block 128-tile kernel; G: plain 128-tile kernel; H: its fp16-split instantiation;
    s: 64-tile kernel; n: 64-tile kernel with C_in % 32 != 0; k: split-K 64-tile kernel + reduction; d: depthwise;
    `*` after a letter: the first conv folded into that layer's loader.  Head: S small-batch, 4 / 1: myg_ln_kernel<4, 8> /
    <1, 32>, m: the unfused head."""
    out = []
    for l in launches:
        if l.get("chunk", 0) != 0 or l["name"] in _SKIP:
            continue
        name = l["name"]
        if name in _LETTER:
            out.append(_LETTER[name])
            continue
        args = [a.strip() for a in name[name.index("<") + 1:-1].split(",")]
        if name.startswith("conv_gemm_ln_w22_kernel<"):
            c, first = "W", args[1]
        else:
            assert name.startswith("conv_gemm_ln_kernel<") and len(args) == 10, name
            c = ("H" if args[8] == "true" else "G") if args[0] == "128" else ("k" if args[9] == "true" else ("s" if args[6] == "true" else "n"))
            first = args[5]
        out.append(c + ("*" if first == "true" else ""))
    return "".join(out)


def tap_windows(launches, B):
    """first_sample of the three kept windows: the first 8, the last 8, and the 8 that straddle the first 128-row tile
    boundary of the deepest 128-tile layer whose tiles span samples (r = rows per sample < 128: sample 128 / r opens the second
    tile, the window starts 4 before it); the last 8 again when the batch has no such boundary.  launches: with_rows()."""
    last = max(0, B - 8)
    straddle = last
    for l in launches:
        if l["chunk"] == 0 and l["tile"] == 128 and l["rps"] < 128 and 128 // l["rps"] < B:
            straddle = min(max(0, 128 // l["rps"] - 4), last)
    return [0, last, straddle]


def rows_per_sample(params):
    """Fo * To of the 16 sub-layers."""
    out = []
    for L in synth.layer_plan(params):
        out += [L["F"] * L["T1"], L["F2"] * L["T1"]]
    return out


def with_rows(launches, params):
    rps = rows_per_sample(params)
    return [dict(l, rps=rps[l["layer"]]) if l["layer"] >= 0 else l for l in launches]


# (model, plan_batch, B, precision, fused)  -- fused: 1 / 0 as pfann_set_fused_layernorm, -1 the context's default
def _default_cases():
    c = []
    for B in (1, 23, 24, 31, 32, 47, 48, 63, 64, 65, 127, 128, 252, 253, 254, 255, 256, 496, 497, 504, 505, 510, 511, 992, 993, 1008, 1009,
              1016, 1017, 1020, 1021):
        c.append(("default", 0, B, 0, 1))
    for B in (1, 2, 3, 19, 63, 64, 65, 129):
        c.append(("default", 9728, B, 0, 1))
    for pb in (65, 256, 304):
        for B in (1, 19, 76):
            c.append(("default", pb, B, 0, 1))
    c += [("default", 9728, 19, 1, 1), ("default", 0, 512, 1, 1)]
    for model, fused in (("default", 0), ("elu_pre_ln", 1)):
        c += [(model, 0, 3, 0, fused), (model, 0, 130, 0, fused), (model, 9728, 19, 0, fused)]
    # (not in the issue's list: precision 1 without ReLU-after-LayerNorm has no fp16-split instantiation and no five-block
    # kernel -- the one way to the plain 128-tile kernel with the first conv folded in that needs no environment switch)
    c.append(("elu_pre_ln", 9728, 19, 1, 1))
    return c


# every other config of the golden test on its default path: each side of the seams its own plan shows below B = 320
# (tests/test_encoder_plan.py recomputes them from the plan and holds this table against them), plus plan 9728 at 1 and 19
OTHER_SEAMS = {
    "tiny": (64, 65), "nafstyle": (64, 65), "n640d64": (64, 65, 255, 256), "seg": (47, 48, 63, 64, 65, 127, 128, 252, 253),
    "elu_full": (64, 65), "strides_pow2": (64, 65), "strides_np2": (),
}


def _other_cases():
    c = []
    for model in GOLDEN_MODELS:
        if model == "default":
            continue
        for B in OTHER_SEAMS[model]:
            c.append((model, 0, B, 0, -1))
        c += [(model, 9728, 1, 0, -1), (model, 9728, 19, 0, -1)]
    c.append(("seg", 0, 3, 0, 0))           # the unfused depthwise kernel (conv_dw_kernel), which no default path runs
    return c


CASES = _default_cases() + _other_cases()


def case_id(case):
    model, pb, B, prec, fused = case
    return "%s-plan%d-B%d%s%s" % (model, pb, B, "-split" if prec else "", {1: "", 0: "-unfused", -1: ""}[fused])


def case_plan(case, taps=0, streams=1):
    """(launches with rows per sample, flags) of the case's call."""
    from pfann_amd.engine import encode_plan
    model, pb, B, prec, fused = case
    params = model_params(model)
    launches, flags = encode_plan(config_from_params(params, MAX_BATCH), B, pb, prec, fused, taps, streams)
    return with_rows(launches, params), flags


def seams(model, lo=1, hi=320, plan_batch=0, fused=-1):
    """Batches B in (lo, hi) whose kernel-variant signature differs from B - 1's: -> sorted [B - 1, B, ...] without repeats."""
    from pfann_amd.engine import encode_plan
    cfg = model_cfg(model)
    out, prev = set(), None
    for B in range(lo, hi):
        sig = signature(encode_plan(cfg, B, plan_batch, 0, fused, 0, 1)[0])
        if prev is not None and sig != prev:
            out.update((B - 1, B))
        prev = sig
    return sorted(out)


# ---- the float64 yardstick and the measurement of one case (needs a GPU only when called) -------------------------------
TAP_CAP, EMB_CAP = 2e-5, 5e-6       # no bar goes above these (include/pfann_amd.h promises fingerprints within 5e-6)
FACTOR = 4.0                        # GPU distance from float64 <= FACTOR x the fp32 oracle's own distance from float64


# The one tap with a stated factor of its own: sub-layer 13 of the unfused path where its K loop has 3072 products (the default
# model's shape: conv along F, 1024 -> 1024 channels, 2 rows per sample).  Measured (profiles/encoder_taps/ratios.json): 5.67 x
# (3.0e-6) on the half-silent pool window -- samples 122..129 of 130 and 11..18 of 19 -- and 3.72 x on the other windows; every
# other unfused tap is <= 3.72 x and stays at FACTOR.
# The step: the sum over K = 3072 in ONE chain of fp32 MFMA accumulations.  tools/encoder_tap_ratios.py --local splits a tap's
# error into what the layer inherits (the float64 layer applied to the GPU's own tap 12) and what its own kernels add:
#     tap 13, 13 pool windows     inherited   added by the layer
#     unfused                       3.2         4.1   (half-silent window: 2.1 + 4.1 -> 5.67 in total)
#     fused, PFANN_NO_SPLITK=1      2.4         4.3   (total 4.25: the same chain, the same step)
#     fused, split-K (chunks of 256) 1.6        0.6
# and taps 9..12 (K = 1536) add 1.0 .. 2.5 on either unsplit path.  So the chain is not special to conv_gemm_kernel: the fused
# 64-tile kernel adds as much wherever it runs sub-layer 13 unsplit (B >= 993, plan 65 above the plan); those cases measure
# <= 3.53 x on the windows they keep and stay at FACTOR.  On the host one chain is 3.9 .. 7.4 x as far from the float64 sum
# as chunks of 256 products (--chain), in line with sqrt(3072 / 268) = 3.4 for random rounding.
# The factor: what a tap inherits is bounded by its predecessor's bar (FACTOR) and what this one step adds measures FACTOR
# again; the two add at worst, hence 2 x FACTOR for this tap.  No kernel changes here; the 2e-5 cap stands.
UNFUSED_TAP13_K = 3072
UNFUSED_TAP13_FACTOR = 8.0


def tap_factors(params, is_fused):
    """FACTOR per tap; UNFUSED_TAP13_FACTOR for sub-layer 13 of the unfused path when its K = 3 C_in is UNFUSED_TAP13_K."""
    out = []
    for L in synth.layer_plan(params):
        for K in (3 * L["ci"], 3 if L["depthwise"] else 3 * L["co"]):          # conv1, conv2
            out.append(UNFUSED_TAP13_FACTOR if not is_fused and len(out) == 13 and K == UNFUSED_TAP13_K else FACTOR)
    return out


def tap_norm(got, want64):
    """Per sample: max-abs error over max(1, max |tap|)."""
    ax = tuple(range(1, want64.ndim))
    return np.abs(got.astype(np.float64) - want64).max(axis=ax) / np.maximum(1.0, np.abs(want64).max(axis=ax))


class Oracle:
    """oracle.encoder.encode on the 13 pool windows, once in fp32 and once in float64, on the host, with taps: every row of
    every batch has its expected embedding and taps from here (row b is window b % 13).  ref_*: the fp32 oracle's own distance
    from float64, the maximum over the 13 windows in the norm the GPU is measured in -- the yardstick of every bar."""

    def __init__(self, model):
        from oracle import encoder as oe
        self.model, self.params = model, model_params(model)
        self.sd = synth.make_state_dict(self.params, seed=123)
        self.x = pool(self.params)
        t32, self.taps = [], []
        emb32 = oe.encode(self.x, self.sd, self.params, norm=True, taps=t32)
        self.emb = oe.encode(self.x, self.sd, self.params, norm=True, taps=self.taps, dtype=np.float64)
        raw32 = oe.encode(self.x, self.sd, self.params, norm=False)
        self.raw = oe.encode(self.x, self.sd, self.params, norm=False, dtype=np.float64)
        self.ref_tap = [float(tap_norm(a, b).max()) for a, b in zip(t32, self.taps)]
        self.ref_emb = float(np.abs(emb32 - self.emb).max())
        self.ref_raw = float(np.abs(raw32 - self.raw).max())


def setup_engine(eng, case, default_fused):
    """Puts the engine into the case's state; -> whether the fused path runs."""
    model, pb, B, prec, fused = case
    want = default_fused if fused < 0 else bool(fused)
    assert eng.set_fused_layernorm(want) == want, case
    assert eng.set_encoder_precision(prec) == (prec if want else 0), case
    assert eng.set_plan_batch(pb) == pb, case
    assert eng.set_streams(1) == 1
    return want


def measure_case(eng, orc, case, x_pool_dev, default_fused):
    """Runs the case: all B embeddings (normalised and raw) with the taps off, taps 1..15 in mode 2 at the three windows of
    tap_windows(), and all 16 taps in mode 1 for the first 8 samples.  -> dict of errors (the norms above) and of
    ratios = error / the fp32 oracle's own distance from float64; "mode2_same_bits": mode 2 left the embeddings' bits alone;
    "tap0_absent": what asking for tap 0 in mode 2 on the fused path raised."""
    import torch
    from pfann_amd.lib import PfannError
    model, pb, B, prec, fused = case
    is_fused = setup_engine(eng, case, default_fused)
    launches, _ = case_plan(case)
    rows = batch_rows(B)
    x = x_pool_dev[torch.as_tensor(rows, device=x_pool_dev.device)].contiguous()
    eng.debug_keep_at(0)
    emb = eng.encode(x, norm=True).cpu().numpy()
    raw = eng.encode(x, norm=False).cpu().numpy()
    out = {"case": case_id(case), "emb_err": float(np.abs(emb - orc.emb[rows]).max()), "raw_err": float(np.abs(raw - orc.raw[rows]).max()),
           "mode2": {}, "mode2_same_bits": True, "tap0_absent": None}

    def taps(first, idxs):
        n = min(8, B)
        return [float(tap_norm(eng.debug_activation(i, n), orc.taps[i][rows[first:first + n]]).max()) for i in idxs]

    for first in sorted(set(tap_windows(launches, B))):
        assert eng.debug_keep_at(2, first) == 2
        out["mode2_same_bits"] &= bool(np.array_equal(eng.encode(x, norm=True).cpu().numpy(), emb))
        if is_fused:
            try:
                eng.debug_activation(0, min(8, B))
                out["tap0_absent"] = "tap 0 was returned"
            except PfannError as e:
                out["tap0_absent"] = str(e)
        out["mode2"][first] = taps(first, range(1, 16))
    eng.debug_keep_at(1, 0)
    eng.encode(x, norm=True)
    out["mode1"] = taps(0, range(16))
    eng.debug_keep_at(0)
    out["emb_ratio"] = out["emb_err"] / orc.ref_emb
    out["raw_ratio"] = out["raw_err"] / orc.ref_raw
    out["mode2_ratio"] = {f: [e / orc.ref_tap[i + 1] for i, e in enumerate(v)] for f, v in out["mode2"].items()}
    out["mode1_ratio"] = [e / orc.ref_tap[i] for i, e in enumerate(out["mode1"])]
    return out


# the signature each case is there for (see the module docstring)
VARIANT = {
    "default-plan0-B1":                "gs*ssskkkkkkkkkkkS",
    "default-plan0-B23":               "gs*ssskkkkkkkkkkkS",
    "default-plan0-B24":               "gs*sssskkkkkkkkkkS",
    "default-plan0-B31":               "gs*sssskkkkkkkkkkS",
    "default-plan0-B32":               "gW*sssskkkkkkkkkkS",
    "default-plan0-B47":               "gW*sssskkkkkkkkkkS",
    "default-plan0-B48":               "gW*ssssskkkkkkkkkS",
    "default-plan0-B63":               "gW*ssssskkkkkkkkkS",
    "default-plan0-B64":               "gW*WsssskkkkkkkkkS",
    "default-plan0-B65":               "gW*Wssskkkkkkkkkk4",
    "default-plan0-B127":              "gW*Wssskkkkkkkkkk4",
    "default-plan0-B128":              "gW*WWWsskkkkkkkkk4",
    "default-plan0-B252":              "gW*WWWsskkkkkkkkk4",
    "default-plan0-B253":              "gW*WWWsskskkkkkkk4",
    "default-plan0-B254":              "gW*WWWsskskkkkkkk4",
    "default-plan0-B255":              "gW*WWWsssskkkkkkk4",
    "default-plan0-B256":              "gW*WWWWssskkkkkkk4",
    "default-plan0-B496":              "gW*WWWWssskkkkkkk4",
    "default-plan0-B497":              "gW*WWWWssskkkskkk4",
    "default-plan0-B504":              "gW*WWWWssskkkskkk4",
    "default-plan0-B505":              "gW*WWWWssssskskkk4",
    "default-plan0-B510":              "gW*WWWWssssskskkk4",
    "default-plan0-B511":              "gW*WWWWWsssskskkk4",
    "default-plan0-B992":              "gW*WWWWWsssskskkk4",
    "default-plan0-B993":              "gW*WWWWWssssksssk4",
    "default-plan0-B1008":             "gW*WWWWWssssksssk4",
    "default-plan0-B1009":             "gW*WWWWWssssssssk4",
    "default-plan0-B1016":             "gW*WWWWWssssssssk4",
    "default-plan0-B1017":             "gW*WWWWWsGssssssk4",
    "default-plan0-B1020":             "gW*WWWWWsGssssssk4",
    "default-plan0-B1021":             "gW*WWWWWWGssssssk4",
    "default-plan9728-B1":             "gW*WWWWWWGWGWGWGG4",
    "default-plan9728-B2":             "gW*WWWWWWGWGWGWGG4",
    "default-plan9728-B3":             "gW*WWWWWWGWGWGWGG4",
    "default-plan9728-B19":            "gW*WWWWWWGWGWGWGG4",
    "default-plan9728-B63":            "gW*WWWWWWGWGWGWGG4",
    "default-plan9728-B64":            "gW*WWWWWWGWGWGWGG4",
    "default-plan9728-B65":            "gW*WWWWWWGWGWGWGG4",
    "default-plan9728-B129":           "gW*WWWWWWGWGWGWGG4",
    "default-plan65-B1":               "gW*Wssskkkkkkkkkk4",
    "default-plan65-B19":              "gW*Wssskkkkkkkkkk4",
    "default-plan65-B76":              "gW*Wsssssssssssss4",
    "default-plan256-B1":              "gW*WWWWssskkkkkkk4",
    "default-plan256-B19":             "gW*WWWWssskkkkkkk4",
    "default-plan256-B76":             "gW*WWWWssskkkkkkk4",
    "default-plan304-B1":              "gW*WWWWssskkkkkkk4",
    "default-plan304-B19":             "gW*WWWWssskkkkkkk4",
    "default-plan304-B76":             "gW*WWWWssskkkkkkk4",
    "default-plan9728-B19-split":      "gH*HHHHHHHHHHHHHH4",
    "default-plan0-B512-split":        "gH*HHHHHsssskskkk4",
    "default-plan0-B3-unfused":        "csssssssssssssssm",
    "default-plan0-B130-unfused":      "cGGGGsssssssssssm",
    "default-plan9728-B19-unfused":    "csssssssssssssssm",
    "elu_pre_ln-plan0-B3":             "cs*ssskkkkkkkkkkkS",
    "elu_pre_ln-plan0-B130":           "cW*WWWsskkkkkkkkk4",
    "elu_pre_ln-plan9728-B19":         "cW*WWWWWWGWGWGWGG4",
    "elu_pre_ln-plan9728-B19-split":   "cG*GGGGGGGGGGGGGG4",
    "tiny-plan0-B64":                  "gn*nnnsssssssssssS",
    "tiny-plan0-B65":                  "gn*nnnsssssssssss4",
    "tiny-plan9728-B1":                "gn*nnnsssssssssss4",
    "tiny-plan9728-B19":               "gn*nnnsssssssssss4",
    "nafstyle-plan0-B64":              "cd*ndndsdsdsdsdsdS",
    "nafstyle-plan0-B65":              "cd*ndndsdsdsdsdsd4",
    "nafstyle-plan9728-B1":            "cd*ndndsdsdsdsdsd4",
    "nafstyle-plan9728-B19":           "cd*ndndsdsdsdsdsd4",
    "n640d64-plan0-B64":               "gd*sdsdsdsdsdsdkdS",
    "n640d64-plan0-B65":               "gd*sdsdsdsdsdsdkd1",
    "n640d64-plan0-B255":              "gd*sdsdsdsdsdsdkd1",
    "n640d64-plan0-B256":              "gd*sdWdsdsdsdsdkd1",
    "n640d64-plan9728-B1":             "gd*sdWdWdGdGdGdGd1",
    "n640d64-plan9728-B19":            "gd*sdWdWdGdGdGdGd1",
    "seg-plan0-B47":                   "gd*sdsdkdkdkdkdkdS",
    "seg-plan0-B48":                   "gd*sdsdsdkdkdkdkdS",
    "seg-plan0-B63":                   "gd*sdsdsdkdkdkdkdS",
    "seg-plan0-B64":                   "gd*WdsdsdkdkdkdkdS",
    "seg-plan0-B65":                   "gd*Wdsdkdkdkdkdkd4",
    "seg-plan0-B127":                  "gd*Wdsdkdkdkdkdkd4",
    "seg-plan0-B128":                  "gd*WdWdsdkdkdkdkd4",
    "seg-plan0-B252":                  "gd*WdWdsdkdkdkdkd4",
    "seg-plan0-B253":                  "gd*WdWdsdsdkdkdkd4",
    "seg-plan9728-B1":                 "gd*WdWdWdGdGdGdGd4",
    "seg-plan9728-B19":                "gd*WdWdWdGdGdGdGd4",
    "elu_full-plan0-B64":              "cn*nnnsssssssssssS",
    "elu_full-plan0-B65":              "cn*nnnsssssssssss4",
    "elu_full-plan9728-B1":            "cn*nnnsssssssssss4",
    "elu_full-plan9728-B19":           "cn*nnnsssssssssss4",
    "strides_pow2-plan0-B64":          "cn*nnnsssssssssssS",
    "strides_pow2-plan0-B65":          "cn*nnnsssssssssss4",
    "strides_pow2-plan9728-B1":        "cn*nnnsssssssssss4",
    "strides_pow2-plan9728-B19":       "cn*nnnsssssssssss4",
    "strides_np2-plan9728-B1":         "csssssssssssssssm",
    "strides_np2-plan9728-B19":        "csssssssssssssssm",
    "seg-plan0-B3-unfused":            "cdsdsdsdsdsdsdsdm",
}
