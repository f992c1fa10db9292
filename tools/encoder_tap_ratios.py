#!/usr/bin/env python
"""The full table behind tests/test_gpu_encoder_taps.py: for every case of tests/encoder_tap_cases.py, the GPU's distance
from the float64 evaluation at every tap and at the embeddings, as a multiple of the fp32 oracle's own distance from float64
(the test's yardstick; its bar is 4).  Needs an MI355X.

    python tools/encoder_tap_ratios.py OUT.json          (the committed table: profiles/encoder_taps/ratios.json)
    python tools/encoder_tap_ratios.py --chain           (no GPU: see chain() below)
    python tools/encoder_tap_ratios.py --local unfused   (or: fused; see local() below)

OUT.json: {"reference": {model: the fp32 oracle's distance from float64 per tap and embedding}, "cases": [{case, variant,
emb_ratio, raw_ratio, mode1_ratio[16], mode2_ratio{first_sample: [15]}}], "worst_by_variant": {letter: [ratio, case, tap]}}.
A tap's ratio counts for the variant letter of the sub-layer that produced it (encoder_tap_cases.signature)."""
import json
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "tests", "golden")]


def main(out_path):
    import torch
    import encoder_tap_cases as tc
    from pfann_amd.engine import Engine
    state, ref, cases, worst = {}, {}, [], {}
    for case in tc.CASES:
        model = case[0]
        if state.get("model") != model:
            state.clear()
            orc = tc.Oracle(model)
            eng = Engine(orc.params, 0, max_batch=tc.MAX_BATCH)
            eng.load_state_dict(orc.sd)
            state.update(model=model, orc=orc, eng=eng, fused=eng.set_fused_layernorm(True), x=torch.as_tensor(orc.x).cuda())
            ref[model] = {"tap": orc.ref_tap, "emb": orc.ref_emb, "raw": orc.ref_raw}
        m = tc.measure_case(state["eng"], state["orc"], case, state["x"], state["fused"])
        letters = re.findall(r"[a-zA-Z0-9]\*?", tc.VARIANT[m["case"]])
        letters1 = re.findall(r"[a-zA-Z0-9]\*?", tc.signature(tc.case_plan(case, taps=1)[0]))       # mode 1: first conv not folded
        assert len(letters) == len(letters1) == 17, letters
        rows = [(r, letters1[i], "mode 1 tap %d" % i) for i, r in enumerate(m["mode1_ratio"])]
        for first, rs in m["mode2_ratio"].items():
            rows += [(r, letters[i + 1], "mode 2 from sample %d tap %d" % (first, i + 1)) for i, r in enumerate(rs)]
        rows += [(m["emb_ratio"], "head " + letters[16], "normalised embedding"), (m["raw_ratio"], "head " + letters[16], "raw embedding")]
        for r, letter, what in rows:
            if r > worst.get(letter, [0.0])[0]:
                worst[letter] = [round(r, 3), m["case"], what]
        cases.append({"case": m["case"], "variant": tc.VARIANT[m["case"]], "emb_ratio": round(m["emb_ratio"], 3), "raw_ratio": round(m["raw_ratio"], 3),
                      "emb_err": m["emb_err"], "mode1_ratio": [round(r, 3) for r in m["mode1_ratio"]],
                      "mode2_ratio": {str(f): [round(r, 3) for r in rs] for f, rs in m["mode2_ratio"].items()}})
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write('{"reference": %s,\n"worst_by_variant": %s,\n"cases": [\n%s\n]}\n' % (
            json.dumps(ref), json.dumps(worst, sort_keys=True), ",\n".join(json.dumps(c) for c in cases)))
    for letter in sorted(worst):
        print("%-8s %6.2fx  %s, %s" % ((letter,) + tuple(worst[letter])))


def chain():
    """How sensitive sub-layer 13 of the default model (K = 3072) is to the summation order, per pool window, on the host:
    from the float64 taps of sub-layer 12, summed (a) in ONE fp32 chain over K, as every kernel without split-K does, and (b) in
    chunks of 256 products, as the split-K path does; both against the float64 sum, as max error over the layer's standard
    deviation.  Background of encoder_tap_cases.UNFUSED_TAP13_FACTOR; local() below measures the same step on the GPU."""
    import numpy as np
    import encoder_tap_cases as tc
    from pfann_amd import synth
    o = tc.Oracle("default")
    L = synth.layer_plan(o.params)[6]
    w = np.asarray(o.sd["f.convs.6.conv2.weight"], np.float32)[:, :, :, 0]             # [co][ci][3]
    W = w.transpose(0, 2, 1).reshape(w.shape[0], -1)                                      # K order: tap, channel
    for win in range(tc.POOL):
        x = np.pad(o.taps[12][win, :, :, 0], ((0, 0), tuple(L["pad2"]))).astype(np.float32)
        A = np.stack([x[:, f * L["s_f"]:f * L["s_f"] + 3] for f in range(L["F2"])]).transpose(0, 2, 1).reshape(L["F2"], -1)
        P = A[:, None, :] * W[None, :, :]                                                 # fp32 products [Fo][co][K]
        exact = (A.astype(np.float64)[:, None, :] * W.astype(np.float64)[None, :, :]).sum(-1)
        one = np.cumsum(P, axis=-1, dtype=np.float32)[..., -1]
        chunked = np.zeros_like(one)
        for k0 in range(0, P.shape[-1], 256):
            chunked = chunked + np.cumsum(P[..., k0:k0 + 256], axis=-1, dtype=np.float32)[..., -1]
        e1, e2 = np.abs(one - exact).max() / exact.std(), np.abs(chunked - exact).max() / exact.std()
        print("window %2d: one chain %.2e, chunks of 256 %.2e of the layer's std: %.1f x" % (win, e1, e2, e1 / e2))


def local(path):
    """Where a deep tap's error comes from (default model, the 13 pool windows, taps 9..13, as multiples of the fp32 oracle's
    distance from float64): `carried` = the float64 evaluation of the sub-layer applied to the GPU's OWN previous tap, against
    the float64 tap -- error the layer inherits; `local` = the GPU's tap against that same evaluation -- error the layer's
    own kernels add.  path: unfused | fused (PFANN_NO_SPLITK=1 in the environment: the fused 64-tile kernel without split-K).
    Recorded in DESIGN.md 2c: at tap 13 (K = 3072) local is 4.1 unfused, 4.3 fused without split-K, 0.6 with split-K."""
    import numpy as np
    import torch
    import torch.nn.functional as Fn
    import encoder_tap_cases as tc
    from pfann_amd import synth
    from pfann_amd.engine import Engine
    o = tc.Oracle("default")
    eng = Engine(o.params, 0, max_batch=16)
    eng.load_state_dict(o.sd)
    assert eng.set_fused_layernorm(path == "fused") == (path == "fused")
    print(path, tc.signature(eng.encode_plan(tc.POOL, fused=int(path == "fused"), taps=2)[0]))
    x, got = torch.as_tensor(o.x).cuda(), {}
    for first in (0, 5):
        eng.debug_keep_at(2, first)
        eng.encode(x, norm=True)
        for i in range(8, 14):
            t = eng.debug_activation(i, 8)
            got[i] = t[:5] if first == 0 else np.concatenate([got[i], t])          # windows 0..4, then 5..12
    plan = synth.layer_plan(o.params)
    g = lambda k: torch.as_tensor(np.asarray(o.sd[k], np.float64))
    for i in range(9, 14):
        L, p, x64 = plan[i // 2], "f.convs.%d." % (i // 2), torch.as_tensor(got[i - 1].astype(np.float64))
        if i % 2 == 0:
            z = Fn.conv2d(Fn.pad(x64, (L["pad1"][0], L["pad1"][1], 0, 0)), g(p + "conv1.weight"), g(p + "conv1.bias"), stride=(1, L["s_t"]))
            w, b = g(p + "ln1.weight"), g(p + "ln1.bias")
        else:
            z = Fn.conv2d(Fn.pad(x64, (0, 0, L["pad2"][0], L["pad2"][1])), g(p + "conv2.weight"), g(p + "conv2.bias"), stride=(L["s_f"], 1))
            w, b = g(p + "ln2.weight"), g(p + "ln2.bias")
        mine = Fn.relu(Fn.layer_norm(z, w.shape, w, b, 1e-5)).numpy()
        total, carried, loc = (tc.tap_norm(a, b64) / o.ref_tap[i] for a, b64 in ((got[i], o.taps[i]), (mine, o.taps[i]), (got[i], mine)))
        print("tap %2d: total %.2f (window %d), carried %.2f, local %.2f (window %d)" % (i, total.max(), total.argmax(), carried.max(), loc.max(), loc.argmax()))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--local" and sys.argv[2] in ("unfused", "fused"):
        local(sys.argv[2])
        sys.exit(0)
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    if sys.argv[1] == "--chain":
        chain()
    else:
        main(sys.argv[1])
