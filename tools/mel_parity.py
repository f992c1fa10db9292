"""Measures, for every run of tests/mel_cases.py, how far the melspec kernel and the fp32 torch.stft oracle each are from
the float64 oracle (the figures tests/test_gpu_mel_cases.py::test_kernel_vs_float64 asserts on) and writes them to
profiles/mel/parity.json.  Needs the GPU:  python tools/mel_parity.py [--out FILE]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import mel_cases as mc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mel", "parity.json"))
    args = ap.parse_args()
    runs = []
    for name, B, rm in mc.RUNS:
        eng = mc.engine(name)
        m = mc.compare(mc.run_kernel(eng, mc.rows(name, B, rm)[0], B, rm), name, B, rm)
        path = dict(zip(("radix8", "in_register", "group_out", "parts"), mc.plan_path(eng, B)))
        runs.append(dict(case=name, B=B, remove_mean=rm, path=path, lds_bytes=eng.melspec_plan(B)["lds_bytes"],
                         factor_allowed=mc.FACTOR[name], ratio=m["noise_got_f64"] / m["noise_ref32_f64"], **m))
        print(json.dumps(runs[-1]))
    doc = {"what": "max |x - float64 oracle| per run of tests/mel_cases.py: lin_err = linear power / window peak (all signals), "
                   "log_err_loud = log units on the bins within exp(-11.5) of the peak (all signals), noise_got_f64 / "
                   "noise_ref32_f64 = kernel / fp32 torch.stft oracle on the noise windows' loud bins (naf_mode: all bins)",
           "runs": runs}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
