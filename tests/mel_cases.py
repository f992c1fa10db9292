"""The case table of the log-mel front end (pfann_amd/csrc/mel.hip: melspec_kernel + plan_melspec), importable without
a GPU: tests/test_gpu_mel_cases.py runs the kernel on every case against oracle.melspec.melspec_f64, tests/test_oracle.py
checks the oracle's side of the same cases (float64 against the fp32 torch.stft statement, the loud-bin mask's cap).

A case = overrides on configs/default.json, the window length L, the batch sizes B one launch gets, the remove_mean values
it runs with, and per B the launch path it was written for, (radix8, in_register, group_out, parts), which the GPU test
asserts through Engine.melspec_plan BEFORE it compares anything: a later change of heuristics cannot silently empty a case.
The paths are what plan_melspec chooses today (3 workgroups per CU of LDS decide the group): with 256 mel rows the default
model's tile of 16 frames does not fit three times into 160 KiB, so it runs with groups of 8 (parts 4), and `mels128_g16`
is the case that reaches groups of 16.
"""
import copy
import functools
import json
import math
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SR16K = dict(sample_rate=16000, f_max=8000)
_FFT256 = dict(stft_n=256, stft_hop=64, n_mels=64)

# name -> (overrides, L, {B: (radix8, in_register, group_out, parts)}, remove_mean values)
CASES = {
    # radix-8 register FFT, statistics from registers, groups of 8 frames; 4 workgroups per window / one (production: 9728)
    "default_parts": ({}, 8000, {8: (1, 1, 8, 4)}, (0, 1)),
    "default_bulk": ({}, 8000, {200: (1, 1, 8, 1)}, (1,)),
    # the widest output group: 128 mel rows leave room for three tiles of 16 frames per CU
    "mels128_g16": (dict(n_mels=128), 8000, {8: (1, 1, 16, 2), 200: (1, 1, 16, 1)}, (0,)),
    # L = 16000 > 8192: statistics from global memory; T = 63: whole tile, 256 % T != 0 output loop, one dead wave
    "sr16k": (_SR16K, 16000, {6: (1, 0, 0, 1)}, (0, 1)),
    "sr16k_max": (dict(_SR16K, spec_norm="max", mel_log="log10"), 16000, {6: (1, 0, 0, 1)}, (0, 1)),
    # L no multiple of 256 or of the hop (ragged last register row, reflection off a ragged end); T = 24: groups of 8
    "t24": ({}, 6100, {6: (1, 1, 8, 3), 200: (1, 1, 8, 1)}, (0, 1)),
    "t20": ({}, 5000, {6: (1, 1, 4, 5)}, (0,)),                        # T = 20: groups of 4
    "t31": ({}, 7900, {6: (1, 1, 0, 1)}, (0,)),                        # T = 31: whole tile, one dead wave in the last group
    # radix-2 FFT in LDS, M = 1024; 57 KB of FFT buffers leave room for groups of 4 only
    "fft2048": (dict(stft_n=2048, stft_hop=512, n_mels=128), 8000, {6: (0, 1, 4, 4), 200: (0, 1, 4, 1)}, (0,)),
    # M = 2048, 146,084 B of LDS (limit 163,840): T = 8 runs as groups of 4 because the LDS rule refuses 8
    "fft4096": (dict(stft_n=4096, stft_hop=1024, n_mels=64), 8000, {4: (0, 1, 4, 2)}, (0,)),
    # radix-2 at M = 128 / M = 32 (narrower than a wave: half of it idles in the butterflies; n_mels < 64).  L = 1601 and
    # 401, not 1600 and 400: the engine wants 1 + L // hop == ceil(L / hop) frames (the encoder's T), which a multiple of
    # the hop does not give; T = 26 as intended, whole tile, two dead waves in the last group
    "fft256": (_FFT256, 1601, {6: (0, 1, 0, 1)}, (0, 1)),
    "fft64": (dict(stft_n=64, stft_hop=16, n_mels=16), 401, {6: (0, 1, 0, 1)}, (0,)),
    # naf_mode: zero padding, power 1, eps 0.06, slaney bank; every log mode
    "naf_ln": (dict(naf_mode=True, mel_log="log"), 8000, {8: (1, 1, 8, 4)}, (0,)),
    "naf_log10": (dict(naf_mode=True, mel_log="log10"), 8000, {8: (1, 1, 8, 4)}, (0,)),
    "naf_nolog": (dict(naf_mode=True, mel_log="none"), 8000, {8: (1, 1, 8, 4)}, (0,)),
    "naf_fft256": (dict(_FFT256, naf_mode=True), 1601, {6: (0, 1, 0, 1)}, (0,)),      # zero padding on the radix-2 gather
    "max_ln": (dict(spec_norm="max"), 8000, {8: (1, 1, 0, 1)}, (0,)),               # max norm, 256 % 32 == 0 output loop
}
RUNS = [(name, B, rm) for name, (_, _, paths, rms) in CASES.items() for B in paths for rm in rms]
# the loud bins: within exp(-11.5) ~ 1e-5 of the window's peak power (tests/test_gpu_parity.py::test_melspec_vs_oracle)
LOUD = 11.5
# how much further from float64 than the fp32 torch.stft oracle the kernel may be on the noise windows' loud bins
# (test_melspec_vs_oracle grants 3)
FACTOR = {name: 3.0 for name in CASES}


def params_for(name):
    over, L = CASES[name][0], CASES[name][1]
    p = json.load(open(os.path.join(REPO, "configs", "default.json")))
    p.update(copy.deepcopy(over))
    p["segment_size"] = (L + 0.5) / p["sample_rate"]              # int(segment_size * sample_rate) == L whatever the rounding
    assert int(p["segment_size"] * p["sample_rate"]) == L
    assert 1 + L // p["stft_hop"] == (L + p["stft_hop"] - 1) // p["stft_hop"]
    return p


def bank_for(params):
    """The bank the engine hands the kernel (fp32, built the way torchaudio builds it)."""
    from pfann_amd.engine import mel_filterbank
    return mel_filterbank(params["sample_rate"], params["stft_n"], params["n_mels"], params["f_min"], params["f_max"],
                          params.get("naf_mode", False)).numpy()


def impulse_positions(params, L):
    M = params["stft_n"] // 2
    return [0, 1, M - 1, M, L - 1 - M, L - 2, L - 1]


@functools.lru_cache(maxsize=None)
def rows(name, B, remove_mean):
    """-> (x float32 [n, L] with n a multiple of B, kinds [n]): every signal of the set, then seeded noise up to a whole
    number of launches of B windows.  kinds: "noise" (white noise at 0.1; on the int16 grid, as PCM arrives; with a DC
    offset of 0.05 in the remove_mean runs; the filler), "song", "impulse", "zero"."""
    from pfann_amd import synth
    p = params_for(name)
    L, sr = CASES[name][1], p["sample_rate"]
    rng = np.random.default_rng(1234 + sorted(CASES).index(name))
    noise = lambda: (rng.standard_normal(L) * 0.1).astype(np.float32)
    song = synth.make_song(3, seconds=math.ceil(L / sr) + 1.0, sr=sr).astype(np.float32) / np.float32(32768.0)
    out = [(noise(), "noise"), (song[sr // 2:sr // 2 + L], "song"),
           ((np.round(noise() * 32768.0) / 32768.0).astype(np.float32), "noise")]
    if remove_mean:
        out.append((noise() + np.float32(0.05), "noise"))
    else:                                        # (an impulse minus its mean is no impulse)
        for pos in impulse_positions(p, L):
            v = np.zeros(L, np.float32)
            v[pos] = 1.0
            out.append((v, "impulse"))
    out.append((np.zeros(L, np.float32), "zero"))
    while len(out) % B:
        out.append((noise(), "noise"))
    x = np.stack([o[0] for o in out])
    x.setflags(write=False)
    return x, tuple(o[1] for o in out)


@functools.lru_cache(maxsize=None)
def references(name, B, remove_mean):
    """-> (ref64 float64, ref32 float32) [n, n_mels, T] of rows(name, B, remove_mean): computed once, shared, read-only."""
    from oracle import melspec as om
    p = params_for(name)
    x, _ = rows(name, B, remove_mean)
    bank = bank_for(p)
    ref64 = om.melspec_f64(x, p, bank, remove_mean=bool(remove_mean))
    x32 = x - x.mean(axis=1, keepdims=True, dtype=np.float32) if remove_mean else x
    ref32 = om.melspec(np.array(x32), p, bank)
    ref64.setflags(write=False)
    ref32.setflags(write=False)
    return ref64, ref32


def to_linear(v, params):
    """The output back in linear units (mel + eps; after spec_norm == "max", relative to the window's maximum), float64."""
    v = np.asarray(v, np.float64)
    mode = params.get("mel_log", "log")
    return np.exp(v) if mode == "log" else 10.0 ** v if mode == "log10" else v


def to_log(v, params):
    """The output in the units the log bar is stated in: itself where the kernel took a log, else its natural log."""
    v = np.asarray(v, np.float64)
    return v if params.get("mel_log", "log") in ("log", "log10") else np.log(v)


def loud_mask(ref64, params):
    lin = to_linear(ref64, params)
    return lin > lin.max(axis=(1, 2), keepdims=True) * math.exp(-LOUD)


def compare(got, name, B, remove_mean):
    """The distances the bars of tests/test_gpu_mel_cases.py are stated on: `got` [n, n_mels, T] (the kernel's output, or
    any other statement of the same rows) against the float64 oracle."""
    p = params_for(name)
    _, kinds = rows(name, B, remove_mean)
    ref64, ref32 = references(name, B, remove_mean)
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    is_noise = np.array([k == "noise" for k in kinds])
    lin_g, lin_r = to_linear(got, p), to_linear(ref64, p)
    lin_err = np.abs(lin_g - lin_r) / lin_r.max(axis=(1, 2), keepdims=True)
    loud = loud_mask(ref64, p)
    log_err = np.abs(to_log(got, p) - to_log(ref64, p))
    tight = np.ones_like(loud) if p.get("naf_mode", False) else loud       # eps 0.06: every bin is well-conditioned
    tight = tight & is_noise[:, None, None]
    return {"lin_err": float(lin_err.max()), "log_err_loud": float(log_err[loud].max()),
            "noise_got_f64": float(np.abs(got - ref64)[tight].max()),
            "noise_ref32_f64": float(np.abs(ref32 - ref64)[tight].max()),
            "noise_loud_share": float(loud[is_noise].mean())}


def floor_level(v, params):
    """Per window, the value of a frame without energy: f(eps), less the window's maximum under spec_norm == "max" (there
    read off the window itself: its smallest value; every impulse window has silent frames)."""
    naf = params.get("naf_mode", False)
    eps = 0.06 if naf else 1e-8
    mode = params.get("mel_log", "log")
    f = math.log(eps) if mode == "log" else math.log10(eps) if mode == "log10" else eps
    if params.get("spec_norm", "l2") == "max":
        return np.asarray(v, np.float64).min(axis=(1, 2))
    return np.full(v.shape[0], f)


def active_frames(v, params):
    """bool [n, T]: frames with any bin more than 1e-6 above the floor."""
    fl = floor_level(v, params)
    return (np.asarray(v, np.float64) > fl[:, None, None] + 1e-6).any(axis=1)


# ------------------------------------------------------------------------------ the kernel's side (needs the GPU)
_ENGINES = {}


def engine(name):
    """One Engine per case for the whole session (front end only: no weights are loaded)."""
    from pfann_amd.engine import Engine
    if name not in _ENGINES:
        _ENGINES[name] = Engine(params_for(name), 0)
    return _ENGINES[name]


def plan_path(eng, B):
    pl = eng.melspec_plan(B)
    return (int(pl["radix8"]), int(pl["in_register"]), pl["group_out"], pl["parts"])


def run_kernel(eng, x, B, remove_mean):
    """pfann_melspec on packed windows x [n, L], B windows per launch -> numpy float32 [n, n_mels, T]."""
    import torch
    from pfann_amd import lib as _l
    xd = torch.as_tensor(np.array(x, dtype=np.float32)).cuda()
    n, L = xd.shape
    assert L == eng.seg_len and n % B == 0
    out = torch.empty((n, eng.F, eng.T), device="cuda", dtype=torch.float32)
    for b0 in range(0, n, B):
        _l.check(eng.lib.pfann_melspec(eng.handle, xd[b0:b0 + B].data_ptr(), B, L, int(remove_mean),
                                       out[b0:b0 + B].data_ptr(), None), "pfann_melspec")
    torch.cuda.synchronize()
    return out.cpu().numpy()
