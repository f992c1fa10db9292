"""The log-mel front end (pfann_amd/csrc/mel.hip) against the float64 statement of the same transform
(oracle.melspec.melspec_f64), on every launch path and mode of tests/mel_cases.py: each case asserts through
Engine.melspec_plan that it runs the path it was written for, then compares.  Run with `pytest -m gpu` on an MI355X."""
import json
import os

import numpy as np
import pytest

import mel_cases as mc
from pfann_amd import synth

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


# --------------------------------------------------------------------------------- (a) + (b): kernel against float64
@pytest.mark.parametrize("name,B,remove_mean", mc.RUNS)
def test_kernel_vs_float64(torch_cuda, name, B, remove_mean):
    """(a) The project's two bars on every signal (linear power within 2e-6 of the window's peak; the log within 2e-3 on
    the bins within 1e-5 of the peak), and on the noise windows the kernel no further from float64 than FACTOR (3) times
    the fp32 torch.stft oracle is, with no floor -- over the loud bins, or over every bin in naf_mode (eps 0.06).
    (b) The impulse windows (at 0, 1, M-1, M, L-1-M, L-2, L-1): the set of (window, frame) pairs above the floor is the
    float64 oracle's set exactly; the all-zero window is the floor, log(eps) within 1e-6, everywhere, and finite."""
    eng = mc.engine(name)
    assert mc.plan_path(eng, B) == mc.CASES[name][2][B], "the case no longer runs the path it was written for"
    p = mc.params_for(name)
    x, kinds = mc.rows(name, B, remove_mean)
    ref64, _ = mc.references(name, B, remove_mean)
    got = mc.run_kernel(eng, x, B, remove_mean)
    assert np.isfinite(got).all()
    m = mc.compare(got, name, B, remove_mean)
    print("mel %s B=%d remove_mean=%d: lin err/peak %.3e, log err (loud) %.3e, noise: kernel-f64 %.3e, oracle32-f64 %.3e "
          "(ratio %.2f)" % (name, B, remove_mean, m["lin_err"], m["log_err_loud"], m["noise_got_f64"],
                            m["noise_ref32_f64"], m["noise_got_f64"] / m["noise_ref32_f64"]))
    assert m["lin_err"] < 2e-6
    assert m["log_err_loud"] < 2e-3
    assert m["noise_got_f64"] <= mc.FACTOR[name] * m["noise_ref32_f64"]
    zero = np.array([k == "zero" for k in kinds])
    fl = mc.floor_level(ref64[zero], p)
    assert np.abs(got[zero].astype(np.float64) - fl[:, None, None]).max() <= 1e-6
    imp = np.array([k == "impulse" for k in kinds])
    if imp.any():
        a_got, a_ref = mc.active_frames(got[imp], p), mc.active_frames(ref64[imp], p)
        assert np.array_equal(a_got, a_ref), np.argwhere(a_got != a_ref).tolist()
        if p.get("spec_norm", "l2") != "max":            # silent frames ARE the floor (under "max" it is read off them)
            silent = np.broadcast_to(~a_got[:, None, :], got[imp].shape)
            assert np.abs(got[imp][silent].astype(np.float64) - mc.floor_level(got[imp], p)[0]).max() <= 1e-6


# ---------------------------------------------------------------------------------------------------- (c) footprint
def _sentinel_out(torch, n, F, T):
    big = torch.full((n + 2, F, T), -12345.0, device="cuda", dtype=torch.float32)
    return big, big[1:n + 1]


@pytest.mark.parametrize("name", ["default_parts", "t24", "t31", "fft64"])
def test_kernel_reads_its_window_and_writes_its_output_only(torch_cuda, name):
    """A window's output depends on its own seg_len samples and nothing else, and the kernel writes inside its output:
    windows seg_stride = L + 64 apart with NaN in every sample between, before and after them, and overlapping windows
    (seg_stride = 4000, remove_mean = 1) of a buffer with 64 samples of NaN on both sides, give the bits of the packed
    call; the output is an interior view of a larger allocation whose sentinel rows stay untouched."""
    torch = torch_cuda
    from pfann_amd import lib as _l
    eng = mc.engine(name)
    B = min(mc.CASES[name][2])
    L, F, T = eng.seg_len, eng.F, eng.T
    x = mc.rows(name, B, 0)[0][:B]
    want = mc.run_kernel(eng, x, B, 0)
    stride = L + 64
    buf = torch.full((64 + B * stride,), float("nan"), device="cuda", dtype=torch.float32)
    for b in range(B):
        buf[64 + b * stride:64 + b * stride + L] = torch.as_tensor(np.array(x[b])).cuda()
    big, out = _sentinel_out(torch, B, F, T)
    _l.check(eng.lib.pfann_melspec(eng.handle, buf.data_ptr() + 64 * 4, B, stride, 0, out.data_ptr(), None), "pfann_melspec")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.isfinite(got).all() and np.array_equal(got, want)
    assert bool((big[0] == -12345.0).all()) and bool((big[B + 1] == -12345.0).all())
    # overlapping windows of one waveform, mean removed per window
    hop = 4000
    n = (B - 1) * hop + L
    rng = np.random.default_rng(77)
    wav = (rng.standard_normal(n) * 0.1 + 0.05).astype(np.float32)
    segs = np.stack([wav[b * hop:b * hop + L] for b in range(B)])
    if hop > L:                                            # (short windows: what lies between them is not theirs either)
        for b in range(B - 1):
            wav[b * hop + L:(b + 1) * hop] = np.nan
    want = mc.run_kernel(eng, segs, B, 1)
    buf = torch.full((n + 128,), float("nan"), device="cuda", dtype=torch.float32)
    buf[64:64 + n] = torch.as_tensor(wav).cuda()
    big, out = _sentinel_out(torch, B, F, T)
    _l.check(eng.lib.pfann_melspec(eng.handle, buf.data_ptr() + 64 * 4, B, hop, 1, out.data_ptr(), None), "pfann_melspec")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.isfinite(got).all() and np.array_equal(got, want)
    assert bool((big[0] == -12345.0).all()) and bool((big[B + 1] == -12345.0).all())


def test_embeddings_do_not_see_the_neighbouring_recording(torch_cuda):
    """The same guard at embedding level (configs/tiny.json): pfann_segment_embed_at over recordings laid back to back
    with NaN between them equals pfann_segment_embed on each recording alone, bit for bit (the encoder's variants are
    pinned to one plan batch, so that a fingerprint does not depend on the size of its batch)."""
    torch = torch_cuda
    from pfann_amd.engine import Engine
    params = json.load(open(os.path.join(REPO, "configs", "tiny.json")))
    eng = Engine(params, 0)
    eng.load_state_dict(synth.make_state_dict(params))
    eng.set_plan_batch(128)
    L, hop = eng.seg_len, 4000
    rng = np.random.default_rng(5)
    recs = [(rng.standard_normal(n) * 0.1 + 0.02).astype(np.float32) for n in (L + 3 * hop, L, L + hop + 123)]
    parts, starts, pos = [np.full(64, np.nan, np.float32)], [], 64
    for r in recs:
        starts += [pos + i * hop for i in range((len(r) - L) // hop + 1)]
        parts += [r, np.full(64, np.nan, np.float32)]
        pos += len(r) + 64
    together = eng.embed_windows(torch.as_tensor(np.concatenate(parts)).cuda(), np.asarray(starts, np.int64)).cpu().numpy()
    alone = np.concatenate([eng.embed_wav(torch.as_tensor(r).cuda(), hop).cpu().numpy() for r in recs])
    assert together.shape == alone.shape == (len(starts), 16) and len(starts) == 7
    assert np.isfinite(together).all() and np.array_equal(together, alone)


# ------------------------------------------------------------------------------- (d) same bits whatever the launch
@pytest.mark.parametrize("name", ["default_parts", "t24", "fft2048"])
def test_a_window_has_the_same_bits_in_every_launch(torch_cuda, name):
    """Rows 0..5 of a call of 200 windows (one workgroup per window) equal the call of those 6 windows alone (several
    workgroups per window): a window's output depends neither on the launch's shape nor on its neighbours."""
    eng = mc.engine(name)
    assert mc.plan_path(eng, 200)[3] == 1 and mc.plan_path(eng, 6)[3] > 1
    x = mc.rows(name, 200, 0)[0][:200]
    bulk = mc.run_kernel(eng, x, 200, 0)
    small = mc.run_kernel(eng, x[:6], 6, 0)
    assert np.array_equal(bulk[:6], small)


# --------------------------------------------------------------------------------------- (e) power-of-two scaling
@pytest.mark.parametrize("remove_mean", [0, 1])
@pytest.mark.parametrize("name", ["default_parts", "sr16k"])
def test_scaling_by_a_power_of_two_changes_no_bit(torch_cuda, name, remove_mean):
    """melspec(2^-10 x) and melspec(2^6 x) equal melspec(x) bit for bit: the mean, the norm (a square root of a sum scaled
    by an even power of two), the one real division and the Markstein quotient all scale exactly."""
    eng = mc.engine(name)
    B = min(mc.CASES[name][2])
    x, kinds = mc.rows(name, B, remove_mean)
    x = x[[i for i, k in enumerate(kinds) if k == "noise"][:B]]
    x = np.concatenate([x, x])[:B] if x.shape[0] < B else x[:B]
    base = mc.run_kernel(eng, x, B, remove_mean)
    for sc in (2.0 ** -10, 2.0 ** 6):
        assert np.array_equal(mc.run_kernel(eng, x * np.float32(sc), B, remove_mean), base), sc
