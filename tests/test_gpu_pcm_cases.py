"""The audio front door on the GPU, on the cases of tests/pcm_cases.py (whose conditions tests/test_pcm_host.py checks on
the CPU): 16-bit PCM -> mono float at the model's rate against the oracle (pcm_to_mono_kernel, pcm_mono8_kernel,
resample_kernel, planar_to_mono_kernel of pfann_amd/csrc/mel.hip), the kernels' footprints, pfann_pcm16_files_to_mono called
directly, and the file-reading paths of pfann_amd/builder.py against each other.  Run with `pytest -m gpu` on an MI355X."""
import ctypes
import os

import numpy as np
import pytest

import pcm_cases as pc
from pfann_amd import synth

pytestmark = pytest.mark.gpu
SENTINEL = -12345.0


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


_ENGINES = {}


def engine(weights=False):
    """One Engine for the module; the one with weights has its kernel variants pinned to a plan batch of 256, so that a
    window's bits do not depend on the batch it is embedded in (include/pfann_amd.h: pfann_set_plan_batch)."""
    from pfann_amd.engine import Engine
    if weights not in _ENGINES:
        p = pc.params()
        eng = Engine(p, 0, max_batch=256)
        if weights:
            eng.load_state_dict(synth.make_state_dict(p))
            assert eng.set_plan_batch(256) == 256
        _ENGINES[weights] = eng
    return _ENGINES[weights]


def _mono(eng, pcm, rate=None):
    return eng.pcm16_to_mono(np.array(pcm), sample_rate=rate).cpu().numpy()


# ------------------------------------------------------------------------------------------------- mono conversion
@pytest.mark.parametrize("name", pc.STEREO)
def test_fake_stereo_rule_at_the_threshold(torch_cuda, name):
    """Ratios 900 and 1100 around the rule's 1000, a heavy-tailed pair that only the mean square puts above it, and
    silence: bit-equal to oracle.segmenter.pcm_to_mono, and to (l + r) / 2 or (l - r) / 2 as the case expects."""
    from oracle import segmenter
    pcm, flip = pc.stereo_case(name)
    got = _mono(engine(), pcm)
    assert np.array_equal(got, pc.mono_by_the_rule(pcm, flip)), "flipped" if not flip else "not flipped"
    assert np.array_equal(got, segmenter.pcm_to_mono(pcm))
    if name == "silent":
        assert not got.any()


def test_fake_stereo_is_decided_after_resampling(torch_cuda):
    """16 kHz pair whose ratio is 62.5 on the file's samples and 3e7 after the resampler: flipped (the opposite-phase part
    survives, max |mono| > 0.3), within the resampler's bars of the oracle."""
    from oracle import segmenter
    from pfann_amd import resample as pr
    pcm = pc.after_resampling_case()
    got = _mono(engine(), pcm, 16000)
    want = segmenter.pcm_to_mono(pcm, 16000, pc.SR, resample_table=pr.filter_table(16000, pc.SR)[0])
    assert got.shape == want.shape == (20000,)
    assert np.abs(got).max() > 0.3
    assert np.abs(got - want).max() < 2e-6
    assert np.abs(got - segmenter.pcm_to_mono(pcm, 16000, pc.SR)).max() < 2e-5


@pytest.mark.parametrize("n", pc.MONO_LENGTHS)
def test_mono_lengths_around_the_eight_sample_kernel(torch_cuda, n):
    from oracle import segmenter
    pcm = pc.mono_case(n)
    assert np.array_equal(_mono(engine(), pcm), segmenter.pcm_to_mono(pcm))


@pytest.mark.parametrize("n_ch", [3, 6])
def test_more_than_two_channels(torch_cuda, n_ch):
    """pcm_to_mono_kernel with 3 and 6 unequal channels: bit-equal to the oracle's fp32 statement (channels added in order,
    one division), and within pc.mean_bound of the float64 channel mean: the samples are exact in fp32, n_ch - 1
    additions each round a partial sum of magnitude <= n_ch (n_ch 2^-24 each, 2^-24 after the division by n_ch), the
    division rounds once more (2^-24): n_ch 2^-24 = 1.8e-7 / 3.6e-7."""
    from oracle import segmenter
    pcm = pc.channels_case(n_ch)
    got = _mono(engine(), pcm)
    m64 = pcm.astype(np.float64).mean(axis=1) / 32768.0
    err = float(np.abs(got - m64).max())
    print("mono of %d channels: worst |kernel - float64 mean| %.3e (bound %.3e)" % (n_ch, err, pc.mean_bound(n_ch)))
    assert got.shape == (pcm.shape[0],)
    assert err <= pc.mean_bound(n_ch)
    assert np.array_equal(got, segmenter.pcm_to_mono(pcm))


def _resample_direct(torch, eng, pcm, rate, pad=16):
    """pfann_resample_to_mono on buffers this test owns: tmp [n_ch, n_out] and wav [n_out] are interior views with `pad`
    sentinel floats on both sides.  -> (tmp, wav, the four sentinel strips) as numpy."""
    from pfann_amd import lib as _l
    from pfann_amd import resample as pr
    tab, old, new, width = pr.filter_table(rate, pc.SR)
    plan, n_out = pr.piece_plan(pcm.shape[0], rate, pc.SR)
    assert n_out > 0
    n_ch = pcm.shape[1]
    p = torch.as_tensor(np.array(pcm)).cuda()
    tab_d, plan_d = torch.as_tensor(tab).cuda(), torch.as_tensor(plan).cuda()
    tmp_big = torch.full((pad + n_ch * n_out + pad,), SENTINEL, device="cuda", dtype=torch.float32)
    wav_big = torch.full((pad + n_out + pad,), SENTINEL, device="cuda", dtype=torch.float32)
    _l.check(eng.lib.pfann_resample_to_mono(eng.handle, p.data_ptr(), n_ch, tab_d.data_ptr(), old, new, width, plan_d.data_ptr(),
                                            plan.shape[0], n_out, tmp_big.data_ptr() + 4 * pad, wav_big.data_ptr() + 4 * pad,
                                            None), "pfann_resample_to_mono")
    torch.cuda.synchronize()
    t, w = tmp_big.cpu().numpy(), wav_big.cpu().numpy()
    return t[pad:-pad].reshape(n_ch, n_out), w[pad:-pad], (t[:pad], t[-pad:], w[:pad], w[-pad:])


def test_three_channels_through_the_planar_path(torch_cuda):
    """3 channels at 12 kHz (resample_kernel per channel, then planar_to_mono_kernel): within the resampler's bars of the
    oracle; the mono signal is the fp32 mean of the kernel's own resampled channels bit for bit, within
    pc.mean_bound(3) max |channel| of their float64 mean."""
    from oracle import segmenter
    from pfann_amd import resample as pr
    pcm = pc.channels_case(3, 7001)
    eng = engine()
    got = _mono(eng, pcm, 12000)
    want = segmenter.pcm_to_mono(pcm, 12000, pc.SR, resample_table=pr.filter_table(12000, pc.SR)[0])
    assert got.shape == want.shape == (2 * 7001 // 3,)
    assert np.abs(got - want).max() < 2e-6
    assert np.abs(got - segmenter.pcm_to_mono(pcm, 12000, pc.SR)).max() < 2e-5
    tmp, wav, strips = _resample_direct(torch_cuda, eng, pcm, 12000)
    assert np.array_equal(wav, got) and all((s == SENTINEL).all() for s in strips)
    assert np.array_equal(wav, tmp.mean(axis=0, dtype=np.float32))
    scale = max(1.0, float(np.abs(tmp).max()))
    err = float(np.abs(wav - tmp.astype(np.float64).mean(axis=0)).max())
    print("planar mono of 3 channels: worst |kernel - float64 mean| %.3e (bound %.3e)" % (err, pc.mean_bound(3) * scale))
    assert err <= pc.mean_bound(3) * scale


# -------------------------------------------------------------------------------------------------------- resampling
_WORST = {}


@pytest.mark.parametrize("rate,label", pc.RESAMPLE, ids=pc.RESAMPLE_IDS)
def test_resampler_vs_oracle(torch_cuda, rate, label):
    """Up- and downsampling, coprime rates, the deep filters of 32 and 96 kHz, the lengths around the 60 s seam and inputs
    shorter than the filter, against oracle.resample: equal shapes, < 2e-6 with the kernel's own table (fp32 sums of at
    most 721 products in another order) and < 2e-5 with the oracle's float64 table -- the bars of
    tests/test_gpu_parity.py::test_resample_to_mono_vs_oracle.  One sample at 12, 32 or 96 kHz gives an empty signal, and
    no launch."""
    pcm = pc.resample_input(rate, label)
    want, own = pc.mono_kernel_table(rate, label), pc.mono_own_table(rate, label)
    got_t = engine().pcm16_to_mono(np.array(pcm), sample_rate=rate)
    torch_cuda.cuda.synchronize()
    got = got_t.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape == own.shape == (pc.expected_n_out(rate, pcm.shape[0]),)
    if got.size == 0:
        assert label == "1smp" and rate in (12000, 32000, 96000)
        return
    e_tab, e_own = float(np.abs(got - want).max()), float(np.abs(got - own).max())
    w = _WORST.setdefault(rate, [0.0, 0.0])
    w[0], w[1] = max(w[0], e_tab), max(w[1], e_own)
    print("resample %d Hz %s: %d -> %d samples; vs oracle with the kernel's table %.3e, with its own %.3e; worst at this "
          "rate so far %.3e / %.3e" % (rate, label, pcm.shape[0], got.size, e_tab, e_own, w[0], w[1]))
    assert np.isfinite(got).all()
    assert e_tab < 2e-6
    assert e_own < 2e-5


@pytest.mark.parametrize("rate,label", [(7350, "3ms"), (4000, "1smp"), (96000, "0.4s")])
def test_resampler_writes_inside_tmp_and_wav(torch_cuda, rate, label):
    """pfann_resample_to_mono on buffers with 16 sentinel floats before and after `tmp` and `wav`: the sentinels stay, and
    the result has the bits of Engine.pcm16_to_mono."""
    pcm = pc.resample_input(rate, label)
    eng = engine()
    tmp, wav, strips = _resample_direct(torch_cuda, eng, pcm, rate)
    assert all((s == SENTINEL).all() for s in strips)
    assert np.isfinite(tmp).all() and np.array_equal(wav, _mono(eng, pcm, rate))
    assert np.abs(tmp - pc.planar_kernel_table(rate, label)).max() < 2e-6


# ------------------------------------------------------------------------------------------- footprint and alignment
@pytest.mark.parametrize("n_ch", [1, 2, 3])
def test_pcm16_to_mono_footprint_and_alignment(torch_cuda, n_ch):
    """lib.pfann_pcm16_to_mono on 1..40 frames, the input starting on a 16-byte boundary or one sample behind it, the
    output on one or one float behind it (the eight-sample kernel needs both aligned; anything else takes the
    one-sample kernel), 16 sentinel floats before and after every output: the sentinels stay, and every placement gives
    the bits of the oracle, hence of the aligned call."""
    torch = torch_cuda
    from oracle import segmenter
    from pfann_amd import lib as _l
    eng = engine()
    N, IN_ROW, OUT_ROW = 40, 256, 96                    # rows of 512 and 384 bytes: every row starts 16-byte aligned
    rng = np.random.default_rng(500 + n_ch)
    src = rng.integers(-32768, 32768, (N, n_ch)).astype(np.int16)
    if n_ch == 2:
        src[:, 1] = -src[:, 0]                          # opposite phase: the stereo power pass decides on n frames only
        src[0] = (7, 7)
    for in_off in (0, 1):
        for out_off in (0, 1):
            pcm_d = torch.full((N, IN_ROW), 31000, device="cuda", dtype=torch.int16)
            out_d = torch.full((N, OUT_ROW), SENTINEL, device="cuda", dtype=torch.float32)
            assert pcm_d.data_ptr() % 16 == 0 and out_d.data_ptr() % 16 == 0
            for n in range(1, N + 1):
                pcm_d[n - 1, 8 + in_off:8 + in_off + n * n_ch] = torch.as_tensor(src[:n].reshape(-1)).cuda()
            for n in range(1, N + 1):
                pin = pcm_d.data_ptr() + 2 * ((n - 1) * IN_ROW + 8 + in_off)
                pout = out_d.data_ptr() + 4 * ((n - 1) * OUT_ROW + 16 + out_off)
                assert pin % 16 == 2 * in_off and pout % 16 == 4 * out_off
                _l.check(eng.lib.pfann_pcm16_to_mono(eng.handle, pin, n, n_ch, pout, None), "pfann_pcm16_to_mono")
            torch.cuda.synchronize()
            out = out_d.cpu().numpy()
            for n in range(1, N + 1):
                row = out[n - 1]
                lo, hi = 16 + out_off, 16 + out_off + n
                assert (row[:lo] == SENTINEL).all() and (row[hi:] == SENTINEL).all(), (n, in_off, out_off)
                assert np.array_equal(row[lo:hi], segmenter.pcm_to_mono(src[:n])), (n, in_off, out_off)


def test_pcm16_files_to_mono_directly(torch_cuda):
    """pfann_pcm16_files_to_mono: five host arrays (lengths 0, 1 and three that are no multiples of 8) placed at scattered
    offsets of a slab pre-filled with 1234: the files' ranges are int16 / 32768 bit for bit, the gaps are 1234 / 32768, and
    the conversion stays inside its output; total == 0 returns 0; a file that ends behind the slab is refused by name, and
    the output stays as it was.  Every pointer is valid throughout."""
    torch = torch_cuda
    from pfann_amd import lib as _l
    eng = engine()
    rng = np.random.default_rng(9)
    lens = [0, 1, 13, 1003, 77]
    offs = [3, 5, 9, 64 + 1, 1200]
    total = 1301                                                          # the last file ends 24 samples before the end
    files = [np.ascontiguousarray(rng.integers(-32768, 32768, max(n, 1)).astype(np.int16)) for n in lens]
    ptrs = (ctypes.c_void_p * 5)(*[f.ctypes.data for f in files])
    c_lens, c_offs = (ctypes.c_int64 * 5)(*lens), (ctypes.c_int64 * 5)(*offs)
    pcm_d = torch.full((total + 8,), 1234, device="cuda", dtype=torch.int16)
    wav_big = torch.full((16 + total + 16,), SENTINEL, device="cuda", dtype=torch.float32)
    rc = eng.lib.pfann_pcm16_files_to_mono(eng.handle, ptrs, c_lens, c_offs, 5, pcm_d.data_ptr(), total,
                                           wav_big.data_ptr() + 64, None)
    assert rc == 0, _l.last_error()
    torch.cuda.synchronize()
    want = np.full(total, 1234, np.int16)
    for f, n, o in zip(files, lens, offs):
        want[o:o + n] = f[:n]
    got = wav_big.cpu().numpy()
    assert (got[:16] == SENTINEL).all() and (got[-16:] == SENTINEL).all()
    assert np.array_equal(got[16:-16], want.astype(np.float32) / np.float32(32768.0))
    assert np.array_equal(pcm_d.cpu().numpy(), np.concatenate([want, np.full(8, 1234, np.int16)]))
    # total == 0: nothing to convert
    zero = (ctypes.c_int64 * 1)(0)
    before = wav_big.clone()
    assert eng.lib.pfann_pcm16_files_to_mono(eng.handle, ptrs, zero, zero, 1, pcm_d.data_ptr(), 0, wav_big.data_ptr() + 64, None) == 0
    # the fifth file one sample too long for the slab: refused, nothing converted
    c_lens[4] = total - offs[4] + 1
    rc = eng.lib.pfann_pcm16_files_to_mono(eng.handle, ptrs, c_lens, c_offs, 5, pcm_d.data_ptr(), total,
                                           wav_big.data_ptr() + 64, None)
    assert rc != 0 and "file 4" in _l.last_error()
    torch.cuda.synchronize()
    assert torch.equal(wav_big, before)


# ------------------------------------------------------------------------------------- the file paths agree
def _per_file(eng, paths):
    """File by file: read_wav_pcm16 + Engine.pcm16_to_mono + embed_windows.  -> [embeddings [n_seg, d] or None]."""
    import wave
    import torch
    from pfann_amd.musicdata import read_wav_pcm16
    out = []
    for p in paths:
        try:
            pcm, sr = read_wav_pcm16(p)
            if pcm.size == 0 and sr != pc.SR:
                raise ValueError("empty file at a foreign rate")           # the reference's resampler raises there
            wav = eng.pcm16_to_mono(pcm, sample_rate=sr)
        except (OSError, ValueError, NotImplementedError, wave.Error):     # load and rate errors only: a 0-segment song
            out.append(None)
            continue
        if wav.shape[0] < pc.SEG:
            wav = torch.nn.functional.pad(wav, (0, pc.SEG - wav.shape[0]))
        n_seg = (wav.shape[0] - pc.SEG) // pc.HOP + 1
        out.append(eng.embed_windows(wav, np.arange(n_seg, dtype=np.int64) * pc.HOP).cpu().numpy())
    return out


def _poisoned(source, log):
    """Wraps a group source of pfann_amd.builder: before a group is handed on, device blocks of the sizes its slab
    assembly will ask for are filled with 1000 and freed, so that the assembly gets them back (the caching allocator
    returns the block just freed to a request of the same size): padding that is not zeroed then shows in the embeddings."""
    import torch

    def wrapped(engine, *a, **k):
        for got in source(engine, *a, **k):
            items, slab = got[0], got[1]
            have = [it[2] if it[0] in ("host", "slab") else it[1].shape[0] for _, n_seg, it in items if n_seg]
            total = sum(max(h, pc.SEG) for h in have)
            log.append((slab is not None, any(h < pc.SEG for h in have), len(items)))
            if total and slab is None:
                f = torch.full((total,), 1000.0, device=engine.device, dtype=torch.float32)
                i = torch.full((total,), 1000, device=engine.device, dtype=torch.int16)
                del f, i
                # the premise, checked: a request of that size gets the poisoned block back
                probe = torch.empty((total,), device=engine.device, dtype=torch.float32)
                assert bool((probe == 1000.0).all()), "the allocator did not hand the poisoned block back"
                del probe
            yield got
    return wrapped


def _batches(eng, paths, batch_windows, monkeypatch, native, log):
    from pfann_amd import builder
    from pfann_amd.musicdata import MusicDataset
    monkeypatch.setenv("PFANN_NATIVE_WAV", "1" if native else "0")
    monkeypatch.setattr(builder, "_native_groups" if native else "_threaded_groups",
                        _poisoned(builder._native_groups if native else builder._threaded_groups, log))
    ds = MusicDataset(paths, pc.params())
    out, groups = {}, 0
    for group in builder.embed_file_batches(eng, ds, pc.HOP, batch_windows=batch_windows, workers=3):
        groups += 1
        for idx, n_seg, emb in group:
            assert idx not in out and (emb is None) == (n_seg == 0)
            out[idx] = None if emb is None else emb.cpu().numpy()
            assert emb is None or emb.shape[0] == n_seg
    assert sorted(out) == list(range(len(paths)))
    return [out[i] for i in range(len(paths))], groups


def _assert_same_files(a, b, kinds, what):
    for x, y, kind in zip(a, b, kinds):
        assert (x is None) == (y is None), "%s: %s is a 0-segment song on one path only" % (what, kind)
        if x is not None:
            assert x.shape == y.shape, "%s: %s has %d and %d windows" % (what, kind, x.shape[0], y.shape[0])
            assert np.array_equal(x, y), "%s: %s differs by %.3e" % (what, kind, np.abs(x - y).max())


def test_file_paths_agree_on_a_mixed_list(torch_cuda, tmp_path, monkeypatch):
    """One list of 16 files -- mono long, exactly one window, shorter than one; stereo, fake stereo, 3 channels, 16 kHz
    stereo, 6 kHz mono, empty at 8 kHz (one window of silence) and at 16 kHz (no window); rates 0 and 0x80000000, 8-bit,
    not a WAV, missing -- embedded three ways: embed_file_batches with the native reader (8 windows per group: uniform
    and mixed groups, one with a short file), the same through the Python threads (PFANN_NATIVE_WAV=0), and file by file.
    Same window counts and same bits everywhere; the malformed files are 0-segment songs everywhere; no filter table is
    built for a rate outside 1..MAX_RATE."""
    from pfann_amd import resample as pr
    eng = engine(weights=True)
    paths, kinds = pc.write_mixed_list(tmp_path)
    asked = []
    real_table = pr.filter_table
    monkeypatch.setattr(pr, "filter_table", lambda a, b: (asked.append((a, b)), real_table(a, b))[1])
    alone = _per_file(eng, paths)
    for kind, e in zip(kinds, alone):
        assert (e is None) == (kind in pc.MIXED_ZERO), kind
        assert e is None or np.isfinite(e).all()
    assert alone[kinds.index("empty_8k")].shape[0] == 1 and alone[kinds.index("mono_1s")].shape[0] == 1
    assert alone[kinds.index("mono_long")].shape[0] == 7 and alone[kinds.index("mono_short")].shape[0] == 1
    log_n, log_t = [], []
    native, groups_n = _batches(eng, paths, 8, monkeypatch, True, log_n)
    threads, groups_t = _batches(eng, paths, 8, monkeypatch, False, log_t)
    assert groups_n >= 4 and groups_t >= 4
    assert any(u for u, _, _ in log_n) and any(not u for u, _, _ in log_n)         # uniform and mixed groups
    assert any(s and not u for u, s, _ in log_n) and any(s for _, s, _ in log_t)   # a group with a short file on each path
    _assert_same_files(native, alone, kinds, "native reader vs file by file")
    _assert_same_files(threads, alone, kinds, "Python threads vs file by file")
    assert set(asked) <= {(2, 1), (3, 4)}, asked                                   # 16 kHz and 6 kHz, nothing else


def test_uniform_slab_agrees_with_the_per_file_path(torch_cuda, tmp_path, monkeypatch):
    """Six mono files at the model's rate, each at least one window long, four of them with sample counts that are no
    multiples of 8: the native reader's uniform groups (one slab, one upload, one conversion, windows addressed across the
    files' boundaries) give the bits of the file-by-file path."""
    eng = engine(weights=True)
    paths, counts = pc.write_uniform_list(tmp_path)
    assert sum(1 for n in counts if n % 8) == 4
    alone = _per_file(eng, paths)
    assert [e.shape[0] for e in alone] == [(n - pc.SEG) // pc.HOP + 1 for n in counts]
    log = []
    native, groups = _batches(eng, paths, 64, monkeypatch, True, log)
    assert log and all(u for u, _, _ in log)
    assert any(n > 1 for _, _, n in log)                                           # a slab of several files
    _assert_same_files(native, alone, ["u%d" % i for i in range(len(paths))], "uniform slab vs file by file")
