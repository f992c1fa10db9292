"""The conditions behind tests/pcm_cases.py, checked without a GPU with float64 numpy and the oracle only (a case whose
condition fails would pass its GPU test for the wrong reason); the three-way table of WAV headers (Python's `wave`,
pfann_amd.musicdata.read_wav_pcm16, pfann_wav_probe + pfann_wav_read); and the native reader under AddressSanitizer and
UndefinedBehaviorSanitizer in a stand-alone program (tests/native/wav_reader_check.cpp)."""
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

import pcm_cases as pc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the fake-stereo rule
def test_threshold_pair_sits_on_both_sides_of_1000():
    """rho900 / rho1100: float64 mean-square ratios at least 1 % from 1000, one on each side; the oracle (fp32 means)
    decides as float64 does.  A rule with a threshold of 100 or 10,000 answers both alike."""
    from oracle import segmenter
    for name, lo, hi in (("rho900", 890.0, 910.0), ("rho1100", 1090.0, 1110.0)):
        pcm, flip = pc.stereo_case(name)
        ms, _ = pc.ratios(pcm)
        print("%s: float64 mean-square ratio %.3f" % (name, ms))
        assert lo < ms < hi and abs(ms / pc.FLIP_AT - 1.0) >= 0.01
        assert flip == (ms > pc.FLIP_AT)
        assert 100.0 < ms < 10000.0
        assert np.array_equal(segmenter.pcm_to_mono(pcm), pc.mono_by_the_rule(pcm, flip))
        assert not np.array_equal(pc.mono_by_the_rule(pcm, True), pc.mono_by_the_rule(pcm, False))


def test_heavy_tailed_pair_tells_the_mean_square_from_other_statistics():
    """heavy: mean-square ratio above 1100 (flip), squared ratio of the mean absolute values below 900 (a rule on those
    does not flip)."""
    from oracle import segmenter
    pcm, flip = pc.stereo_case("heavy")
    ms, ma = pc.ratios(pcm)
    print("heavy: mean-square ratio %.1f, squared ratio of mean absolute values %.1f" % (ms, ma))
    assert ms > 1100.0 and ma < 900.0 and flip
    assert np.array_equal(segmenter.pcm_to_mono(pcm), pc.mono_by_the_rule(pcm, True))


def test_silent_stereo_is_not_flipped_and_stays_zero():
    from oracle import segmenter
    pcm, flip = pc.stereo_case("silent")
    out = segmenter.pcm_to_mono(pcm)
    assert not flip and out.shape == (20000,) and not out.any() and not np.signbit(out).any()


def test_the_16k_pair_flips_only_after_resampling():
    """Raw ratio below 900, the oracle's resampled signal above 1100: only a decision taken after the resampler flips."""
    from oracle import resample as orr
    pcm = pc.after_resampling_case()
    raw, _ = pc.ratios(pcm)
    x = np.multiply(pcm, 1 / 32768, dtype=np.float32).T.copy()
    res, _ = pc.ratios(orr.resample_chunked(x, 16000, pc.SR))
    print("16 kHz pair: ratio %.1f on the file's samples, %.3e after resampling" % (raw, res))
    assert raw < 900.0 and res > 1100.0
    from oracle import segmenter
    assert np.abs(segmenter.pcm_to_mono(pcm, 16000, pc.SR)).max() > 0.3


def test_channel_cases_have_unequal_channels():
    for n_ch in (3, 6):
        pcm = pc.channels_case(n_ch)
        assert pcm.shape == (5003, n_ch) and np.abs(pcm).max() > 20000
        rms = np.sqrt(np.mean(pcm.astype(np.float64) ** 2, axis=0))
        assert np.all(rms[:-1] > 1.2 * rms[1:])              # every channel at a level of its own
        # a kernel that averages the first two channels only, or drops the last, is further off than the bound
        m64 = pcm.astype(np.float64).mean(axis=1) / 32768.0
        assert np.abs(pcm[:, :2].astype(np.float64).mean(axis=1) / 32768.0 - m64).max() > 1e3 * pc.mean_bound(n_ch)
        assert np.abs(pcm[:, :-1].astype(np.float64).mean(axis=1) / 32768.0 - m64).max() > 1e3 * pc.mean_bound(n_ch)


# --------------------------------------------------------------------------------------------------------- resampler
def test_rate_table_is_what_it_says():
    from pfann_amd import resample as pr
    for rate, want in pc.RATES.items():
        tab, old, new, width = pr.filter_table(rate, pc.SR)
        assert (old, new) == want == pr.reduced_rates(rate, pc.SR)
        assert tab.shape == (new, 2 * width + old) and tab.shape[1] <= 721
    assert pr.filter_table(96000, pc.SR)[3] == 305
    assert max(pc.resample_input(r, l).shape[0] for r, l in pc.RESAMPLE) == 1446000


@pytest.mark.parametrize("rate,label", pc.RESAMPLE, ids=pc.RESAMPLE_IDS)
def test_numpy_statement_of_the_kernel_equals_the_oracle(rate, label):
    """piece_plan + filter_table, applied as resample_kernel applies them (float64 accumulate), against
    oracle.resample.resample_chunked with the same table: equal shapes (also restated from the reference's loop:
    pc.expected_n_out), values within 1e-6 (the oracle's conv1d accumulates up to 622 products in fp32).  This pins
    piece_plan to the oracle's reading of the reference's loop at every seam length, without a GPU."""
    pcm = pc.resample_input(rate, label)
    t0 = time.perf_counter()
    want = pc.planar_kernel_table(rate, label)
    got = pc.numpy_resample(pcm, rate)
    assert got.shape == want.shape == (pcm.shape[1], pc.expected_n_out(rate, pcm.shape[0]))
    err = float(np.abs(got - want).max()) if want.size else 0.0
    print("resample %d Hz %s: %d -> %d samples, numpy statement vs oracle %.2e (%.1f s)"
          % (rate, label, pcm.shape[0], want.shape[1], err, time.perf_counter() - t0))
    assert err < 1e-6
    if label == "1smp":
        assert want.shape[1] == pc.RATES[rate][1] // pc.RATES[rate][0]       # 4 kHz: 2 samples; 16 kHz and up: none
    if label == "60s":            # one whole minute less its last half second, and a tail of 1 s less its first
        assert want.shape[1] == 60 * pc.SR
    assert pc.mono_kernel_table(rate, label).shape == (want.shape[1],)


def test_one_sample_at_16k_gives_no_output():
    from pfann_amd import resample as pr
    assert pr.piece_plan(1, 16000, pc.SR)[1] == 0 and pr.piece_plan(1, 4000, pc.SR)[1] == 2
    assert pc.expected_n_out(32000, 1) == 0 and pc.expected_n_out(96000, 1) == 0


def test_rates_no_table_is_built_for():
    """A header's rate is a number like any other: 0 and absurd ones are refused before a table is sized from them
    (old / new = 33554432 / 125 for 0x80000000: a table of 160 GB)."""
    from pfann_amd import resample as pr
    for bad in (0, -8000, 0x80000000, pr.MAX_RATE + 1):
        with pytest.raises(ValueError):
            pr.check_rate(bad)
    assert pr.check_rate(pr.MAX_RATE) == pr.MAX_RATE and pr.check_rate(1) == 1 and pr.MAX_RATE >= 768000


# ------------------------------------------------------------------------------------------ three readers, one table
def _wave_read(path):
    """Python's `wave` module, read the way the reference reads it (datautil/audio.py:130-149: blocks of 1024 frames until
    a short one, each through np.frombuffer; musicdata.py:48 then shapes the samples to [-1, n_ch]).  Asking for more
    frames than the header's count is what hands it a data chunk's stray bytes, on which frombuffer or the reshape raise;
    oracle.segmenter.read_wav_int16 asks for getnframes() and never sees them."""
    import wave
    try:
        with wave.open(path, "rb") as w:
            if w.getsampwidth() != 2:
                raise NotImplementedError("16-bit wav only")
            n_ch, sr, blocks = w.getnchannels(), w.getframerate(), []
            while True:
                dat = w.readframes(1024)
                blocks.append(np.frombuffer(dat, dtype=np.int16))
                if len(dat) < 1024 * n_ch * 2:
                    break
        return n_ch, sr, np.concatenate(blocks).reshape(-1, n_ch)
    except Exception:
        return None


def _python_read(path):
    from pfann_amd.musicdata import read_wav_pcm16
    try:
        pcm, sr = read_wav_pcm16(path)
        return pcm.shape[1], sr, pcm
    except Exception:
        return None


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a[:2] == b[:2] and
                                         a[2].shape == b[2].shape and np.array_equal(a[2], b[2]))


def test_header_table_three_ways(tmp_path):
    """Every row of pc.header_table(): read_wav_pcm16 and pfann_wav_probe + pfann_wav_read agree with the row's stated
    answer and hence with each other -- accept or refuse, channels, rate, frames, samples -- and with Python's `wave`
    module, except on the rows marked as documented differences (there `wave` may refuse what the project reads, never
    the other way round, and never with other samples)."""
    from pfann_amd import lib as L
    table = pc.header_table()
    paths = pc.write_header_table(tmp_path)
    names = list(table)
    native = pc.native_read(L, [paths[n] for n in names] + [str(tmp_path / "missing.wav")])
    assert native[-1][0] == -1 and _python_read(str(tmp_path / "missing.wav")) is None
    for name, (status, n_ch, rate, pcm) in zip(names, native[:-1]):
        want, wave_may_differ = table[name][1], table[name][2]
        nat = (n_ch, rate, pcm) if status == 0 else None
        py = _python_read(paths[name])
        ref = _wave_read(paths[name])
        assert _same(py, want), "read_wav_pcm16 on %s" % name
        assert _same(nat, want), "native reader on %s (status %d)" % (name, status)
        if want is None:
            assert status in (-2, -3, -4), name
        if wave_may_differ:
            assert ref is None or _same(ref, want), name
        else:
            assert _same(ref, want), "the wave module on %s" % name
    for name in ("stray_byte_mono", "stray_sample_stereo", "stray_sample_3ch"):      # the reference fails these files
        assert _wave_read(paths[name]) is None, name


def test_mixed_list_is_cut_into_uniform_and_mixed_groups(tmp_path):
    """The list of tests/test_gpu_pcm_cases.py through builder._native_groups with a stub engine: at 8 windows per group
    it gives uniform groups, mixed groups and a mixed group with a file shorter than a window (the zero-padded slab), the
    window counts the GPU test expects, and 0-segment songs for every malformed file -- the 0x80000000 one without a
    resampling plan or table being asked for."""
    import types
    import torch
    from pfann_amd import builder, lib as L, resample as pr
    from pfann_amd.musicdata import MusicDataset
    paths, kinds = pc.write_mixed_list(tmp_path)
    rates = []

    def fake_mono(pcm, sample_rate=None):
        rates.append(int(sample_rate))
        n = pcm.shape[0] if sample_rate == pc.SR else pr.piece_plan(pcm.shape[0], pr.check_rate(sample_rate), pc.SR)[1]
        return types.SimpleNamespace(shape=(n,))
    eng = types.SimpleNamespace(lib=L.load(), seg_len=pc.SEG, params=pc.params(), pcm16_to_mono=fake_mono)

    class Pool:
        def get(self, n):
            return torch.empty(max(n, 1), dtype=torch.int16)
    seen, shapes = {}, []
    for items, slab, _, _ in builder._native_groups(eng, MusicDataset(paths, pc.params()), pc.HOP, 8, Pool(), 2):
        have = [it[2] if it[0] in ("host", "slab") else it[1].shape[0] for _, n_seg, it in items if n_seg]
        shapes.append((slab is not None, any(h < pc.SEG for h in have)))
        seen.update({kinds[i]: n_seg for i, n_seg, _ in items})
    assert list(seen) == kinds
    assert {k for k, n in seen.items() if n == 0} == set(pc.MIXED_ZERO)
    assert (seen["mono_long"], seen["mono_1s"], seen["mono_short"], seen["empty_8k"], seen["stereo_16k"], seen["mono_6k"]) == \
        (7, 1, 1, 1, 3, 5)
    assert (True, False) in shapes and (False, False) in shapes and (False, True) in shapes
    assert sorted(set(rates)) == [6000, 8000, 16000]


# -------------------------------------------------------------------------- the native reader under the sanitizers
def _clang():
    for c in (os.environ.get("HIP_CLANG_PATH") and os.path.join(os.environ["HIP_CLANG_PATH"], "clang++"),
              os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++"), shutil.which("clang++")):
        if c and os.path.exists(c):
            return c
    return None


def test_native_wav_reader_under_address_and_ub_sanitizers(tmp_path):
    """csrc/wavio.hip (host code only) compiled as C++ with -fsanitize=address,undefined together with a small program
    of its own that probes the header table's files on two threads and reads them into an exactly sized heap buffer: a
    read past the buffer, a misaligned or overflowing header computation, or a race on the info array ends the child
    with a non-zero status."""
    clang = _clang()
    assert clang is not None, "the ROCm clang++ that builds the library is needed"
    exe = str(tmp_path / "wav_reader_check")
    san = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread"]
    probe = tmp_path / "empty.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run([clang] + san + [str(probe), "-o", str(tmp_path / "empty")], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("this compiler cannot link the sanitizer runtime: " + r.stderr[-300:])
    cmd = [clang] + san + ["-I", os.path.join(REPO, "include"), os.path.join(REPO, "tests", "native", "wav_reader_check.cpp"),
                           "-x", "c++", os.path.join(REPO, "pfann_amd", "csrc", "wavio.hip"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    paths = pc.write_header_table(tmp_path)
    files = [paths[n] for n in paths] + [str(tmp_path / "missing.wav")]
    r = subprocess.run([exe] + files, capture_output=True, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    # the program's own account agrees with the table: which files it read, and how many samples
    table = pc.header_table()
    said = dict(line.split()[:2] for line in r.stdout.splitlines() if line.startswith(str(tmp_path)))
    for name, (_, want, _) in table.items():
        assert int(said[paths[name]]) == (want[2].size if want is not None else -1), name
