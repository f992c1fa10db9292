"""The case table of the audio front door, importable without a GPU: 16-bit PCM -> the mono float signal at the model's
rate (pfann_amd/csrc/mel.hip: pcm_to_mono_kernel, pcm_mono8_kernel, resample_kernel, planar_to_mono_kernel; the two WAV
readers, pfann_amd/csrc/wavio.hip and pfann_amd.musicdata.read_wav_pcm16; the slab assembly of pfann_amd/builder.py), on
configs/tiny.json (8000 Hz, 1 s windows every 0.5 s).

Every input is built from a seed, and every case states the CONDITION that makes it mean something (a float64 power ratio
on the far side of a threshold, an oracle output of a given shape); tests/test_pcm_host.py asserts those conditions with
float64 numpy and the oracle only, so that a case cannot silently become vacuous; tests/test_gpu_pcm_cases.py runs the
kernels on the same inputs.  References are computed once per session, shared and read-only."""
import functools
import json
import math
import os
import struct

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 8000                 # configs/tiny.json
SEG, HOP = 8000, 4000
FLIP_AT = 1000.0          # musicdata.py:74-79: pow1 > pow2 * 1000


def params():
    return json.load(open(os.path.join(REPO, "configs", "tiny.json")))


def _i16(x):
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def _frozen(a):
    a.setflags(write=False)
    return a


# ------------------------------------------------------------------------------------------------ the fake-stereo rule
def opposite_pair(a, rho):
    """l = round(a), r = -round(g a) with g = (sqrt(rho) - 1) / (sqrt(rho) + 1): (l - r) / (l + r) = sqrt(rho) up to the
    rounding to int16, so every power ratio of difference to sum is rho."""
    g = (math.sqrt(rho) - 1.0) / (math.sqrt(rho) + 1.0)
    return np.stack([_i16(a), _i16(-np.round(g * a))], 1)


def ratios(x):
    """float64 (mean-square ratio, squared ratio of the mean absolute values) of difference to sum; x [n, 2] or [2, n]
    in any scale.  inf where the sum is silent, nan where both are."""
    x = np.asarray(x, np.float64)
    l, r = (x[:, 0], x[:, 1]) if x.shape[1] == 2 else (x[0], x[1])
    d, s = l - r, l + r
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.mean(d * d) / np.mean(s * s)), float((np.mean(np.abs(d)) / np.mean(np.abs(s))) ** 2)


@functools.lru_cache(maxsize=None)
def stereo_case(name):
    """-> (int16 [n, 2] at the native rate, flip expected).

    rho900 / rho1100: 20,000 samples of 3000 N(0, 1); the float64 mean-square ratio is within 0.1 of its target, at least
    1 % from 1000 -- far beyond what any fp32 or float64 summation order of 2e4 terms moves it (2e4 * 2^-24 ~ 1e-3
    relative at the very worst).  A threshold of 100 or of 10,000 gives both the same answer.
    heavy: a heavy-tailed signal, 20 samples of +-30000 in 19,980 of +-0.52: the little ones round to l = +-1, r = 0, where
    difference and sum are EQUAL, the large ones carry the target ratio 1250.  The mean squares see the large ones only
    (ratio > 1100: flip); the mean absolute values are half little ones (squared ratio < 900: a kernel that compares those
    does not flip).
    silent: all zeros; 0 > 0 * 1000 is false: no flip, and the output is zero."""
    if name in ("rho900", "rho1100"):
        rho = float(name[3:])
        rng = np.random.default_rng(int(rho))
        return _frozen(opposite_pair(np.clip(3000.0 * rng.standard_normal(20000), -32768, 32767), rho)), rho > FLIP_AT
    if name == "heavy":
        rng = np.random.default_rng(7)
        a = 0.52 * np.where(rng.random(20000) < 0.5, -1.0, 1.0)
        at = rng.choice(20000, 20, replace=False)
        a[at] = 30000.0 * np.where(rng.random(20) < 0.5, -1.0, 1.0)
        return _frozen(opposite_pair(a, 1250.0)), True
    if name == "silent":
        return _frozen(np.zeros((20000, 2), np.int16)), False
    raise KeyError(name)


STEREO = ("rho900", "rho1100", "heavy", "silent")


def mono_by_the_rule(pcm, flip):
    """The answer stated without the rule: (l + r) / 2, or (l - r) / 2 where the file is flipped, in fp32 (the channels are
    exact in fp32, so is their sum, and so is its half)."""
    x = pcm.astype(np.float32) / np.float32(32768.0)
    return ((x[:, 0] - x[:, 1]) if flip else (x[:, 0] + x[:, 1])) / np.float32(2.0)


@functools.lru_cache(maxsize=None)
def after_resampling_case():
    """16 kHz stereo, 2.5 s: l = s + h, r = -s + h; s = 0.3 sin(440 Hz) + 0.1 sin(1300 Hz) survives the resampler to
    8 kHz, h = 0.04 sin(6 kHz) does not.  On the file's own samples the ratio is 62.5 (no flip); after resampling the
    sum is all but gone and the ratio is ~3e7 (flip), which is where the reference decides (musicdata.py:72-79 runs
    after the resampler).  -> int16 [40000, 2]."""
    t = np.arange(40000) / 16000.0
    s = 0.3 * np.sin(2 * np.pi * 440.0 * t) + 0.1 * np.sin(2 * np.pi * 1300.0 * t)
    h = 0.04 * np.sin(2 * np.pi * 6000.0 * t)
    return _frozen(np.stack([_i16((s + h) * 32767.0), _i16((-s + h) * 32767.0)], 1))


# ------------------------------------------------------------------------------------------------------ channel counts
@functools.lru_cache(maxsize=None)
def channels_case(n_ch, n=5003):
    """int16 [n, n_ch], every channel with content of its own and a level of its own (n: odd, several blocks)."""
    rng = np.random.default_rng(100 + n_ch)
    t = np.arange(n) / float(SR)
    cols = [0.9 * 0.7 ** c * (np.sin(2 * np.pi * (300.0 + 170.0 * c) * t + c) + 0.05 * rng.standard_normal(n))
            for c in range(n_ch)]
    return _frozen(_i16(np.stack(cols, 1) * 32767.0))


def mean_bound(n_ch):
    """|fp32 channel mean - float64 channel mean| for samples of magnitude <= 1: the samples are exact in fp32; the first
    addition (to 0) is exact, each of the other n_ch - 1 rounds a partial sum of magnitude <= n_ch, i.e. by at most
    n_ch 2^-24 (half an ulp below 2 n_ch, generously); the division by n_ch brings those to 2^-24 each and adds one
    rounding of a quotient of magnitude <= 1, 2^-24 at most: n_ch roundings of 2^-24."""
    return n_ch * 2.0 ** -24


MONO_LENGTHS = (1, 7, 8, 9, 2049)      # below, at and beside the eight-sample kernel's width; more than one block


@functools.lru_cache(maxsize=None)
def mono_case(n):
    rng = np.random.default_rng(300 + n)
    x = rng.integers(-32768, 32768, n).astype(np.int16)
    x[:2] = (-32768, 32767)[:min(n, 2)]
    return _frozen(x[:, None])


# --------------------------------------------------------------------------------------------------------- resampler
RATES = {4000: (1, 2), 6000: (3, 4), 7350: (147, 160), 12000: (3, 2), 32000: (4, 1), 96000: (12, 1)}
SEAM_RATES = (4000, 6000, 12000)


def _lengths(rate):
    """{label: samples}.  The seam lengths (the reference cuts a piece as soon as a whole minute is there,
    musicdata.py:33-65) only at the low rates, where 120.5 s stay below 1.5 M samples."""
    out = {"1smp": 1, "3ms": max(2, int(round(0.003 * rate))), "0.4s": int(0.4 * rate), "1s": rate}
    if rate in SEAM_RATES:
        out.update({"60s-1": 60 * rate - 1, "60s": 60 * rate, "60s+1": 60 * rate + 1, "61s": 61 * rate,
                    "119s": 119 * rate, "120.5s": int(120.5 * rate)})
    return out


RESAMPLE = [(rate, label) for rate in RATES for label in _lengths(rate)]
RESAMPLE_IDS = ["%d-%s" % c for c in RESAMPLE]
SHORT = ("1smp", "3ms", "0.4s", "1s")


@functools.lru_cache(maxsize=None)
def resample_input(rate, label):
    """int16 [n, n_ch]: two tones below the file's Nyquist frequency and white noise above and below the model's; the
    0.4 s files are stereo with unequal channels (the planar power pass runs, and must not flip)."""
    n = _lengths(rate)[label]
    rng = np.random.default_rng(rate + 17 * n % 1000)
    t = np.arange(n) / float(rate)
    x = 0.4 * np.sin(2 * np.pi * 440.0 * t) + 0.2 * np.sin(2 * np.pi * 0.19 * rate * t + 1.0) + 0.1 * rng.standard_normal(n)
    pcm = _i16(x * 32767.0)[:, None]
    if label == "0.4s":
        pcm = np.concatenate([pcm, pcm // 2], 1)
    return _frozen(pcm)


def expected_n_out(rate, n):
    """What the reference's loop yields, restated apart from piece_plan and chunk_plan: whole minutes are cut every 59 s
    while one is left, each gives 60 s less the half seconds at its inner seams; the tail is resampled to
    int(new * tail / old) and loses its leading half second, if it has a piece before it."""
    old, new = RATES[rate]
    n_out, start, first = 0, 0, True
    while n - start >= 60 * rate:
        n_out += 60 * SR - SR // 2 - (0 if first else SR // 2)
        start += 59 * rate
        first = False
    tail = new * (n - start) // old
    return n_out + (tail if first else max(tail - SR // 2, 0))


def numpy_resample(pcm, rate):
    """The kernel's statement in numpy (resample_kernel of csrc/mel.hip), from the host code's own piece_plan and
    filter_table, accumulated in float64: out[c, o] = sum_t K[phase][t] x[clamp(frame old + t - width, 0, len - 1)] within
    the piece that owns output o.  -> float64 [n_ch, n_out]."""
    from pfann_amd import resample as pr
    tab, old, new, width = pr.filter_table(rate, SR)
    plan, n_out = pr.piece_plan(pcm.shape[0], rate, SR)
    x = pcm.astype(np.float64).T / 32768.0
    K = tab.astype(np.float64)
    taps = np.arange(2 * width + old)
    out = np.zeros((x.shape[0], n_out))
    for in_start, in_len, skip, keep, off in plan.tolist():
        piece = x[:, in_start:in_start + in_len]
        for b0 in range(0, keep, 32768):
            jl = skip + np.arange(b0, min(b0 + 32768, keep))
            frame, phase = jl // new, jl % new
            idx = np.clip(frame[:, None] * old - width + taps[None, :], 0, in_len - 1)
            out[:, off + b0:off + b0 + jl.shape[0]] = np.einsum("jt,cjt->cj", K[phase], piece[:, idx])
    return out


@functools.lru_cache(maxsize=None)
def planar_kernel_table(rate, label):
    """oracle.resample.resample_chunked with the table the kernel is given -> float32 [n_ch, n_out], before the channels
    are mixed."""
    from oracle import resample as orr
    from pfann_amd import resample as pr
    pcm = resample_input(rate, label)
    x = np.multiply(pcm, 1 / 32768, dtype=np.float32).T.copy()
    return _frozen(np.ascontiguousarray(orr.resample_chunked(x, rate, SR, pr.filter_table(rate, SR)[0])))


@functools.lru_cache(maxsize=None)
def mono_kernel_table(rate, label):
    from oracle import segmenter
    from pfann_amd import resample as pr
    return _frozen(segmenter.pcm_to_mono(resample_input(rate, label), rate, SR, resample_table=pr.filter_table(rate, SR)[0]))


@functools.lru_cache(maxsize=None)
def mono_own_table(rate, label):
    """... and with the oracle's own table (float64 from the definition)."""
    from oracle import segmenter
    return _frozen(segmenter.pcm_to_mono(resample_input(rate, label), rate, SR))


# ---------------------------------------------------------------------------------------------------------- WAV bytes
def wav_bytes(data, n_ch=1, rate=SR, bits=16, tag=1, fmt_size=16, sub_tag=None, block_align=None, riff_size=None,
              data_size=None, before_fmt=b"", after_data=b"", data_first=False):
    """A RIFF/WAVE file from its parts, every header field as asked for (right or wrong).  fmt_size 18: cbSize = 0;
    40: WAVE_FORMAT_EXTENSIBLE's extension with sub_tag as the first two bytes of the sub-format GUID."""
    data = bytes(data)
    width = (bits + 7) // 8
    align = n_ch * width if block_align is None else block_align
    fmt = struct.pack("<HHIIHH", tag, n_ch, rate & 0xFFFFFFFF, (rate * align) & 0xFFFFFFFF, align, bits)
    if fmt_size == 18:
        fmt += struct.pack("<H", 0)
    elif fmt_size == 40:
        fmt += struct.pack("<HHIH", 22, bits, 0, 1 if sub_tag is None else sub_tag) + bytes.fromhex("000000001000800000aa00389b71")
    assert len(fmt) == fmt_size
    fmt_chunk = b"fmt " + struct.pack("<I", fmt_size) + fmt
    data_chunk = b"data" + struct.pack("<I", len(data) if data_size is None else data_size) + data
    body = b"WAVE" + before_fmt + ((data_chunk + fmt_chunk) if data_first else (fmt_chunk + data_chunk)) + after_data
    return b"RIFF" + struct.pack("<I", len(body) if riff_size is None else riff_size) + body


def chunk(cid, payload):
    """One RIFF chunk, padded to an even length as the format asks."""
    return cid + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")


@functools.lru_cache(maxsize=None)
def header_table():
    """name -> (file bytes, what both readers must say: (n_ch, rate, int16 samples [n, n_ch]) or None for a refusal,
    whether Python's `wave` module may differ).  The last is True for the two documented differences only (DESIGN.md
    section 2): extensible PCM, which the reference accepts through its HackExtensibleWave and `wave` itself only from
    Python 3.12 on, and data chunks with stray bytes, where the reference fails the file (its reshape to [-1, n_ch]
    raises) and this project keeps the whole frames."""
    rng = np.random.default_rng(41)
    s1 = rng.integers(-32768, 32768, 300).astype(np.int16)
    s2, s3 = s1[:200].reshape(100, 2), s1.reshape(100, 3)
    b1, b2, b3 = s1.tobytes(), s2.tobytes(), s3.tobytes()
    ok = lambda pcm, rate=SR: (pcm.shape[1] if pcm.ndim == 2 else 1, rate, pcm if pcm.ndim == 2 else pcm[:, None])
    rows = {
        "plain": (wav_bytes(b1), ok(s1), False),
        "plain_stereo_44k": (wav_bytes(b2, 2, 44100), ok(s2, 44100), False),
        "streamed_size": (wav_bytes(b1, riff_size=0xFFFFFFFF, data_size=0xFFFFFFFF), ok(s1), False),
        "fmt18": (wav_bytes(b1, fmt_size=18), ok(s1), False),
        "extensible_pcm": (wav_bytes(b2, 2, fmt_size=40, tag=0xFFFE, sub_tag=1), ok(s2), True),
        "extensible_float": (wav_bytes(b2, 2, fmt_size=40, tag=0xFFFE, sub_tag=3), None, False),
        "odd_list_before_fmt": (wav_bytes(b1, before_fmt=chunk(b"LIST", b"INFOabc")), ok(s1), False),
        "data_before_fmt": (wav_bytes(b1, data_first=True), None, False),
        "bits8": (wav_bytes(b1[:300], bits=8), None, False),
        # 12 bits in two bytes: `wave` reads (12 + 7) // 8 = 2 bytes per sample, and so do both readers
        "bits12": (wav_bytes(b1, bits=12), ok(s1), False),
        "bits24": (wav_bytes(b1[:300], bits=24), None, False),
        "float_tag": (wav_bytes(b1, bits=32, tag=3), None, False),
        "channels0": (wav_bytes(b1, n_ch=0), None, False),
        "stray_byte_mono": (wav_bytes(b1[:21]), ok(s1[:10]), True),
        "stray_sample_stereo": (wav_bytes(b1[:202], 2), ok(s2[:50]), True),
        "stray_sample_3ch": (wav_bytes(b1[:2 * 100], 3), ok(s3[:33]), True),
        "truncated": (wav_bytes(b1[:400], data_size=600), ok(s1[:200]), False),
        "junk_after_data": (wav_bytes(b1, after_data=chunk(b"junk", b"\x01\x02\x03") + b"\xff" * 7), ok(s1), False),
        "wrong_block_align": (wav_bytes(b2, 2, block_align=3), ok(s2), False),
        "empty_data": (wav_bytes(b"", 2), ok(s2[:0]), False),
        "rate0": (wav_bytes(b1, rate=0), ok(s1, 0), False),
        "rate_0x80000000": (wav_bytes(b1, rate=0x80000000), ok(s1, 0x80000000), False),
        "not_a_wav": (b"RIFX" + b1[:64], None, False),
    }
    return rows


def write_header_table(folder):
    """-> {name: path} of header_table()'s files, written to `folder`."""
    paths = {}
    for name, (raw, _, _) in header_table().items():
        paths[name] = os.path.join(str(folder), name + ".wav")
        with open(paths[name], "wb") as f:
            f.write(raw)
    return paths


def native_read(lib_module, paths, n_threads=2):
    """pfann_wav_probe + pfann_wav_read of `paths` into one exactly sized buffer -> [(status, n_ch, rate, int16 [n, n_ch]
    or None)]."""
    import ctypes
    lib = lib_module.load()
    n = len(paths)
    arr = (ctypes.c_char_p * n)(*[os.fsencode(p) for p in paths])
    info = (lib_module.WavInfo * n)()
    assert lib.pfann_wav_probe(arr, n, n_threads, info) == 0
    sizes = [i.n_frames * i.n_ch if i.status == 0 else 0 for i in info]
    offs = (ctypes.c_int64 * n)(*np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64).tolist())
    total = int(sum(sizes))
    slab = np.full(total + 1, 0x5A5A, np.int16)              # one guard word behind the last sample
    assert lib.pfann_wav_read(arr, n, n_threads, info, offs, slab.ctypes.data, total) == 0
    assert slab[total] == 0x5A5A
    out = []
    for j, i in enumerate(info):
        pcm = slab[offs[j]:offs[j] + sizes[j]].reshape(-1, i.n_ch).copy() if i.status == 0 else None
        out.append((int(i.status), int(i.n_ch), int(i.sample_rate), pcm))
    return out


# ------------------------------------------------------------------------------------------------------ the file lists
def write_mixed_list(folder):
    """The list on which the two file-reading paths differ -> (paths, kinds): well-formed files of every kind the native
    reader's groups tell apart (uniform: mono, native rate, at least a window; anything else: not), and malformed ones,
    which are 0-segment songs on every path."""
    from pfann_amd import synth
    folder = str(folder)
    song = lambda i, sec, sr=SR: synth.make_song(900 + i, seconds=sec, sr=sr)
    l = song(3, 2.6)
    files = [
        ("mono_long", lambda p: synth.write_wav(p, song(0, 4.3))),
        ("mono_1s", lambda p: synth.write_wav(p, song(1, 1.0))),
        ("mono_short", lambda p: synth.write_wav(p, song(2, 0.7)[:4801])),
        ("stereo", lambda p: synth.write_wav(p, np.stack([l, song(4, 2.6) // 3], 1))),
        ("fake_stereo", lambda p: synth.write_wav(p, np.stack([l, -l], 1))),
        ("rate0", lambda p: open(p, "wb").write(wav_bytes(song(5, 1.5).tobytes(), rate=0))),
        ("three_channels", lambda p: synth.write_wav(p, np.stack([l, song(6, 2.6) // 2, song(7, 2.6) // 4], 1))),
        ("stereo_16k", lambda p: synth.write_wav(p, np.stack([song(8, 2.2, 16000), song(9, 2.2, 16000) // 2], 1), sr=16000)),
        ("rate_0x80000000", lambda p: open(p, "wb").write(wav_bytes(song(10, 1.5).tobytes(), rate=0x80000000))),
        ("mono_6k", lambda p: synth.write_wav(p, song(11, 3.1, 6000), sr=6000)),
        ("empty_8k", lambda p: synth.write_wav(p, np.zeros(0, np.int16))),
        ("bits8", lambda p: open(p, "wb").write(wav_bytes(bytes(9000), bits=8))),
        ("empty_16k", lambda p: synth.write_wav(p, np.zeros(0, np.int16), sr=16000)),
        ("not_a_wav", lambda p: open(p, "wb").write(b"not a wav at all")),
        ("missing", lambda p: None),
        ("mono_tail", lambda p: synth.write_wav(p, song(12, 1.9))),
    ]
    paths = []
    for name, write in files:
        paths.append(os.path.join(folder, name + ".wav"))
        write(paths[-1])
    return paths, [name for name, _ in files]


# name -> windows, for the kinds whose count is not (n - SEG) // HOP + 1 of a native-rate file
MIXED_ZERO = ("rate0", "rate_0x80000000", "bits8", "empty_16k", "not_a_wav", "missing")


def write_uniform_list(folder):
    """Mono files at the native rate, each at least one window long: the native reader's uniform slab.  Four of the sample
    counts are no multiples of 8, so the files do not start on the eight-sample kernel's grid."""
    from pfann_amd import synth
    counts = (8000, 12345, 8001, 20003, 16000, 9999)
    paths = []
    for i, n in enumerate(counts):
        paths.append(os.path.join(str(folder), "u%d.wav" % i))
        synth.write_wav(paths[-1], synth.make_song(950 + i, seconds=3.0)[:n])
    return paths, counts
