"""The oracle (oracle/) against the golden vectors generated from the reference's own code
(tests/golden/make_golden.py) and against the probed outputs SURVEY.md §8c records."""
import json
import os

import numpy as np
import pytest

import make_golden as mg
from oracle import encoder, melspec, native, search, segmenter, seqscore
from pfann_amd import synth

G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("name", ["default", "seg", "n640d64", "tiny", "nafstyle", "elu_full", "strides_pow2", "strides_np2"])
def test_encoder_matches_reference(name):
    z = np.load(os.path.join(G, "encoder_%s.npz" % name))
    params = json.loads(str(z["params"]))
    _, _, _, F, T = synth.model_dims(params)
    sd = synth.make_state_dict(params, seed=123)
    x = mg.encoder_inputs(F, T)
    taps = []
    emb = encoder.encode(x, sd, params, norm=True, taps=taps)
    raw = encoder.encode(x, sd, params, norm=False)
    assert np.abs(emb - z["emb"]).max() < 2e-6
    assert np.abs(raw - z["raw"]).max() < 2e-5 * max(1.0, np.abs(z["raw"]).max())
    sums = np.array([[t.astype(np.float64).sum(), np.abs(t.astype(np.float64)).sum()] for t in taps])
    assert np.allclose(sums, z["tap_sums"], rtol=1e-5, atol=1e-2)


def test_segmenter_matches_reference(tmp_path):
    z = np.load(os.path.join(G, "segmenter.npz"))
    params = json.load(open(os.path.join(os.path.dirname(G), "..", "configs", "default.json")))
    inputs = mg.segmenter_inputs()
    for name, pcm in inputs.items():
        synth.write_wav(str(tmp_path / (name + ".wav")), pcm)
    (tmp_path / "notwav.wav").write_bytes(b"this is not a wave file")
    for fsm in (1, 2):
        p = json.loads(json.dumps(params))
        p["indexer"]["frame_shift_mul"] = fsm
        for name in list(inputs) + ["missing", "notwav"]:
            w = segmenter.load_segments(str(tmp_path / (name + ".wav")), p)
            key = "%s_fsm%d" % (name, fsm)
            assert tuple(z[key + "_shape"]) == w.shape, key
            if w.shape[0]:
                # bit-identical rows, and checksums over every row
                assert np.array_equal(w[z[key + "_rows"]], z[key + "_vals"]), key
                sums = np.stack([w.astype(np.float64).sum(1), np.abs(w.astype(np.float64)).sum(1)], 1)
                assert np.allclose(sums, z[key + "_sums"], rtol=0, atol=1e-9), key


DB_CASES = ["clean_hit", "negative_offset", "past_end", "k_gt_ntotal", "duplicate_songs",
            "nonpositive_best", "no_candidates", "frame_shift_mul2", "empty_db", "random_noisy"]


@pytest.mark.parametrize("name", DB_CASES)
def test_seqscore_python_path_matches_reference(name):
    z = np.load(os.path.join(G, "database.npz"))
    db, q, labels = z[name + "_db"], z[name + "_q"], z[name + "_labels"]
    pos = seqscore.song_pos_from_key(z[name + "_key"])
    fsm = int(z[name + "_fsm"])
    score, (song, sec), ss = seqscore.query_embeddings_base(q, labels, db, pos, 0.5, fsm)
    assert song == int(z[name + "_song"])
    assert sec == float(z[name + "_sec"])
    assert score == float(z[name + "_score"]) or abs(score - float(z[name + "_score"])) < 1e-6
    assert np.allclose(ss, z[name + "_song_score"], atol=1e-6)
    # the labels the reference searched with are the exact flat top-k
    if name not in ("no_candidates", "nonpositive_best") and db.shape[0]:
        D, I = search.flat_ip_topk(q, db, labels.shape[1])
        assert np.array_equal(I, labels)
        D2, I2 = native.flat_ip_topk(q, db, labels.shape[1])
        assert np.array_equal(I2, labels)
        assert np.abs(D - D2).max() < 1e-6


@pytest.mark.parametrize("name", DB_CASES)
def test_seqscore_c_path(name):
    """C restatement of cpp/seqscore.cpp: agrees with the Python path wherever SURVEY.md
    §8c says the two reference paths agree, and shows the documented divergences."""
    z = np.load(os.path.join(G, "database.npz"))
    db, q, labels = z[name + "_db"], z[name + "_q"], z[name + "_labels"]
    if db.shape[0] == 0:
        pytest.skip("cpp path has no empty-db branch (database.py:126-127 is python-only)")
    pos = seqscore.song_pos_from_key(z[name + "_key"])
    fsm = int(z[name + "_fsm"])
    best, ss = native.seq_score(db, pos, q, labels, fsm, 0.0)
    hop = 0.5
    if name == "no_candidates":
        assert best == -1 and not ss.any()
        return
    assert best == int(z[name + "_song"])
    if name == "nonpositive_best":
        # song_scores never records a non-positive score; caller reads back 0.0 / 0.0
        assert not ss.any()
        return
    # caller-side scaling of database.py:190-193
    assert abs(ss[best, 0] - float(z[name + "_score"])) < 1e-6
    assert ss[best, 1] * hop / fsm == float(z[name + "_sec"])
    ss2 = ss.copy()
    ss2[:, 1] *= hop / fsm
    assert np.allclose(ss2, z[name + "_song_score"], atol=1e-6)


def test_seqscore_c_probed_values():
    """Known answers recorded from the compiled reference in SURVEY.md §8c:
    4 of 6 rows match with divisor 6 -> 0.6666666269 in fp32."""
    z = np.load(os.path.join(G, "database.npz"))
    n = "negative_offset"
    pos = seqscore.song_pos_from_key(z[n + "_key"])
    best, ss = native.seq_score(z[n + "_db"], pos, z[n + "_q"], z[n + "_labels"], 1, 0.0)
    assert best == 1 and ss[1, 1] == -2.0
    assert abs(float(ss[1, 0]) - 0.6666666269) < 1e-7


def test_seqscore_c_alpha():
    z = np.load(os.path.join(G, "database.npz"))
    n = "random_noisy"
    pos = seqscore.song_pos_from_key(z[n + "_key"])
    db, q, lab = z[n + "_db"], z[n + "_q"], z[n + "_labels"]
    best, ss = native.seq_score(db, pos, q, lab, 1, 2.0)
    assert best == 17
    off = int(ss[17, 1])
    ips = np.array([db[pos[17] + off + i] @ q[i] for i in range(19)], np.float32)
    assert abs(ss[17, 0] - np.exp(-2.0 * (1 - ips) ** 2).mean()) < 1e-5


def test_melspec_restatement_self_consistency():
    """a2 is parity-unpinned (torchaudio absent); check the fp32 torch.stft restatement
    against the independent float64 gather+rfft form and the documented bank shape."""
    params = json.load(open(os.path.join(os.path.dirname(G), "..", "configs", "default.json")))
    fb = melspec.mel_filterbank(8000, 1024, 256, 300, 4000).numpy()
    nz = fb > 0
    assert nz.sum() == 942 and nz.sum(0).max() == 7 and nz.sum(0).min() >= 1
    rows = np.nonzero(nz.sum(1))[0]
    assert rows[0] == 39 and rows[-1] == 511
    pcm = synth.make_song(3, seconds=3.0)
    segs = segmenter.segment(segmenter.pcm_to_mono(pcm[:, None]), 8000, 4000)
    m32 = melspec.melspec(segs, params)
    m64 = melspec.melspec_f64(segs, params)
    assert m32.shape == (5, 256, 32)
    assert np.abs(m32 - m64).max() < 5e-3
    assert np.abs(m32 - m64).mean() < 1e-4


def test_melspec_oracle_vs_independent_third_party():
    """a2 cannot be pinned against torchaudio (absent, version unpinned).  Second opinion from an
    unrelated implementation of the same documented semantics that IS installed here:
    transformers.audio_utils (numpy, fp64): HTK mel bank without normalisation, periodic-hann STFT
    with centre reflect padding, power 2, then ln(x + 1e-8).  The bank differs by the fp32-vs-fp64
    construction only (<= 3.9e-5); the log-mel agrees to 1e-4 in the audible bins."""
    au = pytest.importorskip("transformers.audio_utils")
    from oracle import melspec as om
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = json.load(open(os.path.join(repo, "configs", "default.json")))
    fb = np.asarray(om.mel_filterbank(p["sample_rate"], p["stft_n"], p["n_mels"], p["f_min"], p["f_max"]))
    fb2 = au.mel_filter_bank(num_frequency_bins=p["stft_n"] // 2 + 1, num_mel_filters=p["n_mels"],
                             min_frequency=p["f_min"], max_frequency=p["f_max"], sampling_rate=p["sample_rate"],
                             norm=None, mel_scale="htk")
    assert fb.shape == fb2.shape and np.abs(fb - fb2).max() < 5e-5
    w = au.window_function(p["stft_n"], "hann", periodic=True)
    for seed in (1, 2):
        x = synth.normal(seed, "t/au", 8000).astype(np.float32)
        x[2000:6000] += np.sin(np.arange(4000) * 2 * np.pi * (700 + 300 * seed) / 8000).astype(np.float32) * 3
        x -= x.mean()
        ref = om.melspec(x[None], p)[0]
        xn = (x / max(np.linalg.norm(x), 1e-12)).astype(np.float64)
        sp = au.spectrogram(xn, w, frame_length=p["stft_n"], hop_length=p["stft_hop"], fft_length=p["stft_n"],
                            power=2.0, center=True, pad_mode="reflect", onesided=True, mel_filters=fb2,
                            mel_floor=0.0, log_mel=None)
        lm = np.log(sp + 1e-8)
        assert ref.shape == lm.shape
        loud = ref > ref.max() - 5.0
        assert np.abs(ref - lm)[loud].max() < 3e-4, np.abs(ref - lm)[loud].max()
        assert np.abs(ref - lm).max() < 3e-3


# ------------------------------------------------------------------ a1 at other sample rates (parity unpinned: julius absent)
def test_resampler_restatement_properties():
    """No reference vector exists for julius.ResampleFrac (absent, unpinned): check what the published algorithm
    guarantees -- unit-sum phases (constants preserved), the documented output length, a 1 kHz tone surviving 44.1 -> 8 kHz
    to 1e-5 away from the edges, everything above the new Nyquist removed -- and the reference's minute-wise assembly."""
    from oracle import resample as R
    k, width = R.kernels(44100, 8000)
    assert k.shape == (80, 2 * 140 + 441) and width == 140
    assert float((k.sum(1) - 1).abs().max()) < 1e-6
    assert R.resample_frac(np.full((2, 44100), 0.25, np.float32), 44100, 8000).shape == (2, 8000)
    assert np.abs(R.resample_frac(np.full((1, 50000), 0.25, np.float32), 44100, 8000) - 0.25).max() < 1e-6
    assert R.resample_frac(np.zeros((1, 12345), np.float32), 44100, 8000).shape[1] == int(80 * 12345 / 441)
    x = np.zeros((1, 777), np.float32)
    assert R.resample_frac(x, 8000, 8000) is not None and R.resample_frac(x, 16000, 16000).shape == (1, 777)
    t = np.arange(44100 * 125) / 44100.0
    tone = np.sin(2 * np.pi * 1000 * t).astype(np.float32)[None]
    y = R.resample_chunked(tone, 44100, 8000)
    assert y.shape == (1, 125 * 8000)                                  # two full pieces + tail: seams at 59.5 s and 118.5 s
    ref = np.sin(2 * np.pi * 1000 * np.arange(y.shape[1]) / 8000.0)
    assert np.abs(y[0] - ref)[4000:-4000].max() < 1e-5                 # incl. both seams
    hiss = np.sin(2 * np.pi * 6000 * t[:44100 * 3]).astype(np.float32)[None]     # above the 4 kHz Nyquist
    assert np.abs(R.resample_frac(hiss, 44100, 8000))[0, 400:-400].max() < 2e-3
    # piece plan: 59 s stride, half-second strips, lengths add up
    plan = R.chunk_plan(44100 * 125, 44100, 8000)
    assert plan[0] == (0, 2646000, 0, 476000) and plan[1] == (2601900, 2646000, 4000, 472000)
    assert sum(p[3] for p in plan) == 125 * 8000
    assert R.chunk_plan(1000, 16000, 8000) == [(0, 1000, 0, 500)]


# ---- the canonical fp32 score of the exact search (oracle/exactdot_c.c) ------------------------------------------

from fractions import Fraction


def _round_f32(v):
    """Fraction -> the float32 nearest to it, ties to even, decided exactly against both float32 neighbours (no
    double rounding through float64).  An exact zero is +0: every sum here starts from +0 in round-to-nearest."""
    a = np.float32(float(v))
    if Fraction(float(a)) == v:
        return a
    if Fraction(float(a)) > v:
        lo, hi = np.nextafter(a, np.float32(-np.inf)), a
    else:
        lo, hi = a, np.nextafter(a, np.float32(np.inf))
    dlo, dhi = v - Fraction(float(lo)), Fraction(float(hi)) - v
    if dlo != dhi:
        return lo if dlo < dhi else hi
    return lo if int(lo.view(np.uint32)) & 1 == 0 else hi


def _canon_rational(q, x):
    """The canonical score with every fmaf and add done exactly in rationals and rounded once, as IEEE 754 says."""
    d = q.shape[0]
    p = []
    for l in range(4):
        acc = np.float32(0.0)
        for e in range(4 * l, d, 16):
            for t in range(4):
                acc = _round_f32(Fraction(float(x[e + t])) * Fraction(float(q[e + t])) + Fraction(float(acc)))
        p.append(acc)
    a = _round_f32(Fraction(float(p[0])) + Fraction(float(p[1])))
    b = _round_f32(Fraction(float(p[2])) + Fraction(float(p[3])))
    return _round_f32(Fraction(float(a)) + Fraction(float(b)))


def _canon_pairs(rng, d, kind, n):
    """n (q, x) pairs of one kind: unit rows; heavy cancellation; fp16-subnormal-sized components; norms ~1e3."""
    q = rng.standard_normal((n, d))
    x = rng.standard_normal((n, d))
    if kind == "unit":
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        x /= np.linalg.norm(x, axis=1, keepdims=True)
    elif kind == "cancel":
        # x nearly orthogonal to q, with large terms of both signs: partial sums far above the result
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        x -= (x * q).sum(1, keepdims=True) * q
        x *= 1e3
        x += 1e-4 * rng.standard_normal((n, d))
    elif kind == "tiny":
        # components of the size of fp16 subnormals (6e-8 .. 6e-5), mixed with a few normal ones
        q = q * 2e-6
        x = x * 3e-5
        x[:, ::7] *= 1e4
    elif kind == "big":
        q = 1e3 * q / np.linalg.norm(q, axis=1, keepdims=True)
        x = 1e3 * x / np.linalg.norm(x, axis=1, keepdims=True)
    return q.astype(np.float32), x.astype(np.float32)


@pytest.mark.parametrize("d", [16, 24, 64, 96, 128, 256])
def test_canonical_score_c_matches_rational_statement(d):
    """oracle_canon_scores (C, libm fmaf, -ffp-contract=off) equals, bit for bit, the canonical order evaluated with
    exact rational arithmetic and one correct rounding per operation."""
    rng = np.random.default_rng(1000 + d)
    npair = {16: 200, 24: 200, 64: 120, 96: 100, 128: 80, 256: 40}[d]
    for kind in ("unit", "cancel", "tiny", "big"):
        q, x = _canon_pairs(rng, d, kind, npair)
        idx = np.arange(npair)
        got = native.canon_scores(q, x, idx, idx)
        want = np.array([_canon_rational(q[i], x[i]) for i in range(npair)], np.float32)
        bad = np.flatnonzero(got.view(np.int32) != want.view(np.int32))
        assert bad.size == 0, "d=%d %s: %d of %d pairs differ, first %r vs %r" % (
            d, kind, bad.size, npair, got[bad[0]], want[bad[0]])
        # and the order is not a plain left-to-right sum: the statement is specific (a check on the check)
        if kind == "unit" and d >= 64:
            seq = np.array([np.float32(sum_seq(q[i], x[i])) for i in range(npair)], np.float32)
            assert (seq.view(np.int32) != got.view(np.int32)).any()


def sum_seq(q, x):
    acc = np.float32(0.0)
    for a, b in zip(q, x):
        acc = np.float32(acc + np.float32(a * b))
    return acc


def test_canonical_score_pair_indexing():
    """canon_scores scores the pairs it is given: any (query row, db row) pairing, repeats included."""
    rng = np.random.default_rng(7)
    q = rng.standard_normal((5, 32)).astype(np.float32)
    x = rng.standard_normal((9, 32)).astype(np.float32)
    qi = rng.integers(0, 5, 200)
    xi = rng.integers(0, 9, 200)
    got = native.canon_scores(q, x, qi, xi)
    want = np.array([_canon_rational(q[a], x[b]) for a, b in zip(qi, xi)], np.float32)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert native.canon_scores(q, x, [], []).shape == (0,)


def _tie_db(rng, n, d, scale=1.0):
    """Rows with planted exact ties (copies of rows) and near-ties (copies moved by one ulp in one component)."""
    x = rng.standard_normal((n, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x *= np.float32(scale)
    src = rng.integers(0, n, n // 3)
    dst = rng.permutation(n)[: n // 3]
    x[dst] = x[src]                                              # exact ties
    near = rng.permutation(n)[: n // 4]
    for r in near:
        j = rng.integers(0, d)
        x[r, j] = np.nextafter(x[r, j], np.float32(np.inf) if rng.random() < 0.5 else np.float32(-np.inf))
    return x


@pytest.mark.parametrize("d,n,k,scale", [(16, 300, 10, 1.0), (64, 500, 50, 1.0), (96, 400, 7, 1e3), (128, 257, 300, 1.0),
                                         (128, 600, 1, 3e-2), (24, 100, 100, 1.0)])
def test_canonical_topk_window_matches_brute_force(d, n, k, scale):
    """flat_ip_topk_canonical's proven window gives what scoring every row gives, on data with planted exact ties
    (row copies: ties go to the lower row) and near-ties (one ulp apart), queries taken from the rows themselves (the
    k-th place sits inside a tie group), and k >= n (padding)."""
    rng = np.random.default_rng(d * 1000 + n + k)
    x = _tie_db(rng, n, d, scale)
    q = np.concatenate([x[rng.integers(0, n, 12)] / np.float32(scale), rng.standard_normal((6, d)).astype(np.float32)])
    D, I = search.flat_ip_topk_canonical(q, x, k)
    Db, Ib = search.flat_ip_topk_canonical(q, x, k, brute=True)
    assert np.array_equal(I, Ib)
    assert np.array_equal(D.view(np.int32), Db.view(np.int32))
    kk = min(k, n)
    assert (I[:, kk:] == -1).all() and (D[:, kk:] == -np.finfo(np.float32).max).all()
    # every returned score is the canonical score of its label, scores descend, ties go to the lower row
    mi = np.repeat(np.arange(q.shape[0]), kk)
    assert np.array_equal(D[:, :kk].ravel().view(np.int32), native.canon_scores(q, x, mi, I[:, :kk].ravel()).view(np.int32))
    assert (np.diff(D[:, :kk], axis=1) <= 0).all()
    tie = np.diff(D[:, :kk], axis=1) == 0
    assert (np.diff(I[:, :kk], axis=1)[tie] > 0).all()
    # copies really tie inside the returned lists (the case that needs the row rule)
    if 1 < kk < n:
        assert tie.any()
    # against the float64 top-k: the same rows up to the window's width
    D64, _ = search.flat_ip_topk(q, x, k)
    assert np.abs(D[:, :kk] - D64[:, :kk]).max() <= 2 * search.canon_window(q, x).max()


def test_flat_ip_topk_f16_selects_what_the_stable_sort_keeps():
    """Above 2^24 scores flat_ip_topk_f16 selects instead of sorting every row: the same lists as the stable argsort of the
    definition, on exact ties across the k-th place (300 copies of one row, a query that is that row; an all-zero query:
    every row ties) and ordinary rows."""
    rng = np.random.default_rng(1)
    db = rng.standard_normal((60000, 64)).astype(np.float32)
    db[100:400] = db[100]
    q = rng.standard_normal((300, 64)).astype(np.float32)
    q[1], q[2] = 0.0, db[100]
    assert q.shape[0] * db.shape[0] > (1 << 24)
    D, I = search.flat_ip_topk_f16(q, db, 100)
    s = q.astype(np.float16).astype(np.float64) @ db.astype(np.float16).astype(np.float64).T
    order = np.argsort(-s, axis=1, kind="stable")[:, :100]
    assert np.array_equal(I, order) and np.array_equal(D, np.take_along_axis(s, order, axis=1))
    assert np.array_equal(I[1], np.arange(100)) and np.array_equal(I[2], np.arange(100, 200))


# ------------------------------------------------------------------ a2: the float64 statement of every mode (tests/mel_cases.py)
def _melspec_f64_before_generalisation(x, params, bank=None):
    """oracle.melspec.melspec_f64 as it stood while it stated the default mode only, kept here operation for operation:
    the generalised function must return the same bits in that mode (every earlier caller's numbers depend on them)."""
    import torch
    x = np.asarray(x, dtype=np.float64)
    n_fft, hop = params["stft_n"], params["stft_hop"]
    x = x / np.maximum(np.linalg.norm(x, axis=-1, keepdims=True), 1e-12)
    L = x.shape[-1]
    n_frames = 1 + L // hop
    n = np.arange(n_fft)
    win = 0.5 - 0.5 * np.cos(2 * np.pi * n / n_fft)
    idx = np.arange(n_frames)[:, None] * hop - n_fft // 2 + n[None, :]
    idx = np.where(idx < 0, -idx, idx)
    idx = np.where(idx > L - 1, 2 * (L - 1) - idx, idx)
    frames = x[..., idx] * win
    power = np.abs(np.fft.rfft(frames, axis=-1)) ** 2
    fb = (melspec.mel_filterbank(params["sample_rate"], n_fft, params["n_mels"], params["f_min"], params["f_max"], False)
          if bank is None else torch.as_tensor(np.asarray(bank, np.float32))).double().numpy()
    mel = np.einsum("...tk,km->...mt", power, fb)
    return np.log(mel + 1e-8)


@pytest.mark.parametrize("name", ["default_parts", "sr16k", "t24", "fft256"])
def test_melspec_f64_default_mode_keeps_its_bits(name):
    import mel_cases as mc
    p = mc.params_for(name)
    x, _ = mc.rows(name, min(mc.CASES[name][2]), 0)
    for bank in (None, mc.bank_for(p)):
        want = _melspec_f64_before_generalisation(x, p, bank)
        got = melspec.melspec_f64(x, p, bank)
        assert got.dtype == want.dtype and np.array_equal(got, want)
        assert np.array_equal(melspec.melspec_f64_torch(x, p, bank).numpy(),
                              melspec.melspec_f64_torch(x, p, bank, remove_mean=False).numpy())
    # remove_mean is x - x.mean() in float64 before the normalisation
    xd = x[:3].astype(np.float64) + 0.05
    assert np.array_equal(melspec.melspec_f64(xd, p, remove_mean=True),
                          melspec.melspec_f64(xd - xd.mean(axis=-1, keepdims=True), p))


@pytest.mark.parametrize("name,B,remove_mean", __import__("mel_cases").RUNS)
def test_melspec_f64_states_every_mode_and_case(name, B, remove_mean):
    """The float64 statement (gather + numpy rfft) against the fp32 torch.stft statement, two independent writings of the
    same transform, on every case, signal and mode of the table, under the bars the kernel is held to; the float64 torch
    form agrees with the numpy one to float64 rounding; the loud-bin mask leaves out at most 0.1 % of a noise window's
    bins, so that the GPU test cannot hide behind it; the impulse windows' set of live frames is the same in both
    statements and no value sits within 1e-7 of the 1e-6 threshold that defines it."""
    import mel_cases as mc
    p = mc.params_for(name)
    x, kinds = mc.rows(name, B, remove_mean)
    ref64, ref32 = mc.references(name, B, remove_mean)
    assert ref64.shape == ref32.shape == (x.shape[0], p["n_mels"], 1 + x.shape[1] // p["stft_hop"])
    assert np.isfinite(ref64).all() and np.isfinite(ref32).all()
    m = mc.compare(ref32, name, B, remove_mean)
    print(name, B, remove_mean, m)
    assert m["lin_err"] < 2e-6
    assert m["log_err_loud"] < 2e-3
    assert m["noise_loud_share"] >= 0.999
    t64 = melspec.melspec_f64_torch(x[:4], p, mc.bank_for(p), remove_mean=bool(remove_mean)).numpy()
    assert np.abs(mc.to_linear(t64, p) - mc.to_linear(ref64[:4], p)).max() < 1e-11 * mc.to_linear(ref64[:4], p).max()
    imp = np.array([k == "impulse" for k in kinds])
    if imp.any():
        a64, a32 = mc.active_frames(ref64[imp], p), mc.active_frames(ref32[imp], p)
        assert np.array_equal(a64, a32)
        assert a64.any(axis=1).all() and not a64.all(axis=1).any()           # some frames live, some silent, per impulse
        d = np.abs(ref64[imp] - (mc.floor_level(ref64[imp], p)[:, None, None] + 1e-6))
        assert d.min() > 1e-7
    zero = np.array([k == "zero" for k in kinds])
    assert not mc.active_frames(ref64[zero], p).any()
