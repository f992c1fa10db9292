"""Monitor mode on the GPU: pfann_match_windows (csrc/monitor.hip) and what sits on top of it.

On the exact grid of tests/match_exact.py every field of every window is asserted with `==` against match_exact.exact_match
of the window's slice -- fast path, general path (PFANN_WINDOWS_GENERAL=1 in a subprocess; frame_shift_mul 2 and mode 1 in
this process) and the existing matcher on the expanded window list.  Real-valued rows: byte-identical results for the same
window reached by other hops and batches (the summation-order contract), and parity with the float64 oracle within the
project's 1e-6 per score (2e-6 between two such scores).  The one other tolerance is the module's 2e-6 under score_alpha > 0
(tests/test_gpu_match_exact.py).  End to end: builder.py, then monitor.py on a 3-minute recording of four excerpts."""
import csv
import ctypes
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import match_exact as mx
import monitor_cases as mc

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 128


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


_INDEX = {}


def _index(key, db, pos, storage="f32"):
    from pfann_amd.database import DeviceIndex
    if (key, storage) not in _INDEX:
        idx = DeviceIndex(db.shape[1], 0, storage)
        idx.load(db, pos)
        _INDEX[(key, storage)] = idx
    return _INDEX[(key, storage)]


def _tags_of(fn):
    """-> (fn(), the profiling tags of the kernels it launched)"""
    from pfann_amd import lib as L
    lib = L.load()
    lib.pfann_prof_enable(1)
    lib.pfann_prof_reset()
    try:
        out = fn()
        buf = ctypes.create_string_buffer(4096)
        lib.pfann_prof_tags(buf, 4096)
    finally:
        lib.pfann_prof_enable(0)
    return out, buf.value.decode().split(",")


def _windows(torch, idx, q, labels, rstart, rlen, window, hop, **kw):
    return idx.match_windows(torch.as_tensor(q).cuda(), torch.as_tensor(labels).cuda(), rstart, rlen, window, hop, **kw)


# ------------------------------------------------------------------------------------------------ exact arithmetic, fast path
@pytest.mark.parametrize("k", [20, 100])
def test_every_window_equals_the_exact_oracle(torch_cuda, k):
    """windows 1 / 5 / 19 / 64 x hops 1 / 2 / 7, fp32 and fp16 storage: every field of every window == exact_match of its
    slice, fp16 storage returns fp32 storage's bytes, and the call ran the windowed kernel (not the expansion)."""
    assert "PFANN_WINDOWS_GENERAL" not in os.environ
    db, pos, q, labels, rstart, rlen = mc.grid_recordings(D, k)
    rows = mx.IntRows(db)
    n = 0
    for window in mc.WINDOWS:
        mx.assert_exact_domain(window, D)
        for hop in mc.HOPS:
            want = mc.exact_windows(("grid", k), q, labels, rstart, rlen, rows, pos, window, hop)
            first = None
            for storage in ("f32", "f16"):
                (res, wfirst), tags = _tags_of(lambda: _windows(torch_cuda, _index(("grid", k), db, pos, storage), q, labels,
                                                                 rstart, rlen, window, hop))
                assert tags == ["seq_match_windows"], "window %d hop %d k %d took %r" % (window, hop, k, tags)
                assert np.array_equal(wfirst, mc.wfirst_of(rlen, window, hop)) and res.shape[0] == len(want)
                bad = mc.differing(res, want)
                assert not bad, "window %d hop %d k %d %s: %d of %d windows differ\n%s" % (window, hop, k, storage, len(bad),
                                                                                         len(want), "\n".join(bad[:6]))
                first = first or res.tobytes()
                assert res.tobytes() == first, "fp16-only storage and fp32 storage return different bytes"
            n += len(want)
    ties = sum(1 for w in mc.exact_windows(("grid", k), q, labels, rstart, rlen, rows, pos, 19, 1)
               if len(w["top"]) > 1 and w["top"][0][3] == w["top"][1][3])
    none = sum(1 for w in mc.exact_windows(("grid", k), q, labels, rstart, rlen, rows, pos, 5, 1) if w["song"] < 0)
    print("k=%d: %d windows exact; window 19: %d with an exact tie at the top; window 5: %d without a candidate" % (k, n, ties, none))
    assert ties > 0 and none > 0, "the recordings no longer hold ties / all -1 windows"


def test_small_d_and_wide_rows(torch_cuda):
    """d = 64 (16 float4 chunks: half of each half wave idles) and d = 256 (a whole wave per row)"""
    for d, windows in ((64, (19, 64)), (256, (5, 19))):
        db, pos, q, labels, rstart, rlen = mc.grid_recordings(d, 20, seed=340)
        rows = mx.IntRows(db)
        for window in windows:
            mx.assert_exact_domain(window, d)
            for hop in (1, 3):
                res, _ = _windows(torch_cuda, _index(("grid-d", d), db, pos), q, labels, rstart, rlen, window, hop)
                bad = mc.differing(res, mc.exact_windows(("grid-d", d), q, labels, rstart, rlen, rows, pos, window, hop))
                assert not bad, "d %d window %d hop %d: %d windows differ\n%s" % (d, window, hop, len(bad), "\n".join(bad[:6]))


# ------------------------------------------------------------------------------------------------ against the existing matcher
def test_equals_the_matcher_on_the_expanded_windows(torch_cuda):
    """DeviceIndex.match on the overlapping (qstart, qlen) list: all fields equal on the exact grid"""
    k = 20
    db, pos, q, labels, rstart, rlen = mc.grid_recordings(D, k)
    idx = _index(("grid", k), db, pos)
    for window, hop in ((19, 1), (19, 2), (5, 7), (64, 2), (1, 1)):
        res, _ = _windows(torch_cuda, idx, q, labels, rstart, rlen, window, hop)
        qs, ql = mc.expand(rstart, rlen, window, hop)
        ref, _ = idx.match(torch_cuda.as_tensor(q).cuda(), torch_cuda.as_tensor(labels).cuda(), qs, ql)
        for f in ("song", "offset", "shift", "n_cand", "score"):
            assert np.array_equal(res[f], ref[f]), "window %d hop %d: field %s differs in %d windows" % (
                window, hop, f, int((res[f] != ref[f]).sum()))


# ------------------------------------------------------------------------------------------------ general path
def test_general_path_in_a_subprocess():
    """PFANN_WINDOWS_GENERAL=1: the same windows x hops x storages through the expansion, == the exact oracle"""
    env = dict(os.environ, PYTHONPATH=REPO, PFANN_WINDOWS_GENERAL="1")
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(REPO, "tests", "monitor_cases.py"), "exact-general"],
                       capture_output=True, text=True, env=env, cwd=REPO, timeout=300)
    assert r.returncode == 0 and "exact-general ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.parametrize("fsm,mode", [(2, 0), (1, 1), (2, 1)])
def test_general_path_frame_shift_and_native_mode(torch_cuda, fsm, mode):
    """frame_shift_mul 2 and mode 1 go through the expansion by themselves; long lists (window 128 x k 100 > 8192) too"""
    k = 20
    db, pos, q, labels, rstart, rlen = mc.grid_recordings(D, k, fsm=fsm, seed=320)
    rows = mx.IntRows(db)
    idx = _index(("grid", k), db, pos)
    for window, hop in ((19, 1), (5, 2), (64, 7)):
        (res, _), tags = _tags_of(lambda: _windows(torch_cuda, idx, q, labels, rstart, rlen, window, hop, fsm=fsm, mode=mode))
        assert "seq_match_windows" not in tags and "seq_match" in tags, tags
        bad = mc.differing(res, mc.exact_windows(("grid-fsm", fsm), q, labels, rstart, rlen, rows, pos, window, hop, fsm, mode))
        assert not bad, "fsm %d mode %d window %d hop %d: %d windows differ\n%s" % (fsm, mode, window, hop, len(bad), "\n".join(bad[:6]))


def test_lists_too_long_for_the_lds_take_the_general_path(torch_cuda):
    k = 100
    db, pos, q, labels, rstart, rlen = mc.grid_recordings(D, k)
    rows = mx.IntRows(db)
    window, hop = 128, 5                                  # 100 * (128 + 4) > 8192
    mx.assert_exact_domain(window, D)
    (res, _), tags = _tags_of(lambda: _windows(torch_cuda, _index(("grid", k), db, pos), q, labels, rstart, rlen, window, hop))
    assert "seq_match_windows" not in tags and "seq_match" in tags, tags
    bad = mc.differing(res, mc.exact_windows(("grid", k), q, labels, rstart, rlen, rows, pos, window, hop))
    assert not bad, "%d windows differ\n%s" % (len(bad), "\n".join(bad[:6]))


def test_score_alpha_windows(torch_cuda):
    """mode 1, score_alpha 3 on unit-norm grid rows (expf: the module's 2e-6): the reported score is within 2e-6 of the float64
    score of the reported candidate, and that is within 2e-6 of the float64 best over the window's candidates"""
    k, alpha, tol = 20, 3.0, 2e-6
    key = [int(x) for x in np.diff(mx.std_world(41, D)[1])]
    world = mx.make_world(81, "mon-alpha", key, D, mx.STD_COPIES, (), rows=mx.unit_grid_rows)
    db, pos, q, labels, rstart, rlen = mc.grid_recordings(D, k, rows=mx.unit_grid_rows, world=world, seed=360)
    window, hop = 19, 3
    res, _ = _windows(torch_cuda, _index("alpha", db, pos), q, labels, rstart, rlen, window, hop, alpha=alpha, mode=1)
    qs, ql = mc.expand(rstart, rlen, window, hop)
    worst = 0.0
    for j, (s, n) in enumerate(zip(qs, ql)):
        cands = mc.candidates(labels[s:s + n], pos)
        r = res[j]
        assert int(r["n_cand"]) == len(cands), j
        if not cands:
            assert int(r["song"]) == -1
            continue
        best = max(mc.score64(db, pos, q[s:s + n], c[0], c[1], alpha=alpha) for c in cands)
        mine = mc.score64(db, pos, q[s:s + n], int(r["song"]), int(r["offset"]), alpha=alpha)
        assert (int(r["song"]), int(r["offset"]), 0) in cands, j
        worst = max(worst, abs(float(r["score"]) - mine), best - mine)
        assert abs(float(r["score"]) - mine) <= tol and best - mine <= tol, (j, float(r["score"]), mine, best)
    print("score_alpha windows: %d windows, worst difference %.3g" % (len(qs), worst))


# ------------------------------------------------------------------------------------------------ summation-order contract
def test_a_window_has_the_same_bytes_whatever_reached_it(torch_cuda):
    """real-valued unit-norm rows: one recording at hop 1 and hop 3, alone and batched behind another recording, on fp32
    storage -- the windows common to those runs have byte-identical results"""
    k, window = 100, 19
    db, pos, q, labels = mc.unit_case(7, 120, D, k, 400)
    idx = _index("unit400", db, pos)
    L = q.shape[0]
    h1, _ = _windows(torch_cuda, idx, q, labels, [0], [L], window, 1)
    h3, _ = _windows(torch_cuda, idx, q, labels, [0], [L], window, 3)
    assert h1[::3].tobytes() == h3.tobytes(), "%d windows differ between hop 1 and hop 3" % int((h1[::3] != h3).sum())
    other = 137
    q2, l2 = np.concatenate([q[:other][::-1], q]), np.concatenate([labels[:other][::-1], labels])
    b1, wf = _windows(torch_cuda, idx, q2, l2, [0, other], [other, L], window, 1)
    assert b1[wf[1]:].tobytes() == h1.tobytes(), "batched behind another recording: other bytes"
    b3, wf = _windows(torch_cuda, idx, q2, l2, [0, other], [other, L], window, 3)
    assert b3[wf[1]:].tobytes() == h3.tobytes()
    h7, _ = _windows(torch_cuda, idx, q, labels, [0], [L], window, 7)      # other chunk seams again
    assert h1[::7].tobytes() == h7.tobytes()
    assert len({float(x) for x in h1["score"]}) > len(h1) // 2, "the scores are not real-valued"


# ------------------------------------------------------------------------------------------------ real-valued parity
def _parity(torch, name, db, pos, q, labels, rstart, rlen, window, hop, hop_size, want_equal=None):
    """every window against oracle/seqscore.py (float64 dots of float32 rows): the kernel's candidate, re-scored in float64,
    within 2e-6 of the oracle's best; the reported score within 1e-6 of the float64 score of that candidate"""
    from oracle import seqscore as osq
    res, _ = _windows(torch, _index(name, db, pos), q, labels, rstart, rlen, window, hop)
    qs, ql = mc.expand(rstart, rlen, window, hop)
    same = 0
    worst_pick = worst_score = 0.0
    for j, (s, n) in enumerate(zip(qs, ql)):
        best, (song, t), _ = osq.query_embeddings_base(q[s:s + n], labels[s:s + n], db, pos, hop_size)
        r = res[j]
        assert int(r["song"]) >= 0 and song >= 0, j
        mine = mc.score64(db, pos, q[s:s + n], int(r["song"]), int(r["offset"]))
        worst_pick = max(worst_pick, float(best) - mine)
        worst_score = max(worst_score, abs(float(r["score"]) - mine))
        assert float(best) - mine <= 2e-6, (j, float(best), mine)
        assert abs(float(r["score"]) - mine) <= 1e-6, (j, float(r["score"]), mine)
        same += int(r["song"]) == song and int(r["offset"]) * hop_size == t
    print("%s: %d windows, %d decisions identical, oracle best - kernel's pick <= %.3g, |score - float64| <= %.3g"
          % (name, len(qs), same, worst_pick, worst_score))
    if want_equal:
        assert same == len(qs), "%d of %d decisions differ from the oracle's" % (len(qs) - same, len(qs))


def test_real_valued_parity_on_the_reference_fixture(torch_cuda, repo_root):
    """the committed fixture of tests/test_monitor_host.py (windows answered by the reference's own code): decisions identical
    (its best-to-second margins exceed 4e-6, checked on the CPU), scores within 1e-6"""
    z = np.load(os.path.join(repo_root, "tests", "golden", "monitor_windows.npz"))
    pos = np.pad(np.cumsum(z["landmarkKey"]), (1, 0)).astype(np.int64)
    window, hop, hop_size = int(z["window"]), int(z["hop"]), float(z["hop_size"])
    _parity(torch_cuda, "fixture", z["db"], pos, z["rec"], z["labels"], z["rstart"], z["rlen"], window, hop, hop_size, want_equal=True)
    res, _ = _windows(torch_cuda, _index("fixture", z["db"], pos), z["rec"], z["labels"], z["rstart"], z["rlen"], window, hop)
    assert np.array_equal(res["song"], z["song"])
    assert np.array_equal(res["offset"] * hop_size, z["time"])


def test_real_valued_parity_on_a_larger_case(torch_cuda):
    db, pos, q, labels = mc.unit_case(11, 300, D, 100, 900)
    _parity(torch_cuda, "unit900", db, pos, q, labels, [0, 500], [500, 400], 19, 2, 0.5)


# ------------------------------------------------------------------------------------------------ errors
def test_a_shard_refuses_windows(torch_cuda):
    from pfann_amd import lib as L
    from pfann_amd.database import DeviceIndex
    db, pos = mx.std_world(41, D)
    lo, hi = 10, 30
    idx = DeviceIndex(D, 0)
    idx.load(db[pos[lo]:pos[hi]], pos, int(pos[lo]), song_range=(lo, hi))
    q = torch_cuda.as_tensor(db[:30]).cuda()
    labels = torch_cuda.zeros((30, 4), dtype=torch_cuda.int64).cuda()
    with pytest.raises(L.PfannError, match="shard"):
        idx.match_windows(q, labels, [0], [30], 5, 1)


# ------------------------------------------------------------------------------------------------ end to end
def test_monitor_cli_finds_four_excerpts(tmp_path):
    """~50 synthetic songs, a 3-minute recording of four excerpts at SNR 0 with noise between them: builder.py, monitor.py;
    exactly four detections, right songs, nothing in the gaps at the default --min-score; the per-window CSV equals
    Database.monitor_* called directly; edges and song offsets within one hop_size plus one window hop (1.5 s).

    The float64 oracle on this case (seeded weights with the calibrated head; window 19, hop 2): windows of noise alone score
    0.11 .. 0.182, windows inside an excerpt 0.211 .. 0.386, so the default --min-score is 0.2; two isolated windows that
    half overlap the first excerpt name a chance alignment at 0.215 / 0.216 and are dropped for want of a second agreeing
    window.  The four detections come out, with the right songs and nothing in the gaps.  The long windows' scores alone place the
    edges up to 2.6 s off (the noise rows next to an excerpt add between 0 and 0.14 per row on the song's diagonal, so a
    partly overlapping window does not score the overlap times the plateau); the short windows of --edge-window (7 segments
    at hop 1 here) that stay on the detection's diagonal place them, from the oracle's scores, at (11.0, 47.0, 4.0),
    (57.0, 88.0, 0.0), (100.5, 126.5, 11.5), (134.0, 153.5, 19.0) against the truth (12, 47, 5), (57, 87, 0), (101, 126, 12),
    (135, 155, 20): within the 1.5 s, the last end exactly on it."""
    import torch
    from pfann_amd import synth
    from pfann_amd.monitor import DEFAULT_HOP, default_window
    params = json.load(open(os.path.join(REPO, "configs", "default.json")))
    # the seeded weights with the calibrated head (synth.make_state_dict_calibrated): the raw ones embed every segment
    # within 0.02 of every other, and no window could tell a song from noise
    sd = synth.make_state_dict_calibrated(params, seed=123)
    mdir = tmp_path / "model"
    mdir.mkdir()
    torch.save({n: torch.from_numpy(v) for n, v in sd.items()}, str(mdir / "model.pt"))
    shutil.copy(os.path.join(REPO, "configs", "default.json"), str(mdir / "configs.json"))
    sr, n_songs = 8000, 50
    music, songs = [], []
    for s in range(n_songs):
        path = str(tmp_path / ("song%02d.wav" % s))
        songs.append(synth.make_song(500 + s, seconds=40.0 + (s % 7)))
        synth.write_wav(path, songs[-1])
        music.append(path)
    (tmp_path / "music.txt").write_text("".join(p + "\n" for p in music))
    # the recording: noise 12 s | song 7 from 5 s, 35 s | noise 10 s | song 23 from 0 s, 30 s | noise 14 s |
    #                song 41 from 12 s, 25 s | noise 9 s | song 7 again from 20 s, 20 s | noise 25 s        = 180 s
    plan = [(None, 0, 12), (7, 5, 35), (None, 0, 10), (23, 0, 30), (None, 0, 14), (41, 12, 25), (None, 0, 9), (7, 20, 20), (None, 0, 25)]
    parts, truth, t = [], [], 0.0
    for j, (s, o, n) in enumerate(plan):
        noise = synth.normal(77, "mon/e2e/%d" % j, n * sr).astype(np.float64)
        if s is None:
            x = noise * 2000.0
        else:
            sig = songs[s][o * sr:(o + n) * sr].astype(np.float64)
            x = sig + noise * np.sqrt(np.mean(sig ** 2))          # SNR 0 dB
            truth.append((t, t + n, s, float(o)))
        parts.append(x)
        t += n
    rec = np.concatenate(parts)
    rec = np.clip(rec / np.abs(rec).max() * 30000.0, -32768, 32767).astype(np.int16)
    synth.write_wav(str(tmp_path / "rec.wav"), rec)
    (tmp_path / "recs.txt").write_text(str(tmp_path / "rec.wav") + "\n" + str(tmp_path / "missing.wav") + "\n")

    db = str(tmp_path / "db")
    env = dict(os.environ, PYTHONPATH=REPO)
    for cmd in (["builder.py", str(tmp_path / "music.txt"), db, str(mdir)],
                ["monitor.py", str(tmp_path / "recs.txt"), db, str(tmp_path / "out.tsv")]):
        r = subprocess.run(["timeout", "-k", "10", "400", sys.executable, os.path.join(REPO, cmd[0])] + cmd[1:],
                           capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=460)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [x.split("\t") for x in open(str(tmp_path / "out.tsv")).read().splitlines()]
    assert lines[-1] == [str(tmp_path / "missing.wav"), "error"]
    det = lines[:-1]
    print("detections:\n" + "\n".join("  " + "  ".join(x[1:]) for x in det))
    window, hop_size = default_window(params), params["hop_size"]
    tol = hop_size + DEFAULT_HOP * hop_size
    assert len(det) == 4, "%d detections" % len(det)
    for x, (t0, t1, s, o) in zip(det, truth):
        assert x[0] == str(tmp_path / "rec.wav") and x[3] == music[s], (x, s)
        assert float(x[1]) < t1 and float(x[2]) > t0, ("a detection inside a noise gap", x)

    # ---- the per-window CSV is Database.monitor_* as it stands
    from pfann_amd.database import Database
    from pfann_amd.engine import Engine
    from pfann_amd.musicdata import MusicDataset
    from pfann_amd.builder import embed_files
    cfg = json.load(open(os.path.join(db, "configs.json")))
    engine = Engine(cfg, 0, max_batch=9728)
    engine.set_plan_batch(9728)
    engine.load_state_dict(torch.load(os.path.join(db, "model.pt"), map_location="cpu"))
    ds = MusicDataset([str(tmp_path / "rec.wav")], cfg)
    (_, n_seg, emb), = list(embed_files(engine, ds, ds.hop, batch_windows=9728))
    dbo = Database(db, cfg["indexer"], cfg["hop_size"], d=cfg["model"]["d"])
    rows, = dbo.monitor_finish(dbo.monitor_launch(emb, [0], [n_seg], window, DEFAULT_HOP))
    got = list(csv.reader(open(str(tmp_path / "out_windows.csv"))))
    assert got[0] == ["recording", "w0", "start_s", "song", "score", "time"] and got[-1][1] == "error"
    got = got[1:-1]
    assert len(got) == len(rows) == len(mc.window_starts(n_seg, window, DEFAULT_HOP))
    for g, (w0, score, song, time_s) in zip(got, rows):
        assert (int(g[1]), g[3], float(g[4]), float(g[5])) == (int(w0), music[int(song)], float(score), float(time_s)), (g, w0)
    for x, (t0, t1, s, o) in zip(det, truth):
        assert abs(float(x[1]) - t0) <= tol and abs(float(x[2]) - t1) <= tol and abs(float(x[4]) - o) <= tol, (x, t0, t1, o)
