"""Ranked monitor mode on the GPU: pfann_match_windows_topn (csrc/monitor.hip) and what sits on top of it.

On the exact grid of tests/match_exact.py every entry of every window's list, and n_found, is asserted with `==` against
match_topn_exact.exact_topn of the window's slice -- fast path, general path (PFANN_WINDOWS_GENERAL=1 in a subprocess;
frame_shift_mul 2 and mode 1 in this process against DeviceIndex.match_topn on the expanded windows).  Entry 0 is
match_windows' answer bytewise; lists are prefixes of longer lists and do not depend on hop or batch.  Real-valued rows:
scores within the project's 1e-6 of float64, the ranking equal to float64's wherever its neighbours are 2e-6 apart.  Two songs
at once come out as two overlapping detections.  monitor.py --top 1 writes the files of a run without the flag."""
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
import monitor_topn_cases as tc

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 128


def _four(res):
    """the bytes of (song, offset, shift, score), field by field: everything but n_cand"""
    return b"".join(np.ascontiguousarray(res[f]).tobytes() for f in ("song", "offset", "shift", "score"))


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


def _topn(torch, idx, q, labels, rstart, rlen, window, hop, n, **kw):
    (top, n_found), wfirst = idx.match_windows_topn(torch.as_tensor(q).cuda(), torch.as_tensor(labels).cuda(), rstart, rlen,
                                                    window, hop, n, **kw)
    return top, n_found, wfirst


def _windows(torch, idx, q, labels, rstart, rlen, window, hop, **kw):
    return idx.match_windows(torch.as_tensor(q).cuda(), torch.as_tensor(labels).cuda(), rstart, rlen, window, hop, **kw)


def _is_general(tags):
    return "seq_match_windows_topn" not in tags and "seq_match_windows" not in tags and any(t.startswith("seq_match") for t in tags)


# ------------------------------------------------------------------------------------------------ exact arithmetic
@pytest.mark.parametrize("k", [20, 100])
def test_every_list_equals_the_exact_oracle(torch_cuda, k):
    """windows 1 / 5 / 19 / 64 x hops 1 / 2 / 7 x n 1 / 3 / N_FAST, fp32 and fp16 storage: every entry of every window ==
    exact_topn of its slice in (song, offset, shift, n_cand, score), n_found too; fp16 storage returns fp32 storage's bytes;
    the call ran the ranked windowed kernel wherever a chunk fits (k * (window + hop - 1) <= 8192, the header's rule: every
    pair here) and the expansion where none does (window 128, hop 5 at k = 100)."""
    assert "PFANN_WINDOWS_GENERAL" not in os.environ
    db, pos, q, labels, rstart, rlen = mc.grid_recordings(D, k)
    rows = mx.IntRows(db)
    pairs = [(w, h) for w in mc.WINDOWS for h in mc.HOPS] + ([(128, 5)] if k == 100 else [])
    total = 0
    for window, hop in pairs:
        mx.assert_exact_domain(window, D)
        fits = k * (window + hop - 1) <= 8192
        for n in (1, 3, tc.N_FAST):
            want = tc.exact_window_lists(("grid", k), q, labels, rstart, rlen, rows, pos, window, hop, n)
            first = None
            for storage in ("f32", "f16"):
                (top, n_found, wfirst), tags = _tags_of(lambda: _topn(torch_cuda, _index(("grid", k), db, pos, storage), q, labels,
                                                                      rstart, rlen, window, hop, n))
                if fits:
                    assert tags == ["seq_match_windows_topn"], "window %d hop %d k %d n %d took %r" % (window, hop, k, n, tags)
                else:
                    assert _is_general(tags), tags
                assert np.array_equal(wfirst, mc.wfirst_of(rlen, window, hop))
                bad = tc.differing(top, n_found, *want)
                assert not bad, "window %d hop %d k %d n %d %s: %d of %d windows differ\n%s" % (
                    window, hop, k, n, storage, len(bad), top.shape[0], "\n".join(bad[:6]))
                first = first or (top.tobytes(), n_found.tobytes())
                assert (top.tobytes(), n_found.tobytes()) == first, "fp16-only storage and fp32 storage return different bytes"
            total += top.shape[0]
    # what the recordings must keep exercising: both first-wins rules (tie_storm), padding and empty windows (edges)
    top, n_found = tc.exact_window_lists(("grid", k), q, labels, rstart, rlen, rows, pos, 19, 1, tc.N_FAST)
    song_ties = int(((top["score"][:, :-1] == top["score"][:, 1:]) & (top["song"][:, 1:] >= 0)).sum())
    inner_ties = 0
    for s, L in zip(rstart, rlen):
        for w0, m in mc.window_starts(int(L), 19, 7):
            cands = mc.candidates(labels[s + w0:s + w0 + m], pos)
            best = {}
            for song, off, _ in cands:
                best.setdefault(song, []).append(mc.score64(db, pos, q[s + w0:s + w0 + m], song, off))
            inner_ties += sum(1 for v in best.values() if v.count(max(v)) > 1)
    print("k=%d: %d lists exact; window 19: %d ties between ranked songs, %d songs whose best score two alignments share "
          "(hop 7), %d windows without a candidate, %d padding entries" % (k, total, song_ties, inner_ties, int((n_found == 0).sum()),
                                                                        int((top["song"] < 0).sum())))
    short, _ = tc.exact_window_lists(("grid", k), q, labels, rstart, rlen, rows, pos, 1, 1, 3)
    assert song_ties > 0 and inner_ties > 0 and (n_found == 0).any()
    assert ((short["song"][:, 2] < 0) & (short["song"][:, 0] >= 0)).any(), "no list of n = 3 ends in padding behind a song"


def test_small_d_and_wide_rows(torch_cuda):
    """d = 16 (4 float4 chunks: two rows per wave, most of each half idle) and d = 320 (80 chunks: a lane takes two)"""
    for d, window, hop in ((16, 19, 3), (320, 5, 1)):
        db, pos, q, labels, rstart, rlen = mc.grid_recordings(d, 20, seed=340)
        rows = mx.IntRows(db)
        mx.assert_exact_domain(window, d)
        for n in (1, 8):
            (top, n_found, _), tags = _tags_of(lambda: _topn(torch_cuda, _index(("grid-d", d), db, pos), q, labels, rstart, rlen,
                                                             window, hop, n))
            assert tags == ["seq_match_windows_topn"], tags
            bad = tc.differing(top, n_found, *tc.exact_window_lists(("grid-d", d), q, labels, rstart, rlen, rows, pos, window, hop, n))
            assert not bad, "d %d window %d hop %d n %d: %d windows differ\n%s" % (d, window, hop, n, len(bad), "\n".join(bad[:6]))


# ------------------------------------------------------------------------------------------------ entry 0, prefixes, reach
def _unit40():
    return mc.unit_case(7, 40, D, 20, 400)


def test_entry_0_is_match_windows_bytewise(torch_cuda):
    """song, offset, shift and score of entry 0 are the bytes match_windows returns: on the grid recordings and on
    real-valued unit rows (40 songs, d 128, k 20, 400 recording rows), for short and long lists"""
    k = 20
    db, pos, q, labels, rstart, rlen = mc.grid_recordings(D, k)
    udb, upos, uq, ulabels = _unit40()
    cases = [(_index(("grid", k), db, pos), q, labels, rstart, rlen, [(19, 1), (5, 7), (64, 2), (1, 1)]),
             (_index("unit40", udb, upos), uq, ulabels, [0, 150], [150, 250], [(19, 1), (19, 2), (7, 3)])]
    for idx, cq, cl, rs, rl, pairs in cases:
        for window, hop in pairs:
            res, _ = _windows(torch_cuda, idx, cq, cl, rs, rl, window, hop)
            for n in (1, 8, 64):
                top, _, _ = _topn(torch_cuda, idx, cq, cl, rs, rl, window, hop, n)
                assert _four(top[:, 0]) == _four(res), (window, hop, n)
    assert len({float(x) for x in top["score"][:, 0]}) > top.shape[0] // 2, "the unit rows' scores are not real-valued"


def test_a_list_is_a_prefix_and_has_the_same_bytes_whatever_reached_it(torch_cuda):
    """real-valued rows: n = 3 is the head of n = 8; one recording at hops 1, 2 and 7, alone and batched behind another
    recording -- the windows common to those runs have byte-identical lists and n_found"""
    window = 19
    db, pos, q, labels = _unit40()
    idx = _index("unit40", db, pos)
    L = q.shape[0]
    t8, f8, _ = _topn(torch_cuda, idx, q, labels, [0], [L], window, 1, 8)
    t3, f3, _ = _topn(torch_cuda, idx, q, labels, [0], [L], window, 1, 3)
    assert np.ascontiguousarray(t8[:, :3]).tobytes() == t3.tobytes() and f8.tobytes() == f3.tobytes()
    assert (f8 > 8).any(), "no window here has more songs than the list is long"
    other = 137
    q2, l2 = np.concatenate([q[:other][::-1], q]), np.concatenate([labels[:other][::-1], labels])
    for hop in (1, 2, 7):
        th, fh, _ = _topn(torch_cuda, idx, q, labels, [0], [L], window, hop, 8)
        assert np.ascontiguousarray(t8[::hop]).tobytes() == th.tobytes() and f8[::hop].tobytes() == fh.tobytes(), hop
        tb, fb, wf = _topn(torch_cuda, idx, q2, l2, [0, other], [other, L], window, hop, 8)
        assert tb[wf[1]:].tobytes() == th.tobytes() and fb[wf[1]:].tobytes() == fh.tobytes(), hop


# ------------------------------------------------------------------------------------------------ general path
def test_general_path_in_a_subprocess():
    """PFANN_WINDOWS_GENERAL=1: one window / hop pair per k through the expansion, == the exact oracle"""
    env = dict(os.environ, PYTHONPATH=REPO, PFANN_WINDOWS_GENERAL="1")
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(REPO, "tests", "monitor_topn_cases.py"), "exact-general"],
                       capture_output=True, text=True, env=env, cwd=REPO, timeout=300)
    assert r.returncode == 0 and "exact-general ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.parametrize("fsm,mode", [(2, 0), (1, 1)])
def test_general_path_frame_shift_and_native_mode(torch_cuda, fsm, mode):
    """frame_shift_mul 2 and mode 1 go through the expansion by themselves: n = 64, the bytes of match_topn on the expanded
    windows"""
    k = 20
    db, pos, q, labels, rstart, rlen = mc.grid_recordings(D, k, fsm=fsm, seed=320)
    idx = _index(("grid", k), db, pos)
    for window, hop in ((19, 1), (64, 7)):
        (top, n_found, _), tags = _tags_of(lambda: _topn(torch_cuda, idx, q, labels, rstart, rlen, window, hop, 64, fsm=fsm, mode=mode))
        assert _is_general(tags), tags
        qs, ql = mc.expand(rstart, rlen, window, hop)
        ref, ref_found = idx.match_topn(torch_cuda.as_tensor(q).cuda(), torch_cuda.as_tensor(labels).cuda(), qs, ql, 64, fsm=fsm, mode=mode)
        assert top.tobytes() == ref.tobytes() and n_found.tobytes() == ref_found.tobytes(), (window, hop)
        assert (top["song"][:, 1] >= 0).any()


# ------------------------------------------------------------------------------------------------ real-valued parity
def test_real_valued_parity_with_the_float64_ranking(torch_cuda):
    """unit rows: every entry's score within 1e-6 of score64 of its own (song, offset); the ranked songs are float64's
    wherever float64 separates an entry from both its neighbours in the ranking by more than 2e-6 (two fp32 scorers within
    1e-6 each cannot swap those).  The entries skipped for want of that margin are counted: under 1 % (seed 7 on the CPU,
    float64 oracle alone: 4 of 1528 entries)."""
    window, hop, n = 19, 2, 8
    db, pos, q, labels = _unit40()
    top, n_found, _ = _topn(torch_cuda, _index("unit40", db, pos), q, labels, [0], [q.shape[0]], window, hop, n)
    starts = mc.window_starts(q.shape[0], window, hop)
    assert top.shape == (len(starts), n)
    skipped = entries = 0
    worst = 0.0
    for j, (w0, wl) in enumerate(starts):
        want = tc.ranking64(db, pos, q, labels, w0, wl)
        assert int(n_found[j]) == len(want), j
        for i in range(n):
            e = top[j, i]
            if i >= len(want):
                assert int(e["song"]) == -1 and e["score"] == -np.inf, (j, i)
                continue
            entries += 1
            mine = mc.score64(db, pos, q[w0:w0 + wl], int(e["song"]), int(e["offset"]))
            worst = max(worst, abs(float(e["score"]) - mine))
            assert abs(float(e["score"]) - mine) <= 1e-6, (j, i, float(e["score"]), mine)
            near = [want[x][0] for x in (i - 1, i + 1) if 0 <= x < len(want)]
            if any(abs(want[i][0] - s) <= 2e-6 for s in near):
                skipped += 1
                continue
            assert int(e["song"]) == want[i][1], (j, i, e, want[i])
    print("parity: %d entries, %d skipped for a float64 margin <= 2e-6, |score - float64| <= %.3g" % (entries, skipped, worst))
    assert entries > 1000 and skipped < 0.01 * entries, (skipped, entries)


# ------------------------------------------------------------------------------------------------ two songs at once
def _overlap_case():
    """30 songs of unit rows; one recording of 40 rows, each normalise(A[i] + B[j]): song 4 from its row 3 and song 17 from
    its row 11 at once.  Labels: the float64 top-20 of every row."""
    from pfann_amd import synth
    key = np.full(30, 60, np.int64)
    pos = np.pad(np.cumsum(key), (1, 0)).astype(np.int64)
    db = synth.unit_rows(91, "montop/db", int(pos[-1]), D).astype(np.float32)
    a, oa, b, ob, rows = 4, 3, 17, 11, 40
    q = db[pos[a] + oa:pos[a] + oa + rows].astype(np.float64) + db[pos[b] + ob:pos[b] + ob + rows].astype(np.float64)
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    sc = q.astype(np.float64) @ db.astype(np.float64).T
    labels = np.argsort(-sc, axis=1, kind="stable")[:, :20].astype(np.int64)
    return db, pos, key, q, labels, (a, oa), (b, ob)


def test_two_songs_at_once_rank_first_and_second_and_are_two_detections(torch_cuda, tmp_path):
    from pfann_amd.database import Database
    from pfann_amd.monitor import merge_window_tracks, merge_windows
    window, hop, hop_size = 19, 1, 0.5
    db, pos, key, q, labels, (a, oa), (b, ob) = _overlap_case()
    starts = mc.window_starts(q.shape[0], window, hop)
    # the premise, from the float64 oracle alone: both songs above 0.5 in every window, every other song below 0.3
    for w0, wl in starts:
        rank = tc.ranking64(db, pos, q, labels, w0, wl)
        assert {(s, o) for _, s, o in rank[:2]} == {(a, oa + w0), (b, ob + w0)}, (w0, rank[:3])
        assert rank[1][0] > 0.5 and all(sc < 0.3 for sc, _, _ in rank[2:]), (w0, rank[:4])
    top, n_found, _ = _topn(torch_cuda, _index("overlap", db, pos), q, labels, [0], [q.shape[0]], window, hop, 3)
    for j, (w0, _) in enumerate(starts):
        got = {(int(e["song"]), int(e["offset"])) for e in top[j, :2]}
        assert got == {(a, oa + w0), (b, ob + w0)}, (w0, top[j])
        assert float(top[j, 1]["score"]) > 0.5 and not float(top[j, 2]["score"]) >= 0.3

    # ---- through the Database: search, ranked windows, per-track merge
    (tmp_path / "songList.txt").write_text("".join("song%02d.wav\n" % s for s in range(len(key))))
    key.astype(np.int32).tofile(str(tmp_path / "landmarkKey"))
    db.tofile(str(tmp_path / "embeddings"))
    dbo = Database(str(tmp_path), {"top_k": 20, "frame_shift_mul": 1}, hop_size, d=D)
    emb = torch_cuda.as_tensor(q).cuda()
    p = dbo.monitor_topn_launch(emb, [0], [q.shape[0]], window, hop, 3, edge_window=7)
    (ranked,), (found,) = dbo.monitor_topn_finish(p)
    assert ranked.shape == (len(starts), 3) and ranked.dtype.names == ("w0", "score", "song", "time_s", "votes")
    assert found.shape == (len(starts),) and (found >= 2).all() and (ranked["votes"][:, :2] >= 1).all()
    edge, = p["edge_rows"]
    assert edge.shape == (q.shape[0] - 7 + 1, 3)
    rows, = dbo.monitor_finish(dbo.monitor_launch(emb, [0], [q.shape[0]], window, hop))
    for f in ("w0", "score", "song", "time_s"):
        assert np.array_equal(ranked[f][:, 0], rows[f]), f
    det = merge_window_tracks(ranked, window, hop, hop_size, 0.5, min_windows=2, edge_rows=edge, edge_window=7)
    assert [(d[2], d[6]) for d in det] == [(a, len(starts)), (b, len(starts))], det
    for d, o in zip(det, (oa, ob)):
        assert d[:2] == (0.0, q.shape[0] * hop_size) and d[3] == o * hop_size and d[7] <= 2, d
    assert min(d[7] for d in det) == 1
    # the winners alone: every window belongs to one detection only, so the two songs are never both reported throughout
    # (A and B score (1 + A.B) / |A + B| each, equal in exact arithmetic: which one wins a window is rounding)
    one = merge_windows(rows, window, hop, hop_size, 0.5)
    assert sum(d[6] for d in one) == len(starts) and {d[2] for d in one} <= {a, b}
    assert not all(any(d[2] == s and d[6] == len(starts) for d in one) for s in (a, b))


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(torch_cuda):
    """n outside 1..64: -1 with a message and no launch (at the C ABI and in the Python layer); a shard refuses with
    match_windows' message; recordings that exceed the rows given are caught like match_windows catches them"""
    from pfann_amd import lib as L
    from pfann_amd.database import DeviceIndex
    db, pos = mx.std_world(41, D)
    idx = _index("std", db, pos)
    q = torch_cuda.as_tensor(db[:30]).cuda()
    labels = torch_cuda.zeros((30, 4), dtype=torch_cuda.int64).cuda()
    rs = torch_cuda.zeros(1, dtype=torch_cuda.int64).cuda()
    rl = torch_cuda.full((1,), 30, dtype=torch_cuda.int32).cuda()
    wf = torch_cuda.as_tensor([0, 26]).cuda()
    top = torch_cuda.zeros((26 * 65, 24), dtype=torch_cuda.uint8).cuda()
    lib = L.load()
    for n in (0, 65, -1):
        rc, tags = _tags_of(lambda: lib.pfann_match_windows_topn(idx.handle, q.data_ptr(), labels.data_ptr(), 4, rs.data_ptr(), rl.data_ptr(),
                                                                 1, 5, 1, 1, 0.0, 0, wf.data_ptr(), n, top.data_ptr(), None, None))
        assert rc == -1 and tags == [""], (n, rc, tags)
        with pytest.raises(L.PfannError, match="outside 1..64"):
            L.check(rc, "pfann_match_windows_topn")
        with pytest.raises(L.PfannError, match="outside 1..64"):
            idx.match_windows_topn(q, labels, [0], [30], 5, 1, n)
    torch_cuda.cuda.synchronize()
    assert not top.any(), "a refused call wrote results"
    (t, f, _), tags = _tags_of(lambda: _topn(torch_cuda, idx, q, labels, [0], [30], 5, 1, 64))      # n_found may be NULL: see above; here 64 is legal
    assert tags == ["seq_match_windows_topn"] and t.shape == (26, 64)
    lo, hi = 10, 30
    shard = DeviceIndex(D, 0)
    shard.load(db[pos[lo]:pos[hi]], pos, int(pos[lo]), song_range=(lo, hi))
    for call in (lambda: shard.match_windows(q, labels, [0], [30], 5, 1), lambda: shard.match_windows_topn(q, labels, [0], [30], 5, 1, 3)):
        with pytest.raises(L.PfannError, match="match_windows: the handle holds a shard of the database"):
            call()
    for call in (lambda: idx.match_windows(q, labels, [0, 20], [20, 20], 5, 1), lambda: idx.match_windows_topn(q, labels, [0, 20], [20, 20], 5, 1, 3)):
        with pytest.raises(AssertionError, match="recordings exceed the rows given"):
            call()


def test_n_found_may_be_null(torch_cuda):
    """the C ABI without n_found: the same lists, on both paths"""
    from pfann_amd import lib as L
    k = 20
    db, pos, q, labels, rstart, rlen = mc.grid_recordings(D, k)
    idx = _index(("grid", k), db, pos)
    lib = L.load()
    qd, ld = torch_cuda.as_tensor(q).cuda(), torch_cuda.as_tensor(labels).cuda()
    for fsm in (1, 2):
        window, hop, n = 19, 2, 3
        want, _, wfirst = _topn(torch_cuda, idx, q, labels, rstart, rlen, window, hop, n, fsm=fsm)
        rs = torch_cuda.as_tensor(np.asarray(rstart, np.int64)).cuda()
        rl = torch_cuda.as_tensor(np.asarray(rlen, np.int32)).cuda()
        wf = torch_cuda.as_tensor(wfirst).cuda()
        top = torch_cuda.zeros((int(wfirst[-1]), n, 24), dtype=torch_cuda.uint8).cuda()
        L.check(lib.pfann_match_windows_topn(idx.handle, qd.data_ptr(), ld.data_ptr(), k, rs.data_ptr(), rl.data_ptr(), len(rlen), window,
                                             hop, fsm, 0.0, 0, wf.data_ptr(), n, top.data_ptr(), None, None), "pfann_match_windows_topn")
        torch_cuda.cuda.synchronize()
        assert top.cpu().numpy().tobytes() == want.tobytes(), fsm


# ------------------------------------------------------------------------------------------------ end to end
def _cli_set(tmp_path):
    """the WAV set of tests/test_gpu_monitor.py's end-to-end case: ~50 synthetic songs and a 3-minute recording of four
    excerpts at SNR 0 with noise between them -> (model dir, music list, recording list)"""
    import torch
    from pfann_amd import synth
    params = json.load(open(os.path.join(REPO, "configs", "default.json")))
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
    plan = [(None, 0, 12), (7, 5, 35), (None, 0, 10), (23, 0, 30), (None, 0, 14), (41, 12, 25), (None, 0, 9), (7, 20, 20), (None, 0, 25)]
    parts = []
    for j, (s, o, n) in enumerate(plan):
        noise = synth.normal(77, "mon/e2e/%d" % j, n * sr).astype(np.float64)
        if s is None:
            x = noise * 2000.0
        else:
            sig = songs[s][o * sr:(o + n) * sr].astype(np.float64)
            x = sig + noise * np.sqrt(np.mean(sig ** 2))          # SNR 0 dB
        parts.append(x)
    rec = np.concatenate(parts)
    rec = np.clip(rec / np.abs(rec).max() * 30000.0, -32768, 32767).astype(np.int16)
    synth.write_wav(str(tmp_path / "rec.wav"), rec)
    (tmp_path / "recs.txt").write_text(str(tmp_path / "rec.wav") + "\n" + str(tmp_path / "missing.wav") + "\n")
    return str(mdir), str(tmp_path / "music.txt"), str(tmp_path / "recs.txt")


def test_monitor_cli_top_1_is_the_default_and_top_3_adds_ranks(tmp_path):
    """monitor.py --top 1 writes byte-identical files to a run without the flag; --top 3 writes the rank and votes columns
    and the best_rank column, and its rank-1 rows are the --top 1 rows"""
    mdir, music, recs = _cli_set(tmp_path)
    db = str(tmp_path / "db")
    env = dict(os.environ, PYTHONPATH=REPO)
    runs = [["builder.py", music, db, mdir]]
    runs += [["monitor.py", recs, db, str(tmp_path / (name + ".tsv"))] + flags
             for name, flags in (("plain", []), ("top1", ["--top", "1"]), ("top3", ["--top", "3"]))]
    for cmd in runs:
        r = subprocess.run(["timeout", "-k", "10", "400", sys.executable, os.path.join(REPO, cmd[0])] + cmd[1:],
                           capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=460)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    read = lambda name: open(str(tmp_path / name), "rb").read()
    assert read("plain.tsv") == read("top1.tsv") and read("plain_windows.csv") == read("top1_windows.csv")
    assert len(read("plain.tsv").splitlines()) == 5                          # four detections and the unreadable recording
    one = list(csv.reader(open(str(tmp_path / "top1_windows.csv"))))
    three = list(csv.reader(open(str(tmp_path / "top3_windows.csv"))))
    assert three[0] == one[0] + ["rank", "votes"] and three[-1] == one[-1] and one[-1][1] == "error"
    body = three[1:-1]
    assert all(len(r) == 8 and r[3] != "" or r[6] == "1" for r in body), "a padding entry was written"
    assert [r[:6] for r in body if r[6] == "1"] == one[1:-1]
    assert {r[6] for r in body} == {"1", "2", "3"} and all(int(r[7]) >= 1 for r in body if r[3] != "")
    det1 = [x.split("\t") for x in read("top1.tsv").decode().splitlines()]
    det3 = [x.split("\t") for x in read("top3.tsv").decode().splitlines()]
    assert det3[-1] == det1[-1] and all(len(x) == 9 and 1 <= int(x[8]) <= 3 for x in det3[:-1])
    # the four excerpts are still there, ranked first: a track holds every window of the --top 1 run, so its detection
    # reaches at least as far, to within the end-to-end case's own tolerance (one hop_size plus one window hop, 1.5 s)
    for y in det1[:-1]:
        assert any(x[3] == y[3] and x[8] == "1" and float(x[1]) <= float(y[1]) + 1.5 and float(x[2]) >= float(y[2]) - 1.5
                   for x in det3[:-1]), (y, det3)
