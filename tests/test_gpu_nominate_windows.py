"""Windowed dense nomination on the GPU (pfann_nominate_windows_dense, csrc/nominate_windows.hip).  Every comparison is `==` on
bytes or fields against calls of this library that are pinned elsewhere: pfann_nominate_songs_dense on the windows as queries
(tests/test_gpu_nominate_dense.py), pfann_match_windows_dense_topn on the exact grid, Database.monitor_dense_launch and
monitor.py --dense."""
import csv
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import dense_cases as dc
import dense_topn_cases as dt
import match_exact as mx

pytestmark = pytest.mark.gpu
D = 128
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RLEN = [0, 5, 18, 19, 128, 129, 240]                     # 128, 129 and hop 7: the tile edge at SI = 110
SHAPES = [(19, 2), (19, 1), (19, 7), (1, 1), (64, 1), (64, 70), (7, 1)]      # (64, 70): slots without a window start


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


def _starts(rlen):
    return [int(x) for x in np.pad(np.cumsum(rlen), (1, 0))[:-1]]


def _query_form(idx, qd, rstart, rlen, window, hop, n):
    """pfann_nominate_songs_dense on the windows as queries -> (cand, n_found, n_close, wfirst)"""
    from pfann_amd.database import window_queries
    qstart, qlen, wfirst = window_queries(rstart, rlen, window, hop)
    return idx.nominate_songs_dense(qd, qstart, qlen, n, max_qlen=min(window, 64)) + (wfirst,)


def _assert_same(got, want, what):
    (cand, n_found, n_close), wfirst = got
    rc, rf, rcl, rfirst = want
    assert wfirst.tolist() == rfirst.tolist() and cand.shape == rc.shape, what
    bad = np.flatnonzero((n_found != rf) | (n_close != rcl))
    assert bad.size == 0, "%s: window %d: n_found %d n_close %d, the query form %d %d" % (
        what, bad[0], n_found[bad[0]], n_close[bad[0]], rf[bad[0]], rcl[bad[0]])
    if cand.tobytes() != rc.tobytes():
        w = [i for i in range(len(cand)) if cand[i].tobytes() != rc[i].tobytes()][0]
        raise AssertionError("%s: window %d: %r, the query form %r" % (what, w, cand[w][:3], rc[w][:3]))


# ------------------------------------------------------------------------------------------------ 1. equals the query form
def _grid_recordings(db, seed):
    """sum(RLEN) rows cut from the database in one piece, a fifth of the values replaced by other grid values"""
    total = sum(RLEN)
    assert db.shape[0] >= 40 + total
    noise = mx.grid_rows(seed, "nomwin/noise", total, db.shape[1])
    flip = np.random.default_rng(seed).random((total, db.shape[1])) < 0.2
    return np.where(flip, noise, db[40:40 + total]).astype(np.float32)


def _world(name):
    if name == "packed":
        db, pos, _, _, _ = dt.packed_world(D)
    else:
        db, pos = mx.std_world(41, int(name), long_rows=300 if int(name) == 128 else 0)
    return db, pos, _grid_recordings(db, 911)


@pytest.mark.parametrize("name", ["packed", "64", "128", "136", "256"])
def test_equals_the_query_form(torch_cuda, name):
    db, pos, q = _world(name)
    idx = _index(("nomwin", name), db, pos)
    qd = torch_cuda.as_tensor(q).cuda()
    rstart = _starts(RLEN)
    for window, hop in SHAPES:
        for n in (1, 3, 64):
            got = idx.nominate_windows_dense(qd, rstart, RLEN, window, hop, n)
            _assert_same(got, _query_form(idx, qd, rstart, RLEN, window, hop, n), "%s window %d hop %d n %d" % (name, window, hop, n))
            assert (got[0][1] > 0).all(), "a window without a candidate: the comparison would be empty"


# ------------------------------------------------------------------------------------------------ 2. equals the ranked dense matcher
def test_equals_the_ranked_dense_matcher_on_the_grid(torch_cuda):
    """every value is k/16: fp16 products and fp32 sums are exact, so the approximate score IS the dense score.  Recording 1 is
    cut from song 5, whose copy is song 9; with song 9 excluded it vanishes from the list and from n_found"""
    db, pos = mx.std_world(41, D, long_rows=300)
    mx.assert_exact_domain(64, D)
    idx = _index(("nomwin", "128"), db, pos)
    lens = [150, int(pos[6] - pos[5]), 30, 7]
    parts = [db[int(pos[56]) + 20:int(pos[56]) + 170], db[int(pos[5]):int(pos[6])], db[int(pos[12]) + 1:int(pos[12]) + 31],
             mx.grid_rows(913, "nomwin/free", 7, D)]
    assert [p.shape[0] for p in parts] == lens and lens[1] == 23
    qd = torch_cuda.as_tensor(np.concatenate(parts)).cuda()
    rstart = _starts(lens)
    have = int((np.diff(pos) > 0).sum())
    for window, hop in ((19, 2), (64, 1), (5, 3)):
        for excl in (None, [-1, 9, 12, 3]):
            (ref, ref_found, _), wfirst = idx.match_windows_dense_topn(qd, rstart, lens, window, hop, 64, exclude_song=excl)
            (cand, n_found, n_close), wf = idx.nominate_windows_dense(qd, rstart, lens, window, hop, 64, exclude_song=excl)
            assert wf.tolist() == wfirst.tolist()
            for f in ("song", "n_cand", "score"):
                bad = np.argwhere(cand[f] != ref[f])
                assert bad.size == 0, "window %d hop %d excl %r field %s: window %d entry %d: %r, the dense matcher %r" % (
                    window, hop, excl, f, bad[0][0], bad[0][1], cand[f][tuple(bad[0])], ref[f][tuple(bad[0])])
            assert (cand["offset"] == 0).all() and (cand["shift"] == 0).all()
            assert np.array_equal(n_found, ref_found)
            assert (n_close >= 1).all() and (n_close <= n_found).all()
            a, b = int(wfirst[1]), int(wfirst[2])                    # the windows of the cut from song 5
            if excl is None:
                assert (n_found == have).all()
                assert (cand["song"][a:b, 0] == 5).all() and (cand["song"][a:b, 1] == 9).all()
                assert (cand["score"][a:b, 0] == cand["score"][a:b, 1]).all() and (n_close[a:b] >= 2).all()
            else:
                assert (n_found[a:b] == have - 1).all() and (n_found[:a] == have).all()
                assert (cand["song"][a:b, 0] == 5).all() and not (cand["song"][a:b] == 9).any()
                assert (cand["song"][:a] == 9).any(), "the exclusion of one recording reached another"


# ------------------------------------------------------------------------------------------------ real-valued rows
EXCERPT_SONGS = (0, 1, 3, 6, 8, 10, 11, 0, 3)            # none of the self-match world's duplicates (2/7, 4/9)


@pytest.fixture(scope="module")
def noisy_world(tmp_path_factory):
    """the recipe of tests/test_gpu_nominate_dense.py: dense_cases.selfmatch_world, nine excerpts of 5 / 19 / 40 rows plus noise
    of 0.3 / 1 / 2 times the signal and three pure-noise pieces, here concatenated into two recordings (excerpts 0-5; the rest)
    -> (dir, emb, pos, q, rstart, rlen)"""
    d = str(tmp_path_factory.mktemp("nominate_windows_self"))
    emb, pos = dc.selfmatch_world(d)
    rng = np.random.default_rng(31)
    rows = []
    for i, (n, level) in enumerate((n, level) for n in (5, 19, 40) for level in (0.3, 1.0, 2.0)):
        s = EXCERPT_SONGS[i]
        a = int(pos[s]) + i
        assert a + n <= pos[s + 1]
        noise = rng.standard_normal((n, D)) / np.sqrt(D)
        x = emb[a:a + n].astype(np.float64) + level * noise
        rows.append(x / np.linalg.norm(x, axis=1, keepdims=True))
    for n in (5, 19, 40):
        x = rng.standard_normal((n, D))
        rows.append(x / np.linalg.norm(x, axis=1, keepdims=True))
    rlen = [sum(r.shape[0] for r in rows[:6]), sum(r.shape[0] for r in rows[6:])]
    return d, emb, pos, np.concatenate(rows).astype(np.float32), [0, rlen[0]], rlen


# ------------------------------------------------------------------------------------------------ 3. the byte contract
def test_byte_contract(torch_cuda, noisy_world, monkeypatch):
    torch = torch_cuda
    from pfann_amd import database as dbm
    from pfann_amd.utils import read_config
    dirname, emb, pos, q, rstart, rlen = noisy_world
    idx = _index("self", emb, pos)
    qd = torch.as_tensor(q).cuda()
    monkeypatch.delenv("PFANN_NOMINATE_WINDOWS", raising=False)
    monkeypatch.delenv("PFANN_NOMINATE_WINDOWS_GENERAL", raising=False)
    (full, f, cl), wfirst = idx.nominate_windows_dense(qd, rstart, rlen, 19, 2, 64)
    again = idx.nominate_windows_dense(qd, rstart, rlen, 19, 2, 64)[0]
    assert again[0].tobytes() == full.tobytes() and np.array_equal(again[1], f) and np.array_equal(again[2], cl), "two runs differ"
    # window 7 of recording 1 (rows 14 .. 33 of it): alone, as its own recording; at hop 1 and hop 7 among other neighbours
    w0 = 14
    want = (full[int(wfirst[1]) + 7].tobytes(), int(f[int(wfirst[1]) + 7]), int(cl[int(wfirst[1]) + 7]))
    a = rstart[1] + w0
    (c1, f1, cl1), _ = idx.nominate_windows_dense(torch.as_tensor(q[a:a + 19]).cuda(), [0], [19], 19, 2, 64)
    assert (c1[0].tobytes(), int(f1[0]), int(cl1[0])) == want, "the bytes depend on the neighbours"
    for hop in (1, 7):
        (c, ff, cc), wf = idx.nominate_windows_dense(qd, rstart, rlen, 19, hop, 64)
        w = int(wf[1]) + w0 // hop
        assert (c[w].tobytes(), int(ff[w]), int(cc[w])) == want, "the bytes depend on the hop (%d)" % hop
    # a longer window length elsewhere in the call changes nothing either: the window as a short recording under window 40
    (c, ff, cc), wf = idx.nominate_windows_dense(torch.as_tensor(q[a:a + 19]).cuda(), [0], [19], 40, 3, 64)
    assert (c[0].tobytes(), int(ff[0]), int(cc[0])) == want, "the bytes depend on the window of the call"
    for chunk in ("1", "60"):                            # read per call
        monkeypatch.setenv("PFANN_NOMINATE_WINDOWS", chunk)
        (c, ff, cc), _ = idx.nominate_windows_dense(qd, rstart, rlen, 19, 2, 64)
        assert c.tobytes() == full.tobytes() and np.array_equal(ff, f) and np.array_equal(cc, cl), "the bytes depend on the chunking (%s)" % chunk
    monkeypatch.delenv("PFANN_NOMINATE_WINDOWS")
    (three, f3, cl3), _ = idx.nominate_windows_dense(qd, rstart, rlen, 19, 2, 3)
    assert three.tobytes() == np.ascontiguousarray(full[:, :3]).tobytes() and np.array_equal(f3, f) and np.array_equal(cl3, cl)
    # the expansion behind Database gives the same bytes
    cfg = read_config(os.path.join(dirname, "configs.json"))
    db = dbm.Database(dirname, cfg["indexer"], cfg["hop_size"], d=D)
    outs = []
    for general in (None, "1"):
        if general is not None:
            monkeypatch.setenv("PFANN_NOMINATE_WINDOWS_GENERAL", general)
        p = db.monitor_nominate_launch(qd, rstart, rlen, 19, 2, 4, edge_window=7)
        torch.cuda.synchronize()
        outs.append([p["res"].cpu().numpy().tobytes(), p["n_close"].cpu().numpy().tobytes(), p["fine"][0].cpu().numpy().tobytes(),
                     p["edge_n_close"].cpu().numpy().tobytes()])
    assert outs[0] == outs[1], "PFANN_NOMINATE_WINDOWS_GENERAL=1 changes the bytes"
    assert outs[0][1] == cl.tobytes()


# ------------------------------------------------------------------------------------------------ 4. bad rows
def test_bad_rows(torch_cuda, noisy_world):
    torch = torch_cuda
    from pfann_amd.database import DeviceIndex
    _, emb, pos, q, _, _ = noisy_world
    idx = _index("self", emb, pos)
    rows = q[:60].copy()
    rows[30, 7] = np.nan
    rows[45] *= 7e4                                      # a norm outside fp16's range
    qd = torch.as_tensor(rows).cuda()
    pad = np.asarray([dt.PAD] * 4, DeviceIndex.RESULT_DTYPE).tobytes()
    for window, hop in ((19, 1), (19, 2), (7, 1)):
        got = idx.nominate_windows_dense(qd, [0], [60], window, hop, 4)
        (cand, n_found, n_close), wfirst = got
        hit = np.asarray([any(w0 <= r < w0 + window for r in (30, 45)) for w0 in range(0, 60 - window + 1, hop)])
        assert hit.shape[0] == int(wfirst[-1]) and hit.any() and not hit.all()
        assert (n_found[hit] == -1).all() and (n_close[hit] == -1).all() and all(cand[w].tobytes() == pad for w in np.flatnonzero(hit))
        assert (n_found[~hit] == 11).all() and (n_close[~hit] >= 1).all()
        _assert_same(got, _query_form(idx, qd, [0], [60], window, hop, 4), "bad rows, window %d hop %d" % (window, hop))


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_leave_the_outputs_untouched(torch_cuda):
    from pfann_amd import lib as L
    from pfann_amd.database import DeviceIndex
    torch = torch_cuda
    lib = L.load()
    db, pos = mx.std_world(41, D)
    whole = _index("std", db, pos)
    lo, hi = 10, 30
    shard = DeviceIndex(D, 0)
    shard.load(db[pos[lo]:pos[hi]], pos, int(pos[lo]), song_range=(lo, hi))
    half = _index("std", db, pos, "f16")
    db12, pos12 = mx.std_world(41, 12)
    no_copy = _index("std12", db12, pos12)
    q = torch.as_tensor(db[:30]).cuda()
    q12 = torch.as_tensor(db12[:30]).cuda()
    rs = torch.zeros(1, dtype=torch.int64).cuda()
    rl = torch.full((1,), 30, dtype=torch.int32).cuda()
    wf = torch.as_tensor([0, 6], dtype=torch.int64).cuda()   # window 19, hop 2

    def call(idx, n=3, window=19, hop=2, nR=1, nW=6, cand=True):
        outs = [torch.full((size,), 0xA5, dtype=torch.uint8).cuda() for size in (6 * 65 * ctypes.sizeof(L.MatchResult), 6 * 4, 6 * 4)]
        rc = lib.pfann_nominate_windows_dense(idx.handle, (q12 if idx is no_copy else q).data_ptr(), rs.data_ptr(), rl.data_ptr(), nR,
                                              window, hop, wf.data_ptr(), nW, None, n, outs[0].data_ptr() if cand else None,
                                              outs[1].data_ptr(), outs[2].data_ptr(), None)
        msg = L.last_error()
        torch.cuda.synchronize()
        return rc, msg, [bool((o.cpu() == 0xA5).all()) for o in outs]

    rc, _, untouched = call(whole)                       # the control: the same call on a good handle writes all three
    assert rc == 0 and untouched == [False, False, False]
    for idx, kw, word in ((shard, {}, "shard"), (half, {}, "fp16-only"), (no_copy, {}, "no fp16 copy"),
                          (whole, dict(n=0), "n=0"), (whole, dict(n=65), "n=65"), (whole, dict(window=0), "window=0"),
                          (whole, dict(window=65), "window=65"), (whole, dict(hop=0), "hop=0"), (whole, dict(nR=-1), "nR=-1"),
                          (whole, dict(nW=-1), "n_windows=-1"), (whole, dict(cand=False), "cand_dev"),
                          # several at once: the first one in the stated order
                          (shard, dict(n=0, window=65, hop=0), "shard"), (half, dict(n=65, window=0), "fp16-only"),
                          (no_copy, dict(n=0, hop=0), "no fp16 copy"), (whole, dict(n=0, window=0, hop=0, nR=-1, cand=False), "n=0"),
                          (whole, dict(window=65, hop=0, nW=-1, cand=False), "window=65"),
                          (whole, dict(hop=0, nR=-1, cand=False), "hop=0"), (whole, dict(nW=-1, cand=False), "n_windows=-1")):
        rc, msg, untouched = call(idx, **kw)
        assert rc == -1 and msg and word in msg and all(untouched), (kw, word, rc, msg, untouched)
        assert idx is shard or "nominate_windows_dense" in msg, msg      # (a shard gets pfann_match_windows' message)
    with pytest.raises(L.PfannError) as refused:
        shard.nominate_songs_dense(q, [0], [30], 3)
    assert call(shard)[1] == str(refused.value).split(": ", 1)[1], "a shard is refused with another message than the query form's"
    with pytest.raises(L.PfannError, match="1..64"):
        whole.nominate_windows_dense(q, [0], [30], 19, 2, 65)
    with pytest.raises(ValueError):
        whole.nominate_windows_dense(q, [0], [30], 19, 0, 3)


# ------------------------------------------------------------------------------------------------ 6. the Database layer
def test_database_monitor_nominate(torch_cuda, noisy_world):
    from pfann_amd import database as dbm
    from pfann_amd import lib as L
    from pfann_amd.utils import read_config
    torch = torch_cuda
    dirname, emb, pos, q, rstart, rlen = noisy_world
    cfg = read_config(os.path.join(dirname, "configs.json"))
    db = dbm.Database(dirname, cfg["indexer"], cfg["hop_size"], d=D)
    idx = _index("self", emb, pos)
    qd = torch.as_tensor(q).cuda()
    N, window, hop, edge = 4, 19, 2, 7
    pd = db.monitor_dense_launch(qd, rstart, rlen, window, hop, edge_window=edge)
    dense_rows = db.monitor_finish(pd)
    p = db.monitor_nominate_launch(qd, rstart, rlen, window, hop, N, edge_window=edge)
    rows, n_close, certified = db.monitor_nominate_finish(p)
    assert len(rows) == len(n_close) == len(certified) == 2

    def check(rows, n_close, certified, dense_rows, w, h):
        _, _, ref_close, wfirst = _query_form(idx, qd, rstart, rlen, w, h, N)
        sure = 0
        for r in range(2):
            a, b = int(wfirst[r]), int(wfirst[r + 1])
            assert rows[r].dtype == dense_rows[r].dtype and rows[r].shape == dense_rows[r].shape == (b - a,)
            assert np.array_equal(n_close[r], ref_close[a:b]), (w, h, r)
            assert np.array_equal(certified[r], (ref_close[a:b] >= 0) & (ref_close[a:b] <= N))
            assert np.array_equal(rows[r]["w0"], dense_rows[r]["w0"])
            for i in np.flatnonzero(certified[r]):
                assert rows[r][i:i + 1].tobytes() == dense_rows[r][i:i + 1].tobytes(), (w, h, r, i, rows[r][i], dense_rows[r][i])
            sure += int(certified[r].sum())
        return sure, int(wfirst[-1])
    sure, nW = check(rows, n_close, certified, dense_rows, window, hop)
    print("long windows: %d of %d certified at N = %d" % (sure, nW, N))
    assert sure > 0, "no window is certified: the comparison was empty"
    assert p["edge_rows"] is not None and len(p["edge_rows"]) == 2 and sum(len(x) for x in p["edge_rows"]) > nW
    sure, nE = check(p["edge_rows"], p["edge_n_close"], p["edge_certified"], pd["edge_rows"], edge, 1)
    print("edge windows: %d of %d certified" % (sure, nE))
    assert sure > 0
    # N = 64 lists every song: every window is certified and every row is the dense row
    rows, n_close, certified = db.monitor_nominate_finish(db.monitor_nominate_launch(qd, rstart, rlen, window, hop, 64))
    assert all(c.all() for c in certified) and all(a.tobytes() == b.tobytes() for a, b in zip(rows, dense_rows))
    for change, word in (({"frame_shift_mul": 2}, "frame_shift_mul"), ({"score_alpha": 2.0}, "score_alpha")):
        other = dbm.Database(dirname, dict(cfg["indexer"], **change), cfg["hop_size"], d=D)
        with pytest.raises(L.PfannError, match=word):
            other.monitor_nominate_launch(qd, rstart, rlen, window, hop, N)
    with pytest.raises(L.PfannError, match="1..64"):
        db.monitor_nominate_launch(qd, rstart, rlen, window, hop, 65)


# ------------------------------------------------------------------------------------------------ 7. the CLI
def _run(tmp_path, cmd):
    """one command-line tool as a child under the suite's limits (tests/test_gpu_dense.py::_run)"""
    env = dict(os.environ, PYTHONPATH=REPO)
    r = subprocess.run(["timeout", "-k", "10", "400", sys.executable, os.path.join(REPO, cmd[0])] + cmd[1:],
                       capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=460)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def test_monitor_cli_nominate(tmp_path):
    """the scenario of test_monitor_cli_dense_finds_four_excerpts: builder.py once, monitor.py --dense, then monitor.py --dense
    --nominate 4.  Every _windows.csv row that _nominate.csv certifies is --dense's row; the four excerpts come out as detections;
    every window wholly inside an excerpt is certified.

    That last assertion is a condition of the scenario, from its CPU float64 oracle (oracle/segmenter.py, melspec_f64 and
    encoder.encode in float64 over the 50 songs and the recording; per-song best totals over every alignment, window 19, hop 2):
    the 74 windows wholly inside an excerpt score 0.2107 .. 0.3864 and all name the true song; the gap of their best song's total
    to the second song's is at least 1.7546, against 2 E of at most 0.0413 (E from fp16_margin_cases.margin_ref on the oracle's
    rows), so n_close is 1 there and N = 4 certifies them.  Of the other 97 windows nine have a gap below 2 E: not every window
    can be expected to be certified at N = 1, and none is asserted to be.  ("Windowed dense nomination": this test
    has not been seen to pass on the MI355X; its first child, builder.py, stalled where it was tried.)"""
    from pfann_amd.monitor import DEFAULT_HOP, default_window
    params, mdir, music, truth = dc.four_excerpts(tmp_path)
    db = str(tmp_path / "db")
    recs = str(tmp_path / "recs.txt")
    _run(tmp_path, ["builder.py", str(tmp_path / "music.txt"), db, mdir])
    _run(tmp_path, ["monitor.py", recs, db, str(tmp_path / "dense.tsv"), "--dense"])
    _run(tmp_path, ["monitor.py", recs, db, str(tmp_path / "nom.tsv"), "--dense", "--nominate", "4"])
    assert not (tmp_path / "dense_nominate.csv").exists()
    lines = [x.split("\t") for x in open(str(tmp_path / "nom.tsv")).read().splitlines()]
    assert lines[-1] == [str(tmp_path / "missing.wav"), "error"]
    det = lines[:-1]
    print("detections:\n" + "\n".join("  " + "  ".join(x[1:]) for x in det))
    window, hop_size = default_window(params), params["hop_size"]
    tol = hop_size + DEFAULT_HOP * hop_size
    assert len(det) == 4, "%d detections" % len(det)
    for x, (t0, t1, s, o) in zip(det, truth):
        assert len(x) == 8 and x[0] == str(tmp_path / "rec.wav") and x[3] == music[s], (x, s)
        assert float(x[1]) < t1 and float(x[2]) > t0, ("a detection inside a noise gap", x)
        assert abs(float(x[1]) - t0) <= tol and abs(float(x[2]) - t1) <= tol and abs(float(x[4]) - o) <= tol, (x, t0, t1, o)
    dense = list(csv.reader(open(str(tmp_path / "dense_windows.csv"))))
    nom = list(csv.reader(open(str(tmp_path / "nom_windows.csv"))))
    cert = list(csv.reader(open(str(tmp_path / "nom_nominate.csv"))))
    assert dense[0] == nom[0] == ["recording", "w0", "start_s", "song", "score", "time"] and dense[-1] == nom[-1] and nom[-1][1] == "error"
    assert cert[0] == ["recording", "w0", "n_close", "certified"] and cert[-1] == [str(tmp_path / "missing.wav"), "error", "-1", "0"]
    dense, nom, cert = dense[1:-1], nom[1:-1], cert[1:-1]
    assert len(dense) == len(nom) == len(cert) > 150 and [g[:3] for g in dense] == [g[:3] for g in nom]
    assert [c[:2] for c in cert] == [g[:2] for g in nom]
    inside = sure = 0
    for g, h, c in zip(dense, nom, cert):
        assert c[3] == ("1" if 0 <= int(c[2]) <= 4 else "0"), c
        if c[3] == "1":
            sure += 1
            assert g == h, ("a certified window differs from --dense's", g, h, c)
        start, end = float(g[2]), float(g[2]) + (window - 1) * hop_size + params["segment_size"]
        for t0, t1, s, o in truth:
            if t0 <= start and end <= t1:
                inside += 1
                assert c[3] == "1" and h[3] == music[s], ("a window inside an excerpt is not certified", h, c)
    print("%d of %d windows certified" % (sure, len(cert)))
    assert inside == 74, inside
