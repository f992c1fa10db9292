"""The dense matcher's background statistics on the GPU (pfann_match_windows_dense_stats, csrc/dense.hip): the three integers
of every window against the integer oracle of tests/dense_stats_cases.py -- `==` on the exact grid --, the byte contract, the
exclusion, real-valued rows against float64, the significance they give on a handle, the refusals, and monitor.py --max-fa."""
import csv
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import dense_cases as dc
import dense_stats_cases as sc
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


def _stats(torch, idx, q, rstart, rlen, window, hop, **kw):
    """-> (results, stats, wfirst, match_windows_dense's results for the same arguments)"""
    qd = torch.as_tensor(q).cuda()
    (res, stats), wfirst = idx.match_windows_dense_stats(qd, rstart, rlen, window, hop, **kw)
    plain, wf = idx.match_windows_dense(qd, rstart, rlen, window, hop, **kw)
    assert np.array_equal(wfirst, wf) and stats.shape == res.shape
    return res, stats, wfirst, plain


# ------------------------------------------------------------------------------------------------ exact arithmetic
def _grid_world(d, seed=300):
    world = mx.std_world(41, d, long_rows=300)
    db, pos, q, _, rstart, rlen = mc.grid_recordings(d, 20, world=world, seed=seed)
    return db, pos, q, rstart, rlen


@pytest.mark.parametrize("window", mc.WINDOWS)
def test_every_window_equals_the_integer_oracle(torch_cuda, window):
    """the world of test_gpu_dense.py::test_every_window_equals_the_dense_oracle -- songs of 300 rows (longer than a tile), songs
    shorter than the window, copies, an 11-row and an empty recording --, windows 1 / 5 / 19 / 64 x hops 1 / 2 / 7: n_full,
    sum_q and sumsq_q == the oracle's Python integers in every window, the results byte-equal to match_windows_dense"""
    db, pos, q, rstart, rlen = _grid_world(D)
    assert np.diff(pos).max() == 300 > 128 and 0 < np.diff(pos)[np.diff(pos) > 0].min() < 5 and 11 in rlen and 0 in rlen
    mx.assert_exact_domain(window, D)
    idx = _index("grid", db, pos)
    for hop in mc.HOPS:
        want = sc.stats_oracle(q, db, pos, window, hop, rstart, rlen, key="grid")
        res, stats, wfirst, plain = _stats(torch_cuda, idx, q, rstart, rlen, window, hop)
        assert np.array_equal(wfirst, mc.wfirst_of(rlen, window, hop)) and stats.shape[0] == len(want) > 0
        bad = sc.differing(stats, want)
        assert not bad, "window %d hop %d: %d of %d windows differ\n%s" % (window, hop, len(bad), len(want), "\n".join(bad[:6]))
        assert res.tobytes() == plain.tobytes(), "window %d hop %d: the results are not match_windows_dense's" % (window, hop)
    want = sc.stats_oracle(q, db, pos, window, 1, rstart, rlen, key="grid")
    assert any(w["sum_q"] != 0 for w in want) and any(w["sumsq_q"] != 0 for w in want)
    if window > 11:                                      # the 11-row recording: one window of 11 rows, with its own count
        short = want[int(mc.wfirst_of(rlen, window, 1)[rlen.index(11)])]
        assert short["n_full"] == int(np.maximum(np.diff(pos) - 11 + 1, 0).sum()) != want[0]["n_full"]


@pytest.mark.parametrize("d", [64, 256])
def test_other_row_widths(torch_cuda, d):
    db, pos, q, rstart, rlen = _grid_world(d, seed=340)
    mx.assert_exact_domain(19, d)
    for hop in (1, 3):
        want = sc.stats_oracle(q, db, pos, 19, hop, rstart, rlen, key=("grid-d", d))
        res, stats, _, plain = _stats(torch_cuda, _index(("grid-d", d), db, pos), q, rstart, rlen, 19, hop)
        bad = sc.differing(stats, want)
        assert not bad, "d %d hop %d: %d of %d windows differ\n%s" % (d, hop, len(bad), len(want), "\n".join(bad[:6]))
        assert res.tobytes() == plain.tobytes()


def test_excluded_song(torch_cuda):
    """dense_cases.small_world, one excluded song per recording: the statistics omit exactly that song's full pieces"""
    db, pos, q, rstart, rlen = dc.small_world()
    lens = np.diff(pos)
    order = np.argsort(-lens, kind="stable")
    excl = [int(order[0]), -1, int(order[1])]            # the two longest songs: longer than every window below
    idx = _index("small", db, pos)
    for window, hop in ((5, 1), (19, 2)):
        mx.assert_exact_domain(window, db.shape[1])
        res, stats, _, plain = _stats(torch_cuda, idx, q, rstart, rlen, window, hop, exclude_song=excl)
        want = sc.stats_oracle(q, db, pos, window, hop, rstart, rlen, excl=excl)
        bad = sc.differing(stats, want)
        assert not bad, "window %d hop %d: %d windows differ\n%s" % (window, hop, len(bad), "\n".join(bad[:6]))
        assert res.tobytes() == plain.tobytes()
        _, none, wfirst, _ = _stats(torch_cuda, idx, q, rstart, rlen, window, hop)
        _, minus, _, _ = _stats(torch_cuda, idx, q, rstart, rlen, window, hop, exclude_song=[-1] * len(rlen))
        assert none.tobytes() == minus.tobytes(), "NULL and all -1 give different bytes"
        for r, ex in enumerate(excl):
            a, b = int(wfirst[r]), int(wfirst[r + 1])
            n = min(window, rlen[r])
            gone = max(int(lens[ex]) - n + 1, 0) if ex >= 0 else 0
            assert b > a and (none["n_full"][a:b] - stats["n_full"][a:b] == gone).all(), (window, r)
            if ex < 0:
                assert none[a:b].tobytes() == stats[a:b].tobytes()
            else:
                assert gone > 0 and (none["sumsq_q"][a:b] >= stats["sumsq_q"][a:b]).all()
    one = _index("one-song", db[pos[2]:pos[3]], np.asarray([0, int(lens[2])], np.int64))
    _, stats, _, _ = _stats(torch_cuda, one, q, rstart, rlen, 5, 1, exclude_song=[0] * len(rlen))
    assert len(stats) > 0 and not stats.view(np.int64).any(), "everything excluded: the statistics are zeros"


# ------------------------------------------------------------------------------------------------ real-valued rows
@pytest.fixture(scope="module")
def unit400():
    return mc.unit_case(7, 120, D, 100, 400)


def test_a_window_has_the_same_bytes_whatever_reached_it(torch_cuda, unit400):
    """hop 1 against hops 3 and 7, alone and batched behind a second recording of 137 rows, twice in a row: a window's 24 stats
    bytes are equal everywhere"""
    db, pos, q, _ = unit400
    window, L, other = 19, q.shape[0], 137
    idx = _index("unit400", db, pos)
    _, h1, _, _ = _stats(torch_cuda, idx, q, [0], [L], window, 1)
    _, again, _, _ = _stats(torch_cuda, idx, q, [0], [L], window, 1)
    assert h1.dtype.itemsize == 24 and h1.tobytes() == again.tobytes(), "two runs, other bytes"
    q2 = np.concatenate([q[:other][::-1], q])
    for hop in (3, 7):
        _, h, _, _ = _stats(torch_cuda, idx, q, [0], [L], window, hop)
        assert h1[::hop].tobytes() == h.tobytes(), "%d windows differ between hop 1 and hop %d" % (int((h1[::hop] != h).sum()), hop)
        _, b, wf, _ = _stats(torch_cuda, idx, q2, [0, other], [other, L], window, hop)
        assert b[wf[1]:].tobytes() == h.tobytes(), "batched behind another recording at hop %d: other bytes" % hop
    _, b1, wf, _ = _stats(torch_cuda, idx, q2, [0, other], [other, L], window, 1)
    assert b1[wf[1]:].tobytes() == h1.tobytes(), "batched behind another recording: other bytes"
    assert len({int(x) for x in h1["sum_q"]}) > len(h1) // 2, "the sums are not real-valued"


def test_real_valued_rows(torch_cuda, unit400):
    """against the float64 oracle.  A kernel total is within tau = n * 1e-6 of its float64 value (test_gpu_dense.py's per-score
    tolerance times the divisor) and the fixed point adds at most half a unit per candidate, so with Tmax the oracle's largest
    |total|: n_full ==, |mean - mean64| <= tau + 2^-24, |mean square - meansq64| <= 2 Tmax tau + tau^2 + 2^-18."""
    db, pos, q, _ = unit400
    window, hop, L = 19, 2, q.shape[0]
    idx = _index("unit400", db, pos)
    res, stats, _, plain = _stats(torch_cuda, idx, q, [0], [L], window, hop)
    want = sc.stats_oracle(q, db, pos, window, hop, [0], [L], key="unit400")
    assert len(stats) == len(want) > 100 and res.tobytes() == plain.tobytes()
    tau = window * 1e-6
    worst_mean = worst_sq = 0.0
    for j, w in enumerate(want):
        nf = int(stats["n_full"][j])
        assert nf == w["n_full"] > 0, j
        d_mean = abs(int(stats["sum_q"][j]) / 2.0 ** 24 / nf - w["mean"])
        d_sq = abs(int(stats["sumsq_q"][j]) / 2.0 ** 18 / nf - w["meansq"])
        worst_mean, worst_sq = max(worst_mean, d_mean), max(worst_sq, d_sq)
    print("unit400: %d windows, |mean - float64| <= %.3g (allowed %.3g), |mean square - float64| <= %.3g (allowed >= %.3g)"
          % (len(want), worst_mean, tau + 2.0 ** -24, worst_sq, tau * tau + 2.0 ** -18))
    for j, w in enumerate(want):
        nf = int(stats["n_full"][j])
        assert abs(int(stats["sum_q"][j]) / 2.0 ** 24 / nf - w["mean"]) <= tau + 2.0 ** -24, j
        assert abs(int(stats["sumsq_q"][j]) / 2.0 ** 18 / nf - w["meansq"]) <= 2.0 * w["tmax"] * tau + tau * tau + 2.0 ** -18, j


# ------------------------------------------------------------------------------------------------ significance on a handle
def test_significance_of_a_copy_and_of_its_absence(torch_cuda, tmp_path):
    """dense_cases.selfmatch_world: song 7 is a copy of song 2.  Song 2's rows as the recording, song 2 excluded: every window
    names song 7 with log10_fa <= -6 (the float64 oracle on the CPU: -461 .. -556).  With songs 2 and 7 removed from the
    handle every window has log10_fa > -3 (the oracle: -0.91 .. 0), and the handle answers as a fresh one loaded without them."""
    from pfann_amd import significance as sg
    from pfann_amd.database import DeviceIndex
    emb, pos = dc.selfmatch_world(str(tmp_path))
    q = emb[pos[2]:pos[3]]
    L = q.shape[0]
    window, hop = dc.SELF_WINDOW, dc.SELF_HOP
    idx = DeviceIndex(D, 0)
    idx.load(emb, pos)

    def log10_fa(index, song_pos):
        res, stats, _, _ = _stats(torch_cuda, index, q, [0], [L], window, hop, exclude_song=[2])
        lens = np.diff(song_pos)
        fa = sg.log10_false_alarms(res, stats, window, 2, sg.OverlapHistograms(lens), lens)
        assert (stats["n_full"] == sg.overlap_histogram(lens, window, 2)[window]).all()
        assert (res["n_cand"] == sg.overlap_histogram(lens, window, 2).sum()).all()
        return res, stats, fa
    res, stats, fa = log10_fa(idx, pos)
    want = sc.stats_oracle(q, emb, pos, window, hop, [0], [L], excl=[2], as_float32=True)
    assert len(res) == len(want) >= 10 and (res["song"] == 7).all() and all(w["song"] == 7 for w in want)
    print("copy present: log10_fa %.1f .. %.1f" % (fa.min(), fa.max()))
    assert (fa <= -6.0).all(), fa
    idx.remove_songs([2, 7])
    lens = np.diff(pos)
    lens[[2, 7]] = 0
    pos2 = np.pad(np.cumsum(lens), (1, 0)).astype(np.int64)
    assert np.array_equal(idx.song_pos, pos2)
    res, stats, fa = log10_fa(idx, pos2)
    print("copy removed: log10_fa %.2f .. %.2f" % (fa.min(), fa.max()))
    assert (res["song"] >= 0).all() and (res["song"] != 7).all() and (fa > -3.0).all(), fa
    fresh = DeviceIndex(D, 0)
    fresh.load(np.concatenate([emb[pos[s]:pos[s + 1]] for s in range(12) if s not in (2, 7)]), pos2)
    res2, stats2, _, _ = _stats(torch_cuda, fresh, q, [0], [L], window, hop, exclude_song=[2])
    assert res.tobytes() == res2.tobytes() and stats.tobytes() == stats2.tobytes(), "after remove_songs: not a fresh handle's answer"


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_both_outputs_untouched(torch_cuda):
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
    q = torch.as_tensor(db[:30]).cuda()
    rs = torch.zeros(1, dtype=torch.int64).cuda()
    rl = torch.full((1,), 30, dtype=torch.int32).cuda()

    def call(idx, window, hop, null_stats=False):
        nW = int(mc.wfirst_of([30], max(window, 1), max(hop, 1))[-1])
        wf = torch.as_tensor(np.asarray([0, nW], np.int64)).cuda()
        res = torch.full((max(nW, 1) * ctypes.sizeof(L.MatchResult),), 0xA5, dtype=torch.uint8).cuda()
        stats = torch.full((max(nW, 1) * 24,), 0xA5, dtype=torch.uint8).cuda()
        rc = lib.pfann_match_windows_dense_stats(idx.handle, q.data_ptr(), rs.data_ptr(), rl.data_ptr(), 1, window, hop, wf.data_ptr(),
                                                 nW, None, res.data_ptr(), None if null_stats else stats.data_ptr(), None)
        msg = L.last_error()
        torch.cuda.synchronize()
        return rc, msg, bool((res.cpu() == 0xA5).all()), bool((stats.cpu() == 0xA5).all())

    rc, _, res_untouched, stats_untouched = call(whole, 5, 1)        # the control: the same call on a good handle writes both
    assert rc == 0 and not res_untouched and not stats_untouched
    for idx, window, hop, null_stats, word in ((shard, 5, 1, False, "shard"), (half, 5, 1, False, "fp16"), (whole, 0, 1, False, "window"),
                                               (whole, 65, 1, False, "window"), (whole, 5, 0, False, "hop"), (whole, 5, 1, True, "stats_dev"),
                                               (shard, 65, 1, False, "shard")):  # two refusals at once: the first one is reported
        rc, msg, res_untouched, stats_untouched = call(idx, window, hop, null_stats)
        assert rc == -1 and word in msg and res_untouched and stats_untouched, (window, hop, word, rc, msg, res_untouched, stats_untouched)
    with pytest.raises(L.PfannError, match="shard"):
        shard.match_windows_dense_stats(q, [0], [30], 5, 1)
    try:
        shard.match_windows_dense(q, [0], [30], 5, 1)
    except L.PfannError as e:
        plain = str(e).split(": ", 1)[1]
    assert call(shard, 5, 1)[1] == plain, "a shard is refused with another message than pfann_match_windows_dense's"


# ------------------------------------------------------------------------------------------------ end to end
def _run(tmp_path, cmd):
    env = dict(os.environ, PYTHONPATH=REPO)
    r = subprocess.run(["timeout", "-k", "10", "400", sys.executable, os.path.join(REPO, cmd[0])] + cmd[1:],
                       capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=460)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


MAX_FA = "9.86e-3"                                      # log10: -2.006, see the docstring below


def test_monitor_cli_max_fa_finds_four_excerpts(tmp_path):
    """the scenario of test_gpu_dense.py::test_monitor_cli_dense_finds_four_excerpts, builder.py once, then monitor.py --dense and
    monitor.py --dense --max-fa X (with --min-score 0.99, which must not be consulted).
    X from the float64 oracle's rows on the CPU (totals rounded to float32, window 19, hop 2, 171 long windows): the least
    significant of the 74 windows wholly inside an excerpt has log10_fa -3.084, the most significant of the 25 windows wholly in
    noise -0.928; X = 10^-2.006 lies halfway in log10.  With it the oracle's rows merge into (11.0, 47.0, 4.0), (57.0, 88.0, 0.0),
    (100.5, 126.5, 11.5), (134.0, 153.5, 19.0), min_log10_fa -8.9 / -7.1 / -6.4 / -9.2: the detections of the fixed --min-score.
    Asserted: those four detections within that test's 1.5 s, the ninth column at or below log10 X, every window inside an excerpt
    names its song at or below log10 X, the seventh column of the windows file, its first six equal to --dense's; and without
    the flag the files keep the columns and the header that test pins."""
    from pfann_amd.monitor import DEFAULT_HOP, default_window
    params, mdir, music, truth = dc.four_excerpts(tmp_path)
    db = str(tmp_path / "db")
    recs = str(tmp_path / "recs.txt")
    _run(tmp_path, ["builder.py", str(tmp_path / "music.txt"), db, mdir])
    _run(tmp_path, ["monitor.py", recs, db, str(tmp_path / "dense.tsv"), "--dense"])
    _run(tmp_path, ["monitor.py", recs, db, str(tmp_path / "fa.tsv"), "--dense", "--max-fa", MAX_FA, "--min-score", "0.99"])
    lines = [x.split("\t") for x in open(str(tmp_path / "fa.tsv")).read().splitlines()]
    assert lines[-1] == [str(tmp_path / "missing.wav"), "error"]
    det = lines[:-1]
    print("detections:\n" + "\n".join("  " + "  ".join(x[1:]) for x in det))
    window, hop_size = default_window(params), params["hop_size"]
    tol = hop_size + DEFAULT_HOP * hop_size
    assert len(det) == 4, "%d detections" % len(det)
    for x, (t0, t1, s, o) in zip(det, truth):
        assert len(x) == 9 and x[0] == str(tmp_path / "rec.wav") and x[3] == music[s], (x, s)
        assert float(x[1]) < t1 and float(x[2]) > t0, ("a detection inside a noise gap", x)
        assert abs(float(x[1]) - t0) <= tol and abs(float(x[2]) - t1) <= tol and abs(float(x[4]) - o) <= tol, (x, t0, t1, o)
        assert float(x[8]) <= math.log10(float(MAX_FA)), ("min_log10_fa above the threshold", x)
    fa = list(csv.reader(open(str(tmp_path / "fa_windows.csv"))))
    dense = list(csv.reader(open(str(tmp_path / "dense_windows.csv"))))
    assert fa[0] == ["recording", "w0", "start_s", "song", "score", "time", "log10_fa"] and fa[-1][1] == "error" and len(fa[-1]) == 7
    # without the flag: the files of the parent commit, columns and header as test_monitor_cli_dense_finds_four_excerpts pins them
    assert dense[0] == ["recording", "w0", "start_s", "song", "score", "time"] and all(len(g) == 6 for g in dense)
    plain = [x.split("\t") for x in open(str(tmp_path / "dense.tsv")).read().splitlines()]
    assert len(plain) == 5 and all(len(x) == 8 for x in plain[:-1]) and plain[-1] == lines[-1]
    assert [g[:6] for g in fa[1:-1]] == dense[1:-1] and len(dense) > 150, "the six columns of --dense changed under --max-fa"
    inside = 0
    for g in fa[1:-1]:
        assert len(g) == 7 and float(g[6]) <= 0.0, g
        start, end = float(g[2]), float(g[2]) + (window - 1) * hop_size + params["segment_size"]
        for t0, t1, s, o in truth:
            if t0 <= start and end <= t1:
                inside += 1
                assert g[3] == music[s] and float(g[6]) <= math.log10(float(MAX_FA)), ("a window inside an excerpt", g, s)
    assert inside == 74, inside
