"""The dense matcher on the GPU (pfann_match_windows_dense, csrc/dense.hip): every alignment of every window against the
float64 oracle of tests/dense_cases.py -- `==` on the exact grid, the tolerances of tests/test_gpu_monitor.py's parity check
on real-valued rows --, the byte contract, the exclusion, the refusals, and monitor.py / Database.self_match with it."""
import csv
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import dense_cases as dc
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


def _dense(torch, idx, q, rstart, rlen, window, hop, **kw):
    return idx.match_windows_dense(torch.as_tensor(q).cuda(), rstart, rlen, window, hop, **kw)


# ------------------------------------------------------------------------------------------------ exact arithmetic
def _grid_world(d, seed=300):
    world = mx.std_world(41, d, long_rows=300)
    db, pos, q, _, rstart, rlen = mc.grid_recordings(d, 20, world=world, seed=seed)
    return db, pos, q, rstart, rlen


@pytest.mark.parametrize("window", mc.WINDOWS)
def test_every_window_equals_the_dense_oracle(torch_cuda, window):
    """songs of 300 rows (longer than a tile) and songs shorter than the window, copies and periodic songs (exact ties), an
    11-row recording, an empty one, recordings of up to 300 rows; windows 1 / 5 / 19 / 64 x hops 1 / 2 / 7: every field =="""
    db, pos, q, rstart, rlen = _grid_world(D)
    assert np.diff(pos).max() == 300 > 128 and 0 < np.diff(pos)[np.diff(pos) > 0].min() < 5 and 11 in rlen and 0 in rlen
    mx.assert_exact_domain(window, D)
    idx = _index("grid", db, pos)
    for hop in mc.HOPS:
        want = dc.dense_oracle(q, db, pos, window, hop, rstart, rlen, key="grid")
        res, wfirst = _dense(torch_cuda, idx, q, rstart, rlen, window, hop)
        assert np.array_equal(wfirst, mc.wfirst_of(rlen, window, hop)) and res.shape[0] == len(want) > 0
        bad = mc.differing(res, want)
        assert not bad, "window %d hop %d: %d of %d windows differ\n%s" % (window, hop, len(bad), len(want), "\n".join(bad[:6]))
    if window == 19:
        ties = sum(1 for w in dc.dense_oracle(q, db, pos, 19, 1, rstart, rlen, key="grid")
                   if len(w["top"]) > 1 and w["top"][0][3] == w["top"][1][3])
        assert ties > 0, "the recordings no longer hold exact ties at the top"


@pytest.mark.parametrize("d", [64, 256])
def test_other_row_widths(torch_cuda, d):
    db, pos, q, rstart, rlen = _grid_world(d, seed=340)
    mx.assert_exact_domain(19, d)
    for hop in (1, 3):
        want = dc.dense_oracle(q, db, pos, 19, hop, rstart, rlen, key=("grid-d", d))
        res, _ = _dense(torch_cuda, _index(("grid-d", d), db, pos), q, rstart, rlen, 19, hop)
        bad = mc.differing(res, want)
        assert not bad, "d %d hop %d: %d of %d windows differ\n%s" % (d, hop, len(bad), len(want), "\n".join(bad[:6]))


def test_equals_the_matcher_with_every_row_as_a_label(torch_cuda):
    """the product's own matcher on the expanded windows, labels = all rows, k = ntotal (3,800 candidates per window, inside
    the in-LDS list): every field =="""
    db, pos, q, rstart, rlen = dc.small_world()
    window = 19
    assert window * db.shape[0] <= mx.MAXC
    idx = _index("small", db, pos)
    labels = dc.all_labels(q.shape[0], db.shape[0])
    for hop in (1, 2):
        res, _ = _dense(torch_cuda, idx, q, rstart, rlen, window, hop)
        qs, ql = mc.expand(rstart, rlen, window, hop)
        ref, _ = idx.match(torch_cuda.as_tensor(q).cuda(), torch_cuda.as_tensor(labels).cuda(), qs, ql)
        for f in ("song", "offset", "shift", "n_cand", "score"):
            assert np.array_equal(res[f], ref[f]), "hop %d: field %s differs in %d windows" % (hop, f, int((res[f] != ref[f]).sum()))


# ------------------------------------------------------------------------------------------------ real-valued rows
@pytest.fixture(scope="module")
def unit400():
    return mc.unit_case(7, 120, D, 100, 400)


def test_real_valued_rows(torch_cuda, unit400):
    """the kernel's pick re-scored in float64 within 2e-6 of the oracle's best, the reported score within 1e-6 of the float64
    score of the pick, and every dense score >= the nominated matcher's for the same window - 1e-6 (its candidates are a subset)"""
    db, pos, q, labels = unit400
    window, hop, L = 19, 2, q.shape[0]
    idx = _index("unit400", db, pos)
    res, _ = _dense(torch_cuda, idx, q, [0], [L], window, hop)
    want = dc.dense_oracle(q, db, pos, window, hop, [0], [L], key="unit400")
    nom, _ = idx.match_windows(torch_cuda.as_tensor(q).cuda(), torch_cuda.as_tensor(labels).cuda(), [0], [L], window, hop)
    qs, ql = mc.expand([0], [L], window, hop)
    assert len(res) == len(want) == len(nom) == len(qs) > 100
    worst_pick = worst_score = 0.0
    for j, (s, n) in enumerate(zip(qs, ql)):
        r = res[j]
        assert int(r["song"]) >= 0 and int(r["n_cand"]) == want[j]["n_cand"], j
        mine = mc.score64(db, pos, q[s:s + n], int(r["song"]), int(r["offset"]))
        worst_pick = max(worst_pick, want[j]["score"] - mine)
        worst_score = max(worst_score, abs(float(r["score"]) - mine))
        assert want[j]["score"] - mine <= 2e-6, (j, want[j]["score"], mine)
        assert abs(float(r["score"]) - mine) <= 1e-6, (j, float(r["score"]), mine)
        assert float(r["score"]) >= float(nom[j]["score"]) - 1e-6, (j, float(r["score"]), float(nom[j]["score"]))
    print("unit400: %d windows, oracle best - kernel's pick <= %.3g, |score - float64| <= %.3g" % (len(qs), worst_pick, worst_score))


def test_a_window_has_the_same_bytes_whatever_reached_it(torch_cuda, unit400):
    """hop 1 against hops 3 and 7, alone and batched behind a second recording of 137 rows, twice in a row"""
    db, pos, q, _ = unit400
    window, L, other = 19, q.shape[0], 137
    idx = _index("unit400", db, pos)
    h1, _ = _dense(torch_cuda, idx, q, [0], [L], window, 1)
    again, _ = _dense(torch_cuda, idx, q, [0], [L], window, 1)
    assert h1.tobytes() == again.tobytes(), "two runs, other bytes"
    q2 = np.concatenate([q[:other][::-1], q])
    for hop in (3, 7):
        h, _ = _dense(torch_cuda, idx, q, [0], [L], window, hop)
        assert h1[::hop].tobytes() == h.tobytes(), "%d windows differ between hop 1 and hop %d" % (int((h1[::hop] != h).sum()), hop)
        b, wf = _dense(torch_cuda, idx, q2, [0, other], [other, L], window, hop)
        assert b[wf[1]:].tobytes() == h.tobytes(), "batched behind another recording at hop %d: other bytes" % hop
    b1, wf = _dense(torch_cuda, idx, q2, [0, other], [other, L], window, 1)
    assert b1[wf[1]:].tobytes() == h1.tobytes(), "batched behind another recording: other bytes"
    assert len({float(x) for x in h1["score"]}) > len(h1) // 2, "the scores are not real-valued"


# ------------------------------------------------------------------------------------------------ exclusion
def test_excluded_song(torch_cuda):
    db, pos, _, _, _ = _grid_world(D)
    A = int(np.flatnonzero(np.diff(pos) == 300)[0])
    cut = db[pos[A] + 40:pos[A] + 150]
    q = np.concatenate([cut, cut])
    rstart, rlen, excl = [0, cut.shape[0]], [cut.shape[0]] * 2, [A, -1]
    idx = _index("grid", db, pos)
    for window, hop in ((19, 2), (5, 1), (64, 7)):
        res, _ = _dense(torch_cuda, idx, q, rstart, rlen, window, hop, exclude_song=excl)
        want = dc.dense_oracle(q, db, pos, window, hop, rstart, rlen, excl=excl)
        bad = mc.differing(res, want)
        assert not bad, "window %d hop %d: %d windows differ\n%s" % (window, hop, len(bad), "\n".join(bad[:6]))
        half = len(res) // 2
        assert (res["song"][:half] != A).all() and (res["song"][half:] == A).all()
        assert (res["n_cand"][half:] - res["n_cand"][:half] == 300 + window - 1).all()
        none, _ = _dense(torch_cuda, idx, q, rstart, rlen, window, hop)
        minus, _ = _dense(torch_cuda, idx, q, rstart, rlen, window, hop, exclude_song=[-1, -1])
        assert none.tobytes() == minus.tobytes(), "NULL and all -1 give different bytes"
        assert none[half:].tobytes() == res[half:].tobytes()
    one = _index("one-song", cut, np.asarray([0, cut.shape[0]], np.int64))
    res, _ = _dense(torch_cuda, one, q, rstart, rlen, 19, 2, exclude_song=[0, 0])
    assert len(res) > 0 and not mc.differing(res, [dc.NONE] * len(res))
    res, _ = _dense(torch_cuda, one, q, rstart, rlen, 19, 2)
    assert (res["song"] == 0).all() and (res["offset"] == 2 * np.tile(np.arange(len(res) // 2), 2)).all()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_results_untouched(torch_cuda):
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

    def call(idx, window, hop):
        nW = int(mc.wfirst_of([30], max(window, 1), max(hop, 1))[-1])
        wf = torch.as_tensor(np.asarray([0, nW], np.int64)).cuda()
        res = torch.full((max(nW, 1) * ctypes.sizeof(L.MatchResult),), 0xA5, dtype=torch.uint8).cuda()
        rc = lib.pfann_match_windows_dense(idx.handle, q.data_ptr(), rs.data_ptr(), rl.data_ptr(), 1, window, hop, wf.data_ptr(),
                                           nW, None, res.data_ptr(), None)
        msg = L.last_error()
        torch.cuda.synchronize()
        return rc, msg, bool((res.cpu() == 0xA5).all())

    rc, _, untouched = call(whole, 5, 1)                 # the control: the same call on a good handle writes
    assert rc == 0 and not untouched
    for idx, window, hop, word in ((shard, 5, 1, "shard"), (half, 5, 1, "fp16"), (whole, 0, 1, "window"), (whole, 65, 1, "window"),
                                   (whole, 5, 0, "hop"),
                                   (shard, 65, 1, "shard")):         # two refusals at once: the first one is reported
        rc, msg, untouched = call(idx, window, hop)
        assert rc == -1 and word in msg and untouched, (window, hop, word, rc, msg, untouched)
    with pytest.raises(L.PfannError, match="shard"):
        shard.match_windows_dense(q, [0], [30], 5, 1)
    try:
        shard.match_windows(q, torch.zeros((30, 4), dtype=torch.int64).cuda(), [0], [30], 5, 1)
    except L.PfannError as e:
        nominated = str(e).split(": ", 1)[1]
    assert call(shard, 5, 1)[1] == nominated, "a shard is refused with another message than pfann_match_windows'"


def test_database_methods_refuse_what_the_dense_form_does_not_define(torch_cuda, tmp_path, monkeypatch):
    from pfann_amd import database as dbm
    from pfann_amd import lib as L
    from pfann_amd.utils import read_config
    dc.selfmatch_world(str(tmp_path))
    cfg = read_config(os.path.join(str(tmp_path), "configs.json"))
    emb = torch_cuda.zeros((30, D)).cuda()
    for change, word in (({"frame_shift_mul": 2}, "frame_shift_mul"), ({"score_alpha": 2.0}, "score_alpha")):
        db = dbm.Database(str(tmp_path), dict(cfg["indexer"], **change), cfg["hop_size"], d=D)
        with pytest.raises(L.PfannError, match=word):
            db.monitor_dense_launch(emb, [0], [30], 19, 2)
        with pytest.raises(L.PfannError, match=word):
            db.self_match_launch(0, 12, 19, 2, dense=True)
    db = dbm.Database(str(tmp_path), cfg["indexer"], cfg["hop_size"], d=D)
    monkeypatch.setattr(dbm, "cpp_accelerate", True)
    with pytest.raises(L.PfannError, match="native"):
        db.monitor_dense_launch(emb, [0], [30], 19, 2)
    with pytest.raises(L.PfannError, match="native"):
        list(db.self_match(0, 12, 19, 2, dense=True))


# ------------------------------------------------------------------------------------------------ end to end
def _run(tmp_path, cmd):
    env = dict(os.environ, PYTHONPATH=REPO)
    r = subprocess.run(["timeout", "-k", "10", "400", sys.executable, os.path.join(REPO, cmd[0])] + cmd[1:],
                       capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=460)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def test_monitor_cli_dense_finds_four_excerpts(tmp_path):
    """the scenario of test_monitor_cli_finds_four_excerpts, builder.py once, then monitor.py and monitor.py --dense on the same
    database: the dense run has exactly four detections, the right songs, nothing inside a noise gap, edges and song offsets
    within that test's 1.5 s; every window inside an excerpt names the true song; every dense window score >= the
    nominated run's - 1e-6.  (From the oracle's rows, on the CPU: the dense path gives (11.0, 47.0, 4.0), (57.0, 88.0, 0.0),
    (100.5, 126.5, 11.5), (134.0, 153.5, 19.0), the places the nominated path gives, and all 171 long windows are identical.)"""
    from pfann_amd.monitor import DEFAULT_HOP, default_window
    params, mdir, music, truth = dc.four_excerpts(tmp_path)
    db = str(tmp_path / "db")
    recs = str(tmp_path / "recs.txt")
    _run(tmp_path, ["builder.py", str(tmp_path / "music.txt"), db, mdir])
    _run(tmp_path, ["monitor.py", recs, db, str(tmp_path / "nom.tsv")])
    _run(tmp_path, ["monitor.py", recs, db, str(tmp_path / "dense.tsv"), "--dense"])
    lines = [x.split("\t") for x in open(str(tmp_path / "dense.tsv")).read().splitlines()]
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
    assert dense[0] == nom[0] == ["recording", "w0", "start_s", "song", "score", "time"] and dense[-1][1] == nom[-1][1] == "error"
    dense, nom = dense[1:-1], nom[1:-1]
    assert len(dense) == len(nom) > 150 and [g[:3] for g in dense] == [g[:3] for g in nom]
    inside = 0
    for g, h in zip(dense, nom):
        assert float(g[4]) >= float(h[4]) - 1e-6, (g, h)
        start, end = float(g[2]), float(g[2]) + (window - 1) * hop_size + params["segment_size"]
        for t0, t1, s, o in truth:
            if t0 <= start and end <= t1:
                inside += 1
                assert g[3] == music[s], ("a window inside an excerpt names another song", g, s)
    assert inside == 74, inside


# ------------------------------------------------------------------------------------------------ self-match
def test_self_match_dense_reports_the_planted_pairs(torch_cuda, tmp_path):
    from pfann_amd.database import Database
    from pfann_amd.monitor import merge_windows
    from pfann_amd.utils import read_config
    emb, pos = dc.selfmatch_world(str(tmp_path))
    cfg = read_config(os.path.join(str(tmp_path), "configs.json"))
    db = Database(str(tmp_path), cfg["indexer"], cfg["hop_size"], d=cfg["model"]["d"])

    def pairs(dense):
        out, rows_of = set(), {}
        for s, rows in db.self_match(0, 12, dc.SELF_WINDOW, dc.SELF_HOP, max_rows=150, dense=dense):
            rows_of[s] = rows
            n = int(pos[s + 1] - pos[s])
            for det in merge_windows(rows, min(dc.SELF_WINDOW, n) if n else dc.SELF_WINDOW, dc.SELF_HOP, dc.SELF_HOP_S, min_windows=2):
                out.add((s, int(det[2])))
        return out, rows_of
    nominated, _ = pairs(False)
    dense, rows_of = pairs(True)
    assert {(7, 2), (2, 7), (9, 4), (4, 9)} <= nominated <= dense, (sorted(nominated), sorted(dense))
    assert sorted(rows_of) == list(range(12)) and len(rows_of[5]) == 0
    for s, rows in rows_of.items():
        assert (rows["song"] != s).all() and (len(rows) == 0 or (rows["song"] >= 0).all()), s
    assert (rows_of[7]["song"] == 2).all() and (rows_of[2]["song"] == 7).all() and rows_of[7]["score"].min() > 0.99
    # the windows against the oracle with the song's own alignments excluded: the pick within 2e-6, the score within 1e-6
    rlen = np.diff(pos)
    want = dc.dense_oracle(emb, emb, pos, dc.SELF_WINDOW, dc.SELF_HOP, pos[:-1], rlen, excl=list(range(12)))
    got = [r for s in range(12) for r in rows_of[s]]
    qs, ql = mc.expand(pos[:-1], rlen, dc.SELF_WINDOW, dc.SELF_HOP)
    assert len(got) == len(want) == len(qs)
    for j, (s, n) in enumerate(zip(qs, ql)):
        mine = mc.score64(emb, pos, emb[s:s + n], int(got[j]["song"]), int(round(float(got[j]["time_s"]) / dc.SELF_HOP_S)))
        assert want[j]["score"] - mine <= 2e-6 and abs(float(got[j]["score"]) - mine) <= 1e-6, (j, want[j]["score"], mine, got[j])
