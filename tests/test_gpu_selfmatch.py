"""Self-match on the GPU: Database.self_match (the masked search + the windowed matcher) and the selfmatch.py CLI on a
database directory the test writes itself: 12 songs of 40..80 random unit rows, song 7 is song 2 under another name (plus
1e-3 noise), song 9 carries rows 10..40 of song 4 in its middle, song 5 has no rows."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import monitor_cases as mc
import search_excl_cases as sx

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, K, WINDOW, HOP, HOP_S = 128, 100, 19, 2, 0.5
MID = 17                                   # song 9's rows [MID, MID + 30) are song 4's rows [10, 40)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def dbdir(tmp_path_factory):
    rng = np.random.default_rng(2026)
    key = rng.integers(40, 81, 12)
    key[5] = 0
    key[7] = key[2]
    key[9] = max(int(key[9]), MID + 30 + 8)
    pos = np.pad(np.cumsum(key), (1, 0)).astype(np.int64)
    emb = rng.standard_normal((int(pos[-1]), D))
    emb[pos[7]:pos[8]] = emb[pos[2]:pos[3]] / np.linalg.norm(emb[pos[2]:pos[3]], axis=1, keepdims=True) \
        + 1e-3 * rng.standard_normal((int(key[2]), D))
    emb[pos[9] + MID:pos[9] + MID + 30] = emb[pos[4] + 10:pos[4] + 40]
    emb = (emb / np.linalg.norm(emb, axis=1, keepdims=True)).astype(np.float32)
    d = tmp_path_factory.mktemp("selfdb")
    shutil.copy(os.path.join(REPO, "configs", "default.json"), str(d / "configs.json"))
    with open(str(d / "songList.txt"), "w") as f:
        f.write("".join("song%02d.wav\n" % s for s in range(12)))
    key.astype(np.int32).tofile(str(d / "landmarkKey"))
    emb.tofile(str(d / "embeddings"))
    return str(d), emb, pos


def _database(dbdir):
    from pfann_amd.database import Database
    from pfann_amd.utils import read_config
    cfg = read_config(os.path.join(dbdir[0], "configs.json"))
    assert cfg["hop_size"] == HOP_S and cfg["indexer"]["top_k"] == K
    return Database(dbdir[0], cfg["indexer"], cfg["hop_size"], d=cfg["model"]["d"])


def test_windows_equal_the_masked_oracle_search_plus_the_window_oracle(torch_cuda, dbdir):
    """labels == the delete-the-rows oracle's (canonical scores: this storage re-scores), windows == the windowed matcher on
    the ORACLE's labels byte for byte, and every window against the float64 window oracle as tests/test_gpu_monitor.py's
    parity check has it (pick within 2e-6 of the oracle's best, score within 1e-6 of the float64 score of the pick)"""
    from oracle import seqscore as osq
    from pfann_amd.database import self_match_ranges
    _, emb, pos = dbdir
    db = _database(dbdir)
    assert db.index.search_plan(int(pos[-1]), K)[1]["canonical_scores"] == "1"
    rstart, rlen, lo, hi = self_match_ranges(pos, 0, 12)
    Dr, Ir = sx.masked_topk(emb, emb, K, lo, hi, "canonical")
    p = db.self_match_launch(0, 12, WINDOW, HOP)
    q_dev, I_dev = p["keep"]
    assert np.array_equal(I_dev.cpu().numpy(), Ir) and np.array_equal(q_dev.cpu().numpy(), emb)
    res = db.index.results_to_host(p["res"])
    want, wfirst = db.index.match_windows(torch_cuda.as_tensor(emb).cuda(), torch_cuda.as_tensor(Ir).cuda(), rstart, rlen, WINDOW, HOP)
    assert np.array_equal(p["wfirst"], wfirst) and np.array_equal(wfirst, mc.wfirst_of(rlen, WINDOW, HOP))
    assert wfirst[6] == wfirst[5], "the song without rows has windows"
    for f in ("song", "offset", "shift", "n_cand", "score"):
        assert np.array_equal(res[f], want[f]), f
    qs, ql = mc.expand(rstart, rlen, WINDOW, HOP)
    own = np.searchsorted(pos[:-1], qs, side="right") - 1
    for j, (s, n) in enumerate(zip(qs, ql)):
        best, (song, t), _ = osq.query_embeddings_base(emb[s:s + n], Ir[s:s + n], emb, pos, HOP_S)
        r = res[j]
        assert int(r["song"]) >= 0 and int(r["song"]) != own[j], j            # own-song rows cannot be nominated
        mine = mc.score64(emb, pos, emb[s:s + n], int(r["song"]), int(r["offset"]))
        assert float(best) - mine <= 2e-6 and abs(float(r["score"]) - mine) <= 1e-6, (j, float(best), mine, float(r["score"]))
    # the generator: song order, launch groups of a few songs, the same rows
    rows = dict(db.self_match(0, 12, WINDOW, HOP, max_rows=150))
    assert sorted(rows) == list(range(12)) and len(rows[5]) == 0
    one = db.self_match_finish(p)
    for s in range(12):
        assert rows[s].tobytes() == one[s].tobytes(), s
    assert (rows[7]["song"] == 2).all() and (rows[2]["song"] == 7).all() and rows[7]["score"].min() > 0.99


def _cli(dbdir, out, *extra):
    env = dict(os.environ, PYTHONPATH=REPO)
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(REPO, "selfmatch.py"), dbdir[0], out] + list(extra),
                       capture_output=True, text=True, env=env, timeout=150)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return [x.split("\t") for x in open(out).read().splitlines()]


def test_cli_finds_the_duplicate_and_the_containment(torch_cuda, dbdir, tmp_path):
    _, emb, pos = dbdir
    lines = _cli(dbdir, str(tmp_path / "out.tsv"))
    name = lambda s: "song%02d.wav" % s
    by = {}
    for f in lines:
        assert len(f) == 8
        by.setdefault((f[0], f[3]), []).append([float(x) for x in f[1:3] + f[4:7]] + [int(f[7])])
    assert set(by) == {(name(7), name(2)), (name(2), name(7)), (name(9), name(4)), (name(4), name(9))}, sorted(by)
    n2 = int(pos[3] - pos[2])
    for a, b in ((7, 2), (2, 7)):                        # whole-song detections, offset 0
        (d0, d1, s0, mean, best, nw), = by[(name(a), name(b))]
        assert d0 == 0.0 and abs(d1 - n2 * HOP_S) <= HOP * HOP_S and s0 == 0.0 and mean > 0.99 and nw == len(mc.window_starts(n2, WINDOW, HOP))
    (d0, d1, s0, mean, best, nw), = by[(name(9), name(4))]
    assert abs((s0 - d0) - (10 - MID) * HOP_S) < 1e-3            # the diagonal: row MID of song 9 is row 10 of song 4
    assert abs(d0 - MID * HOP_S) <= 2.0 and abs(d1 - (MID + 30) * HOP_S) <= 2.0 and best > 0.99
    (d0, d1, s0, mean, best, nw), = by[(name(4), name(9))]
    assert abs((s0 - d0) - (MID - 10) * HOP_S) < 1e-3 and best > 0.99
    win = open(str(tmp_path / "out_windows.csv")).read().splitlines()
    rlen = np.diff(pos)
    assert win[0] == "recording,w0,start_s,song,score,time" and len(win) - 1 == int(mc.wfirst_of(rlen, WINDOW, HOP)[-1])
    assert not [w for w in win[1:] if w.startswith(name(5))]
    # --songs limits the songs queried, not the songs searched
    only = _cli(dbdir, str(tmp_path / "only.tsv"), "--songs", "7:8")
    assert [f[0] for f in only] == [name(7)] and only[0][3] == name(2)
    assert only[0] == [f for f in lines if f[0] == name(7)][0]
