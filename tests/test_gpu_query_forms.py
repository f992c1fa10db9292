"""The three query forms answer one query alike: query_batch, entry 0 of query_topn_batch and the monitor's row of a window
as long as the query are built from one formatter (pfann_amd.database.format_results), in both modes of the reference's
cpp_accelerate switch.  A database directory the test writes itself: 6 songs of 30..50 random unit rows, the tiny config."""
import json
import os
import shutil

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUERIES = [(1, 7, 1), (3, 0, 19), (4, 11, 25)]             # (song, first row in the song, rows)


@pytest.fixture(scope="module")
def database(tmp_path_factory):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from pfann_amd.database import Database
    cfg = json.load(open(os.path.join(REPO, "configs", "tiny.json")))
    rng = np.random.default_rng(18)
    key = rng.integers(30, 51, 6)
    pos = np.pad(np.cumsum(key), (1, 0)).astype(np.int64)
    emb = rng.standard_normal((int(pos[-1]), cfg["model"]["d"]))
    emb = (emb / np.linalg.norm(emb, axis=1, keepdims=True)).astype(np.float32)
    d = tmp_path_factory.mktemp("formsdb")
    shutil.copy(os.path.join(REPO, "configs", "tiny.json"), str(d / "configs.json"))
    (d / "songList.txt").write_text("".join("song%d.wav\n" % s for s in range(6)))
    key.astype(np.int32).tofile(str(d / "landmarkKey"))
    emb.tofile(str(d / "embeddings"))
    db = Database(str(d), cfg["indexer"], cfg["hop_size"], d=cfg["model"]["d"])
    assert db.top_k == cfg["indexer"]["top_k"] == 20 and db.frame_shift_mul == 1
    return db, emb, pos, torch


@pytest.mark.parametrize("cpp", [False, True])
def test_query_topn_and_monitor_answer_alike(database, monkeypatch, cpp):
    import pfann_amd.database as pdb
    db, emb, pos, torch = database
    monkeypatch.setattr(pdb, "cpp_accelerate", cpp)
    cuts = [emb[pos[s] + o:pos[s] + o + n] for s, o, n in QUERIES]
    q = torch.as_tensor(np.concatenate(cuts)).cuda()
    qlen = [n for _, _, n in QUERIES]
    qstart = np.concatenate([[0], np.cumsum(qlen)[:-1]])
    plain = db.query_batch(q, qstart, qlen)
    ranked = db.query_topn_batch(q, qstart, qlen, n=3)
    assert len(plain) == len(ranked) == 3
    for j, (s, o, n) in enumerate(QUERIES):
        p = db.monitor_launch(torch.as_tensor(cuts[j]).cuda(), [0], [n], n, 1)
        assert p["mode"] == (1 if cpp else 0)
        rows, = db.monitor_finish(p)
        assert len(rows) == 1 and int(rows[0]["w0"]) == 0
        window = (float(rows[0]["score"]), (int(rows[0]["song"]), float(rows[0]["time_s"])))
        score, (song, time_s) = plain[j][:2]
        assert plain[j][2] is None and 1 <= len(ranked[j]) <= 3
        for what, got in (("top-N entry 0", ranked[j][0]), ("monitor window", window)):
            assert got[0] == score and got[1][0] == song and got[1][1] == time_s, (cpp, j, what, got, plain[j][:2])
        # the query is rows of the database: its own song, where it was cut
        assert (song, time_s) == (s, o * db.hop_size) and score > 0, (cpp, j, plain[j][:2])
        assert (type(score), type(song), type(time_s)) == (float, int, float)
