"""The dense matcher as N ranks (2 and 3 ranks sharing this box's one GPU over gloo, as tests/test_gpu_ranks.py runs the other
sharded paths): `Database(.., ranks=)`'s dense methods are collective and return what the single process returns, and
`PFANN_GPUS=2 python monitor.py .. --dense --max-fa X` writes the single process's two files byte for byte."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from pfann_amd import synth

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(REPO, "tests")
DROP = ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PFANN_DIST_BACKEND", "PFANN_FORCE_DEVICE", "PFANN_GPUS", "PFANN_FORCE_SHARDED",
        "PFANN_EXCHANGE_STREAM")

WORKER = r'''
import json, os, pickle, sys
sys.path.insert(0, %(tests)r)
from pfann_amd.dist import self_launch_if_asked
rc = self_launch_if_asked(sys.argv)                 # PFANN_GPUS=N: N ranks of this script
if rc is not None:
    sys.exit(rc)
import numpy as np
import torch
import dense_cases as dc
from pfann_amd import lib as L
from pfann_amd.database import Database
from pfann_amd.dist import finish_ranks, init_ranks

dbdir, out = sys.argv[1], sys.argv[2]
ranks = init_ranks()
params = json.load(open(os.path.join(dbdir, "configs.json")))
db = Database(dbdir, params["indexer"], params["hop_size"], d=dc.SELF_D, ranks=ranks)
pos = db.song_pos
emb = np.fromfile(os.path.join(dbdir, "embeddings"), np.float32).reshape(-1, dc.SELF_D)
assert (ranks is not None and ranks.world > 1) == (db.index.ntotal < emb.shape[0])

# recordings: rows cut from the database plus noise (the same on every rank), one of them shorter than the window
rng = np.random.default_rng(31)
cuts = [np.r_[pos[2] + 3:pos[2] + 40, pos[10]:pos[10] + 25], np.r_[pos[9] + 5:pos[9] + 60], np.r_[pos[0] + 1:pos[0] + 8]]
rlen = [len(c) for c in cuts]
rstart = [int(x) for x in np.pad(np.cumsum(rlen), (1, 0))[:-1]]
q = emb[np.concatenate(cuts)] + 0.05 * rng.standard_normal((sum(rlen), dc.SELF_D))
q = torch.as_tensor((q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)).cuda()

got = {}
p = db.monitor_dense_launch(q, rstart, rlen, 19, 2, edge_window=7, stats=True)
rows, fa = db.monitor_dense_stats_finish(p)
got["stats rows"] = [r.tobytes() for r in rows]
got["stats log10_fa"] = [np.asarray(f).tobytes() for f in fa]
got["stats edge rows"] = [r.tobytes() for r in p["edge_rows"]]
got["songs named"] = sorted(set(int(s) for r in rows for s in r["song"]))
p = db.monitor_dense_launch(q, rstart, rlen, 19, 2)
got["plain rows"] = [r.tobytes() for r in db.monitor_finish(p)]
p = db.monitor_dense_topn_launch(q, rstart, rlen, 19, 2, 3, edge_window=7)
top, n_found = db.monitor_dense_topn_finish(p)
got["ranked rows"] = [r.tobytes() for r in top]
got["ranked n_found"] = [np.asarray(f).tobytes() for f in n_found]
got["ranked edge rows"] = [r.tobytes() for r in p["edge_rows"]]
qlen = [19, 5, 64, 1]
qstart = [0, 19, 30, rstart[2]]
got["query"] = repr(db.query_dense_batch(q, qstart, qlen, n=3))
if ranks is not None:
    refused = []
    for call in (lambda: db.query_dense_batch(q, qstart, qlen, n=3, want_song_scores=True),
                 lambda: list(db.self_match(0, 3, 19, 2, emb=emb, dense=True)),
                 lambda: db.monitor_launch(q, rstart, rlen, 19, 2)):
        try:
            call()
            refused.append(None)
        except L.PfannError as x:
            refused.append(str(x))
    got["refused"] = refused
if ranks is None or ranks.rank == 0:
    pickle.dump(got, open(out, "wb"))
finish_ranks(ranks)
'''


def _env(**kw):
    e = {k: v for k, v in os.environ.items() if k not in DROP}
    e.update(PYTHONPATH=REPO, MASTER_ADDR="127.0.0.1")
    e.update(kw)
    return e


def _ranks(n, **kw):
    return _env(PFANN_GPUS=str(n), PFANN_DIST_BACKEND="gloo", PFANN_FORCE_DEVICE="0", **kw)


def _run(cmd, cwd, env, seconds=300, status=0):
    """every subprocess under its own time limit; the test stops at the first unexpected status"""
    r = subprocess.run(["timeout", "-k", "10", str(seconds)] + cmd, capture_output=True, text=True, env=env, cwd=cwd)
    assert r.returncode == status, "status %d: %s\n%s%s" % (r.returncode, " ".join(cmd), r.stdout[-3000:], r.stderr[-4000:])
    return r


def test_database_dense_methods_are_collective_and_equal_one_process(tmp_path):
    sys.path.insert(0, TESTS)
    import dense_cases as dc
    tmp = str(tmp_path)
    dbdir = os.path.join(tmp, "db")
    os.makedirs(dbdir)
    emb, pos = dc.selfmatch_world(dbdir)
    assert len(pos) - 1 == 12 and pos[6] == pos[5]
    worker = os.path.join(tmp, "worker.py")
    open(worker, "w").write(WORKER % {"tests": TESTS})
    outs = {}
    for n in (1, 2, 3):
        outs[n] = os.path.join(tmp, "out%d.pkl" % n)
        _run([sys.executable, worker, dbdir, outs[n]], tmp, _env() if n == 1 else _ranks(n))
    one = pickle.load(open(outs[1], "rb"))
    assert {2, 7} & set(one["songs named"]) and len(one["stats rows"]) == 3 and all(len(x) > 0 for x in one["stats rows"])
    for n in (2, 3):
        got = pickle.load(open(outs[n], "rb"))
        refused = got.pop("refused")
        assert all(refused) and "want_song_scores" in refused[0] and "self_match" in refused[1] and "song-sharded" in refused[2], refused
        assert sorted(got) == sorted(one)
        for k in one:
            assert got[k] == one[k], "%d ranks: %s differs from the single process" % (n, k)


def test_monitor_cli_dense_two_ranks_byte_identical(tmp_path):
    """configs/tiny.json with seeded weights, five short songs, a recording of two excerpts, a short one and a missing file:
    only identity is asserted, so the tiny model's quality does not matter"""
    import torch
    tmp = str(tmp_path)
    params = json.load(open(os.path.join(REPO, "configs", "tiny.json")))
    sd = synth.make_state_dict(params, seed=9)
    mdir = os.path.join(tmp, "model")
    os.makedirs(mdir)
    torch.save({n: torch.from_numpy(np.asarray(v)) for n, v in sd.items()}, os.path.join(mdir, "model.pt"))
    json.dump(params, open(os.path.join(mdir, "configs.json"), "w"))
    songs, music = [], []
    for s in range(5):
        songs.append(synth.make_song(500 + s, seconds=9.0 + 2 * s))
        music.append(os.path.join(tmp, "m%d.wav" % s))
        synth.write_wav(music[-1], songs[-1])
    open(os.path.join(tmp, "music.txt"), "w").write("".join(p + "\n" for p in music))
    sr = 8000
    rec = np.concatenate([songs[1][2 * sr:9 * sr], songs[3][1 * sr:12 * sr]])
    synth.write_wav(os.path.join(tmp, "rec.wav"), rec)
    synth.write_wav(os.path.join(tmp, "short.wav"), songs[4][3 * sr:7 * sr])
    open(os.path.join(tmp, "recs.txt"), "w").write("".join(os.path.join(tmp, f) + "\n" for f in ("rec.wav", "missing.wav", "short.wav")))
    db = os.path.join(tmp, "db")
    tool = lambda name: [sys.executable, os.path.join(REPO, name)]
    _run(tool("builder.py") + [os.path.join(tmp, "music.txt"), db, mdir], tmp, _env())
    args = [os.path.join(tmp, "recs.txt"), db]
    r1, r2 = os.path.join(tmp, "r1.txt"), os.path.join(tmp, "r2.txt")
    _run(tool("monitor.py") + args + [r1, "--dense", "--max-fa", "1e-2"], tmp, _env())
    two = _run(tool("monitor.py") + args + [r2, "--dense", "--max-fa", "1e-2"], tmp, _ranks(2))
    assert two.stdout.count("monitor: 3 recordings") == 1              # rank 0 alone speaks
    for a, b in ((r1, r2), (r1[:-4] + "_windows.csv", r2[:-4] + "_windows.csv")):
        x, y = open(a, "rb").read(), open(b, "rb").read()
        assert len(x) > 0 and x == y, "%s and %s differ" % (a, b)
    # the header, the 18 s recording's 35 segments in windows of 19 at hop 2, the missing file's error row, the short recording's one
    assert len(open(r1[:-4] + "_windows.csv").readlines()) == 1 + ((35 - 19) // 2 + 1) + 1 + 1
    # without --dense several ranks are refused as before
    r = _run(tool("monitor.py") + args + [os.path.join(tmp, "r3.txt")], tmp, _ranks(2), status=2)
    assert "song-sharded multi-GPU monitor mode is not supported" in r.stderr and not os.path.exists(os.path.join(tmp, "r3.txt"))
