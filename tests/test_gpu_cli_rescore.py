"""matcher.py --rescore N end to end, on the small synthetic dataset of tests/test_gpu_cli_topn.py (tiny config, 12 songs, 12
queries and one unreadable file): the TSV, `_detail.csv` and `_top.csv` come from Database.query_rescore_batch's lists, no `.bin`
is written, the unreadable query keeps its error rows, and without the flag every output is what it was."""
import csv
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from pfann_amd import synth

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, TOP = 8, 3


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """builder once, then the matcher: plain, --no-bin --top 3, and --rescore 8 --no-bin --top 3.  -> (result paths, query list,
    database dir)"""
    import torch
    tmp = tmp_path_factory.mktemp("cli_rescore")
    params = json.load(open(os.path.join(REPO, "configs", "tiny.json")))
    sd = synth.make_state_dict(params, seed=11)
    mdir = tmp / "model"
    mdir.mkdir()
    torch.save({n: torch.from_numpy(v) for n, v in sd.items()}, str(mdir / "model.pt"))
    shutil.copy(os.path.join(REPO, "configs", "tiny.json"), str(mdir / "configs.json"))
    env = dict(os.environ, PYTHONPATH=REPO)
    data = str(tmp / "data")

    def run(*cmd):
        r = subprocess.run(["timeout", "-k", "10", "400", sys.executable] + list(cmd), capture_output=True, text=True, env=env,
                           cwd=str(tmp), timeout=460)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        return r

    run(os.path.join(REPO, "tools", "gen_synth_dataset.py"), data, "--songs", "12", "--queries", "12", "--seconds", "5",
        "--song-seconds", "12", "--snr", "0")
    qlist = os.path.join(data, "query_snr0", "list.txt")
    open(qlist, "a").write(os.path.join(data, "nope.wav") + "\n")
    db = str(tmp / "db")
    run(os.path.join(REPO, "builder.py"), os.path.join(data, "music.txt"), db, str(mdir))
    out = {}
    for name, flags in (("plain", []), ("nobin", ["--no-bin", "--top", str(TOP)]),
                        ("rescore", ["--rescore", str(N), "--no-bin", "--top", str(TOP)])):
        out[name] = str(tmp / (name + ".txt"))
        run(os.path.join(REPO, "matcher.py"), qlist, db, out[name], *flags)
    return out, qlist, db


def _stem(p):
    return os.path.splitext(p)[0]


def _rows(path):
    with open(path, encoding="utf8", newline="") as f:
        return list(csv.reader(f))


def test_rescored_files_are_query_rescore_batchs_answers(runs):
    import torch
    from pfann_amd.builder import embed_files
    from pfann_amd.database import Database
    from pfann_amd.engine import Engine
    from pfann_amd.musicdata import MusicDataset
    out, qlist, dbdir = runs
    songs = [ln.rstrip("\n") for ln in open(os.path.join(dbdir, "songList.txt"), encoding="utf8")]
    tsv = [ln.rstrip("\n").split("\t") for ln in open(out["rescore"], encoding="utf8")]
    detail = _rows(_stem(out["rescore"]) + "_detail.csv")
    top = _rows(_stem(out["rescore"]) + "_top.csv")
    assert not os.path.exists(out["rescore"] + ".bin")
    assert detail[0] == ["query", "answer", "score", "time", "part_scores"] and top[0] == ["query", "rank", "answer", "score", "time"]
    assert len(tsv) == len(detail) - 1 == 13
    cfg = json.load(open(os.path.join(dbdir, "configs.json")))
    dataset = MusicDataset(qlist, cfg)
    engine = Engine(cfg, 0, max_batch=9728)
    engine.set_plan_batch(9728)
    if not engine.weights_loaded:
        engine.load_state_dict(torch.load(os.path.join(dbdir, "model.pt"), map_location="cpu"))
    embs = [(i, n, e) for i, n, e in embed_files(engine, dataset, dataset.hop, batch_windows=9728) if n]
    assert [i for i, _, _ in embs] == list(range(12)) and max(n for _, n, _ in embs) <= 64
    db = Database(dbdir, cfg["indexer"], cfg["hop_size"], d=cfg["model"]["d"])
    qlen = [n for _, n, _ in embs]
    qstart = np.concatenate([[0], np.cumsum(qlen)[:-1]])
    emb = torch.cat([e for _, _, e in embs])
    answers, ranked = db.query_rescore_batch(emb, qstart, qlen, N)
    dense_answers, _ = db.query_dense_batch(emb, qstart, qlen, n=1)
    nominated = db.query_topn_batch(emb, qstart, qlen, N)
    same_as_dense = 0
    for j, (score, (song, time_s), block) in enumerate(answers):
        name, ans, sco, tim = detail[1 + j][:4]
        assert block is None and name == tsv[j][0] and ans == tsv[j][1] == songs[song], (j, detail[1 + j], song)
        assert abs(float(sco) - score) <= 1e-6 and abs(float(tim) - time_s) <= 1e-6, (j, detail[1 + j], score, time_s)
        mine = [r for r in top[1:] if r[0] == name]
        assert [int(r[1]) for r in mine] == list(range(1, len(mine) + 1)) and 1 <= len(mine) == min(TOP, len(ranked[j]))
        assert [mine[0][0], mine[0][2], mine[0][3], mine[0][4]] == detail[1 + j][:4], "rank 1 is not the detail answer"
        for r, (sc, (sg, tm)) in zip(mine, ranked[j]):
            assert r[2] == songs[sg] and abs(float(r[3]) - sc) <= 1e-6 and abs(float(r[4]) - tm) <= 1e-6, (r, sc, sg, tm)
        assert score >= nominated[j][0][0] - 1e-6, "query %d: the rescored score is below the nominated one" % j
        if dense_answers[j][1][0] in {s for _, (s, _) in nominated[j]}:
            assert answers[j][:2] == dense_answers[j][:2], j
            same_as_dense += 1
    assert same_as_dense >= 6, "the dense answers' songs were hardly ever nominated: the comparison was nearly empty"


def test_unreadable_query_keeps_its_error_rows(runs):
    out, _, _ = runs
    tsv = [ln.rstrip("\n").split("\t") for ln in open(out["rescore"], encoding="utf8")]
    detail = _rows(_stem(out["rescore"]) + "_detail.csv")
    top = _rows(_stem(out["rescore"]) + "_top.csv")
    name = tsv[-1][0]
    assert name.endswith("nope.wav") and tsv[-1][1] == "error" and detail[-1] == [name, "error", "-inf", "0"]
    assert [r for r in top if r[0] == name] == [[name, "1", "error", "-inf", "0"]]
    plain_tsv = [ln.rstrip("\n").split("\t") for ln in open(out["plain"], encoding="utf8")]
    assert [r[0] for r in tsv] == [r[0] for r in plain_tsv]


def test_without_the_flag_every_output_is_what_it_was(runs):
    """the parent's flags only: --no-bin --top 3 writes the plain run's TSV and detail, its own _top.csv and no .bin"""
    out, _, _ = runs
    assert open(out["nobin"], "rb").read() == open(out["plain"], "rb").read()
    assert open(_stem(out["nobin"]) + "_detail.csv", "rb").read() == open(_stem(out["plain"]) + "_detail.csv", "rb").read()
    assert os.path.exists(out["plain"] + ".bin") and not os.path.exists(out["nobin"] + ".bin")
    assert not os.path.exists(_stem(out["plain"]) + "_top.csv")
    top = _rows(_stem(out["nobin"]) + "_top.csv")
    detail = _rows(_stem(out["nobin"]) + "_detail.csv")
    first = [r for r in top[1:] if r[1] == "1"]
    assert len(first) == len(detail) - 1 == 13
    for t, d in zip(first, detail[1:]):
        assert [t[0], t[2], t[3], t[4]] == d[:4], (t, d)
