"""matcher.py --top N / --no-bin end to end, on a small synthetic dataset (tiny config, 12 songs, 12 queries and one
unreadable file): the flags change none of the existing outputs, rank 1 of `_top.csv` is the `_detail.csv` answer, the later
ranks are the host-side ranking of the `.bin` rows, and --no-bin writes the same `_top.csv` without a `.bin`."""
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
TOP = 5


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """builder once, then the matcher three times: plain, --top 5, --top 5 --no-bin.  -> (result paths, song list)"""
    import torch
    tmp = tmp_path_factory.mktemp("cli_topn")
    params = json.load(open(os.path.join(REPO, "configs", "tiny.json")))
    sd = synth.make_state_dict(params, seed=11)
    mdir = tmp / "model"
    mdir.mkdir()
    torch.save({n: torch.from_numpy(v) for n, v in sd.items()}, str(mdir / "model.pt"))
    shutil.copy(os.path.join(REPO, "configs", "tiny.json"), str(mdir / "configs.json"))
    env = dict(os.environ, PYTHONPATH=REPO)
    data = str(tmp / "data")

    def run(*cmd):
        r = subprocess.run([sys.executable] + list(cmd), capture_output=True, text=True, env=env, cwd=str(tmp), timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]

    run(os.path.join(REPO, "tools", "gen_synth_dataset.py"), data, "--songs", "12", "--queries", "12", "--seconds", "5",
        "--song-seconds", "12", "--snr", "0")
    qlist = os.path.join(data, "query_snr0", "list.txt")
    open(qlist, "a").write(os.path.join(data, "nope.wav") + "\n")
    db = str(tmp / "db")
    run(os.path.join(REPO, "builder.py"), os.path.join(data, "music.txt"), db, str(mdir))
    out = {}
    for name, flags in (("plain", []), ("top", ["--top", str(TOP)]), ("nobin", ["--top", str(TOP), "--no-bin"])):
        out[name] = str(tmp / (name + ".txt"))
        run(os.path.join(REPO, "matcher.py"), qlist, db, out[name], *flags)
    songs = [ln.rstrip("\n") for ln in open(os.path.join(db, "songList.txt"), encoding="utf8")]
    return out, songs


def _stem(p):
    return os.path.splitext(p)[0]


def _rows(path):
    with open(path, encoding="utf8", newline="") as f:
        return list(csv.reader(f))


def test_top_changes_none_of_the_existing_outputs(runs):
    out, _ = runs
    for a, b in ((out["plain"], out["top"]), (_stem(out["plain"]) + "_detail.csv", _stem(out["top"]) + "_detail.csv"),
                 (out["plain"] + ".bin", out["top"] + ".bin")):
        assert open(a, "rb").read() == open(b, "rb").read(), (a, b)
    assert not os.path.exists(_stem(out["plain"]) + "_top.csv")


def test_rank_1_is_the_detail_answer(runs):
    out, _ = runs
    top = _rows(_stem(out["top"]) + "_top.csv")
    detail = _rows(_stem(out["top"]) + "_detail.csv")
    assert top[0] == ["query", "rank", "answer", "score", "time"]
    first = [r for r in top[1:] if r[1] == "1"]
    assert len(first) == len(detail) - 1 == 13
    for t, d in zip(first, detail[1:]):
        assert [t[0], t[2], t[3], t[4]] == d[:4], (t, d)
    assert first[-1][2:] == ["error", "-inf", "0"] and sum(1 for r in top[1:] if r[0] == first[-1][0]) == 1
    for name in {r[0] for r in top[1:]}:
        ranks = [int(r[1]) for r in top[1:] if r[0] == name]
        assert ranks == list(range(1, len(ranks) + 1)) and len(ranks) <= TOP


def test_later_ranks_are_the_ranking_of_the_bin_rows(runs):
    """python path: a song's `.bin` slot is float32(score) when that is > 0 (else 0), so the positive float32 scores of a
    query's ranked rows are the largest slots of its block, in order, each in its own song's slot"""
    out, songs = runs
    top = _rows(_stem(out["top"]) + "_top.csv")[1:]
    names = [r[0] for r in _rows(_stem(out["top"]) + "_detail.csv")[1:]]
    blocks = np.fromfile(out["top"] + ".bin", dtype=np.float32).reshape(len(names), len(songs), 2)
    checked = 0
    for j, name in enumerate(names[:-1]):
        rows = [r for r in top if r[0] == name]
        s32 = np.array([np.float32(float(r[3])) for r in rows], np.float32)
        n_pos = int((s32 > 0).sum())
        assert (s32[:n_pos] > 0).all()                                         # ranked: the positive ones come first
        slots = np.sort(blocks[j, :, 0])[::-1]
        assert n_pos == min(TOP, int((slots > 0).sum())), (name, rows)
        assert np.array_equal(s32[:n_pos], slots[:n_pos]), (name, rows)
        for r, s in zip(rows[:n_pos], s32):
            assert blocks[j, songs.index(r[2]), 0] == s, (name, r)
        checked += max(0, n_pos - 1)
    assert checked > 0, "no later rank with a positive score: the comparison was empty"


def test_no_bin_writes_the_same_top_without_a_bin(runs):
    out, _ = runs
    assert not os.path.exists(out["nobin"] + ".bin")
    assert open(_stem(out["nobin"]) + "_top.csv", "rb").read() == open(_stem(out["top"]) + "_top.csv", "rb").read()
    for suffix in ("", ):
        assert open(out["nobin"] + suffix, "rb").read() == open(out["top"] + suffix, "rb").read()
    assert open(_stem(out["nobin"]) + "_detail.csv", "rb").read() == open(_stem(out["top"]) + "_detail.csv", "rb").read()
