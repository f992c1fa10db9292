"""The host side of self-match (pfann_amd/selfmatch.py, the range helpers of pfann_amd/database.py): no GPU."""
import csv
import io
import json
import os
import shutil

import numpy as np
import pytest

from pfann_amd import selfmatch
from pfann_amd.database import self_match_groups, self_match_ranges, song_pos_from_key
from pfann_amd.monitor import DEFAULT_HOP, DEFAULT_MIN_SCORE, DEFAULT_MIN_WINDOWS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_arguments():
    a = selfmatch.parse_args(["selfmatch.py", "dbdir", "out.tsv"])
    assert (a.db, a.result, a.window, a.hop, a.min_score, a.min_windows, a.max_gap, a.songs, a.topk) == (
        "dbdir", "out.tsv", None, DEFAULT_HOP, DEFAULT_MIN_SCORE, DEFAULT_MIN_WINDOWS, 0, None, None)
    a = selfmatch.parse_args("selfmatch.py d o --window 7 --hop 3 --min-score 0.5 --min-windows 1 --max-gap 2 --songs 7:8 --topk 20".split())
    assert (a.window, a.hop, a.min_score, a.min_windows, a.max_gap, a.songs, a.topk) == (7, 3, 0.5, 1, 2, "7:8", 20)
    with pytest.raises(SystemExit):
        selfmatch.parse_args(["selfmatch.py", "only-one"])
    assert selfmatch.parse_songs(None, 12) == (0, 12) and selfmatch.parse_songs("7:8", 12) == (7, 8)
    assert selfmatch.parse_songs(":5", 12) == (0, 5) and selfmatch.parse_songs("5:", 12) == (5, 12)
    assert selfmatch.parse_songs("10:40", 12) == (10, 12) and selfmatch.parse_songs("3:3", 12) == (3, 3)
    for bad in ("7", "8:7", "-1:3", "a:b"):
        with pytest.raises(ValueError):
            selfmatch.parse_songs(bad, 12)
    assert selfmatch.main(["selfmatch.py", "d", "o", "--hop", "0"]) == 2
    assert selfmatch.main(["selfmatch.py", "d", "o", "--topk", "2000"]) == 2


def test_ranges_from_the_landmark_key():
    """song s is recording s - song_lo; every row leaves its own song out; 0-row songs have no rows and no range"""
    key = np.array([3, 0, 2, 0, 0, 4], np.int32)
    pos = song_pos_from_key(key)
    rstart, rlen, lo, hi = self_match_ranges(pos, 0, 6)
    assert rstart.tolist() == [0, 3, 3, 5, 5, 5] and rlen.tolist() == [3, 0, 2, 0, 0, 4]
    assert lo.tolist() == [0, 0, 0, 3, 3, 5, 5, 5, 5] and hi.tolist() == [3, 3, 3, 5, 5, 9, 9, 9, 9]
    assert lo.dtype == np.int64 and hi.dtype == np.int64 and rstart.dtype == np.int64 and rlen.dtype == np.int32
    rstart, rlen, lo, hi = self_match_ranges(pos, 2, 6)              # a later group: rstart counts from ITS first row,
    assert rstart.tolist() == [0, 2, 2, 2] and rlen.tolist() == [2, 0, 0, 4]
    assert lo.tolist() == [3, 3, 5, 5, 5, 5] and hi.tolist() == [5, 5, 9, 9, 9, 9]      # ... the ranges stay labels
    rstart, rlen, lo, hi = self_match_ranges(pos, 3, 5)              # only 0-row songs
    assert rlen.tolist() == [0, 0] and lo.size == 0 and hi.size == 0
    assert self_match_ranges(pos, 4, 4)[1].size == 0


def test_launch_groups():
    pos = song_pos_from_key(np.array([30, 0, 50, 200, 10, 0, 0, 70], np.int32))
    assert self_match_groups(pos, 0, 8, 100) == [(0, 3), (3, 4), (4, 8)]        # 80 rows | one song above the limit | 80 rows
    assert self_match_groups(pos, 0, 8, 10 ** 6) == [(0, 8)]
    assert self_match_groups(pos, 2, 5, 60) == [(2, 3), (3, 4), (4, 5)]
    assert self_match_groups(pos, 5, 5, 60) == []
    # a limit below every song: one song per group (songs without rows ride along with each other)
    assert self_match_groups(pos, 0, 8, 1) == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 7), (7, 8)]


def test_tsv_and_csv_lines():
    names = ["a.wav", "b.wav", "c.wav"]
    rows = np.zeros(6, dtype=[("w0", "<i8"), ("score", "<f8"), ("song", "<i8"), ("time_s", "<f8")])
    rows["w0"] = np.arange(6) * 2
    rows["song"] = [2, 2, 2, 2, -1, 1]
    rows["score"] = [0.9, 0.8, 0.85, 0.9, -np.inf, 0.05]
    rows["time_s"] = [5.0, 6.0, 7.0, 8.0, 0.0, 1.0]               # song c from second 5 on: one diagonal (hop_size 0.5)
    fout, fwin = io.StringIO(), io.StringIO()
    nw, nd = selfmatch.write_song(fout, csv.writer(fwin), "a.wav", rows, names, 4, 2, 0.5, 0.2, 0, 2)
    assert (nw, nd) == (6, 1)
    (line,) = fout.getvalue().splitlines()
    f = line.split("\t")
    assert f[0] == "a.wav" and f[3] == "c.wav" and f[7] == "4" and len(f) == 8
    assert float(f[1]) == 0.0 and float(f[2]) == 5.0 and float(f[4]) == 5.0          # rows 0..10 of a are c from 5 s on
    assert abs(float(f[5]) - 0.8625) < 1e-6 and float(f[6]) == 0.9
    win = list(csv.reader(io.StringIO(fwin.getvalue())))
    assert win[0] == ["a.wav", "0", "0.0", "c.wav", "0.9", "5.0"] and win[4][3] == "" and win[5][3] == "b.wav" and len(win) == 6
    assert selfmatch.detection_line("x", (1.0, 2.5, 1, 0.25, 0.5, 0.75, 3), names) == "x\t1.000\t2.500\tb.wav\t0.250\t0.500000\t0.750000\t3"
    # a song without rows: no windows, no lines
    fout, fwin = io.StringIO(), io.StringIO()
    assert selfmatch.write_song(fout, csv.writer(fwin), "a.wav", rows[:0], names, 19, 2, 0.5, 0.2, 0, 2) == (0, 0)
    assert fout.getvalue() == "" and fwin.getvalue() == ""


def test_the_cli_fails_loudly_without_a_gpu(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from pfann_amd import lib
    shutil.copy(os.path.join(REPO, "configs", "default.json"), str(tmp_path / "configs.json"))
    with pytest.raises(lib.PfannError):
        selfmatch.main(["selfmatch.py", str(tmp_path), str(tmp_path / "out.tsv")])
    assert json.load(open(str(tmp_path / "configs.json")))["indexer"]["top_k"] == 100
