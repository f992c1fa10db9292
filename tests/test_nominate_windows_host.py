"""Windowed dense nomination, the parts that need no GPU: database.window_queries against a loop written out here,
monitor.py's --nominate flag and its refusals, the rows of `<stem>_nominate.csv`, and the declaration in the public header."""
import os
import re

import numpy as np
import pytest

from pfann_amd import monitor
from pfann_amd.database import window_counts, window_queries

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RLEN = [0, 1, 18, 19, 20, 128, 129]


def _by_loop(rstart, rlen, window, hop):
    """the rule of include/pfann_amd.h (pfann_match_windows): starts 0, hop, .. while w0 + window <= L; one window over all
    rows when 0 < L < window; none when L == 0"""
    qstart, qlen, wfirst = [], [], [0]
    for s, L in zip(rstart, rlen):
        if 0 < L < window:
            qstart.append(s)
            qlen.append(L)
        else:
            w0 = 0
            while L > 0 and w0 + window <= L:
                qstart.append(s + w0)
                qlen.append(window)
                w0 += hop
        wfirst.append(len(qstart))
    return qstart, qlen, wfirst


@pytest.mark.parametrize("hop", [1, 2, 7, 70])
@pytest.mark.parametrize("window", [1, 19, 64])
def test_window_queries_against_the_loop(window, hop):
    for rlen in (RLEN, RLEN[::-1], [129], [0], []):
        rstart = [5 + 3 * i + sum(rlen[:i]) for i in range(len(rlen))]       # gaps between the recordings
        qstart, qlen, wfirst = window_queries(rstart, rlen, window, hop)
        want = _by_loop(rstart, rlen, window, hop)
        assert qstart.dtype == np.int64 and qlen.dtype == np.int32 and wfirst.dtype == np.int64
        assert (qstart.tolist(), qlen.tolist(), wfirst.tolist()) == want, (rlen, window, hop)
        assert np.diff(wfirst).tolist() == window_counts(rlen, window, hop).tolist()
        assert qstart.shape == qlen.shape == (int(wfirst[-1]),)


# ------------------------------------------------------------------------------------------------ the flag
BASE = ["monitor.py", "recs.txt", "db", "out.tsv"]


def test_parse_args_nominate():
    assert monitor.parse_args(BASE).nominate is None
    assert monitor.parse_args(BASE + ["--dense"]).nominate is None
    a = monitor.parse_args(BASE + ["--dense", "--nominate", "4"])
    assert a.nominate == 4 and a.dense and a.top == 1 and a.max_fa is None and monitor.check_nominate(a) is None
    for n in (1, 64):
        assert monitor.check_nominate(monitor.parse_args(BASE + ["--dense", "--nominate", str(n)])) is None
    assert monitor.check_nominate(monitor.parse_args(BASE + ["--top", "3"])) is None


@pytest.mark.parametrize("args,env,word", [
    (["--nominate", "4"], {}, "--dense"),
    (["--dense", "--nominate", "4", "--max-fa", "0.01"], {}, "--max-fa"),
    (["--dense", "--nominate", "4", "--top", "3"], {}, "--top"),
    (["--dense", "--nominate", "0"], {}, "1..64"),
    (["--dense", "--nominate", "65"], {}, "1..64"),
    (["--dense", "--nominate", "4"], {"PFANN_GPUS": "2"}, "multi-GPU"),
    (["--dense", "--nominate", "4"], {"WORLD_SIZE": "2"}, "multi-GPU"),
])
def test_refusals_return_status_2(tmp_path, monkeypatch, capsys, args, env, word):
    monkeypatch.delenv("PFANN_GPUS", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    out = tmp_path / "out.tsv"
    rc = monitor.main(["monitor.py", str(tmp_path / "recs.txt"), str(tmp_path / "db"), str(out)] + args)
    err = capsys.readouterr().err
    assert rc == 2 and word in err and err.startswith("monitor: ") and len(err.strip().splitlines()) == 1, (args, rc, err)
    assert "--nominate" in err
    assert not out.exists() and not (tmp_path / "out_nominate.csv").exists() and not (tmp_path / "out_windows.csv").exists()


def test_nominate_csv_rows():
    assert monitor.NOMINATE_HEADER == ["recording", "w0", "n_close", "certified"]
    rows = np.zeros(4, dtype=[("w0", "<i8"), ("score", "<f8"), ("song", "<i4"), ("time_s", "<f8")])
    rows["w0"] = [0, 2, 4, 6]
    n_close = np.asarray([1, 4, 5, -1], np.int32)
    got = monitor.nominate_csv("a,b.wav", rows, n_close, (n_close >= 0) & (n_close <= 4))
    assert got == [["a,b.wav", 0, 1, 1], ["a,b.wav", 2, 4, 1], ["a,b.wav", 4, 5, 0], ["a,b.wav", 6, -1, 0]]
    assert all(type(v) is int for row in got for v in row[1:])
    assert monitor.nominate_csv("x", rows[:0], n_close[:0], []) == []
    with pytest.raises(AssertionError):
        monitor.nominate_csv("x", rows, n_close[:3], [True] * 3)


# ------------------------------------------------------------------------------------------------ the declaration
def test_the_header_declares_the_call():
    """tests/test_host.py::test_c_abi_exports_every_declared_symbol then holds the library and the bindings to it"""
    from pfann_amd import lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "pfann_amd.h")).read(), flags=re.S)
    decl = re.search(r"int pfann_nominate_windows_dense\s*\(([^;]*)\)\s*;", hdr)
    assert decl, "include/pfann_amd.h does not declare pfann_nominate_windows_dense"
    args = [a.strip() for a in decl.group(1).split(",")]
    assert len(args) == 15 and args[0] == "pfann_db *db" and args[-1] == "void *stream" and "excl_song_dev" in args[9]
    assert len(lib.SYMBOLS["pfann_nominate_windows_dense"][1]) == 15
    assert "nominate_windows.hip" in open(os.path.join(REPO, "pfann_amd", "build.py")).read()
