"""Ranked dense answers without a GPU: the oracle of tests/dense_topn_cases.py pinned to the exact top-N oracle fed with every
database row as a label of every query row and to the dense oracle, and the argument rules of the command-line tools."""
import sys

import numpy as np
import pytest

import dense_cases as dc
import dense_topn_cases as dt
import match_exact as mx
import match_topn_exact as mt
import monitor_cases as mc


@pytest.mark.parametrize("window", [1, 5, 19])
def test_ranked_oracle_equals_the_exact_topn_matcher_with_every_row_as_a_label(window):
    """the small world (a copied pair, a periodic song, a one-row song): every field of every entry and n_found ==
    match_topn_exact.exact_topn (mode 0, frame_shift_mul 1); entry 0 == dense_oracle; the block holds entry s's float32 pair"""
    db, pos, q, rstart, rlen = dc.small_world()
    rows = mx.IntRows(db)
    mx.assert_exact_domain(window, db.shape[1])
    labels = dc.all_labels(q.shape[0], db.shape[0])
    n_songs = int((np.diff(pos) > 0).sum())
    ties = 0
    for hop, n in ((1, 4), (3, 64)):
        got = dt.dense_topn_oracle(q, db, pos, window, hop, rstart, rlen, n, key="small")
        first = dc.dense_oracle(q, db, pos, window, hop, rstart, rlen, key="small")
        qs, ql = mc.expand(rstart, rlen, window, hop)
        assert len(got) == len(first) == len(qs) > 0
        for j, (s, m) in enumerate(zip(qs, ql)):
            want = mt.exact_topn(q[s:s + m], labels[s:s + m], rows, pos, 1, 0, n)
            assert got[j]["top"] == want["top"], (window, hop, j, got[j]["top"][:3], want["top"][:3])
            assert got[j]["n_found"] == want["n_found"] == n_songs
            e = got[j]["top"][0]
            assert (e[0], e[1], e[2], e[4]) == (first[j]["song"], first[j]["offset"], first[j]["shift"], first[j]["score"])
            ties += got[j]["top"][0][4] == got[j]["top"][1][4]
            for song, off, _, _, score in got[j]["top"]:
                if song >= 0:
                    pair = (np.float32(score), np.float32(off)) if np.float32(score) > 0 else (0, 0)
                    assert tuple(got[j]["block"][song]) == pair
            if n == 64:
                assert got[j]["top"][n_songs:] == [dt.PAD] * (64 - n_songs)
                assert (got[j]["block"][np.diff(pos) == 0] == 0).all()
    assert ties > 0, "no window of the small world has an exact tie at the top"


def test_ranked_oracle_exclusion_and_no_candidate():
    db, pos, q, rstart, rlen = dc.small_world()
    a = dt.dense_topn_oracle(q, db, pos, 5, 2, rstart, rlen, 3)
    ex = a[0]["top"][0][0]
    b = dt.dense_topn_oracle(q, db, pos, 5, 2, rstart, rlen, 3, excl=[ex] * len(rlen))
    assert all(e[0] != ex for w in b for e in w["top"]) and all(x["n_found"] - y["n_found"] == 1 for x, y in zip(a, b))
    assert all((w["block"][ex] == 0).all() for w in b) and b[0]["top"][:2] == a[0]["top"][1:]
    lens = np.diff(pos)
    one = dt.dense_topn_oracle(q, db[pos[2]:pos[3]], [0, int(lens[2])], 5, 2, rstart, rlen, 3, excl=[0] * len(rlen))
    assert one and all(w["top"] == [dt.PAD] * 3 and w["n_found"] == 0 and (w["block"] == 0).all() for w in one)


def test_matcher_dense_flag_is_checked_before_torch_is_imported(monkeypatch, capsys):
    from pfann_amd import launch, matcher
    assert launch.matcher_dense_flag(["--top", "3", "--dense"]) == (True, None) and launch.matcher_dense_flag(["--no-bin"]) == (False, None)
    assert launch.matcher_flags(["--dense", "--top", "3", "--no-bin"]) == (3, True, None)
    monkeypatch.setitem(sys.modules, "torch", None)      # an `import torch` would raise from here on
    monkeypatch.setenv("PFANN_GPUS", "2")
    assert matcher.main(["matcher.py", "q.txt", "dbdir", "out.tsv", "--dense"]) == 2
    assert "--dense" in capsys.readouterr().err
    monkeypatch.delenv("PFANN_GPUS")
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert matcher.main(["matcher.py", "q.txt", "dbdir", "out.tsv", "--dense"]) == 2
    assert "--dense" in capsys.readouterr().err
    monkeypatch.delenv("WORLD_SIZE")
    assert matcher.main(["matcher.py", "q.txt", "dbdir", "out.tsv", "--dense", "--top", "65"]) == 2
    assert "--top" in capsys.readouterr().err


def test_selfmatch_top_argument_rule(capsys):
    from pfann_amd import selfmatch
    assert selfmatch.parse_args(["selfmatch.py", "dbdir", "out.tsv"]).top == 1
    args = selfmatch.parse_args(["selfmatch.py", "dbdir", "out.tsv", "--dense", "--top", "3"])
    assert args.top == 3 and args.dense
    assert selfmatch.parse_args(["selfmatch.py", "dbdir", "out.tsv", "--top", "64"]).top == 64
    for bad in ("0", "65"):
        assert selfmatch.main(["selfmatch.py", "dbdir", "out.tsv", "--top", bad]) == 2
        assert "--top" in capsys.readouterr().err


def test_monitor_dense_with_top_n_is_still_refused(monkeypatch, capsys):
    from pfann_amd import monitor
    monkeypatch.setitem(sys.modules, "torch", None)
    assert monitor.main(["monitor.py", "recs.txt", "dbdir", "out.tsv", "--dense", "--top", "2"]) == 2
    assert "--dense" in capsys.readouterr().err
