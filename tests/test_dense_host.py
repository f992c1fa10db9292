"""The dense matcher without a GPU: its oracle (tests/dense_cases.py) pinned to the exact sequence-matcher oracle fed with
every database row as a label of every query row, and the argument rule of the command-line tools."""
import sys

import numpy as np
import pytest

import dense_cases as dc
import match_exact as mx
import monitor_cases as mc


@pytest.mark.parametrize("window", [1, 5, 19])
def test_dense_oracle_equals_the_exact_matcher_with_every_row_as_a_label(window):
    """~200 rows with a copied and a periodic song: song, offset, shift, score and n_cand of every window, =="""
    db, pos, q, rstart, rlen = dc.small_world()
    assert 150 <= db.shape[0] <= 300 and (np.diff(pos) == 1).any()
    rows = mx.IntRows(db)
    mx.assert_exact_domain(window, db.shape[1])
    labels = dc.all_labels(q.shape[0], db.shape[0])
    n = ties = 0
    for hop in (1, 3):
        got = dc.dense_oracle(q, db, pos, window, hop, rstart, rlen, key="small")
        qs, ql = mc.expand(rstart, rlen, window, hop)
        assert len(got) == len(qs) > 0
        for j, (s, m) in enumerate(zip(qs, ql)):
            want = mx.exact_match(q[s:s + m], labels[s:s + m], rows, pos, 1, 0)
            for f in ("song", "offset", "shift", "score", "n_cand"):
                assert got[j][f] == want[f], (window, hop, j, f, got[j], want["top"])
            assert got[j]["n_cand"] == db.shape[0] + int((np.diff(pos) > 0).sum()) * (m - 1)
            ties += len(want["top"]) > 1 and want["top"][0][3] == want["top"][1][3]
            n += 1
    assert ties > 0, "no window of the small world has an exact tie at the top"


def test_dense_oracle_exclusion_and_no_candidate():
    db, pos, q, rstart, rlen = dc.small_world()
    a = dc.dense_oracle(q, db, pos, 5, 2, rstart, rlen)
    songs = sorted({w["song"] for w in a})
    ex = [songs[0]] * len(rlen)
    b = dc.dense_oracle(q, db, pos, 5, 2, rstart, rlen, excl=ex)
    assert all(w["song"] != songs[0] for w in b) and any(x != y for x, y in zip(a, b))
    lens = np.diff(pos)
    assert all(x["n_cand"] - y["n_cand"] == lens[songs[0]] + 4 for x, y in zip(a, b) if x["n_cand"] > lens.sum())
    one = dc.dense_oracle(q, db[pos[2]:pos[3]], [0, int(lens[2])], 5, 2, rstart, rlen, excl=[0] * len(rlen))
    assert one and all(w == dc.NONE for w in one)
    assert all(w == dc.NONE for w in dc.dense_oracle(q, db[:0], [0, 0], 5, 2, rstart, rlen))


def test_dense_with_top_n_is_refused_before_torch_is_imported(monkeypatch, capsys):
    from pfann_amd import monitor
    monkeypatch.setitem(sys.modules, "torch", None)      # an `import torch` would raise from here on
    assert monitor.main(["monitor.py", "recs.txt", "dbdir", "out.tsv", "--dense", "--top", "2"]) == 2
    assert "--dense" in capsys.readouterr().err
    assert monitor.main(["monitor.py", "recs.txt", "dbdir", "out.tsv", "--dense", "--window", "65"]) == 2
    assert "--dense" in capsys.readouterr().err


def test_selfmatch_dense_argument_rule(capsys):
    from pfann_amd import selfmatch
    args = selfmatch.parse_args(["selfmatch.py", "dbdir", "out.tsv", "--dense"])
    assert args.dense and not selfmatch.parse_args(["selfmatch.py", "dbdir", "out.tsv"]).dense
    assert selfmatch.main(["selfmatch.py", "dbdir", "out.tsv", "--dense", "--window", "65"]) == 2
    assert "--dense" in capsys.readouterr().err
