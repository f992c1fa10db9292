"""merge_window_tracks (pfann_amd/monitor.py): ranked per-window answers -> detections that may overlap.  Host code only.

With one rank and max_gap = 0 it must be merge_windows (on the inputs of tests/test_monitor_host.py and on seeded random
sequences); with two ranks it must report two songs that play at once; at max_gap > 0 it differs from merge_windows in the
documented way (U T U)."""
import numpy as np

import test_monitor_host as tmh
from pfann_amd.database import MONITOR_TOPN_DTYPE
from pfann_amd.monitor import merge_window_tracks, merge_windows, ranked_window_csv

H = tmh.H
_run = tmh._run
BLANK = (-np.inf, -1, 0.0)


def _by_start(dets):
    return sorted(dets, key=lambda d: (d[0], d[2]))


def _host_cases():
    """(rows, window, hop, keyword arguments) of the merge_windows tests of tests/test_monitor_host.py"""
    partial = [(0, 0.3, 3, 5 * H)] + _run(3, 5, range(3, 30, 3), 0.9) + [(30, 0.45, 3, 35 * H)]
    low = [(10, 0.01, 3, 15 * H)]
    other = [(10, 0.9, 7, 1.0), (12, 0.9, 8, 1.0)]
    fine = [(2, 0.9, 3, 7 * H)] + [(w0, 0.5, 3, (5 + w0) * H) for w0 in (13, 14, 20, 36)]
    fine += [(10, 0.9, 3, 99.0), (11, 0.9, 4, 16 * H), (47, 0.9, 3, 52 * H)]
    fine.sort()
    lone = [(0, 0.9, 7, 1.0)] + _run(3, 5, range(2, 12, 2)) + [(12, 0.9, 8, 1.0)]
    return [
        (_run(3, 5, range(0, 20, 2)), 19, 2, dict(min_score=0.15)),
        (partial, 18, 3, dict(min_score=0.15)),
        (partial, 18, 3, dict(min_score=0.15, refine=False)),
        (_run(3, 5, range(0, 10, 2)) + _run(4, -8, range(10, 20, 2)), 19, 2, {}),
        (_run(3, 5, range(0, 10, 2)) + _run(3, 9, range(10, 20, 2)), 19, 2, {}),
        (_run(3, 5, range(0, 10, 2)) + low + _run(3, 5, range(12, 20, 2)), 19, 2, dict(min_score=0.15)),
        (_run(3, 5, range(0, 10, 2)) + other + _run(3, 5, range(14, 20, 2)), 19, 2, dict(min_score=0.15)),
        (_run(3, 5, range(0, 10, 2), 0.1), 19, 2, dict(min_score=0.15)),
        ([(0, -np.inf, -1, 0.0), (2, -np.inf, -1, 0.0)], 19, 2, dict(min_score=0.15)),
        (lone, 19, 2, dict(min_score=0.15)),
        (lone, 19, 2, dict(min_score=0.15, min_windows=2)),
        ([(0, 0.7, 2, 1.5)], 7, 2, dict(min_windows=2)),
        (partial, 18, 3, dict(min_score=0.15, edge_rows=fine, edge_window=5)),
        (partial, 18, 3, dict(min_score=0.15, edge_rows=[(10, 0.9, 3, 99.0)], edge_window=5)),
        ([], 19, 2, {}),
        ([(0, 0.7, 2, 1.5)], 7, 2, {}),
    ]


def test_one_rank_without_bridging_is_merge_windows():
    """max_gap = 0, one entry per window: the same detections, field for field, each with best_rank 1 -- whether the rows
    come as one answer per window or as lists of one entry"""
    n = 0
    for rows, window, hop, kw in _host_cases():
        want = _by_start(merge_windows(rows, window, hop, H, **kw))
        for form in (rows, [[r] for r in rows]):
            if "edge_rows" in kw and form is not rows:
                kw = dict(kw, edge_rows=[[r] for r in kw["edge_rows"]])
            got = merge_window_tracks(form, window, hop, H, **kw)
            assert [d[:7] for d in got] == want and all(d[7] == 1 for d in got), (rows, kw, got, want)
        n += len(want)
    assert n > 15


def _random_rows(rng, n_win, hop):
    """windows of a few songs on a few diagonals in runs of random length, low-scoring and empty windows between them"""
    rows, w = [], 0
    while len(rows) < n_win:
        kind = rng.integers(0, 10)
        run = int(rng.integers(1, 6))
        song, diag = int(rng.integers(0, 3)), int(rng.integers(-2, 2)) * 7
        for _ in range(min(run, n_win - len(rows))):
            w0 = w * hop
            if kind == 0:
                rows.append((w0,) + BLANK)
            else:
                score = float(rng.choice([0.1, 0.3, 0.5, 0.8])) if kind < 3 else float(rng.choice([0.4, 0.6, 0.9]))
                rows.append((w0, score, song, (diag + w0) * H))
            w += 1
    return rows


def test_one_rank_without_bridging_is_merge_windows_on_random_sequences():
    rng = np.random.default_rng(20240611)
    n_det = 0
    for case in range(300):
        hop = int(rng.integers(1, 4))
        rows = _random_rows(rng, int(rng.integers(1, 40)), hop)
        fine = _random_rows(rng, len(rows) * hop + 10, 1) if case % 3 == 0 else None
        kw = dict(min_score=float(rng.choice([0.2, 0.45])), min_windows=int(rng.integers(1, 4)), refine=bool(case % 2),
                  edge_rows=fine, edge_window=5 if fine else 0)
        want = _by_start(merge_windows(rows, 19, hop, H, **kw))
        got = merge_window_tracks(rows, 19, hop, H, **kw)
        assert [d[:7] for d in got] == want and all(d[7] == 1 for d in got), (case, rows, kw)
        n_det += len(want)
    assert n_det > 600, n_det


def _overlap(window=19, hop=1):
    """song A (diagonal 5) over windows 0..9, song B (diagonal -30) over windows 6..15; they swap ranks at window 8"""
    ranked = []
    for i in range(16):
        a = (i, 0.9 - 0.05 * i, 1, (5 + i) * H) if i <= 9 else None
        b = (i, 0.3 + 0.03 * i, 2, (30 + i) * H) if i >= 6 else None
        both = sorted([e for e in (a, b) if e], key=lambda e: -e[1])
        ranked.append(both + [(i,) + BLANK] * (2 - len(both)))
    assert [r[0][2] for r in ranked[6:10]] == [1, 1, 2, 2]
    return ranked


def test_two_songs_at_once_are_two_overlapping_detections():
    ranked = _overlap()
    det = merge_window_tracks(ranked, 19, 1, H, 0.2, refine=False)
    assert [(d[2], d[0], d[1], d[6], d[7]) for d in det] == [(1, 0.0, (9 + 19) * H, 10, 1), (2, 6 * H, (15 + 19) * H, 10, 1)]
    assert det[0][3] == 5 * H and det[1][3] == 36 * H
    # the same windows with only their winners: B starts where it wins, and A ends there
    top1 = merge_window_tracks([r[:1] for r in ranked], 19, 1, H, 0.2, refine=False)
    assert [(d[2], d[0], d[6]) for d in top1] == [(1, 0.0, 8), (2, 8 * H, 8)]
    assert [d[:7] for d in top1] == _by_start(merge_windows([r[0] for r in ranked], 19, 1, H, 0.2, refine=False))
    # a song that never ranks first is still reported, with the rank it held
    under = [[(i, 0.9, 1, (5 + i) * H), (i, 0.5, 2, (30 + i) * H) if 3 <= i <= 6 else (i,) + BLANK] for i in range(10)]
    det = merge_window_tracks(under, 19, 1, H, 0.2, refine=False)
    assert [(d[2], d[6], d[7]) for d in det] == [(1, 10, 1), (2, 4, 2)]


def test_bridging_differs_from_merge_windows_as_documented():
    """U T U at max_gap = 1: merge_windows lets U's bridge swallow T; merged per track, T is a detection of its own"""
    rows = [(0, 0.8, 4, 5 * H), (1, 0.8, 9, 40 * H), (2, 0.8, 4, 7 * H)]
    one = merge_windows(rows, 19, 1, H, 0.2, max_gap=1, min_windows=1)
    assert [(d[2], d[6]) for d in one] == [(4, 3)]
    got = merge_window_tracks(rows, 19, 1, H, 0.2, max_gap=1, min_windows=1)
    assert [(d[2], d[6], d[7]) for d in got] == [(4, 3, 1), (9, 1, 1)]
    assert got[0][:7] == one[0]
    # without bridging the two agree again: U, T, U
    assert [d[:7] for d in merge_window_tracks(rows, 19, 1, H, 0.2, min_windows=1)] == _by_start(merge_windows(rows, 19, 1, H, 0.2, min_windows=1))
    assert "U T U" in merge_window_tracks.__doc__


def test_ranked_rows_as_the_database_returns_them_and_their_csv():
    """the [windows, n] structured array of Database.monitor_topn_finish merges like nested tuples; the CSV rows carry rank
    and votes, keep rank 1 of every window and drop the padding behind it"""
    ranked = _overlap()
    arr = np.zeros((len(ranked), 3), dtype=MONITOR_TOPN_DTYPE)
    for i, row in enumerate(ranked):
        for j in range(3):
            e = row[j] if j < 2 else (i,) + BLANK
            arr[i, j] = e + (7 - j if e[2] >= 0 else 0,)
    arr = np.concatenate([arr, np.zeros((1, 3), dtype=MONITOR_TOPN_DTYPE)])
    arr[-1] = [(16,) + BLANK + (0,)] * 3                   # a window without any candidate
    assert merge_window_tracks(arr, 19, 1, H, 0.2) == merge_window_tracks(ranked, 19, 1, H, 0.2)
    names = ["s0", "s1", "s2"]
    out = ranked_window_csv("rec", arr, H, names)
    assert all(len(r) == 8 for r in out)
    per = {w: [r for r in out if r[1] == w] for w in range(17)}
    assert [len(per[w]) for w in (0, 5, 6, 9, 10, 15, 16)] == [1, 1, 2, 2, 1, 1, 1]
    assert per[7] == [["rec", 7, 7 * H, "s1", 0.9 - 0.05 * 7, 12 * H, 1, 7], ["rec", 7, 7 * H, "s2", 0.3 + 0.03 * 7, 37 * H, 2, 6]]
    assert per[16] == [["rec", 16, 16 * H, "", -np.inf, 0.0, 1, 0]]
    assert [r[6] for r in per[8]] == [1, 2] and [r[3] for r in per[8]] == ["s2", "s1"]
