"""Monitor mode without a GPU: the reference pin of the windowed answers (tests/golden/monitor_windows.npz, written by
tests/golden/make_golden_monitor.py from the reference's own Database.query_embeddings), merge_windows on hand-written
window tables, and the window rule against the counts the Python layer and the CLI use."""
import os

import numpy as np
import pytest

import monitor_cases as mc
from oracle import seqscore
from pfann_amd.monitor import default_window, merge_windows

G = os.path.join(os.path.dirname(__file__), "golden")
REF = "/root/reference"


def _fixture():
    z = np.load(os.path.join(G, "monitor_windows.npz"))
    return z, seqscore.song_pos_from_key(z["landmarkKey"])


# ------------------------------------------------------------------------------------------------ reference pin
def test_oracle_answers_every_window_as_the_reference_did():
    z, pos = _fixture()
    window, hop, hop_size = int(z["window"]), int(z["hop"]), float(z["hop_size"])
    qs, ql = mc.expand(z["rstart"], z["rlen"], window, hop)
    assert len(qs) == z["song"].shape[0] == 23
    assert int(z["rlen"][1]) < window and ql[-1] == int(z["rlen"][1])           # the short recording: one window, all rows
    songs = set()
    for j, (s, n) in enumerate(zip(qs, ql)):
        score, (song, sec), _ = seqscore.query_embeddings_base(z["rec"][s:s + n], z["labels"][s:s + n], z["db"], pos, hop_size)
        assert song == int(z["song"][j]) and sec == float(z["time"][j]), j
        assert score == float(z["score"][j]) or abs(score - float(z["score"][j])) < 1e-6, j     # as tests/test_oracle.py
        songs.add(song)
    assert songs == {2, 5, 7, 9}
    assert len(set(z["song"][:16].tolist())) == 2 and z["song"][7] != z["song"][8]     # a song boundary inside the run of windows


def test_fixture_margins_leave_room_for_two_fp32_scorers():
    """best-to-second margin of the float64 oracle > 4e-6 in every window: the GPU test may then demand identical decisions"""
    z, pos = _fixture()
    qs, ql = mc.expand(z["rstart"], z["rlen"], int(z["window"]), int(z["hop"]))
    for j, (s, n) in enumerate(zip(qs, ql)):
        sc = sorted((mc.score64(z["db"], pos, z["rec"][s:s + n], c[0], c[1]) for c in mc.candidates(z["labels"][s:s + n], pos)),
                    reverse=True)
        assert len(sc) > 1 and sc[0] - sc[1] > 4e-6, (j, sc[:2])


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference checkout is not on this machine")
def test_fixture_regenerates_identically():
    import make_golden_monitor as mgm
    z, _ = _fixture()
    out = mgm.generate()
    assert sorted(out) == sorted(z.files)
    for name in z.files:
        assert np.array_equal(out[name], z[name]) and np.asarray(out[name]).dtype == z[name].dtype, name


# ------------------------------------------------------------------------------------------------ merge_windows
H = 0.5


def _run(song, diag, w0s, score=0.8):
    """windows of one song on one diagonal (in segments): time_s = (diag + w0) * H"""
    return [(w0, score, song, (diag + w0) * H) for w0 in w0s]


def test_a_single_run_is_one_detection():
    det = merge_windows(_run(3, 5, range(0, 20, 2)), 19, 2, H, 0.15)
    assert det == [(0.0, (18 + 19) * H, 3, 5 * H, 0.8, 0.8, 10)]


def test_partial_windows_move_the_edges_inwards():
    """a window that scores a third of the best overlaps the song by a third: the edge moves in by two thirds of a window"""
    rows = [(0, 0.3, 3, 5 * H)] + _run(3, 5, range(3, 30, 3), 0.9) + [(30, 0.45, 3, 35 * H)]
    (d0, d1, song, s0, mean, best, n), = merge_windows(rows, 18, 3, H, 0.15)
    assert (song, best, n) == (3, 0.9, 11)
    assert d0 == pytest.approx(12 * H) and d1 == pytest.approx((30 + 9) * H) and s0 == pytest.approx((5 + 12) * H)
    (e0, e1, *_), = merge_windows(rows, 18, 3, H, 0.15, refine=False)
    assert (e0, e1) == (0.0, 48 * H)


def test_two_songs_back_to_back():
    det = merge_windows(_run(3, 5, range(0, 10, 2)) + _run(4, -8, range(10, 20, 2)), 19, 2, H)
    assert [(d[2], d[6]) for d in det] == [(3, 5), (4, 5)]
    assert det[1][0] == 5.0 and det[1][3] == 1.0          # song 4 is at its second 1 when the second detection begins


def test_the_same_song_at_another_diagonal_is_a_new_detection():
    det = merge_windows(_run(3, 5, range(0, 10, 2)) + _run(3, 9, range(10, 20, 2)), 19, 2, H)
    assert [(d[2], d[3], d[6]) for d in det] == [(3, 2.5, 5), (3, 9.5, 5)]


def test_below_threshold_windows_separate_and_max_gap_bridges():
    low = [(10, 0.01, 3, 15 * H)]                          # right song and diagonal, but below min_score
    rows = _run(3, 5, range(0, 10, 2)) + low + _run(3, 5, range(12, 20, 2))
    assert [d[6] for d in merge_windows(rows, 19, 2, H, 0.15)] == [5, 4]
    (d,) = merge_windows(rows, 19, 2, H, 0.15, max_gap=1)
    assert d[6] == 10 and d[4] == pytest.approx(0.8) and d[:2] == (0.0, 18.5)
    other = [(10, 0.9, 7, 1.0), (12, 0.9, 8, 1.0)]         # two disagreeing windows: max_gap 1 does not bridge, 2 does
    rows = _run(3, 5, range(0, 10, 2)) + other + _run(3, 5, range(14, 20, 2))
    assert [(d[2], d[6]) for d in merge_windows(rows, 19, 2, H, 0.15, max_gap=1)] == [(3, 5), (7, 1), (8, 1), (3, 3)]
    assert [(d[2], d[6]) for d in merge_windows(rows, 19, 2, H, 0.15, max_gap=2)] == [(3, 10)]
    assert merge_windows(_run(3, 5, range(0, 10, 2), 0.1), 19, 2, H, 0.15) == []
    assert merge_windows([(0, -np.inf, -1, 0.0), (2, -np.inf, -1, 0.0)], 19, 2, H, 0.15) == []


def test_min_windows_drops_uncorroborated_windows():
    rows = [(0, 0.9, 7, 1.0)] + _run(3, 5, range(2, 12, 2)) + [(12, 0.9, 8, 1.0)]
    assert [(d[2], d[6]) for d in merge_windows(rows, 19, 2, H, 0.15)] == [(7, 1), (3, 5), (8, 1)]
    assert [(d[2], d[6]) for d in merge_windows(rows, 19, 2, H, 0.15, min_windows=2)] == [(3, 5)]
    assert len(merge_windows([(0, 0.7, 2, 1.5)], 7, 2, H, min_windows=2)) == 1      # a recording of one window keeps it


def test_short_windows_place_the_edges():
    """the short windows on the detection's diagonal, between its first window and the end of its last, give the edges;
    those on another diagonal or song, or outside that span, do not count; without any the score-ratio edges stand"""
    rows = [(0, 0.3, 3, 5 * H)] + _run(3, 5, range(3, 30, 3), 0.9) + [(30, 0.45, 3, 35 * H)]
    fine = [(2, 0.9, 3, 7 * H)]                                          # on the diagonal, but ...
    fine += [(w0, 0.5, 3, (5 + w0) * H) for w0 in (13, 14, 20, 36)]      # ... 13 is the first, 36 + 5 the end
    fine += [(10, 0.9, 3, 99.0), (11, 0.9, 4, 16 * H), (47, 0.9, 3, 52 * H)]   # other diagonal, other song, past the span
    fine.sort()
    (d0, d1, song, s0, *_), = merge_windows(rows, 18, 3, H, 0.15, edge_rows=fine, edge_window=5)
    assert (d0, d1, song, s0) == (2 * H, 41 * H, 3, 7 * H)
    (e0, e1, *_), = merge_windows(rows, 18, 3, H, 0.15, edge_rows=[(10, 0.9, 3, 99.0)], edge_window=5)
    assert e0 == pytest.approx(12 * H) and e1 == pytest.approx(39 * H)


def test_short_and_empty_recordings():
    assert merge_windows([], 19, 2, H) == []
    assert merge_windows([(0, 0.7, 2, 1.5)], 7, 2, H) == [(0.0, 3.5, 2, 1.5, 0.7, 0.7, 1)]     # 7 rows: one window over all of them


# ------------------------------------------------------------------------------------------------ window enumeration
def test_window_rule_matches_the_python_layer():
    from pfann_amd.database import window_counts
    lens = [0, 1, 2, 18, 19, 20, 21, 26, 64, 65, 300, 7199]
    for window in (1, 5, 19, 64):
        for hop in (1, 2, 7, 19, 30):
            want = [len(mc.window_starts(L, window, hop)) for L in lens]
            assert window_counts(lens, window, hop).tolist() == want, (window, hop)
            for L in lens:
                ws = mc.window_starts(L, window, hop)
                assert all(w0 % hop == 0 and w0 + n <= L for w0, n in ws)
                assert (not ws) == (L == 0) and (L >= window or ws == [(0, L)][:len(ws)])
                if L >= window:
                    assert ws[-1][0] + window + hop > L and all(n == window for _, n in ws)
    assert mc.wfirst_of([30, 0, 5, 19], 19, 2).tolist() == [0, 6, 6, 7, 8]


def test_default_window_is_a_ten_second_clip():
    import json
    cfg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs")
    assert default_window(json.load(open(os.path.join(cfg, "default.json")))) == 19
