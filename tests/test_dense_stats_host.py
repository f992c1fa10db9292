"""The significance of a dense window without a GPU (pfann_amd/significance.py): the overlap histogram against brute force,
log10_false_alarm against a direct float64 evaluation, its calibration on iid rows, and the argument rule of monitor.py."""
import math
import sys

import numpy as np
import pytest

import dense_cases as dc
import dense_stats_cases as sc
from pfann_amd import significance as sg


# ------------------------------------------------------------------------------------------------ the overlap histogram
@pytest.mark.parametrize("n", [1, 2, 5, 19, 64])
def test_overlap_histogram_against_brute_force(n):
    """songs of 0, 1, fewer than n, exactly n and more than n rows; with and without an excluded song; hist[n] is the number of
    full candidates and hist.sum() the result's n_cand, both as the float64 oracle of the kernel counts them"""
    lens = np.asarray([0, 1, 3, 7, 0, 19, 18, 20, 64, 63, 65, 200, 1, 2], np.int64)
    pos = np.pad(np.cumsum(lens), (1, 0))
    hists = sg.OverlapHistograms(lens)
    for excl in (-1, 0, 1, 5, 8, 11, 13):
        want = sc.brute_histogram(pos, n, excl)
        got = sg.overlap_histogram(lens, n, excl)
        assert got.dtype == np.int64 and got.shape == (n + 1,) and np.array_equal(got, want), (n, excl, got, want)
        assert got[0] == 0
        keep = np.asarray([L for s, L in enumerate(lens) if s != excl])
        assert got[n] == int(np.maximum(keep - n + 1, 0).sum())                      # n_full of include/pfann_amd.h
        assert got.sum() == int((keep[keep > 0] + n - 1).sum())                      # n_cand
        assert hists(n, excl) is hists(n, excl) and np.array_equal(hists(n, excl), want)
    assert not sg.overlap_histogram([], n).any() and not sg.overlap_histogram([0, 0], n).any()


def test_overlap_histogram_equals_the_stats_oracle():
    """hist[n] == n_full and hist.sum() == n_cand of every window of the small world, excluded songs included"""
    db, pos, q, rstart, rlen = dc.small_world()
    excl = [3, -1, 6]
    for window in (1, 5, 19, 64):
        want = sc.stats_oracle(q, db, pos, window, 3, rstart, rlen, excl=excl)
        j = 0
        for r, L in enumerate(rlen):
            hist = sg.overlap_histogram(np.diff(pos), min(window, L), excl[r])
            for _ in sc.mc.window_starts(L, window, 3):
                assert hist[-1] == want[j]["n_full"] and hist.sum() == want[j]["n_cand"], (window, r, j)
                j += 1
        assert j == len(want) > 0


# ------------------------------------------------------------------------------------------------ log10_false_alarm
def _direct(T, n, N, mean, meansq, hist):
    """the definition in plain float64, no logarithms: needs p well inside the double range"""
    var = meansq - mean * mean
    p = sum(int(hist[m]) * 0.5 * math.erfc((T - mean * m / n) / math.sqrt(var * m / n) / math.sqrt(2.0)) for m in range(1, n + 1))
    return min(0.0, math.log10(p))


def _world(seed=5, n=19, N=400):
    rng = np.random.default_rng(seed)
    lens = np.asarray([50, 7, 0, 120, 19, 30], np.int64)
    tot = rng.standard_normal(N).astype(np.float32).astype(np.float64) * 0.4 + 0.05
    return lens, tot, sg.overlap_histogram(lens, n)


def test_log10_false_alarm_against_a_direct_evaluation():
    n = 19
    lens, tot, hist = _world(n=n)
    s1, s2 = sc.quantise(tot)
    N = tot.shape[0]
    changed = 0
    for T in (0.3, 1.0, 1.7, 2.5, 4.0):
        T = float(np.float32(T))
        # the best hangs over its song's edge (offset < 0, offset > len - n): every full total stays in the moments
        for song, offset in ((0, -3), (0, 32), (1, 0), (3, 102)):
            got = sg.log10_false_alarm(T / n, n, song, offset, (N, s1, s2), hist, lens)
            want = _direct(T, n, N, s1 / 2.0 ** 24 / N, s2 / 2.0 ** 18 / N, hist)
            assert got <= 0.0 and abs(got - want) <= 1e-9 * max(1.0, abs(want)), (T, song, offset, got, want)
        # the best is a full piece (0 <= offset <= len - n): its own three integers leave the sums
        q1, q2 = sc.quantise([T])
        for song, offset in ((0, 0), (0, 31), (3, 101), (4, 0)):
            got = sg.log10_false_alarm(T / n, n, song, offset, (N + 1, s1 + q1, s2 + q2), hist, lens)
            want = _direct(T, n, N, s1 / 2.0 ** 24 / N, s2 / 2.0 ** 18 / N, hist)
            assert abs(got - want) <= 1e-9 * max(1.0, abs(want)), (T, song, offset, got, want)
            kept = sg.log10_false_alarm(T / n, n, song, offset, (N, s1, s2), hist, lens)
            assert kept != got or want == 0.0, "leave-one-out changed nothing"
            changed += kept != got
    assert changed >= 12
    # a score far below the background: p > 1, reported as 0
    assert sg.log10_false_alarm(-5.0 / n, n, 0, -3, (N, s1, s2), hist, lens) == 0.0
    # the recovered total is the float32 behind the score
    for t in tot[:50].astype(np.float32):
        assert sg.best_total(float(np.float64(t) / np.float64(n)), n) == float(t)


def test_log10_false_alarm_degenerate_cases_are_never_significant():
    n = 19
    lens, tot, hist = _world(n=n)
    s1, s2 = sc.quantise(tot)
    N = tot.shape[0]
    good = sg.log10_false_alarm(4.0 / n, n, 0, -3, (N, s1, s2), hist, lens)
    assert good < -6.0
    assert sg.log10_false_alarm(-np.inf, n, -1, 0, (0, 0, 0), np.zeros(n + 1, np.int64), lens) == 0.0     # no candidate
    assert sg.log10_false_alarm(4.0 / n, n, 0, -3, (N, s1, s2), np.zeros(n + 1, np.int64), lens) == 0.0
    a1, a2 = sc.quantise(tot[:1])
    assert sg.log10_false_alarm(4.0 / n, n, 0, -3, (0, 0, 0), hist, lens) == 0.0                         # N < 2
    assert sg.log10_false_alarm(4.0 / n, n, 0, -3, (1, a1, a2), hist, lens) == 0.0
    b1, b2 = sc.quantise(tot[:2])
    T = float(np.float32(4.0))
    q1, q2 = sc.quantise([T])
    assert sg.log10_false_alarm(T / n, n, 0, 0, (2, a1 + q1, a2 + q2), hist, lens) == 0.0                # N < 2 once the best is out
    assert sg.log10_false_alarm(T / n, n, 0, -3, (2, b1, b2), hist, lens) < 0.0                          # two left: defined
    c1, c2 = sc.quantise([0.5, 0.5, 0.5])
    assert sg.log10_false_alarm(4.0 / n, n, 0, -3, (3, c1, c2), hist, lens) == 0.0                       # var <= 0


def test_log10_false_alarm_stays_finite_far_out():
    """z above 30, where erfc is left for the asymptotic logarithm, and above 38, where erfc underflows: finite, decreasing,
    continuous at the seam"""
    n = 19
    lens, tot, hist = _world(n=n)
    s1, s2 = sc.quantise(tot)
    N = tot.shape[0]
    sd = math.sqrt(s2 / 2.0 ** 18 / N - (s1 / 2.0 ** 24 / N) ** 2)
    last = 0.0
    for z in (5, 20, 29.9, 30.1, 37, 40, 100, 150):
        got = sg.log10_false_alarm(z * sd / n, n, 0, -3, (N, s1, s2), hist, lens)
        assert math.isfinite(got) and got < last, (z, got, last)
        last = got
    assert last < -4000
    assert abs(sg.log10_upper_tail(30.0) - sg.log10_upper_tail(30.0 - 1e-9)) < 1e-6
    assert abs(sg.log10_upper_tail(30.0) - math.log10(0.5 * math.erfc(30.0 / math.sqrt(2.0)))) < 1e-5


# ------------------------------------------------------------------------------------------------ calibration on iid rows
_CAL = {}


def _calibration(window, hop):
    if (window, hop) not in _CAL:
        db, pos, rec, planted = sc.iid_world()
        want = sc.stats_oracle(rec, db, pos, window, hop, [0], [rec.shape[0]], key="iid", as_float32=True)
        lens = np.diff(pos)
        hist = sg.overlap_histogram(lens, window)
        fa = np.asarray([sg.log10_false_alarm(w["score"], window, w["song"], w["offset"], (w["n_full"], w["sum_q"], w["sumsq_q"]),
                                              hist, lens) for w in want])
        w0 = np.arange(len(want)) * hop
        _CAL[(window, hop)] = dict(fa=fa, score=np.asarray([w["score"] for w in want]), song=np.asarray([w["song"] for w in want]),
                                   planted=(w0 + window > 303) & (w0 < 337), noise=(w0 + window <= 300) | (w0 >= 340), s=planted)
    return _CAL[(window, hop)]


@pytest.mark.parametrize("window,hop", [(19, 2), (7, 1), (64, 4)])
def test_calibration_on_iid_rows(window, hop):
    """random unit rows, one planted excerpt at SNR 0.  Caps, not measurements: at most 0.03 of the noise windows flagged at
    1e-2, at most 0.2 at 1e-1, at least 0.9 of the planted windows kept at 1e-3.  Measured with this module (float64 totals
    rounded to float32), false alarms at 1e-1 / 1e-2 / 1e-3 and planted windows kept at 1e-3:
    19 / 2: 0.0773 / 0.0055 / 0.0000, 1.00;   7 / 1: 0.0709 / 0.0080 / 0.0013, 1.00;   64 / 4: 0.1313 / 0.0063 / 0.0000, 0.96.
    At 64 / 4 the best noise window scores 0.0510 and the weakest planted window 0.0442: no --min-score separates them."""
    c = _calibration(window, hop)
    noise, planted = c["noise"], c["planted"]
    assert noise.sum() > 100 and planted.sum() >= 10
    rate = lambda x: float((c["fa"][noise] <= math.log10(x)).mean())
    kept = float((c["fa"][planted] <= -3.0).mean())
    print("window %d hop %d: false alarms %.4f / %.4f / %.4f at 1e-1 / 1e-2 / 1e-3, planted kept at 1e-3 %.3f; noise scores <= %.4f, "
          "planted scores >= %.4f" % (window, hop, rate(1e-1), rate(1e-2), rate(1e-3), kept, c["score"][noise].max(),
                                      c["score"][planted].min()))
    assert rate(1e-2) <= 0.03
    assert rate(1e-1) <= 0.2
    assert kept >= 0.9
    if (window, hop) == (64, 4):
        assert c["score"][noise].max() > c["score"][planted].min(), "a fixed score would have separated them"


# ------------------------------------------------------------------------------------------------ the merge and the CLI
def test_merge_windows_good_replaces_the_score_test():
    from pfann_amd.monitor import merge_windows
    rows = [(2 * i, sc_, song, 10.0 + i) for i, (sc_, song) in enumerate([(0.01, 4), (0.02, 4), (0.03, 4), (0.9, 4), (0.9, -1), (0.02, 4)])]
    plain = merge_windows(rows, 19, 2, 0.5, min_score=0.2)
    assert merge_windows(rows, 19, 2, 0.5, min_score=0.2, good=None) == plain and len(plain) == 1 and plain[0][6] == 1
    by_flag = merge_windows(rows, 19, 2, 0.5, min_score=0.2, good=[True, True, True, False, True, True])
    assert [d[6] for d in by_flag] == [3, 1] and all(d[2] == 4 for d in by_flag), by_flag      # (a window still has to name a song)
    with pytest.raises(AssertionError):
        merge_windows(rows, 19, 2, 0.5, good=[True])


def test_max_fa_is_refused_before_torch_is_imported(monkeypatch, capsys):
    from pfann_amd import monitor
    monkeypatch.setitem(sys.modules, "torch", None)      # an `import torch` would raise from here on
    assert monitor.main(["monitor.py", "recs.txt", "dbdir", "out.tsv", "--max-fa", "1e-3"]) == 2
    assert "--dense" in capsys.readouterr().err
    for x in ("0", "-0.1", "1.5", "nan"):
        assert monitor.main(["monitor.py", "recs.txt", "dbdir", "out.tsv", "--dense", "--max-fa", x]) == 2, x
        assert "--max-fa" in capsys.readouterr().err


def test_significance_imports_neither_torch_nor_the_oracle():
    import subprocess
    code = "import sys; import pfann_amd.significance; assert 'torch' not in sys.modules and 'oracle' not in sys.modules"
    assert subprocess.run([sys.executable, "-c", code], cwd=dc.REPO).returncode == 0
