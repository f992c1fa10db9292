"""Calibrated ranked dense answers without a GPU: the per-entry rule of significance.log10_false_alarms_ranked and the argument
rule of matcher.py --max-fa (pfann_amd/launch.py: matcher_max_fa_flag), refused before torch is imported."""
import math
import sys

import numpy as np

import dense_stats_cases as sc
from pfann_amd import significance as sg

RESULT_DTYPE = np.dtype([("song", "<i4"), ("offset", "<i4"), ("shift", "<i4"), ("n_cand", "<i4"), ("score", "<f8")])   # pfann_match_result


def _world(seed=5, n=19, N=400):
    """the background of tests/test_dense_stats_host.py: song lengths, N full totals (float32 values), the overlap histogram"""
    rng = np.random.default_rng(seed)
    lens = np.asarray([50, 7, 0, 120, 19, 30], np.int64)
    tot = rng.standard_normal(N).astype(np.float32).astype(np.float64) * 0.4 + 0.05
    return lens, tot, sg.overlap_histogram(lens, n)


def _entries(rows, n, pad=0):
    """rows: (song, offset, fp32 total) best first -> RESULT_DTYPE entries as the ranked call leaves them, `pad` padding entries"""
    e = np.zeros(len(rows) + pad, dtype=RESULT_DTYPE)
    e["song"], e["score"] = -1, -np.inf
    for i, (song, offset, T) in enumerate(rows):
        e[i]["song"], e[i]["offset"], e[i]["score"] = song, offset, float(np.float32(T)) / n
    return e


def _sums(tot, rows, lens, n):
    """the window's three integers: the background totals and every row that is a full candidate"""
    full = [float(np.float32(T)) for s, o, T in rows if 0 <= o <= lens[s] - n]
    s1, s2 = sc.quantise(np.concatenate([tot, full]))
    return len(tot) + len(full), s1, s2


ROWS = [(3, 40, 4.0), (0, 5, 3.5), (5, -3, 3.0), (4, 0, 2.5), (0, 31, 2.0), (1, 0, 1.5), (3, 101, 1.25), (5, 11, 1.0)]
#        full         full        edge         full (19 rows)  full      short song   full          full


def test_entry_0_is_log10_false_alarm():
    n = 19
    lens, tot, hist = _world(n=n)
    for rows in (ROWS, ROWS[2:], ROWS[5:]):              # the best: a full candidate, an edge candidate, one of a song shorter than n
        stats = _sums(tot, rows, lens, n)
        e = _entries(rows, n)
        got = sg.log10_false_alarms_ranked(e, n, stats, hist, lens)
        assert got.dtype == np.float64 and got.shape == (len(rows),)
        want = sg.log10_false_alarm(e[0]["score"], n, e[0]["song"], e[0]["offset"], stats, hist, lens)
        assert got[0] == want < 0.0, (got[0], want)


def test_an_entry_does_not_depend_on_the_length_of_the_list():
    """the prefix rule: the lists of 3 and of 8 of one window agree on their first 3 values, bit for bit"""
    n = 19
    lens, tot, hist = _world(n=n)
    stats = _sums(tot, ROWS, lens, n)                    # the window's sums do not depend on the list asked for
    e8 = _entries(ROWS, n)
    got8 = sg.log10_false_alarms_ranked(e8, n, stats, hist, lens)
    got3 = sg.log10_false_alarms_ranked(e8[:3], n, stats, hist, lens)
    got1 = sg.log10_false_alarms_ranked(e8[:1], n, stats, hist, lens)
    assert np.array_equal(got8[:3], got3) and got8[0] == got1[0]
    assert (got8 <= 0.0).all() and (np.diff(got8) >= 0.0).all() and got8[0] < got8[-1], got8     # lower totals are less surprising


def test_better_ranked_full_entries_leave_the_sums_and_edge_entries_do_not():
    """entry i against a direct evaluation: the background is the window's full candidates without the full ones among 0..i"""
    n = 19
    lens, tot, hist = _world(n=n)
    stats = _sums(tot, ROWS, lens, n)
    got = sg.log10_false_alarms_ranked(_entries(ROWS, n), n, stats, hist, lens)
    for i, (song, offset, T) in enumerate(ROWS):
        left = [float(np.float32(t)) for s, o, t in ROWS[i + 1:] if 0 <= o <= lens[s] - n]
        N, s1, s2 = len(tot) + len(left), *sc.quantise(np.concatenate([tot, left]))
        mean, meansq = s1 / 2.0 ** 24 / N, s2 / 2.0 ** 18 / N
        var = meansq - mean * mean
        p = sum(int(hist[m]) * 0.5 * math.erfc((float(np.float32(T)) - mean * m / n) / math.sqrt(var * m / n) / math.sqrt(2.0))
                for m in range(1, n + 1))
        want = min(0.0, math.log10(p))
        assert abs(got[i] - want) <= 1e-9 * max(1.0, abs(want)), (i, got[i], want)
    # a partial (edge) entry takes nothing out: entry 3 is judged by the same sums whether entry 2 is the edge candidate or absent
    without = ROWS[:2] + ROWS[3:]
    alt = sg.log10_false_alarms_ranked(_entries(without, n), n, stats, hist, lens)
    assert alt[2] == got[3] and np.array_equal(alt[2:], got[3:])
    # a full one does: with entry 1 made an edge candidate of the same total (the window's sums unchanged), the later values move
    moved = [ROWS[0], (0, -2, ROWS[1][2])] + ROWS[2:]
    alt = sg.log10_false_alarms_ranked(_entries(moved, n), n, stats, hist, lens)
    assert alt[0] == got[0] and alt[1] != got[1] and alt[3] != got[3]


def test_padding_and_degenerate_windows_are_never_significant():
    n = 19
    lens, tot, hist = _world(n=n)
    stats = _sums(tot, ROWS[:2], lens, n)
    got = sg.log10_false_alarms_ranked(_entries(ROWS[:2], n, pad=3), n, stats, hist, lens)
    assert got.shape == (5,) and (got[:2] < 0.0).all() and (got[2:] == 0.0).all()
    assert np.array_equal(got[:2], sg.log10_false_alarms_ranked(_entries(ROWS[:2], n), n, stats, hist, lens))
    allpad = sg.log10_false_alarms_ranked(_entries([], n, pad=3), n, (0, 0, 0), np.zeros(n + 1, np.int64), lens)
    assert allpad.shape == (3,) and (allpad == 0.0).all()
    assert (sg.log10_false_alarms_ranked(_entries(ROWS[:2], n), n, stats, np.zeros(n + 1, np.int64), lens) == 0.0).all()
    # N < 2 after the removals: background totals 0.1, 0.2, 0.15 and two full entries 4.0 and 3.9 (the sums hold all five)
    pair = [(3, 40, 4.0), (0, 5, 3.9)]
    small = _sums(np.asarray([0.1, 0.2, 0.15]), pair, lens, n)
    got = sg.log10_false_alarms_ranked(_entries(pair, n), n, small, hist, lens)
    assert small[0] == 5 and got[1] < -6.0, got                           # entry 1: judged by the three background totals alone
    small = _sums(np.asarray([0.1]), pair, lens, n)
    got = sg.log10_false_alarms_ranked(_entries(pair, n), n, small, hist, lens)
    assert small[0] == 3 and got[1] == 0.0, got                           # entry 1: one total left
    edge = [(3, 40, 4.0), (0, -2, 3.9)]                                    # the same with entry 1 over an edge: two are left
    small = _sums(np.asarray([0.1, 0.2]), edge, lens, n)
    got = sg.log10_false_alarms_ranked(_entries(edge, n), n, small, hist, lens)
    assert small[0] == 3 and got[1] < -6.0, got
    # var <= 0 after the removals: the background is three equal totals
    flat = _sums(np.asarray([0.5, 0.5, 0.5]), ROWS[:1], lens, n)
    assert sg.log10_false_alarms_ranked(_entries(ROWS[:1], n), n, flat, hist, lens)[0] == 0.0
    assert sg.log10_false_alarms_ranked(_entries(ROWS[:1], n), n, _sums(tot, ROWS[:1], lens, n), hist, lens)[0] < 0.0    # the control


# ------------------------------------------------------------------------------------------------ matcher.py --max-fa
def test_matcher_max_fa_flag():
    from pfann_amd.launch import matcher_max_fa_flag
    assert matcher_max_fa_flag([]) == (None, None) and matcher_max_fa_flag(["--dense", "--top", "3", "--no-bin"]) == (None, None)
    assert matcher_max_fa_flag(["--dense", "--max-fa", "0.01"]) == (0.01, None)
    assert matcher_max_fa_flag(["--top", "3", "--max-fa=1e-3", "--no-bin", "--dense"]) == (1e-3, None)
    assert matcher_max_fa_flag(["--dense", "--max-fa", "1"]) == (1.0, None)
    for x in ("0", "-0.1", "1.5", "nan", "inf", "x", ""):
        v, err = matcher_max_fa_flag(["--dense", "--max-fa", x] if x else ["--dense", "--max-fa"])
        assert v is None and "--max-fa" in err and "0 < X <= 1" in err, (x, v, err)
    assert "--dense" in matcher_max_fa_flag(["--max-fa", "0.01"])[1]
    assert "--rescore" in matcher_max_fa_flag(["--dense", "--max-fa", "0.01", "--rescore", "8", "--no-bin"])[1]
    assert "--rescore" in matcher_max_fa_flag(["--dense", "--max-fa", "0.01", "--rescore=8", "--no-bin"])[1]


def test_max_fa_is_refused_before_torch_is_imported(monkeypatch, capsys):
    from pfann_amd import launch, matcher
    # the three existing parsers skip the flag and answer what they always answered
    assert launch.matcher_flags(["--dense", "--top", "3", "--no-bin"]) == (3, True, None)
    assert launch.matcher_flags(["--dense", "--max-fa", "0.01", "--top", "3", "--no-bin"]) == (3, True, None)
    assert launch.matcher_dense_flag(["--top", "3", "--dense"]) == (True, None) and launch.matcher_dense_flag(["--no-bin"]) == (False, None)
    assert launch.matcher_dense_flag(["--max-fa", "0.01", "--dense"]) == (True, None)
    assert launch.matcher_rescore_flag([]) == (0, None) and launch.matcher_rescore_flag(["--top", "5", "--no-bin"]) == (0, None)
    assert launch.matcher_rescore_flag(["--rescore", "8", "--no-bin", "--top", "3"]) == (8, None)
    assert launch.matcher_rescore_flag(["--no-bin", "--rescore=64", "--top=64"]) == (64, None)
    assert launch.matcher_rescore_flag(["--rescore", "8", "--no-bin", "--max-fa", "0.01"]) == (8, None)
    monkeypatch.setitem(sys.modules, "torch", None)      # an `import torch` would raise from here on
    base = ["matcher.py", "q.txt", "dbdir", "out.tsv"]
    assert matcher.main(base + ["--max-fa", "1e-3"]) == 2
    err = capsys.readouterr().err
    assert "--dense" in err and len(err.strip().splitlines()) == 1
    assert matcher.main(base + ["--max-fa", "1e-3", "--rescore", "8", "--no-bin"]) == 2            # without --dense: that refusal
    assert "--max-fa" in capsys.readouterr().err
    assert matcher.main(base + ["--dense", "--max-fa", "1e-3", "--rescore", "8", "--no-bin"]) == 2
    err = capsys.readouterr().err
    assert "--rescore" in err and len(err.strip().splitlines()) == 1
    # one order of refusals for the script and for main: the line is launch.matcher_flag_error's
    for flags in (["--max-fa", "1e-3"], ["--dense", "--max-fa", "1e-3", "--rescore", "8", "--no-bin"], ["--dense", "--max-fa", "7", "--top", "99"]):
        assert matcher.main(base + flags) == 2 and capsys.readouterr().err.strip() == launch.matcher_flag_error(flags)
    for x in ("0", "-0.1", "1.5", "nan", "many"):
        assert matcher.main(base + ["--dense", "--max-fa", x]) == 2, x
        err = capsys.readouterr().err
        assert "--max-fa" in err and len(err.strip().splitlines()) == 1, err


def test_the_script_refuses_max_fa_without_importing_torch():
    """matcher.py itself (the file users start): status 2 and one line on stderr; torch made unimportable in the child"""
    import os
    import subprocess
    code = ("import sys, runpy; sys.modules['torch'] = None; sys.argv = ['matcher.py', 'q.txt', 'dbdir', 'out.tsv', '--max-fa', '0.5']; "
            "runpy.run_path(%r, run_name='__main__')" % os.path.join(sc.dc.REPO, "matcher.py"))
    r = subprocess.run([sys.executable, "-c", code], cwd=sc.dc.REPO, capture_output=True, text=True)
    assert r.returncode == 2 and "--dense" in r.stderr and len(r.stderr.strip().splitlines()) == 1, (r.returncode, r.stderr)
