"""The oracle of the dense matcher's background statistics (tests/test_dense_stats_host.py, tests/test_gpu_dense_stats.py).

pfann_match_windows_dense_stats returns, per window of n rows, the number of its FULL candidates -- (song, offset) with
0 <= offset <= len - n, song not the excluded one -- and the sums of rint(total * 2^24) and rint(total^2 * 2^18) over them
(include/pfann_amd.h).  stats_oracle restates that on a float64 q @ db.T with the candidate numbering of tests/dense_cases.py
and keeps the sums as Python integers; on the exact grid of tests/match_exact.py every total is the kernel's fp32 total, so
the three numbers compare with ==."""
import numpy as np

import dense_cases as dc
import monitor_cases as mc

SUM_ONE, SQ_ONE = float(1 << 24), float(1 << 18)
_G, _HOP1 = {}, {}


def window_totals(G, pos, sg, r0, n, tab=None):
    """every candidate of the window G[r0:r0 + n] in (song, offset) order -> (song, offset, is a candidate, float64 total)"""
    song, off, ok = tab if tab is not None else dc._ids(pos, n)
    N = G.shape[1]
    tot = np.zeros(song.shape[0])
    base = np.arange(N) + sg * (n - 1) + (n - 1)
    for t in range(n):                                   # row t of the window meets db row g on the alignment id base[g] - t
        tot[base - t] += G[r0 + t]
    return song, off, ok, tot


def quantise(tot):
    """float64 totals -> (sum of rint(t * 2^24), sum of rint(t * t * 2^18)) as Python integers"""
    tot = np.asarray(tot, np.float64)
    return (sum(int(x) for x in np.rint(tot * SUM_ONE).astype(np.int64)),
            sum(int(x) for x in np.rint(tot * tot * SQ_ONE).astype(np.int64)))


def stats_oracle(q, db, pos, window, hop, rstart, rlen, excl=None, key=None, as_float32=False):
    """-> per window, in result order, a dict: n_full, sum_q, sumsq_q (Python integers), mean, meansq (float64, of the float64
    totals; nan without a full candidate), tmax (largest |total| among the full candidates), and the window's best candidate
    by dense_cases' rule (song, offset, score).  as_float32: every total is rounded to float32 first, as the kernel's are.
    excl, key: as dense_cases.dense_oracle."""
    pos = np.asarray(pos, np.int64)
    N = int(pos[-1])
    lens = np.diff(pos)
    if key is None or key not in _G:
        G = np.asarray(q, np.float64) @ np.asarray(db, np.float64).T if N else np.zeros((len(q), 0))
        if key is not None:
            _G[key] = G
    else:
        G = _G[key]
    sg = np.searchsorted(pos[:-1], np.arange(N), side="right") - 1
    ck = (key, window, None if excl is None else tuple(int(e) for e in excl), as_float32)
    if key is not None and ck in _HOP1:
        per = _HOP1[ck]
    else:
        per, tabs = [], {}
        for r, (s, L) in enumerate(zip(rstart, rlen)):
            ex = -1 if excl is None else int(excl[r])
            ans = []
            for w0, n in mc.window_starts(int(L), window, 1):
                if n not in tabs:
                    tabs[n] = dc._ids(pos, n)
                song, off, ok, tot = window_totals(G, pos, sg, int(s) + w0, n, tabs[n])
                if as_float32:
                    tot = tot.astype(np.float32).astype(np.float64)
                ok = ok & (song != ex)
                full = ok & (off >= 0) & (off <= lens[song] - n)
                ft = tot[full]
                s1, s2 = quantise(ft)
                a = dict(n_full=int(full.sum()), sum_q=s1, sumsq_q=s2, mean=float(ft.mean()) if ft.size else np.nan,
                         meansq=float((ft * ft).mean()) if ft.size else np.nan, tmax=float(np.abs(ft).max()) if ft.size else 0.0,
                         n_cand=int(ok.sum()), song=-1, offset=0, score=-np.inf)
                if ok.any():
                    b = int(np.argmax(np.where(ok, tot, -np.inf)))
                    a.update(song=int(song[b]), offset=int(off[b]), score=float(tot[b]) / n)
                ans.append(a)
            per.append(ans)
        if key is not None:
            _HOP1[ck] = per
    out = []
    for ans, L in zip(per, rlen):
        out += [ans[w0] for w0, _ in mc.window_starts(int(L), window, hop)]
    return out


def differing(stats, want):
    """-> messages for the windows whose (n_full, sum_q, sumsq_q) is not the oracle's, compared with =="""
    bad = []
    for j, w in enumerate(want):
        got = (int(stats["n_full"][j]), int(stats["sum_q"][j]), int(stats["sumsq_q"][j]))
        exp = (w["n_full"], w["sum_q"], w["sumsq_q"])
        if got != exp:
            bad.append("window %d: kernel (n_full, sum_q, sumsq_q) %r, oracle %r" % (j, got, exp))
    return bad


def brute_histogram(pos, n, excl=-1):
    """overlap lengths of every candidate of a window of n rows, one offset at a time -> int64 [n + 1]"""
    hist = np.zeros(n + 1, np.int64)
    for s, L in enumerate(np.diff(np.asarray(pos, np.int64))):
        if s == excl or L <= 0:
            continue
        for o in range(-(n - 1), int(L)):
            hist[min(n, int(L) - o) - max(0, -o)] += 1
    return hist


# ------------------------------------------------------------------------------------------------ calibration on iid rows
PLANT_LO, PLANT_ROWS = 300, 40


def iid_world():
    """90 songs of 3..119 random unit rows (d 128), an 800-row recording of random unit rows whose rows 300..339 are the first 40
    rows of the longest song plus unit noise of equal norm, renormalised.  -> (db, pos, recording, planted song)"""
    rng = np.random.default_rng(7)
    d = 128
    unit = lambda x: x / np.linalg.norm(x, axis=1, keepdims=True)
    lens = rng.integers(3, 120, 90)
    pos = np.pad(np.cumsum(lens), (1, 0)).astype(np.int64)
    db = unit(rng.standard_normal((int(pos[-1]), d)))
    rec = unit(rng.standard_normal((800, d)))
    s = int(np.argmax(lens))
    assert lens[s] >= PLANT_ROWS
    rec[PLANT_LO:PLANT_LO + PLANT_ROWS] = unit(db[pos[s]:pos[s] + PLANT_ROWS] + unit(rng.standard_normal((PLANT_ROWS, d))))
    return db.astype(np.float32), pos, rec.astype(np.float32), s
