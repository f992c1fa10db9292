"""How surprising is a dense window's best score, given the scores of all its other alignments?

The dense matcher scores every alignment of every song in a window and can return, beside the best one, the count and the
first two moments of the window's FULL candidates -- the alignments whose n rows all lie inside their song
(pfann_match_windows_dense_stats, include/pfann_amd.h).  Those moments are the window's own background: what a total of n
row dots looks like when the window holds nothing of that song.  This module turns them into the probability that the best
of ALL the window's candidates reaches the observed total by chance:

    p = sum over the overlap lengths m of hist[m] * Q((T - mu * m / n) / sqrt(var * m / n))

T is the best total, mu and var are the mean and the variance of the full totals with the best candidate left out (a true
match must not vouch for itself), a candidate that overlaps its song in only m of the n rows has m / n of both, hist[m] counts
the candidates per overlap length (from the song lengths alone), and Q is the normal upper tail.  It is a union bound under a
normal model of the totals, reported as log10 p (<= 0): a window is a detection at false-alarm level X when log10 p <= log10 X.

A RANKED list (pfann_match_windows_dense_topn_stats: the n best songs of the window and the same moments from one pass) gets one
such number per entry, log10_false_alarms_ranked: entry i is judged with entries 0..i left out of the background.

numpy and math only; pure host code.
"""
import math

import numpy as np

SUM_SHIFT = 24                                          # PFANN_DENSE_STATS_SUM_SHIFT
SQ_SHIFT = 18                                           # PFANN_DENSE_STATS_SQ_SHIFT
STATS_DTYPE = np.dtype([("n_full", "<i8"), ("sum_q", "<i8"), ("sumsq_q", "<i8")])     # pfann_dense_stats
_LOG10E = math.log10(math.e)


def overlap_histogram(song_len, n, excl=-1):
    """-> int64 [n + 1]: entry m = the candidates of a window of n rows whose window overlaps their song in exactly m rows.
    A song of len > 0 rows has the offsets -(n-1) <= o <= len - 1 with m(o) = min(n, len - o) - max(0, -o): two offsets for
    every m below k = min(n, len) -- one at each edge -- and len + n + 1 - 2 k offsets at k.  Song `excl` is left out.
    hist[n] is pfann_dense_stats.n_full, hist.sum() the result's n_cand."""
    n = int(n)
    lens = np.asarray(song_len, dtype=np.int64).copy()
    if 0 <= excl < lens.shape[0]:
        lens[excl] = 0
    lens = lens[lens > 0]
    k = np.minimum(lens, n)
    hist = np.zeros(n + 1, dtype=np.int64)
    if lens.shape[0]:
        np.add.at(hist, k, lens + n + 1 - 2 * k)
        edges = np.bincount(k, minlength=n + 1)[:n + 1]             # songs per k
        above = edges[::-1].cumsum()[::-1]                          # songs with k >= m
        hist[1:n] += 2 * above[2:n + 1]                             # m < k  <=>  k >= m + 1
    return hist


class OverlapHistograms:
    """overlap_histogram of one list of song lengths, kept per (n, excl)"""

    def __init__(self, song_len):
        self.song_len = np.asarray(song_len, dtype=np.int64)
        self._kept = {}

    def __call__(self, n, excl=-1):
        key = (int(n), int(excl))
        if key not in self._kept:
            self._kept[key] = overlap_histogram(self.song_len, key[0], key[1])
        return self._kept[key]


def log10_upper_tail(z):
    """log10 of the normal upper tail Q(z): math.erfc below z = 30, the asymptotic series of its logarithm above (erfc
    underflows near z = 38)"""
    if z < 30.0:
        return math.log10(0.5 * math.erfc(z / math.sqrt(2.0)))
    z2 = z * z
    return (-0.5 * z2 - math.log(z * math.sqrt(2.0 * math.pi)) + math.log1p(-1.0 / z2 + 3.0 / (z2 * z2))) * _LOG10E


def best_total(score, n):
    """the fp32 total behind a dense score = (double)total / (double)n"""
    return float(np.float32(float(score) * int(n)))


def quantised(T):
    """the three integers a full candidate of fp32 total T adds to pfann_dense_stats"""
    return 1, int(round(T * float(1 << SUM_SHIFT))), int(round(T * T * float(1 << SQ_SHIFT)))    # round(): half to even, as rint


def log10_false_alarm(score, n, song, offset, stats, hist, song_len):
    """log10 of the chance that the best of a window's candidates scores `score` or more (module docstring), <= 0.
    score, song, offset: the window's dense answer; n: its rows; stats: its (n_full, sum_q, sumsq_q); hist:
    overlap_histogram for (n, the recording's excluded song); song_len: rows per song.
    0 -- never significant -- when the window has no candidate, when fewer than two full candidates are left beside the best,
    or when their variance is not positive."""
    n, song, offset = int(n), int(song), int(offset)
    if song < 0 or n < 1 or int(np.sum(hist)) == 0:
        return 0.0
    T = best_total(score, n)
    N, S1, S2 = (int(x) for x in stats)
    if 0 <= offset <= int(song_len[song]) - n:          # the best is a full candidate: its own integers are in the sums
        c, s1, s2 = quantised(T)
        N, S1, S2 = N - c, S1 - s1, S2 - s2
    return _log10_tail(T, n, N, S1, S2, hist)


def _log10_tail(T, n, N, S1, S2, hist):
    """the module docstring's formula for a total T against the background (N, S1, S2) of a window of n rows"""
    if N < 2:
        return 0.0
    mu = S1 / float(1 << SUM_SHIFT) / N
    var = S2 / float(1 << SQ_SHIFT) / N - mu * mu
    if not var > 0.0:
        return 0.0
    terms = []
    for m in range(1, n + 1):
        c = int(hist[m])
        if c > 0:
            f = m / float(n)
            terms.append(math.log10(c) + log10_upper_tail((T - mu * f) / math.sqrt(var * f)))
    top = max(terms)
    if top == -math.inf:
        return -math.inf
    return min(0.0, top + math.log10(sum(10.0 ** (t - top) for t in terms)))


def log10_false_alarms(results, stats, n, excl, hists, song_len):
    """log10_false_alarm for every window of one recording: results (song, offset, score fields) and stats (STATS_DTYPE)
    aligned, all windows of n rows, excl the recording's excluded song, hists an OverlapHistograms -> float64 array"""
    hist = hists(n, excl)
    return np.asarray([log10_false_alarm(r["score"], n, r["song"], r["offset"], (s["n_full"], s["sum_q"], s["sumsq_q"]), hist, song_len)
                       for r, s in zip(results, stats)], dtype=np.float64)


def log10_false_alarms_ranked(entries, n, stats, hist, song_len):
    """log10_false_alarm for every entry of one window's ranked list (pfann_match_windows_dense_topn_stats): entries (song,
    offset, score fields, best first, padding song -1 last), n the window's rows, stats its (n_full, sum_q, sumsq_q), hist
    overlap_histogram for (n, the recording's excluded song) -> float64 [len(entries)].
    Entry i is judged against the window's full candidates with entries 0..i left out: every one of them that is itself a full
    candidate (0 <= offset <= len_s - n) takes its three quantised integers out of the sums.  A true match must not vouch for
    itself, nor may a better-ranked one: a second copy of a stretch would inflate the variance the third copy is judged by.
    Only 0..i are taken out, so an entry's value does not depend on how long a list was asked for (the prefix rule), and
    entry 0 is exactly log10_false_alarm.  Padding takes nothing out and gets 0."""
    n = int(n)
    out = np.zeros(len(entries), dtype=np.float64)
    N, S1, S2 = (int(x) for x in stats)
    if n < 1 or int(np.sum(hist)) == 0:
        return out
    for i, e in enumerate(entries):
        song, offset = int(e["song"]), int(e["offset"])
        if song < 0:
            continue
        T = best_total(e["score"], n)
        if 0 <= offset <= int(song_len[song]) - n:
            c, s1, s2 = quantised(T)
            N, S1, S2 = N - c, S1 - s1, S2 - s2
        out[i] = _log10_tail(T, n, N, S1, S2, hist)
    return out
