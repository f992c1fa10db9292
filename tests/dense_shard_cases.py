"""The song-sharded dense matcher restated in numpy (tests/test_dense_shard_host.py, tests/test_gpu_dense_shard.py,
tests/test_gpu_dense_ranks.py).

pfann_match_windows_dense_part leaves, per window, the largest packed word among the candidates of the handle's OWNED songs --
here the pair (float64 total, id) with the candidate numbering of tests/dense_cases.py, id(s, o) = pos[s] + s (n-1) + o + (n-1)
formed from the GLOBAL song_pos --, the three integers over its own full candidates, and (ranked form) the n best of its own
songs.  pfann_match_windows_dense_merge takes the maximum word (higher total, then smaller id), adds the integers and decodes
with the global sizes; pfann_match_windows_dense_topn_merge keeps the n best of all parts' entries by (score descending, song
ascending) and adds n_found.  sharded_oracle does exactly that, part by part; the tests pin it with == to the whole-database
oracles (dense_cases.dense_oracle, dense_stats_cases.stats_oracle, dense_topn_cases.dense_topn_oracle) for every cut below."""
import numpy as np

import dense_cases as dc
import dense_stats_cases as ds
import dense_topn_cases as dt
import monitor_cases as mc

_G = {}


def cuts_of(pos):
    """name -> [(song_lo, song_hi)], contiguous ranges that cover the song list: what dist.shard_songs gives 2 / 3 / 8 ranks, and
    a cut right after the first song that has rows (that shard holds fewer rows than most windows)"""
    from pfann_amd.dist import shard_songs
    pos = np.asarray(pos, np.int64)
    n_songs = pos.shape[0] - 1
    first = int(np.flatnonzero(np.diff(pos) > 0)[0]) + 1
    return {"2": shard_songs(pos, 2), "3": shard_songs(pos, 3), "8": shard_songs(pos, 8), "first": [(0, first), (first, n_songs)]}


def with_rowless_tail(pos):
    """-> (pos with a song without rows appended, {name: cut}): the appended song alone on the second shard, and on the first
    shard with NO song left for the second; either way the second shard has no rows at all"""
    pos = np.append(np.asarray(pos, np.int64), np.int64(pos[-1]))
    n_songs = pos.shape[0] - 1
    return pos, {"rowless-right": [(0, n_songs - 1), (n_songs - 1, n_songs)], "rowless-left": [(0, n_songs), (n_songs, n_songs)]}


def _windows(rstart, rlen, window, hop, excl):
    """-> (first row, rows, excluded song) of every window, in result order"""
    for r, (s, L) in enumerate(zip(rstart, rlen)):
        for w0, n in mc.window_starts(int(L), window, hop):
            yield int(s) + w0, n, -1 if excl is None else int(excl[r])


def part_of_window(G, pos, sg, r0, n, ex, lo, hi):
    """one window on the shard that owns the songs [lo, hi) -> dict: word = (total, id) of its best candidate or None, stats =
    (n_full, sum_q, sumsq_q) over its full candidates, heads = its songs' best candidates ranked, (song, offset, 0, n_cand, score)"""
    lens = np.diff(pos)
    song, off, ok, tot = ds.window_totals(G, pos, sg, r0, n)
    mine = ok & (song >= lo) & (song < hi) & (song != ex)
    ids = np.flatnonzero(mine)
    word = None
    if ids.size:
        b = int(ids[np.argmax(tot[ids])])                # the first maximum: the smallest id
        word = (float(tot[b]), b)
    full = mine & (off >= 0) & (off <= lens[song] - n)
    s1, s2 = ds.quantise(tot[full])
    f = pos + np.arange(pos.shape[0]) * (n - 1)
    heads = []
    for c in range(lo, hi):
        if lens[c] > 0 and c != ex:
            seg = tot[f[c]:f[c] + lens[c] + n - 1]
            b = int(np.argmax(seg))
            heads.append((c, b - (n - 1), 0, int(lens[c]) + n - 1, float(seg[b]) / n))
    heads.sort(key=lambda h: (-h[4], h[0]))
    return dict(word=word, stats=(int(full.sum()), s1, s2), heads=heads)


def merge_of_window(parts, pos, n, ex, n_top):
    """the parts of one window, in any order -> dict(song, offset, shift, score, n_cand, n_full, sum_q, sumsq_q, top, n_found)"""
    lens = np.diff(pos)
    words = [p["word"] for p in parts if p["word"] is not None]
    out = dict(song=-1, offset=0, shift=0, score=-np.inf, n_cand=0)
    if words:
        tot, b = max(words, key=lambda w: (w[0], -w[1]))
        song, off, _ = dc._ids(pos, n)
        n_cand = sum(int(L) + n - 1 for c, L in enumerate(lens) if L > 0 and c != ex)
        out = dict(song=int(song[b]), offset=int(off[b]), shift=0, score=tot / n, n_cand=n_cand)
    out["n_full"], out["sum_q"], out["sumsq_q"] = (sum(p["stats"][i] for p in parts) for i in range(3))
    entries = sorted((e for p in parts for e in p["heads"][:n_top]), key=lambda h: (-h[4], h[0]))
    out["top"] = entries[:n_top] + [dt.PAD] * max(0, n_top - len(entries))
    out["n_found"] = sum(len(p["heads"]) for p in parts)
    return out


def sharded_oracle(q, db, pos, window, hop, rstart, rlen, cut, n_top, excl=None, key=None, reverse=False):
    """-> one merge_of_window dict per window, in result order, from one part_of_window per (window, shard of `cut`).
    key: a name for (q, db): the float64 product is then computed once."""
    pos = np.asarray(pos, np.int64)
    N = int(pos[-1])
    if key is None or key not in _G:
        G = np.asarray(q, np.float64) @ np.asarray(db, np.float64).T if N else np.zeros((len(q), 0))
        if key is not None:
            _G[key] = G
    else:
        G = _G[key]
    sg = np.searchsorted(pos[:-1], np.arange(N), side="right") - 1
    cut = list(cut)[::-1] if reverse else list(cut)
    return [merge_of_window([part_of_window(G, pos, sg, r0, n, ex, lo, hi) for lo, hi in cut], pos, n, ex, n_top)
            for r0, n, ex in _windows(rstart, rlen, window, hop, excl)]


RESULT_FIELDS = ("song", "offset", "shift", "score", "n_cand")
STATS_FIELDS = ("n_full", "sum_q", "sumsq_q")


def against_whole(got, dense, stats, topn):
    """sharded_oracle's windows against the three whole-database oracles' -> messages for the windows that differ, =="""
    bad = []
    for j, (g, a, b, c) in enumerate(zip(got, dense, stats, topn)):
        for what, want, fields in (("result", a, RESULT_FIELDS), ("stats", b, STATS_FIELDS), ("ranked", c, ("top", "n_found"))):
            x, y = tuple(g[f] for f in fields), tuple(want[f] for f in fields)
            if x != y:
                bad.append("window %d %s: sharded %r, whole %r" % (j, what, x, y))
    assert len(got) == len(dense) == len(stats) == len(topn)
    return bad
