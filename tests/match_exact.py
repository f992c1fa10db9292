"""Exact-arithmetic checks of the sequence matcher (csrc/rerank.hip): inputs on which fp32 is exact, an int64-grade oracle, the
launch plan a call takes, and label generators that each stress one thing.

Rows are drawn from the grid {j/16 : |j| <= 16}: every value is exact in fp16 and fp32, every product is a multiple of 1/256 of
magnitude <= 1, so any partial sum of up to qlen * d <= 65536 products is a multiple of 1/256 below 2^24 and exact in fp32 in ANY
summation order, with or without fma.  The matcher's fp32 dot therefore equals the integer dot / 256 whatever lanes, unrolling
or path produced it; equal scores are really equal; and every output field can be asserted with `==`.

exact_match is written from the reference's semantics (database.py:129-163 `query_embeddings_base`, mode 0;
cpp/seqscore.cpp:49-135 `seq_score`, mode 1) and pinned against oracle/seqscore.py and oracle/seqscore_c.c by
tests/test_match_exact.py.  Integers are carried in float64 (every intermediate is an integer below 2^53, so BLAS is exact)."""
import os
from collections import namedtuple

import numpy as np

from pfann_amd import synth

MAXC = 8192            # csrc/rerank.hip: candidate slots of the in-LDS list
PHASED_MAX = 64        # csrc/api.hip pfann_match: up to here the three-launch (phased) form
PLANS = ("phased_rank", "phased_lds", "phased_hbm", "single_lds", "single_hbm")

Batch = namedtuple("Batch", "q labels qstart qlen")


# ------------------------------------------------------------------------------------------------ the exact domain
def _ri(seed, tag, n, lo, hi):
    """n int64 values in [lo, hi), a pure function of (seed, tag)."""
    u = synth.uniform01(seed, "mx/" + tag, n).astype(np.float64)
    return lo + np.minimum(np.floor(u * (hi - lo)).astype(np.int64), hi - lo - 1)


def grid_rows(seed, tag, n, d):
    """float32 [n, d] on the grid {j/16 : |j| <= 16}, a pure function of its arguments."""
    return (_ri(seed, "grid/" + tag, n * d, -16, 17).reshape(n, d) / 16.0).astype(np.float32)


def unit_grid_rows(seed, tag, n, d):
    """float32 [n, d] grid rows of norm exactly 1: sixteen coordinates of +-1/4 (for score_alpha > 0, whose
    exp(-alpha (1 - ip)^2) is flat at 0 on rows of norm ~7)."""
    u = synth.uniform01(seed, "mx/unit/" + tag, n * d).reshape(n, d)
    cols = np.argsort(u, axis=1, kind="stable")[:, :16]
    sign = np.where(_ri(seed, "unit/s/" + tag, n * 16, 0, 2).reshape(n, 16) == 0, -0.25, 0.25)
    out = np.zeros((n, d), np.float32)
    np.put_along_axis(out, cols, sign.astype(np.float32), axis=1)
    return out


def assert_exact_domain(max_qlen, d):
    assert max_qlen * d <= 65536, "qlen %d x d %d leaves the domain on which fp32 sums are exact" % (max_qlen, d)


class IntRows:
    """Grid rows as integers (units of 1/16), transposed, in float64: t[d, n]."""

    def __init__(self, rows):
        a = np.asarray(rows, np.float64) * 16.0
        assert np.array_equal(a, np.rint(a)) and (a.size == 0 or np.abs(a).max() <= 16), "rows are not on the grid"
        self.n, self.d = a.shape
        self.t = np.ascontiguousarray(a.T)


# ------------------------------------------------------------------------------------------------ the oracle
def exact_match(q, labels, db, song_pos, fsm, mode, song_range=None):
    """One query.  -> dict(song, offset, shift, score (float64), n_cand, ss float32 [n_songs, 2] = (best score, alignment in
    fine frames t * fsm - shift), top = the three best candidates (song, offset, shift, score) for messages).
    mode 0: candidates ordered (shift, song, offset), strict `>` first wins, score = dot / sub_len in float64, per-song slot
    float32 and compared as float32.  mode 1 (alpha 0): order (song, offset, shift), score = fp32 dot / fp32 sub_len, ties to
    the smaller song.  song_range (lo, hi): only candidates of those songs (the owner side of a sharded database)."""
    rows = db if isinstance(db, IntRows) else IntRows(db)
    song_pos = np.asarray(song_pos, np.int64)
    n_songs = song_pos.shape[0] - 1
    q = np.asarray(q)
    qlen, d = q.shape
    assert_exact_domain(qlen, d)
    labels = np.asarray(labels, np.int64).reshape(qlen, -1)
    ss = np.zeros((n_songs, 2), np.float32)
    none = dict(song=-1, offset=0, shift=0, score=-np.inf, n_cand=0, ss=ss, top=[])
    t_idx = np.nonzero(labels >= 0)[0]
    lab = labels[labels >= 0]
    if rows.n == 0 or lab.size == 0:
        return none
    assert lab.max() < song_pos[-1]
    song = np.searchsorted(song_pos[:n_songs], lab, side="right") - 1
    tim, shift = t_idx // fsm, t_idx % fsm
    off = lab - song_pos[song] - tim
    if song_range is not None:
        keep = (song >= song_range[0]) & (song < song_range[1])
        song, off, shift = song[keep], off[keep], shift[keep]
        if song.size == 0:
            return none
    if mode == 0:
        c = np.unique(np.stack([shift, song, off], 1), axis=0)
        shift, song, off = c[:, 0], c[:, 1], c[:, 2]
    else:
        c = np.unique(np.stack([song, off, shift], 1), axis=0)
        song, off, shift = c[:, 0], c[:, 1], c[:, 2]
    nc = c.shape[0]
    sub_len = (qlen - shift + fsm - 1) // fsm
    start = song_pos[song]
    slen = song_pos[song + 1] - start
    G = IntRows(q).t.T @ rows.t                              # [qlen, n]: integer dots in units of 1/256
    j = np.arange(int(sub_len.max()))[None, :]
    r = off[:, None] + j
    ok = (j < sub_len[:, None]) & (r >= 0) & (r < slen[:, None])
    qrow = np.minimum(j * fsm + shift[:, None], qlen - 1)
    S = np.where(ok, G[qrow, np.where(ok, start[:, None] + r, 0)], 0.0).sum(1)
    assert np.abs(S).max() < 2 ** 24
    if mode == 0:
        sco = (S / 256.0) / sub_len                          # database.py:157: exact fp32 dot, divided in float64
    else:
        sco = ((S / 256.0).astype(np.float32) / np.maximum(sub_len, 1).astype(np.float32)).astype(np.float64)
    b = int(np.argmax(sco))                                  # first maximum in candidate order
    # per song: the slot is float32 and the comparison happens in float32, so the first candidate of the song that reaches
    # the largest ROUNDED score wins, if that is > 0
    s32 = sco.astype(np.float32)
    o = np.lexsort((np.arange(nc), -s32.astype(np.float64), song))
    first = o[np.unique(song[o], return_index=True)[1]]
    first = first[s32[first] > 0]
    ss[song[first], 0] = s32[first]
    ss[song[first], 1] = (off[first] * fsm - shift[first]).astype(np.float32)
    top = [(int(song[i]), int(off[i]), int(shift[i]), float(sco[i])) for i in np.lexsort((np.arange(nc), -sco))[:3]]
    return dict(song=int(song[b]), offset=int(off[b]), shift=int(shift[b]), score=float(sco[b]), n_cand=nc, ss=ss, top=top)


def exact_batch(batch, db, song_pos, fsm, mode, song_range=None):
    rows = db if isinstance(db, IntRows) else IntRows(db)
    return [exact_match(batch.q[s:s + n], batch.labels[s:s + n], rows, song_pos, fsm, mode, song_range)
            for s, n in zip(batch.qstart, batch.qlen)]


def n_top_ties(q, labels, db, song_pos, fsm, mode):
    """number of distinct candidates that reach the best score of this query"""
    w = exact_match(q, labels, db, song_pos, fsm, mode)
    return sum(1 for t in w["top"] if t[3] == w["score"])


# ------------------------------------------------------------------------------------------------ the plan
def match_plan(nQ, max_qlen, k):
    """-> (plan, dedup): which launches pfann_match (csrc/api.hip) and launch_match (csrc/rerank.hip) make for this call, and
    how the longest query's candidate list loses its duplicates: 'count' (the rank sort keeps them, phase 3 counts the distinct
    keys), 'compact' (register compaction, lists of <= 8192 keys) or 'resort' (blank and sort again)."""
    assert os.environ.get("PFANN_MATCH_PHASED_MAX") is None and os.environ.get("PFANN_NO_RANK_SORT") is None
    assert os.environ.get("PFANN_PROF_LAYERS") is None
    P = 1
    while P < max_qlen * k:
        P <<= 1
    if nQ <= PHASED_MAX:
        if 1024 <= P <= 4096:
            return "phased_rank", "count"
        if P <= MAXC:
            return "phased_lds", "compact"
        return "phased_hbm", "resort"
    if P > MAXC:
        return "single_hbm", "resort"
    return "single_lds", "compact"


def coarse_entries(n_songs):
    """the songs whose song_pos entry the matcher's coarse lookup table holds (every 2^cshift-th, csrc/rerank.hip)"""
    cshift = 0
    while (n_songs >> cshift) > 1023:
        cshift += 1
    return [i << cshift for i in range((n_songs >> cshift) + 1)]


# ------------------------------------------------------------------------------------------------ worlds
def make_world(seed, tag, key, d, copies=(), periodic=(), rows=grid_rows):
    """-> (db float32 [n, d], song_pos int64 [n_songs + 1]).  key: rows per song; periodic (song, p): the song's rows repeat
    with period p; copies (src, dst): song dst becomes a byte-identical copy of song src (and takes its length)."""
    key = [int(x) for x in key]
    for src, dst in copies:
        key[dst] = key[src]
    pos = np.pad(np.cumsum(np.asarray(key, np.int64)), (1, 0))
    db = rows(seed, "w/" + tag, int(pos[-1]), d)
    for s, p in periodic:
        seg = db[pos[s]:pos[s + 1]]
        seg[:] = seg[np.arange(seg.shape[0]) % p]
    for src, dst in copies:
        db[pos[dst]:pos[dst + 1]] = db[pos[src]:pos[src + 1]]
    return db, pos


def _pack(items, d, k):
    qlen = [x[0].shape[0] for x in items]
    qstart = np.pad(np.cumsum(qlen), (1, 0))[:-1]
    q = np.concatenate([x[0] for x in items]).astype(np.float32).reshape(-1, d)
    labels = np.concatenate([x[1] for x in items]).astype(np.int64).reshape(-1, k)
    return Batch(q, labels, [int(x) for x in qstart], [int(x) for x in qlen])


def _cut(db, pos, s, off, qlen, fsm, fill):
    """query rows along the alignment (song s, offset off): row t is db row off + t // fsm of the song, `fill` where that
    leaves the song.  -> (q, label of every row or -1)"""
    r = off + np.arange(qlen) // fsm
    ok = (r >= 0) & (r < pos[s + 1] - pos[s])
    q = fill.copy()
    q[ok] = db[pos[s] + r[ok]]
    return q, np.where(ok, pos[s] + r, -1)


def _songs_with_rows(pos):
    return np.flatnonzero(np.diff(pos) > 0)


# ------------------------------------------------------------------------------------------------ label generators
def aligned(seed, db, pos, qlens, k, fsm=1):
    """the true alignment in one (seeded) column of every row, grid-random distractor rows in the others; a quarter of the
    query's coordinates are replaced by grid noise"""
    n, d = db.shape
    have = _songs_with_rows(pos)
    items = []
    for j, ql in enumerate(qlens):
        tag = "al%d" % j
        s = int(have[_ri(seed, tag + "/s", 1, 0, have.size)[0]])
        off = int(_ri(seed, tag + "/o", 1, -2, pos[s + 1] - pos[s])[0])
        noise = grid_rows(seed, tag + "/n", ql, d)
        q, lab = _cut(db, pos, s, off, ql, fsm, noise)
        q = np.where(_ri(seed, tag + "/m", ql * d, 0, 4).reshape(ql, d) == 0, noise, q)
        L = _ri(seed, tag + "/L", ql * k, 0, n).reshape(ql, k)
        col = _ri(seed, tag + "/c", ql, 0, k)
        t = np.flatnonzero(lab >= 0)
        L[t, col[t]] = lab[t]
        items.append((q, L))
    return _pack(items, d, k)


def tie_storm(seed, db, pos, qlens, k, copies, periodic, fsm=1, kinds=(0, 1, 2, 3)):
    """queries cut WITHOUT noise from copied and periodic songs, labelled with every alignment that ties with the true one
    (the other copy, the offsets one or more periods away), in an order that differs from row to row; every fourth query is
    all zero (kind 1: every score 0) and every fourth is the negated cut with tying labels only (kind 3: best score < 0);
    kind 4 is the plain cut with tying labels only; kinds: the cycle of query kinds"""
    n, d = db.shape
    per = dict(periodic)
    pairs = list(copies)
    items = []
    for j, ql in enumerate(qlens):
        tag = "ts%d" % j
        kind = kinds[j % len(kinds)]
        src, dst = pairs[j % len(pairs)]
        p = per.get(src)
        slen = int(pos[src + 1] - pos[src])
        off = int(_ri(seed, tag + "/o", 1, 0, max(1, slen - 1))[0])
        noise = grid_rows(seed, tag + "/n", ql, d)
        q, _ = _cut(db, pos, src, off, ql, fsm, noise)
        offs = [off] if p is None else [o for o in range(off % p - p, slen + p, p)]
        targets = [(s, o) for o in offs for s in (dst, src)]                         # every one of them ties (inside the song)
        L = _ri(seed, tag + "/L", ql * k, 0, n).reshape(ql, k)
        n_tie = k if kind >= 3 else min(k, max(2, (3 * k) // 4))
        for t in range(ql):
            labs = []
            for s, o in targets:
                r = o + t // fsm
                if 0 <= r < pos[s + 1] - pos[s]:
                    labs.append(int(pos[s] + r))
            for i in range(n_tie):
                L[t, i] = labs[(t + i) % len(labs)] if labs else -1
        if kind == 1:
            q = np.zeros_like(q)
        elif kind == 3:
            q = -q
        items.append((q, L))
    return _pack(items, d, k)


def edges(seed, db, pos, qlens, k, fsm=1):
    """labels on the first and last rows of songs (offsets down to -(qlen - 1) // fsm, alignments that run past the end), in
    one-row songs, next to songs without rows, in the first and the last song that has rows; every fifth query has scattered
    -1, every fifth whole rows of -1, every fifth is all -1"""
    n, d = db.shape
    n_songs = pos.shape[0] - 1
    have = _songs_with_rows(pos)
    lens = np.diff(pos)
    special = [int(have[0]), int(have[-1])] + [int(s) for s in have if lens[s] == 1]
    for s in np.flatnonzero(lens == 0):
        special += [int(x) for x in (s - 1, s + 1) if 0 <= x < n_songs and lens[x] > 0]
    items = []
    for j, ql in enumerate(qlens):
        tag = "ed%d" % j
        kind = j % 5
        s = special[j % len(special)]
        first, last = int(pos[s]), int(pos[s + 1] - 1)
        noise = grid_rows(seed, tag + "/n", ql, d)
        off = -((ql - 1) // fsm) // 2 if j % 2 == 0 else int(lens[s]) - 1 - ((ql - 1) // fsm) // 2
        q, lab = _cut(db, pos, s, off, ql, fsm, noise)
        L = _ri(seed, tag + "/L", ql * k, 0, n).reshape(ql, k)
        near = [int(x) for x in have[max(0, np.searchsorted(have, s) - 1): np.searchsorted(have, s) + 2]]
        ends = [first, last] + [int(pos[x]) for x in near] + [int(pos[x + 1] - 1) for x in near]
        for t in range(ql):
            for i in range(min(k, len(ends) + 1)):
                L[t, (t + i) % k] = ends[i - 1] if i else (lab[t] if lab[t] >= 0 else first)
        if kind == 2:
            L[_ri(seed, tag + "/x", ql * k, 0, 10).reshape(ql, k) < 3] = -1
        elif kind == 3:
            L[::2] = -1
        elif kind == 4:
            L[:] = -1
        items.append((q, L))
    return _pack(items, d, k)


def collapse(seed, db, pos, qlens, k, fsm=1):
    """labels[t][i] = base + t // fsm for every i, -1 from the end of base's song on: one candidate per shift
    (n_cand == min(fsm, qlen))"""
    n, d = db.shape
    have = _songs_with_rows(pos)
    items = []
    for j, ql in enumerate(qlens):
        tag = "co%d" % j
        s = int(have[_ri(seed, tag + "/s", 1, 0, have.size)[0]])
        off = int(_ri(seed, tag + "/b", 1, 0, max(1, (pos[s + 1] - pos[s]) // 2))[0])
        q, lab = _cut(db, pos, s, off, ql, fsm, grid_rows(seed, tag + "/q", ql, d))
        if j % 2:
            q = grid_rows(seed, tag + "/r", ql, d)
        items.append((q, np.repeat(lab[:, None], k, axis=1)))
    return _pack(items, d, k)


def full(seed, db, pos, qlens, k, fsm=1):
    """all qlen * k candidates distinct (label - t // fsm takes qlen * k different values, in a seeded order): with qlen * k
    a power of two the candidate list has no padding and n_cand == P.  Needs qlen * k + qlen rows."""
    n, d = db.shape
    items = []
    for j, ql in enumerate(qlens):
        tag = "fu%d" % j
        assert n >= ql * k + ql
        base = int(_ri(seed, tag + "/b", 1, 0, n - ql * k - ql + 1)[0])
        perm = np.argsort(synth.uniform01(seed, "mx/" + tag + "/p", ql * k), kind="stable").reshape(ql, k)
        L = base + (np.arange(ql) // fsm)[:, None] + perm
        q = grid_rows(seed, tag + "/q", ql, d)
        items.append((q, L))
    return _pack(items, d, k)


LADDER = (1, 3, 1023, 1024, 1025, 2047, 2048, 5000)


def ladder_world(seed, n_songs, d):
    """n_songs songs of 0..3 rows (uneven), the first and the last one with rows"""
    key = _ri(seed, "lad/key%d" % n_songs, n_songs, 0, 4)
    key[0] = max(key[0], 2)
    key[-1] = max(key[-1], 1)
    return make_world(seed, "lad%d" % n_songs, key, d)


def ladder(seed, db, pos, qlens, k, fsm=1):
    """labels on the first and the last row of the songs on either side of coarse-table entries (the first ones, the last
    ones and seeded ones in between); the query is cut from one of them"""
    n, d = db.shape
    n_songs = pos.shape[0] - 1
    ent = coarse_entries(n_songs)
    lens = np.diff(pos)
    items = []
    for j, ql in enumerate(qlens):
        tag = "la%d" % j
        pick = [ent[0], ent[-1], ent[len(ent) // 2]] + [ent[int(x)] for x in _ri(seed, tag + "/e", 3, 0, len(ent))]
        if j % 3 == 1:
            pick = ent[:6]
        elif j % 3 == 2:
            pick = ent[-6:]
        songs = sorted({s for e in pick for s in (e - 1, e, e + 1) if 0 <= s < n_songs and lens[s] > 0})
        ends = [int(pos[s]) for s in songs] + [int(pos[s + 1] - 1) for s in songs]
        s0 = songs[j % len(songs)]
        q, lab = _cut(db, pos, s0, 0, ql, fsm, grid_rows(seed, tag + "/n", ql, d))
        L = _ri(seed, tag + "/L", ql * k, 0, n).reshape(ql, k)
        for t in range(ql):
            for i in range(min(k, len(ends))):
                L[t, (t + i) % k] = ends[(i + t) % len(ends)]
            if lab[t] >= 0:
                L[t, t % k] = lab[t]
        items.append((q, L))
    return _pack(items, d, k)


# ------------------------------------------------------------------------------------------------ the standard world
STD_COPIES = ((5, 9), (12, 30), (20, 41))
STD_PERIODIC = ((5, 4), (20, 3))


def std_world(seed, d, long_rows=0):
    """56 songs of 0..39 rows: songs 0, 17, 18 and the last without rows, songs 3 and 25 with one row, songs 9 / 30 / 41
    copies of 5 / 12 / 20, songs 5 and 20 (and their copies) periodic; with long_rows, three songs of that many rows follow
    (room for the `full` generator), separated by a rowless and a one-row song."""
    key = _ri(seed, "std/key", 56, 2, 40)
    key[[0, 17, 18, 55]] = 0
    key[[3, 25]] = 1
    key[[5, 12, 20]] = (23, 31, 17)
    key = [int(x) for x in key]
    if long_rows:
        key = key[:-1] + [long_rows, 0, long_rows, 1, long_rows, 0]
    return make_world(seed, "std%d_%d" % (d, long_rows), key, d, STD_COPIES, STD_PERIODIC)
