"""Inputs and the oracle of the rescoring-stage tests (tests/test_songs_dense_host.py, tests/test_gpu_songs_dense.py).

The rescored list of a query (include/pfann_amd.h, pfann_match_songs_dense): the listed songs are the distinct ids of the list
that name a song with rows; every listed song gets the entry the ranked dense matcher gives it for a window of the query's rows;
the entries rank by score descending, ties to the lower song; padding follows.  songs_dense_oracle takes dense_topn_oracle
(tests/dense_topn_cases.py) for a one-window recording per query, restricts it to the listed songs and re-ranks."""
import numpy as np

import dense_topn_cases as dt
import match_exact as mx

LENGTHS = (1, 2, 19, 63, 64)
MS = (1, 3, 64)


def songs_dense_oracle(q, db, pos, qstart, qlen, lists, key=None):
    """-> one dict per query: top = len(lists[j]) tuples (song, offset, shift, n_cand, score float64) padded with dt.PAD, n_found,
    block None -- what dense_topn_cases.differing compares.  Queries of 1..64 rows, or 0 rows (all padding).  key: a name for
    (q, db, pos): a query's full ranking is then computed once per (qstart, qlen) and shared."""
    pos = np.asarray(pos, np.int64)
    n_songs = pos.shape[0] - 1
    lens = np.diff(pos)
    out = []
    for j, (s, n) in enumerate(zip(qstart, qlen)):
        s, n, m = int(s), int(n), len(lists[j])
        if n == 0:
            out.append(dict(top=[dt.PAD] * m, n_found=0, block=None))
            continue
        assert 1 <= n <= 64
        full = dt.dense_topn_oracle(q[s:s + n], db, pos, n, 1, [0], [n], max(n_songs, 1), key=None if key is None else (key, s, n))
        assert len(full) == 1
        listed = {int(x) for x in lists[j] if 0 <= int(x) < n_songs and lens[int(x)] > 0}
        keep = [h for h in full[0]["top"] if h[0] in listed]                 # (already ranked: score descending, then song)
        assert len(keep) == len(listed)
        out.append(dict(top=keep + [dt.PAD] * (m - len(keep)), n_found=len(keep), block=None))
    return out


def cut_queries(n_rows, lengths=LENGTHS):
    """query slices of the recordings' rows: every length at the first row, in the middle and at the last rows -> (qstart, qlen)"""
    qstart, qlen = [], []
    for L in lengths:
        for s in sorted({0, (n_rows - L) // 2, n_rows - L}):
            qstart.append(int(s))
            qlen.append(int(L))
    return qstart, qlen


def make_lists(pos, n_queries, m, seed):
    """int32 [n_queries, m] of song ids.  Across the queries of a call: padding -1 in the middle of a list, a song twice, a song
    without rows (where the world has one), the id n_songs, the first and the last song of the database, unsorted."""
    pos = np.asarray(pos, np.int64)
    n_songs = pos.shape[0] - 1
    lens = np.diff(pos)
    have, empty = np.flatnonzero(lens > 0), np.flatnonzero(lens == 0)
    rowless = int(empty[0]) if empty.size else n_songs
    special = [0, n_songs - 1, n_songs, -1, rowless, int(have[0]), int(have[-1]), n_songs + 5]
    rng = np.random.default_rng(seed)
    out = np.empty((n_queries, m), np.int32)
    for j in range(n_queries):
        a, b = (int(x) for x in rng.choice(have, 2, replace=False))
        if m == 1:
            out[j] = [(special + [a, b])[j % (len(special) + 2)]]
        elif m == 3:
            out[j] = ([a, -1, b], [a, b, a], [rowless, n_songs - 1, 0], [n_songs, b, -1])[j % 4]
        else:
            pool = rng.choice(have, int(rng.integers(2, have.size + 1)), replace=False)
            row = rng.choice(pool, m)                                    # with replacement: duplicates
            row[m // 2] = -1
            row[m // 2 + 1] = -1
            row[1:1 + len(special)] = special
            row[0], row[m - 1] = a, a
            if j % 3 == 0:                                               # every song with rows, when they fit: the whole ranking
                row[:min(m, have.size)] = have[::-1][:m]
            out[j] = row
    return out


def leak_lengths(n, tile=128):
    """lengths of A: shorter than the query; one candidate fewer than, exactly and one more than a column tile owns
    (len + n - 1 candidates against tile - (n-1) owned columns); one row fewer than, exactly and one more than that width"""
    own = tile - (n - 1)
    return tuple(sorted({max(1, n - 5), max(1, own - (n - 1) - 1), max(1, own - (n - 1)), own - (n - 1) + 1, own - 1, own, own + 1}))


def leak_world(n, d=128, seed=91, a_lens=None):
    """A database in which every song A_i (leak_lengths(n)[i] random grid rows) stands between two songs that hold the query's own rows
    right at A_i's edges: the n-1 rows before A_i are the query's rows 0..n-2, the n-1 rows behind it its rows 1..n-1.  A kernel
    that reads past A_i's first row at offset -(n-1), or past its last at offset len-1, adds n-1 self-products.
    -> (db, pos, q [n, d], ids of the A songs)"""
    a_lens = leak_lengths(n) if a_lens is None else a_lens
    q = mx.grid_rows(seed, "leak/q", n, d)
    filler = lambda tag: mx.grid_rows(seed, "leak/" + tag, 7, d)
    songs, a_ids = [], []
    for i, L in enumerate(a_lens):
        songs.append(np.concatenate([q[1:n], filler("f%d" % i), q[0:n - 1]]))        # behind A_{i-1}, before A_i
        a_ids.append(len(songs))
        songs.append(mx.grid_rows(seed, "leak/a%d" % i, L, d))
    songs.append(np.concatenate([q[1:n], filler("last")]))
    pos = np.pad(np.cumsum([x.shape[0] for x in songs]), (1, 0)).astype(np.int64)
    return np.concatenate(songs).astype(np.float32), pos, q, a_ids
