"""Exact oracle of the ranked top-N matcher (pfann_match_topn, include/pfann_amd.h), on the integer grid of match_exact.py.

Written from the header's semantics, not from the kernel: candidates, their order and their scores are those of
match_exact.exact_match; per song the first candidate in candidate order with the largest float64 score wins (strict >);
songs rank by score descending, ties to the song whose best candidate comes first in candidate order; n_cand of an entry is
the number of distinct candidates of its song; entries past the candidate songs are padding; n_found is the number of
distinct candidate songs."""
import numpy as np

from match_exact import IntRows, assert_exact_domain

PAD = (-1, 0, 0, 0, -np.inf)                 # (song, offset, shift, n_cand, score)
FIELDS = ("song", "offset", "shift", "n_cand", "score")


def exact_topn(q, labels, db, song_pos, fsm, mode, n, song_range=None):
    """One query.  -> dict(top = n tuples (song, offset, shift, n_cand, score float64), padded with PAD; n_found;
    f32_alone = per entry, True when no OTHER candidate of the entry's song rounds to the entry's float32 score (only then is
    the alignment the float32 per-song block records necessarily this entry's))."""
    rows = db if isinstance(db, IntRows) else IntRows(db)
    song_pos = np.asarray(song_pos, np.int64)
    n_songs = song_pos.shape[0] - 1
    q = np.asarray(q)
    qlen, d = q.shape
    assert_exact_domain(qlen, d)
    labels = np.asarray(labels, np.int64).reshape(qlen, -1)
    none = dict(top=[PAD] * n, n_found=0, f32_alone=[True] * n)
    t_idx = np.nonzero(labels >= 0)[0]
    lab = labels[labels >= 0]
    if rows.n == 0 or lab.size == 0:
        return none
    song = np.searchsorted(song_pos[:n_songs], lab, side="right") - 1
    tim, shift = t_idx // fsm, t_idx % fsm
    off = lab - song_pos[song] - tim
    if song_range is not None:
        keep = (song >= song_range[0]) & (song < song_range[1])
        song, off, shift = song[keep], off[keep], shift[keep]
        if song.size == 0:
            return none
    if mode == 0:
        c = np.unique(np.stack([shift, song, off], 1), axis=0)             # candidate order (shift, song, offset)
        shift, song, off = c[:, 0], c[:, 1], c[:, 2]
    else:
        c = np.unique(np.stack([song, off, shift], 1), axis=0)             # candidate order (song, offset, shift)
        song, off, shift = c[:, 0], c[:, 1], c[:, 2]
    nc = c.shape[0]
    sub_len = (qlen - shift + fsm - 1) // fsm
    start = song_pos[song]
    slen = song_pos[song + 1] - start
    G = IntRows(q).t.T @ rows.t                                            # [qlen, rows]: integer dots in units of 1/256
    j = np.arange(int(sub_len.max()))[None, :]
    r = off[:, None] + j
    ok = (j < sub_len[:, None]) & (r >= 0) & (r < slen[:, None])
    qrow = np.minimum(j * fsm + shift[:, None], qlen - 1)
    S = np.where(ok, G[qrow, np.where(ok, start[:, None] + r, 0)], 0.0).sum(1)
    assert np.abs(S).max() < 2 ** 24
    if mode == 0:
        sco = (S / 256.0) / sub_len
    else:
        sco = ((S / 256.0).astype(np.float32) / np.maximum(sub_len, 1).astype(np.float32)).astype(np.float64)
    heads = []                                                             # per song: (best score, index of its first maximum, votes)
    for s in np.unique(song):
        idx = np.flatnonzero(song == s)                                    # ascending: candidate order
        b = idx[int(np.argmax(sco[idx]))]                                  # first maximum, strict >
        heads.append((float(sco[b]), int(b), int(idx.size)))
    heads.sort(key=lambda h: (-h[0], h[1]))
    top, alone = [], []
    for score, b, votes in heads[:n]:
        top.append((int(song[b]), int(off[b]), int(shift[b]), votes, score))
        same = np.flatnonzero((song == song[b]) & (sco.astype(np.float32) == np.float32(score)))
        alone.append(same.size == 1)
    pad = n - len(top)
    return dict(top=top + [PAD] * pad, n_found=len(heads), f32_alone=alone + [True] * pad)


def exact_topn_batch(batch, db, song_pos, fsm, mode, n, song_range=None):
    rows = db if isinstance(db, IntRows) else IntRows(db)
    return [exact_topn(batch.q[s:s + m], batch.labels[s:s + m], rows, song_pos, fsm, mode, n, song_range)
            for s, m in zip(batch.qstart, batch.qlen)]


def as_array(tops, dtype):
    """list of exact_topn results -> structured array [nQ, n] of the library's result dtype"""
    out = np.zeros((len(tops), len(tops[0]["top"])), dtype=dtype)
    for j, t in enumerate(tops):
        for i, e in enumerate(t["top"]):
            out[j, i] = e
    return out
