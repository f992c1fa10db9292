"""Inputs and the oracle of the ranked dense-matcher tests (tests/test_dense_topn_host.py, tests/test_gpu_dense_topn.py).

The ranked dense answer of a window (include/pfann_amd.h, pfann_match_windows_dense_topn): the candidates and totals of the
dense matcher (tests/dense_cases.py); per song the largest total, ties to the smaller offset; songs rank by score descending,
ties to the lower song; n_cand of an entry = len_s + n - 1; padding past the songs; n_found = the songs with rows without the
excluded one; the block row holds (float32 score, float32 offset) where the float32 score is > 0 and zeros elsewhere.
dense_topn_oracle restates that on a float64 q @ db.T; on the grid of match_exact.grid_rows every product and sum is exact."""
import os
import shutil

import numpy as np

import dense_cases as dc
import match_exact as mx
import monitor_cases as mc

PAD = (-1, 0, 0, 0, -np.inf)                 # (song, offset, shift, n_cand, score)
FIELDS = ("song", "offset", "shift", "n_cand", "score")

_G, _HOP1 = {}, {}


def dense_topn_oracle(q, db, pos, window, hop, rstart, rlen, n, excl=None, key=None):
    """-> one dict per window, in result order: top = n tuples (song, offset, shift, n_cand, score float64) padded with PAD,
    n_found, block = float32 [n_songs, 2].  excl: one song id per recording (-1: none).  key: a name for (q, db, pos, rstart,
    rlen): the float64 product and the full hop-1 rankings are then computed once and shared."""
    pos = np.asarray(pos, np.int64)
    n_songs, N = pos.shape[0] - 1, int(pos[-1])
    lens = np.diff(pos)
    if key is None or key not in _G:
        G = np.asarray(q, np.float64) @ np.asarray(db, np.float64).T if N else np.zeros((len(q), 0))
        if key is not None:
            _G[key] = G
    else:
        G = _G[key]
    sg = np.searchsorted(pos[:-1], np.arange(N), side="right") - 1       # song of every db row
    ck = (key, window, None if excl is None else tuple(int(e) for e in excl))
    if key is not None and ck in _HOP1:
        per = _HOP1[ck]
    else:
        per = []
        for r, (s, L) in enumerate(zip(rstart, rlen)):
            ex = -1 if excl is None else int(excl[r])
            ans = []
            for w0, m in mc.window_starts(int(L), window, 1):
                f = pos + np.arange(n_songs + 1) * (m - 1)               # ids of song s: [f[s], f[s + 1]), offset = id - f[s] - (m-1)
                tot = np.zeros(int(f[-1]))
                base = np.arange(N) + sg * (m - 1) + (m - 1)
                for t in range(m):
                    tot[base - t] += G[s + w0 + t]
                heads, block = [], np.zeros((n_songs, 2), np.float32)
                for c in np.flatnonzero(lens > 0):
                    if c == ex:
                        continue
                    seg = tot[f[c]:f[c] + lens[c] + m - 1]
                    b = int(np.argmax(seg))                              # first maximum: the smaller offset
                    score, off = float(seg[b]) / m, b - (m - 1)
                    heads.append((int(c), off, 0, int(lens[c]) + m - 1, score))
                    if np.float32(score) > 0:
                        block[c] = (np.float32(score), np.float32(off))
                heads.sort(key=lambda h: (-h[4], h[0]))
                ans.append((heads, block))
            per.append(ans)
        if key is not None:
            _HOP1[ck] = per
    out = []
    for ans, L in zip(per, rlen):
        for w0, _ in mc.window_starts(int(L), window, hop):
            heads, block = ans[w0]
            out.append(dict(top=heads[:n] + [PAD] * max(0, n - len(heads)), n_found=len(heads), block=block))
    return out


def differing(top, n_found, block, want):
    """-> messages for the windows whose entries, n_found or block row are not the oracle's, compared with =="""
    bad = []
    for j, w in enumerate(want):
        got = [tuple(x.item() for x in (e["song"], e["offset"], e["shift"], e["n_cand"], e["score"])) for e in top[j]]
        if got != w["top"]:
            i = next(i for i in range(len(got)) if got[i] != w["top"][i])
            bad.append("window %d entry %d: kernel %r, oracle %r" % (j, i, got[i], w["top"][i]))
        elif int(n_found[j]) != w["n_found"]:
            bad.append("window %d: n_found %d, oracle %d" % (j, int(n_found[j]), w["n_found"]))
        elif block is not None and not np.array_equal(block[j], w["block"]):
            s = int(np.flatnonzero((block[j] != w["block"]).any(1))[0])
            bad.append("window %d block slot %d: kernel %r, oracle %r" % (j, s, block[j][s].tolist(), w["block"][s].tolist()))
    return bad


def packed_world(d=128, seed=77):
    """200 one-row songs in a row with an empty song after every 16th -- a 128-column tile holds up to 128 distinct songs and a
    stretch of `window` columns up to `window` pieces --, then two songs of 300 rows (longer than a tile).  Two recordings cut
    from it: 90 rows that walk the one-row songs, 150 rows out of the long songs.  -> (db, pos, q, rstart, rlen)"""
    lens = []
    for s in range(200):
        lens.append(1)
        if s % 16 == 15:
            lens.append(0)
    lens += [300, 300]
    pos = np.pad(np.cumsum(lens), (1, 0)).astype(np.int64)
    db = mx.grid_rows(seed, "packed/db", int(pos[-1]), d)
    q = np.concatenate([db[60:150], db[200 + 250:200 + 400]])
    noise = mx.grid_rows(seed, "packed/noise", q.shape[0], d)
    flip = np.random.default_rng(seed).random(q.shape) < 0.2
    q = np.where(flip, noise, q).astype(np.float32)
    return db, pos, q, [0, 90], [90, 150]


def triple_world(dirname):
    """dense_cases.selfmatch_world with a third copy of song 2 (plus 1e-3 noise) appended as song 12, written as a database
    directory.  -> (emb, pos)"""
    emb, pos = dc.selfmatch_world(dirname)
    rng = np.random.default_rng(2027)
    n2 = int(pos[3] - pos[2])
    third = emb[pos[2]:pos[3]].astype(np.float64) + 1e-3 * rng.standard_normal((n2, emb.shape[1]))
    third = (third / np.linalg.norm(third, axis=1, keepdims=True)).astype(np.float32)
    emb = np.concatenate([emb, third])
    pos = np.concatenate([pos, [pos[-1] + n2]]).astype(np.int64)
    with open(os.path.join(dirname, "songList.txt"), "a") as f:
        f.write("song12.wav\n")
    np.diff(pos).astype(np.int32).tofile(os.path.join(dirname, "landmarkKey"))
    emb.tofile(os.path.join(dirname, "embeddings"))
    return emb, pos
