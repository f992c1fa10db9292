"""Inputs and the oracle of the dense-matcher tests (tests/test_dense_host.py, tests/test_gpu_dense.py).

The dense answer of a window of n rows is what the sequence matcher returns for that slice when every row's label list is the
whole database (include/pfann_amd.h, pfann_match_windows_dense): candidates = every (song with rows, offset) with
-(n-1) <= offset <= len - 1, total = the sum of the row dots that fall inside the song, score = total / n, strict-> first-wins
argmax in (song, offset) order, n_cand = sum over the songs with rows of len + n - 1.  dense_oracle restates that on a float64
q @ db.T; on the grid of match_exact.grid_rows every product and sum is exact, so every field compares with ==."""
import json
import os
import shutil

import numpy as np

import match_exact as mx
import monitor_cases as mc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = dict(song=-1, offset=0, shift=0, score=-np.inf, n_cand=0, top=[])


def _ids(pos, n):
    """the candidates of a window of n rows in (song, offset) order: id(s, o) = pos[s] + s * (n-1) + o + (n-1), the ids of a
    song with rows fill [pos[s] + s * (n-1), pos[s+1] + (s+1) * (n-1)).  -> (song of id, offset of id, id is a candidate)"""
    pos = np.asarray(pos, np.int64)
    n_songs = pos.shape[0] - 1
    lens = np.diff(pos)
    f = pos + np.arange(n_songs + 1) * (n - 1)
    M = int(f[-1])
    song = np.repeat(np.arange(n_songs), np.diff(f))
    off = np.arange(M) - f[song] - (n - 1)
    return song, off, lens[song] > 0


_G, _HOP1 = {}, {}


def dense_oracle(q, db, pos, window, hop, rstart, rlen, excl=None, key=None):
    """-> one dict (song, offset, shift, score, n_cand, top = best three for messages) per window, in result order.
    excl: one song id per recording (-1: none) whose alignments are no candidates.  key: a name for (q, db, pos, rstart, rlen,
    excl): the float64 product and the hop-1 answers are then computed once and shared (a window's answer does not depend on
    the hop that reached it)."""
    pos = np.asarray(pos, np.int64)
    N = int(pos[-1])
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
        per, tabs = [], {}
        for r, (s, L) in enumerate(zip(rstart, rlen)):
            ex = -1 if excl is None else int(excl[r])
            ans = []
            for w0, n in mc.window_starts(int(L), window, 1):
                if n not in tabs:
                    tabs[n] = _ids(pos, n)
                song, off, ok = tabs[n]
                ok = ok & (song != ex)
                if not ok.any():
                    ans.append(NONE)
                    continue
                tot = np.zeros(song.shape[0])
                base = np.arange(N) + sg * (n - 1) + (n - 1)
                for t in range(n):                           # row t of the window meets db row g on the alignment id base[g] - t
                    tot[base - t] += G[s + w0 + t]
                sco = np.where(ok, tot / n, -np.inf)
                b = int(np.argmax(sco))                      # first maximum in (song, offset) order
                top = [(int(song[i]), int(off[i]), 0, float(sco[i])) for i in np.lexsort((np.arange(sco.shape[0]), -sco))[:3]]
                ans.append(dict(song=int(song[b]), offset=int(off[b]), shift=0, score=float(sco[b]), n_cand=int(ok.sum()), top=top))
            per.append(ans)
        if key is not None:
            _HOP1[ck] = per
    out = []
    for ans, L in zip(per, rlen):
        out += [ans[w0] for w0, _ in mc.window_starts(int(L), window, hop)]
    return out


def small_world(d=128, lo=3, hi=14):
    """songs lo..hi-1 of the standard world: ~200 rows with a copied pair (5, 9) and a periodic song (5, period 4), a one-row
    song (3), and three short recordings cut from it -- aligned pieces, exact ties, song edges.
    -> (db, pos, q, rstart, rlen)"""
    full, fpos = mx.std_world(41, d)
    db = np.ascontiguousarray(full[fpos[lo]:fpos[hi]])
    pos = (fpos[lo:hi + 1] - fpos[lo]).astype(np.int64)
    a = mx.aligned(610, db, pos, [23, 30, 7], 2)
    t = mx.tie_storm(611, db, pos, [21, 26, 9], 2, ((5 - lo, 9 - lo),), ((5 - lo, 4),))
    e = mx.edges(612, db, pos, [12, 19, 5], 2)
    parts = [a.q, t.q, e.q]
    rlen = [int(p.shape[0]) for p in parts]
    rstart = [int(x) for x in np.pad(np.cumsum(rlen), (1, 0))[:-1]]
    return db, pos, np.concatenate(parts), rstart, rlen


def all_labels(n_rows, ntotal):
    """every db row as a label of every query row"""
    return np.tile(np.arange(ntotal, dtype=np.int64), (n_rows, 1))


# ------------------------------------------------------------------------------------------------ the self-match world
SELF_D, SELF_K, SELF_WINDOW, SELF_HOP, SELF_HOP_S, SELF_MID = 128, 100, 19, 2, 0.5, 17


def selfmatch_world(dirname):
    """the duplicate world of tests/test_gpu_selfmatch.py, written as a database directory: 12 songs of 40..80 random unit
    rows, song 7 is song 2 under another name (plus 1e-3 noise), song 9 carries rows 10..40 of song 4 from its row SELF_MID on,
    song 5 has no rows.  -> (emb, pos)"""
    rng = np.random.default_rng(2026)
    key = rng.integers(40, 81, 12)
    key[5] = 0
    key[7] = key[2]
    key[9] = max(int(key[9]), SELF_MID + 30 + 8)
    pos = np.pad(np.cumsum(key), (1, 0)).astype(np.int64)
    emb = rng.standard_normal((int(pos[-1]), SELF_D))
    emb[pos[7]:pos[8]] = emb[pos[2]:pos[3]] / np.linalg.norm(emb[pos[2]:pos[3]], axis=1, keepdims=True) \
        + 1e-3 * rng.standard_normal((int(key[2]), SELF_D))
    emb[pos[9] + SELF_MID:pos[9] + SELF_MID + 30] = emb[pos[4] + 10:pos[4] + 40]
    emb = (emb / np.linalg.norm(emb, axis=1, keepdims=True)).astype(np.float32)
    shutil.copy(os.path.join(REPO, "configs", "default.json"), os.path.join(dirname, "configs.json"))
    with open(os.path.join(dirname, "songList.txt"), "w") as f:
        f.write("".join("song%02d.wav\n" % s for s in range(12)))
    key.astype(np.int32).tofile(os.path.join(dirname, "landmarkKey"))
    emb.tofile(os.path.join(dirname, "embeddings"))
    return emb, pos


# ------------------------------------------------------------------------------------------------ the end-to-end scenario
def four_excerpts(tmp_path):
    """the scenario of tests/test_gpu_monitor.py::test_monitor_cli_finds_four_excerpts: 50 synthetic songs, the seeded weights
    with the calibrated head, a 180 s recording of four excerpts at SNR 0 with noise between them.  Writes the model directory,
    the songs, music.txt, rec.wav and recs.txt (the recording and a missing file) under tmp_path.
    -> (params, model dir, music paths, truth [(t0, t1, song, offset_s)])"""
    import torch
    from pfann_amd import synth
    params = json.load(open(os.path.join(REPO, "configs", "default.json")))
    sd = synth.make_state_dict_calibrated(params, seed=123)
    mdir = tmp_path / "model"
    mdir.mkdir()
    torch.save({n: torch.from_numpy(v) for n, v in sd.items()}, str(mdir / "model.pt"))
    shutil.copy(os.path.join(REPO, "configs", "default.json"), str(mdir / "configs.json"))
    sr, n_songs = 8000, 50
    music, songs = [], []
    for s in range(n_songs):
        path = str(tmp_path / ("song%02d.wav" % s))
        songs.append(synth.make_song(500 + s, seconds=40.0 + (s % 7)))
        synth.write_wav(path, songs[-1])
        music.append(path)
    (tmp_path / "music.txt").write_text("".join(p + "\n" for p in music))
    plan = [(None, 0, 12), (7, 5, 35), (None, 0, 10), (23, 0, 30), (None, 0, 14), (41, 12, 25), (None, 0, 9), (7, 20, 20), (None, 0, 25)]
    parts, truth, t = [], [], 0.0
    for j, (s, o, n) in enumerate(plan):
        noise = synth.normal(77, "mon/e2e/%d" % j, n * sr).astype(np.float64)
        if s is None:
            x = noise * 2000.0
        else:
            sig = songs[s][o * sr:(o + n) * sr].astype(np.float64)
            x = sig + noise * np.sqrt(np.mean(sig ** 2))          # SNR 0 dB
            truth.append((t, t + n, s, float(o)))
        parts.append(x)
        t += n
    rec = np.concatenate(parts)
    rec = np.clip(rec / np.abs(rec).max() * 30000.0, -32768, 32767).astype(np.int16)
    synth.write_wav(str(tmp_path / "rec.wav"), rec)
    (tmp_path / "recs.txt").write_text(str(tmp_path / "rec.wav") + "\n" + str(tmp_path / "missing.wav") + "\n")
    return params, str(mdir), music, truth
