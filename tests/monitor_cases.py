"""Inputs and oracles of the monitor-mode tests (tests/test_monitor_host.py, tests/test_gpu_monitor.py): recordings on the
exact grid of tests/match_exact.py, the window rule restated in plain Python, and float64 re-scoring of one candidate.

Run as a script (`python tests/monitor_cases.py exact-general`) it checks pfann_match_windows against the exact oracle in
THIS process -- the GPU test starts it with PFANN_WINDOWS_GENERAL=1 in the environment, which the library reads per call."""
import os
import sys

import numpy as np

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import match_exact as mx

WINDOWS = (1, 5, 19, 64)
HOPS = (1, 2, 7)


def window_starts(L, window, hop):
    """the rule of include/pfann_amd.h in plain Python: starts 0, hop, .. while w0 + window <= L; one window over all rows
    when 0 < L < window; none when L == 0.  -> [(w0, rows of the window)]"""
    if L <= 0:
        return []
    if L < window:
        return [(0, L)]
    out, w0 = [], 0
    while w0 + window <= L:
        out.append((w0, window))
        w0 += hop
    return out


def wfirst_of(rlen, window, hop):
    return np.pad(np.cumsum([len(window_starts(int(L), window, hop)) for L in rlen]), (1, 0)).astype(np.int64)


def expand(rstart, rlen, window, hop):
    """-> (qstart, qlen) of every window of every recording, in result order"""
    qs, ql = [], []
    for s, L in zip(rstart, rlen):
        for w0, n in window_starts(int(L), window, hop):
            qs.append(int(s) + w0)
            ql.append(n)
    return qs, ql


def grid_recordings(d, k, fsm=1, rows=mx.grid_rows, world=None, seed=300):
    """-> (db, pos, q, labels, rstart, rlen): five recordings over the standard world -- `aligned` pieces cut from many songs
    (random distractor labels, a quarter of the coordinates noise), `tie_storm` pieces (copied and periodic songs: exact
    ties), `edges` pieces (first / last rows of songs, scattered and whole rows of -1 labels, an all -1 piece), one
    recording of 11 rows (shorter than most windows) and an empty one.  Pieces are 3..45 rows and songs at most 39, so
    windows straddle song edges and piece seams all the time.  Recordings hold 60..300 rows."""
    db, pos = world if world is not None else mx.std_world(41, d)
    ql_a = [3 + (11 * j + 5) % 43 for j in range(11)]
    ql_t = [4 + (7 * j + 2) % 30 for j in range(8)]
    ql_e = [5 + (5 * j + 1) % 24 for j in range(10)]
    a = mx.aligned(seed, db, pos, ql_a, k, fsm)
    t = mx.tie_storm(seed + 1, db, pos, ql_t, k, mx.STD_COPIES, mx.STD_PERIODIC if rows is mx.grid_rows else (), fsm)
    e = mx.edges(seed + 2, db, pos, ql_e, k, fsm)
    s = mx.aligned(seed + 3, db, pos, [11], k, fsm)
    parts = [a, t, e, s]
    q = np.concatenate([p.q for p in parts])
    labels = np.concatenate([p.labels for p in parts])
    rlen = [int(p.q.shape[0]) for p in parts] + [0]
    rstart = [int(x) for x in np.pad(np.cumsum(rlen), (1, 0))[:-1]]
    assert all(60 <= L <= 300 for L in rlen[:3]), rlen
    return db, pos, q, labels, rstart, rlen


_EXACT = {}


def exact_windows(key, q, labels, rstart, rlen, db_rows, pos, window, hop, fsm=1, mode=0):
    """match_exact.exact_match of every window, in result order; the hop-1 answers are computed once per (key, window)
    and the other hops take their subset (a window's answer does not depend on the hop that reached it)"""
    ck = (key, window, fsm, mode)
    if ck not in _EXACT:
        per = []
        for s, L in zip(rstart, rlen):
            per.append([mx.exact_match(q[s + w0:s + w0 + n], labels[s + w0:s + w0 + n], db_rows, pos, fsm, mode)
                        for w0, n in window_starts(int(L), window, 1)])
        _EXACT[ck] = per
    out = []
    for per, L in zip(_EXACT[ck], rlen):
        out += [per[w0] for w0, _ in window_starts(int(L), window, hop)]
    return out


def differing(res, want):
    """-> messages for the windows whose (song, offset, shift, score, n_cand) is not the oracle's, compared with =="""
    bad = []
    for j, w in enumerate(want):
        r = res[j]
        got = (int(r["song"]), int(r["offset"]), int(r["shift"]), float(r["score"]), int(r["n_cand"]))
        exp = (w["song"], w["offset"], w["shift"], w["score"], w["n_cand"])
        if got != exp:
            bad.append("window %d: kernel (song, offset, shift, score, n_cand) %r, oracle %r, oracle's best three %r"
                       % (j, got, exp, w["top"]))
    return bad


def score64(db, pos, q, song, off, shift=0, fsm=1, alpha=None):
    """one candidate of one window restated in float64: mean of the row dots (alpha None: rows outside the song add 0), or
    of exp(-alpha (1 - dot)^2) over the rows inside the song; the divisor is always sub_len"""
    sub = np.asarray(q, np.float64)[shift::fsm]
    slen = int(pos[song + 1] - pos[song])
    tot = 0.0
    for j in range(sub.shape[0]):
        if 0 <= off + j < slen:
            ip = float(sub[j] @ np.asarray(db[pos[song] + off + j], np.float64))
            tot += ip if alpha is None else np.exp(-alpha * (1.0 - ip) ** 2)
    return tot / max(sub.shape[0], 1)


def candidates(labels, pos, fsm=1):
    """unique (song, offset, shift) nominated by a window's labels"""
    labels = np.asarray(labels, np.int64)
    t, _ = np.nonzero(labels >= 0)
    lab = labels[labels >= 0]
    song = np.searchsorted(pos[:-1], lab, side="right") - 1
    return sorted({(int(s), int(l - pos[s] - tt // fsm), int(tt % fsm)) for s, l, tt in zip(song, lab, t)})


def unit_case(seed, n_songs, d, k, rec_rows, noise=0.35):
    """real-valued unit-norm rows: a db of n_songs songs of 30..90 rows and one recording cut from consecutive excerpts of
    random songs (20..60 rows each, gaps of pure noise rows), every row perturbed and renormalised; labels = the exact
    float64 top-k of every row.  -> (db, pos, q, labels)"""
    from pfann_amd import synth
    key = 30 + (np.floor(synth.uniform01(seed, "mon/key", n_songs) * 61)).astype(np.int64)
    pos = np.pad(np.cumsum(key), (1, 0)).astype(np.int64)
    db = synth.unit_rows(seed, "mon/db", int(pos[-1]), d).astype(np.float32)
    u = synth.uniform01(seed, "mon/plan", 4 * rec_rows)
    rows, i = [], 0
    while len(rows) < rec_rows:
        s = int(u[i] * n_songs)
        n = 20 + int(u[i + 1] * 41)
        o = int(u[i + 2] * max(1, int(key[s]) - n))
        gap = int(u[i + 3] * 12)
        i += 4
        rows += [int(pos[s]) + o + j for j in range(min(n, int(key[s]) - o))] + [-1] * gap
    rows = np.asarray(rows[:rec_rows])
    nz = synth.unit_rows(seed + 1, "mon/noise", rec_rows, d).astype(np.float64)
    q = np.where(rows[:, None] >= 0, db[np.maximum(rows, 0)].astype(np.float64), 0.0) + noise * nz * np.where(rows[:, None] >= 0, 1.0, 3.0)
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    sc = q.astype(np.float64) @ db.astype(np.float64).T
    labels = np.argsort(-sc, axis=1, kind="stable")[:, :k].astype(np.int64)
    return db, pos, q, labels


def _main(argv):
    """exact-general: every window x hop of the grid recordings through pfann_match_windows as the environment routes it"""
    import torch
    from pfann_amd import lib as L
    from pfann_amd.database import DeviceIndex
    assert argv[1] == "exact-general" and os.environ.get("PFANN_WINDOWS_GENERAL") == "1"
    d, k = 128, 20
    db, pos, q, labels, rstart, rlen = grid_recordings(d, k)
    rows = mx.IntRows(db)
    lib = L.load()
    first = {}
    for storage in ("f32", "f16"):
        idx = DeviceIndex(d, 0, storage)
        idx.load(db, pos)
        for window in WINDOWS:
            for hop in HOPS:
                lib.pfann_prof_enable(1)
                lib.pfann_prof_reset()
                res, wfirst = idx.match_windows(torch.as_tensor(q).cuda(), torch.as_tensor(labels).cuda(), rstart, rlen, window, hop)
                tags = L.ctypes.create_string_buffer(4096)
                lib.pfann_prof_tags(tags, 4096)
                lib.pfann_prof_enable(0)
                assert b"seq_match_windows" not in tags.value and b"seq_match" in tags.value, tags.value
                assert np.array_equal(wfirst, wfirst_of(rlen, window, hop))
                bad = differing(res, exact_windows("grid", q, labels, rstart, rlen, rows, pos, window, hop))
                assert not bad, "general path, window %d hop %d %s: %d windows differ\n%s" % (window, hop, storage, len(bad), "\n".join(bad[:6]))
                assert first.setdefault((window, hop), res.tobytes()) == res.tobytes(), "fp16 storage returns other bytes"
    print("exact-general ok: %d windows" % sum(len(window_starts(int(x), w, h)) for x in rlen for w in WINDOWS for h in HOPS))
    return 0


if __name__ == "__main__":
    sys.exit(_main(sys.argv))
