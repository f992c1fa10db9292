"""Oracles of the ranked monitor-mode tests (tests/test_gpu_monitor_topn.py): match_topn_exact.exact_topn applied to every
window of monitor_cases' recordings, and the float64 ranking of a window's songs on real-valued rows.

Run as a script (`python tests/monitor_topn_cases.py exact-general`) it checks pfann_match_windows_topn against the exact
oracle in THIS process -- the GPU test starts it with PFANN_WINDOWS_GENERAL=1 in the environment, which the library reads
per call."""
import os
import sys

import numpy as np

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import match_exact as mx
import match_topn_exact as mt
import monitor_cases as mc

N_FAST = 64                                   # include/pfann_amd.h: the longest list the windowed kernel serves
_EXACT = {}


RESULT_DTYPE = np.dtype([("song", "<i4"), ("offset", "<i4"), ("shift", "<i4"), ("n_cand", "<i4"), ("score", "<f8")])


def exact_window_lists(key, q, labels, rstart, rlen, db_rows, pos, window, hop, n, fsm=1, mode=0):
    """exact_topn of every window, in result order -> (top [nW, n] of the library's result dtype, n_found int32 [nW]).
    The hop-1 lists of N_FAST entries are computed once per (key, window); other hops take their subset and a shorter list
    its prefix (a window's list depends on neither)."""
    ck = (key, window, fsm, mode)
    if ck not in _EXACT:
        per = [[mt.exact_topn(q[s + w0:s + w0 + m], labels[s + w0:s + w0 + m], db_rows, pos, fsm, mode, N_FAST)
                for w0, m in mc.window_starts(int(L), window, 1)] for s, L in zip(rstart, rlen)]
        _EXACT[ck] = [(mt.as_array(p, RESULT_DTYPE) if p else np.zeros((0, N_FAST), RESULT_DTYPE),
                       np.asarray([t["n_found"] for t in p], np.int32)) for p in per]
    tops, found = [], []
    for (top, nf), L in zip(_EXACT[ck], rlen):
        at = [w0 for w0, _ in mc.window_starts(int(L), window, hop)]
        tops.append(top[at, :n])
        found.append(nf[at])
    return np.concatenate(tops), np.concatenate(found)


def differing(top, n_found, want_top, want_found):
    """-> messages for the windows whose list or n_found is not the oracle's, every field compared with =="""
    assert top.shape == want_top.shape and n_found.shape == want_found.shape, (top.shape, want_top.shape)
    same = np.ones(top.shape, bool)
    for f in mt.FIELDS:
        same &= top[f] == want_top[f]
    bad = []
    for j in np.flatnonzero(~same.all(1) | (n_found != want_found)):
        i = int(np.argmin(same[j]))
        bad.append("window %d: n_found %d, oracle %d; first differing entry %d: kernel %r, oracle %r"
                   % (j, int(n_found[j]), int(want_found[j]), i, top[j, i], want_top[j, i]))
    return bad


def ranking64(db, pos, q, labels, w0, wl):
    """float64 ranking of the songs of the window q[w0:w0 + wl]: every candidate of the window's own labels scored as
    monitor_cases.score64 does (mean of the float64 row dots, rows outside the song add 0), per song the best one, songs by
    score descending.  -> [(score, song, offset)]"""
    best = {}
    for song, off, _ in mc.candidates(labels[w0:w0 + wl], pos):
        sc = mc.score64(db, pos, q[w0:w0 + wl], song, off)
        if song not in best or sc > best[song][0]:
            best[song] = (sc, song, off)
    return sorted(best.values(), key=lambda e: (-e[0], e[1], e[2]))


def _main(argv):
    """exact-general: one window / hop pair per k of the grid recordings through pfann_match_windows_topn as the environment
    routes it, n = 1, 3 and N_FAST, both storages"""
    import torch
    from pfann_amd import lib as L
    from pfann_amd.database import DeviceIndex
    assert argv[1] == "exact-general" and os.environ.get("PFANN_WINDOWS_GENERAL") == "1"
    d, total = 128, 0
    lib = L.load()
    for k, window, hop in ((20, 19, 2), (100, 5, 7)):
        db, pos, q, labels, rstart, rlen = mc.grid_recordings(d, k)
        rows = mx.IntRows(db)
        first = {}
        for storage in ("f32", "f16"):
            idx = DeviceIndex(d, 0, storage)
            idx.load(db, pos)
            for n in (1, 3, N_FAST):
                lib.pfann_prof_enable(1)
                lib.pfann_prof_reset()
                (top, n_found), wfirst = idx.match_windows_topn(torch.as_tensor(q).cuda(), torch.as_tensor(labels).cuda(), rstart,
                                                                rlen, window, hop, n)
                tags = L.ctypes.create_string_buffer(4096)
                lib.pfann_prof_tags(tags, 4096)
                lib.pfann_prof_enable(0)
                assert b"seq_match_windows" not in tags.value and b"seq_match" in tags.value, tags.value
                assert np.array_equal(wfirst, mc.wfirst_of(rlen, window, hop))
                bad = differing(top, n_found, *exact_window_lists(("grid", k), q, labels, rstart, rlen, rows, pos, window, hop, n))
                assert not bad, "general path, k %d n %d %s: %d windows differ\n%s" % (k, n, storage, len(bad), "\n".join(bad[:6]))
                assert first.setdefault(n, top.tobytes()) == top.tobytes(), "fp16 storage returns other bytes"
                total += top.shape[0]
    print("exact-general ok: %d lists" % total)
    return 0


if __name__ == "__main__":
    sys.exit(_main(sys.argv))
