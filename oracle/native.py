"""ctypes access to the C restatements (oracle/seqscore_c.c, oracle/exactdot_c.c).  TEST INFRASTRUCTURE."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_build", "liboracle.so")
_lib = None


# source -> its own flags.  exactdot_c.c states one fp32 summation order bit for bit: no contraction of a*b+c into an
# fma the source does not write, no fast-math reassociation (its fmaf calls are libm's correctly rounded ones)
_SOURCES = {"seqscore_c.c": ["-O2"], "exactdot_c.c": ["-O2", "-ffp-contract=off", "-fno-fast-math"]}


def build(force=False):
    srcs = [os.path.join(_HERE, f) for f in _SOURCES]
    if force or not os.path.exists(_SO) or any(os.path.getmtime(_SO) < os.path.getmtime(s) for s in srcs):
        os.makedirs(os.path.dirname(_SO), exist_ok=True)
        # objects and the library are built under names of this process and the library moved into place at once:
        # processes that build at the same time never see each other's half-written files
        tag = ".%d" % os.getpid()
        objs = []
        try:
            for f, flags in _SOURCES.items():
                obj = os.path.join(os.path.dirname(_SO), f[:-2] + tag + ".o")
                objs.append(obj)
                subprocess.check_call(["gcc"] + flags + ["-fopenmp", "-fPIC", "-c", os.path.join(_HERE, f), "-o", obj])
            tmp = _SO + tag + ".tmp"
            subprocess.check_call(["gcc", "-fopenmp", "-shared"] + objs + ["-lm", "-o", tmp])
            os.replace(tmp, _SO)
        finally:
            for obj in objs:
                if os.path.exists(obj):
                    os.remove(obj)
    return _SO


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build())
        f32p, i64p = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int64)
        _lib.oracle_seq_score.argtypes = [f32p, ctypes.c_int, i64p, ctypes.c_int, f32p, ctypes.c_int,
                                          i64p, ctypes.c_int, f32p, ctypes.c_int, ctypes.c_float]
        _lib.oracle_seq_score.restype = ctypes.c_int
        _lib.oracle_flat_ip_topk.argtypes = [f32p, ctypes.c_int64, ctypes.c_int, f32p, ctypes.c_int,
                                             ctypes.c_int, f32p, i64p]
        _lib.oracle_flat_ip_topk.restype = None
        _lib.oracle_canon_scores.argtypes = [f32p, f32p, ctypes.c_int, i64p, i64p, ctypes.c_int64, f32p]
        _lib.oracle_canon_scores.restype = None
    return _lib


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def seq_score(db, song_pos, query, labels, frame_shift_mul=1, score_alpha=0.0):
    """-> (best_song, song_scores float32[n_songs,2] with offsets in frames)."""
    db = np.ascontiguousarray(db, np.float32)
    query = np.ascontiguousarray(query, np.float32)
    labels = np.ascontiguousarray(labels, np.int64)
    song_pos = np.ascontiguousarray(song_pos, np.int64)
    n_songs = song_pos.shape[0] - 1
    d = query.shape[1]
    ss = np.zeros((n_songs, 2), np.float32)
    best = lib().oracle_seq_score(_p(db, ctypes.c_float), d, _p(song_pos, ctypes.c_int64), n_songs,
                                  _p(query, ctypes.c_float), query.shape[0],
                                  _p(labels, ctypes.c_int64), labels.shape[1],
                                  _p(ss, ctypes.c_float), frame_shift_mul, score_alpha)
    return best, ss


def flat_ip_topk(query, db, k):
    db = np.ascontiguousarray(db, np.float32)
    query = np.ascontiguousarray(query, np.float32)
    nq, d = query.shape
    D = np.empty((nq, k), np.float32)
    I = np.empty((nq, k), np.int64)
    lib().oracle_flat_ip_topk(_p(db, ctypes.c_float), db.shape[0], d, _p(query, ctypes.c_float), nq, k,
                              _p(D, ctypes.c_float), _p(I, ctypes.c_int64))
    return D, I


def canon_scores(query, db, qi, xi):
    """float32[len(qi)]: the canonical fp32 score (oracle/exactdot_c.c) of each pair (query[qi[i]], db[xi[i]])."""
    query = np.ascontiguousarray(query, np.float32)
    db = np.ascontiguousarray(db, np.float32)
    d = query.shape[1]
    assert d % 4 == 0 and db.shape[1] == d
    qi = np.ascontiguousarray(qi, np.int64).ravel()
    xi = np.ascontiguousarray(xi, np.int64).ravel()
    assert qi.shape == xi.shape
    assert qi.size == 0 or (0 <= qi.min() and qi.max() < query.shape[0] and 0 <= xi.min() and xi.max() < db.shape[0])
    out = np.empty(qi.size, np.float32)
    lib().oracle_canon_scores(_p(query, ctypes.c_float), _p(db, ctypes.c_float), d, _p(qi, ctypes.c_int64),
                              _p(xi, ctypes.c_int64), qi.size, _p(out, ctypes.c_float))
    return out
