"""The one formatter of match results (pfann_amd.database.format_results) and the tuples query_finish, query_topn_finish and
the monitor make from it, against the reference's formulas written out as scalar Python: query_embeddings_base
(database.py:148, mode 0) and query_embeddings_cpp (database.py:166-195, mode 1: float32 score, float32 fine-frame time,
only scores > 0).  Values with ==, types with type(), element for element.  No GPU."""
import itertools

import numpy as np
import pytest

from pfann_amd import lib as L
from pfann_amd.database import (MONITOR_DTYPE, DeviceIndex, format_results, monitor_rows, result_tuples, topn_tuples)

RES = DeviceIndex.RESULT_DTYPE
FSMS, HOPS = (1, 2, 4), (0.5, 0.3)
# 1e-46 is 0 in float32; 0.1 is not a float32 value; 2**24 + 1 rounds in float32 for every fsm; 2**30 + 7 times fsm 4 passes 2**32
SCORES = (0.75, 0.1, 0.0, -0.0, -0.25, 1e-46)
OFFSETS = (0, 3, -3, 2 ** 24 + 1, 2 ** 30 + 7)


def _rows(fsm):
    rows = [(song, off, shift, 7, score) for song, off, shift, score in
            itertools.product((-1, 0, 5), OFFSETS, range(fsm), SCORES)]
    return np.array(rows, dtype=RES)


def _ref(r, mode, fsm, hop_size, empty_db=False):
    """one result -> (score, (song, time)) as the reference's two paths give it"""
    song, off, shift, score = int(r["song"]), int(r["offset"]), int(r["shift"]), float(r["score"])
    if mode == 1:
        sc32 = float(np.float32(score)) if song >= 0 else 0.0
        if song < 0 or not sc32 > 0.0:
            return (0.0, (song if song >= 0 else -1, 0.0))
        fine = float(np.float32(off * fsm - shift))
        return (sc32, (song, fine * hop_size / fsm))
    if empty_db or song < 0:
        return (-1e999, (-1, 0))
    return (score, (song, (off - shift / fsm) * hop_size))


def _same(got, want):
    """== on the values and type() on every element: (float, (int, float-or-int))"""
    assert got == want, (got, want)
    assert (type(got[0]), type(got[1][0]), type(got[1][1])) == (type(want[0]), type(want[1][0]), type(want[1][1])), (got, want)
    assert type(got) is tuple and type(got[1]) is tuple and len(got) == 2 and len(got[1]) == 2


CASES = list(itertools.product((0, 1), FSMS, HOPS, (False, True)))


@pytest.mark.parametrize("mode,fsm,hop_size,empty_db", CASES)
def test_format_results_and_query_tuples_equal_the_reference_formulas(mode, fsm, hop_size, empty_db):
    res = _rows(fsm)
    assert (res["offset"].astype(np.int64) * fsm - res["shift"]).max() > 2 ** 24
    want = [_ref(r, mode, fsm, hop_size, empty_db) for r in res]
    score, song, time_s = format_results(res, mode, fsm, hop_size, empty_db)
    assert (score.dtype, song.dtype, time_s.dtype) == (np.float64, np.int64, np.float64)
    assert score.shape == song.shape == time_s.shape == res.shape
    assert list(zip(score.tolist(), zip(song.tolist(), time_s.tolist()))) == want
    got = result_tuples(res, mode, fsm, hop_size, empty_db)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        _same(g, w)
    # any shape: a [n, 3] block gives the same numbers in that shape
    block = res[:len(res) // 3 * 3].reshape(-1, 3)
    for a, b in zip(format_results(block, mode, fsm, hop_size, empty_db), (score, song, time_s)):
        assert a.shape == block.shape and np.array_equal(a.ravel(), b[:block.size])


def test_the_mode_0_answer_without_a_candidate_keeps_the_int_zero():
    res = np.array([(-1, 0, 0, 0, 0.0), (3, 4, 1, 2, 0.5)], dtype=RES)
    none, hit = result_tuples(res, 0, 2, 0.5)
    assert none == (-1e999, (-1, 0)) and type(none[1][1]) is int and type(none[0]) is float
    assert hit == (0.5, (3, 1.75)) and type(hit[1][1]) is float
    none, hit = result_tuples(res, 0, 2, 0.5, empty_db=True)
    assert none == hit == (-1e999, (-1, 0)) and type(hit[1][1]) is int
    none, hit = result_tuples(res, 1, 2, 0.5)
    assert none == (0.0, (-1, 0.0)) and type(none[1][1]) is float and hit == (0.5, (3, 1.75))


@pytest.mark.parametrize("mode,fsm,hop_size", [c[:3] for c in CASES if not c[3]])
def test_monitor_rows_carry_the_same_numbers(mode, fsm, hop_size):
    res = _rows(fsm)
    wfirst = np.array([0, 5, 5, len(res) - 4, len(res)], dtype=np.int64)          # one recording without windows
    out = monitor_rows(res, wfirst, 3, mode, fsm, hop_size)
    assert len(out) == 4 and [len(x) for x in out] == np.diff(wfirst).tolist()
    for rows, a in zip(out, wfirst):
        assert rows.dtype == MONITOR_DTYPE and rows["w0"].tolist() == [3 * i for i in range(len(rows))]
        for i, row in enumerate(rows):
            sc, (song, t) = _ref(res[a + i], mode, fsm, hop_size)
            assert (float(row["score"]), int(row["song"]), float(row["time_s"])) == (sc, song, float(t)), (a + i, row)


def _ref_topn(top, mode, fsm, hop_size, empty_db=False):
    """the top-N rules on top of the formulas: later entries stop at the first song < 0, mode-1 later entries whose float32
    score is not > 0 are skipped, entry 0 is always there"""
    out = []
    for lst in top:
        rows = []
        for i, r in enumerate(lst):
            if i and r["song"] < 0:
                break
            if i and mode == 1 and not float(np.float32(r["score"])) > 0.0:
                continue
            rows.append(_ref(r, mode, fsm, hop_size, empty_db))
        out.append(rows)
    return out


@pytest.mark.parametrize("mode,fsm,hop_size", [c[:3] for c in CASES if not c[3]])
def test_topn_rules(mode, fsm, hop_size):
    pad = (-1, 0, 0, 0, -np.inf)
    big = 2 ** 24 + 1
    top = np.array([
        [(4, 10, 0, 9, 0.9), (2, big, fsm - 1, 5, 0.5), (7, 3, 0, 2, 0.1), (1, -2, fsm - 1, 1, 0.05)],   # a full list
        [pad, pad, pad, pad],                                                                      # no candidate: entry 0 stays
        [(4, 10, 0, 9, 0.9), (2, 5, 0, 5, 0.5), pad, (7, 3, 0, 2, 0.1)],                           # stops at the first song < 0
        [(4, 10, 0, 9, 0.9), (2, 5, 0, 5, 1e-46), (7, 3, 0, 2, -0.25), (1, 8, 0, 1, 0.05)],        # mode 1 skips, does not stop
        [(4, 10, 0, 9, 0.0), (2, 5, 0, 5, -0.0), pad, pad],                                        # entry 0 stays at score 0
    ], dtype=RES)
    want = _ref_topn(top, mode, fsm, hop_size)
    assert [len(w) for w in want] == ([4, 1, 2, 2, 1] if mode == 1 else [4, 1, 2, 4, 2])
    got = topn_tuples(top, mode, fsm, hop_size)
    assert type(got) is list and [len(g) for g in got] == [len(w) for w in want]
    for g_rows, w_rows in zip(got, want):
        assert type(g_rows) is list
        for g, w in zip(g_rows, w_rows):
            _same(g, w)
    # entry 0 is what the plain query answers for the same result, whatever the mode
    for g_rows, first in zip(got, result_tuples(top[:, 0], mode, fsm, hop_size)):
        _same(g_rows[0], first)
    # a single-entry list and an empty batch
    one = topn_tuples(top[:, :1], mode, fsm, hop_size)
    assert [len(x) for x in one] == [1] * 5 and [x[0] for x in one] == [g[0] for g in got]
    assert topn_tuples(top[:0], mode, fsm, hop_size) == []
    assert topn_tuples(top, mode, fsm, hop_size, empty_db=True)[0][0] == _ref(top[0, 0], mode, fsm, hop_size, True)


def test_the_one_decode_refuses_song_minus_two_from_host_bytes():
    import torch
    good = np.array([(3, 4, 1, 2, 0.5), (-1, 0, 0, 0, -np.inf), (0, 1, 0, 1, 0.25), (5, 6, 0, 3, 0.125)], dtype=RES)
    assert RES.itemsize == 24
    out = DeviceIndex.decode_results(good.tobytes())
    assert out.dtype == RES and out.shape == (4,) and out.tobytes() == good.tobytes()
    assert DeviceIndex.decode_results(good.tobytes(), (2, 2)).shape == (2, 2)
    as_tensor = torch.frombuffer(bytearray(good.tobytes()), dtype=torch.uint8)
    assert DeviceIndex.decode_results(as_tensor.view(4, 24)).shape == (4,)                 # a [nQ, 24] result tensor
    lists = DeviceIndex.decode_results(as_tensor.view(2, 2, 24))                           # a [nQ, n, 24] top-N block
    assert lists.shape == (2, 2) and lists.tobytes() == good.tobytes()
    assert DeviceIndex.decode_results(b"").shape == (0,)
    bad = good.copy()
    bad["song"][2] = -2
    for raw in (bad.tobytes(), torch.frombuffer(bytearray(bad.tobytes()), dtype=torch.uint8).view(2, 2, 24)):
        with pytest.raises(L.PfannError, match="refused"):
            DeviceIndex.decode_results(raw)
