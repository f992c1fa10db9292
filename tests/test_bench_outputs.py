"""bench.py --dump-outputs on the host (no GPU): the files it writes, and the fixed seeded row sample it falls back to
when a step's decisions exceed 8 MB or its fingerprints 48 MB (64 MB in all)."""
import os

import numpy as np
import torch

import bench
from pfann_amd.database import DeviceIndex

FIELDS = ("song", "offset", "shift", "n_cand", "score")


def _step(n_queries, n_rows):
    """a step's return values whose rows say where they came from: decision field j of query i = i + j, fingerprint row r
    starts with r"""
    res = np.zeros(n_queries, DeviceIndex.RESULT_DTYPE)
    for j, f in enumerate(FIELDS):
        res[f] = np.arange(n_queries) + j
    emb = torch.zeros((n_rows, 128), dtype=torch.float32)
    emb[:, 0] = torch.arange(n_rows, dtype=torch.float32)
    return res, emb


def _load(path):
    return {f: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


def test_seeded_rows_is_a_fixed_sorted_sample_without_duplicates():
    assert bench._seeded_rows(100, 100) == slice(None) and bench._seeded_rows(100, 250) == slice(None)
    a, b = bench._seeded_rows(100000, 1234), bench._seeded_rows(100000, 1234)
    assert a.shape == (1234,) and np.array_equal(a, b)
    assert (np.diff(a) > 0).all() and a[0] >= 0 and a[-1] < 100000


def test_dump_outputs_writes_every_row_of_a_small_step(tmp_path):
    res, emb = _step(16, 16 * 19)
    bench.dump_outputs(str(tmp_path), res, emb)
    out = _load(str(tmp_path))
    assert sorted(out) == sorted(["decision_%s.npy" % f for f in FIELDS] + ["fingerprints.npy"])
    for f in FIELDS:
        a = out["decision_%s.npy" % f]
        assert a.dtype == np.float64 and np.array_equal(a, res[f].astype(np.float64)), f
    assert out["fingerprints.npy"].dtype == np.float32 and np.array_equal(out["fingerprints.npy"], emb.numpy())


def test_dump_outputs_samples_a_large_step_within_64_mb(tmp_path):
    n_q, n_rows = 300000, 120000                  # 12 MB of decisions, 61 MB of fingerprints
    res, emb = _step(n_q, n_rows)
    outs = []
    for run in range(2):
        d = str(tmp_path / ("run%d" % run))
        bench.dump_outputs(d, res, emb)
        assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64 << 20
        outs.append(_load(d))
    out = outs[0]
    keep_q = bench.DUMP_DECISION_BYTES // (8 * len(FIELDS))
    keep_r = bench.DUMP_FINGERPRINT_BYTES // (4 * 128)
    rows_q = out["decision_song.npy"].astype(np.int64)
    assert rows_q.shape == (keep_q,) and np.array_equal(rows_q, bench._seeded_rows(n_q, keep_q))
    for j, f in enumerate(FIELDS):                # every field sampled at the same queries
        assert np.array_equal(out["decision_%s.npy" % f], (rows_q + j).astype(np.float64)), f
    fp = out["fingerprints.npy"]
    assert fp.shape == (keep_r, 128) and fp.dtype == np.float32
    assert np.array_equal(fp[:, 0].astype(np.int64), bench._seeded_rows(n_rows, keep_r))
    for f in out:                                 # the same sample in every run
        assert np.array_equal(out[f], outs[1][f]), f
