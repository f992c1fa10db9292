"""Inputs and the oracle of the masked search's tests (tests/test_gpu_search_excl.py, tests/test_gpu_selfmatch.py):
pfann_search_topk_excl leaves one range of rows out per query row.

The oracle does not mask scores: it DELETES the range's rows from the database, asks the existing oracles for the plain
top-k of what is left, and maps the labels back.  The databases are made of "songs" -- a random unit vector plus small noise
per row -- and the queries are database rows with their own song as the range, so the excluded range holds more than k rows
that beat every row outside it: the case in which filtering the plain answer afterwards returns nothing at all."""
import numpy as np

from score_bits import canonical_topk

FLT_MAX = np.finfo(np.float32).max


def song_db(seed, lengths, d, noise=0.05):
    """-> (db float32 [sum(lengths), d] unit rows, pos int64 prefix sums): song s = one random unit vector + noise per row"""
    rng = np.random.default_rng(seed)
    pos = np.pad(np.cumsum(np.asarray(lengths, np.int64)), (1, 0)).astype(np.int64)
    c = rng.standard_normal((len(lengths), d))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    db = np.repeat(c, lengths, axis=0) + noise * rng.standard_normal((int(pos[-1]), d))
    db /= np.linalg.norm(db, axis=1, keepdims=True)
    return db.astype(np.float32), pos


def song_lengths(seed, n):
    """lengths of 20..300 rows (a small database: 20..n/5, so that it still holds several songs) summing to exactly n; the
    last song takes what is left, up to 20 rows more"""
    rng = np.random.default_rng(seed)
    top = min(300, max(20, int(n) // 5))
    out, left = [], int(n)
    while left > top + 20:
        out.append(int(rng.integers(20, top + 1)))
        left -= out[-1]
    if left < 20 and out:
        left += out.pop()
    out.append(left)
    assert sum(out) == n
    return out


def own_song_ranges(pos, rows):
    """-> (lo, hi): for every row its own song's rows"""
    s = np.searchsorted(pos[:-1], rows, side="right") - 1
    return pos[s].astype(np.int64), pos[s + 1].astype(np.int64)


def clip_ranges(lo, hi, n, label_base=0):
    """label ranges -> row ranges of the shard as the header states them: clipped; lo >= hi is empty, written (0, 0)"""
    lo = np.clip(np.asarray(lo, np.int64) - label_base, 0, n)
    hi = np.clip(np.asarray(hi, np.int64) - label_base, 0, n)
    empty = lo >= hi
    return np.where(empty, 0, lo), np.where(empty, 0, hi)


def masked_topk(q, db, k, lo, hi, kind, label_base=0):
    """The oracle.  kind: "canonical" (score_bits.canonical_topk: D float32 bits), "f32" (oracle.search.flat_ip_topk) or
    "f16" (flat_ip_topk_f16: D float64).  Query rows are grouped by range, the range's rows deleted, labels mapped back."""
    from oracle import search as osr
    n, nq = db.shape[0], q.shape[0]
    lo, hi = clip_ranges(lo, hi, n, label_base)
    fn = {"canonical": canonical_topk, "f32": osr.flat_ip_topk, "f16": osr.flat_ip_topk_f16}[kind]
    D = np.full((nq, k), -FLT_MAX, np.float64 if kind == "f16" else np.float32)
    I = np.full((nq, k), -1, np.int64)
    for a, b in sorted(set(zip(lo.tolist(), hi.tolist()))):
        rows = np.flatnonzero((lo == a) & (hi == b))
        rest = np.concatenate([db[:a], db[b:]])
        # (big groups: the argpartition form of the same definition, as tests/test_gpu_parity.py _check_topk takes it)
        big = kind == "f32" and rows.size * rest.shape[0] > (1 << 24)
        Dg, Ig = (osr.flat_ip_topk_blas if big else fn)(q[rows], rest, k)
        Ig = np.where(Ig >= a, Ig + (b - a), Ig)
        D[rows] = Dg
        I[rows] = np.where(Ig >= 0, Ig + label_base, -1)
    return D, I


def assert_masked(D, I, q, db, k, lo, hi, kind, label_base=0, want=None, what=""):
    """(D, I) of the device against the oracle, by the rule tests/test_gpu_parity.py applies to that storage:
      canonical  labels equal and scores bit-equal (assert_canonical_topk's rule);
      f32        MFMA-order fp32 scores (_check_topk): scores within 2e-6 of the oracle's, label sets equal except for rows
                 that tie with the k-th score to 2e-6, reported scores belong to the reported labels;
      f16        fp16 rows, fp32 accumulation (test_search_fp16_storage_*): scores within 2e-5, label sets equal except for
                 ties with the k-th score to 2e-5.
    In every kind: no label inside its row's range, padding exactly where fewer than k rows remain, descending order."""
    D, I = np.asarray(D), np.asarray(I)
    n, nq = db.shape[0], q.shape[0]
    Dr, Ir = want if want is not None else masked_topk(q, db, k, lo, hi, kind, label_base)
    rlo, rhi = clip_ranges(lo, hi, n, label_base)
    left = np.minimum(k, n - (rhi - rlo))
    col = np.arange(k)[None, :]
    pad = col >= left[:, None]
    assert ((I == -1) == pad).all() and ((D == -FLT_MAX) == pad).all(), "%s: padding is not where fewer than k rows remain" % what
    row = I - label_base
    assert not ((I >= 0) & (row >= rlo[:, None]) & (row < rhi[:, None])).any(), "%s: an excluded row came back" % what
    assert (np.diff(D.astype(np.float64), axis=1) <= 0).all(), "%s: not descending" % what        # (the padding is -FLT_MAX)
    if kind == "canonical":
        bad = np.flatnonzero((I != Ir).any(1))
        assert bad.size == 0, "%s: %d query rows differ from the masked canonical top-%d (first %d: %r vs %r)" % (
            what, bad.size, k, bad[0], I[bad[0]][:8], Ir[bad[0]][:8])
        assert np.array_equal(D.view(np.int32), Dr.view(np.int32)), "%s: scores are not the canonical bits" % what
        return Dr, Ir
    tol = 2e-6 if kind == "f32" else 2e-5
    ok = ~pad
    assert np.abs(np.where(ok, D.astype(np.float64) - Dr.astype(np.float64), 0.0)).max(initial=0.0) < tol, what
    q64, x64 = (q, db) if kind == "f32" else (q.astype(np.float16), db.astype(np.float16))
    q64, x64 = q64.astype(np.float64), x64.astype(np.float64)
    for r in range(nq):
        kk = int(left[r])
        got, exp = row[r, :kk], Ir[r, :kk] - label_base
        assert np.abs(x64[got] @ q64[r] - D[r, :kk]).max(initial=0.0) < tol, "%s: row %d scores do not belong to the labels" % (what, r)
        a, b = set(got.tolist()), set(exp.tolist())
        if a != b:
            kth = float(Dr[r, kk - 1])
            for lab in a ^ b:
                assert abs(float(x64[lab] @ q64[r]) - kth) < tol, "%s: row %d label %d is not a tie at the k-th score" % (what, r, lab)
    return Dr, Ir
