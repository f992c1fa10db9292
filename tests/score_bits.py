"""Bit-exact checks of the exact search's scores (GPU tests): which calls return the canonical fp32 score (oracle/exactdot_c.c,
csrc/search_common.h canon_part / canon_sum), and the assertion that a result is the canonical top-k, bit for bit."""
import os

import numpy as np

SMALL_MAX_ROWS = 8192         # CAP (csrc/search_common.h): the small path's dense single pass up to here


def rescoring_path(db, q, prefilter=True, storage="f32"):
    """True when search_topk (csrc/search.hip) answers this call through a path whose every score is re-computed in the
    canonical order.  This is the INDEPENDENT statement of that fact: the library's own, the `canonical_scores` flag of its
    launch plan (csrc/search_plan.h, pfann_search_plan), is asserted equal to it over a sweep of shapes on the CPU
    (tests/test_search_plan.py) and in every GPU test that calls this.
      - the shard keeps fp32 rows AND an fp16 copy, and the pre-filter is on: pfann_db_set_prefilter (csrc/api.hip) hands
        the copy to search_topk only when it is on; pfann_db_load makes the copy only for d % 8 == 0 and a largest row norm
        below 1e4;
      - and then every path re-scores: nq > 32 (the fp16 scans: group-maximum pass or survivor ladder), nq <= 32 with d in
        {64, 128} (the small path: the fp16 pre-filter for n > CAP, the dense pass + canonical re-scoring for n <= CAP).
        nq <= 32 with any other d takes the fp32 MFMA ladder (scan_emit_kernel + select_kernel): MFMA-order scores.
    An empty shard returns no scores at all (False).  Two A/B switches of the library leave the default dispatch:
    PFANN_NO_F16_PREFILTER (pfann_db_load makes no fp16 copy: the fp32 MFMA ladder everywhere) and PFANN_SMALL_F32 (nq <= 32
    and n > CAP stream the fp32 rows with MFMA scores final); with either set, the calls it touches are not re-scoring
    paths."""
    n = db.shape[0]
    xmax = float(np.sqrt((np.asarray(db, np.float64) ** 2).sum(1)).max()) if n and db.shape[1] % 8 == 0 else 0.0
    return rescoring_path_of_shape(n, q.shape[1], q.shape[0], xmax, prefilter, storage)


def rescoring_path_of_shape(n, d, nq, xmax, prefilter=True, storage="f32"):
    """rescoring_path from the shapes and the largest row norm alone."""
    if storage != "f32" or not prefilter or n == 0 or nq == 0 or d % 8 != 0:
        return False
    if os.environ.get("PFANN_NO_F16_PREFILTER") is not None:
        return False
    if os.environ.get("PFANN_SMALL_F32") is not None and nq <= 32 and n > SMALL_MAX_ROWS:
        return False
    if not xmax < 1e4:
        return False
    return nq > 32 or d in (64, 128)


def canonical_topk(q, db, k):
    from oracle import search as osr
    return osr.flat_ip_topk_canonical(q, db, k, chunk=max(1, (1 << 25) // max(1, db.shape[0])))


def assert_canonical_topk(D, I, q, db, k, want=None, what=""):
    """I equals the exact top-k under the canonical score (ties to the lower row, no tolerance) and D holds the canonical
    bits of the returned labels.  want: (Dc, Ic) if the oracle's answer is already at hand.  Returns (Dc, Ic)."""
    from oracle import native
    D, I = np.asarray(D), np.asarray(I)
    Dc, Ic = want if want is not None else canonical_topk(q, db, k)
    kk = min(k, db.shape[0])
    diff = np.zeros((I.shape[0], kk), bool)
    if kk:
        mi = np.repeat(np.arange(q.shape[0]), kk)
        want_bits = native.canon_scores(q, db, mi, I[:, :kk].clip(0).ravel()).view(np.int32).reshape(-1, kk)
        diff = D[:, :kk].view(np.int32) != want_bits
    bad = np.flatnonzero((I != Ic).any(1))
    assert bad.size == 0 and not diff.any(), (
        "%s: %d of %d label entries (%d query rows, first row %d) differ from the canonical top-%d; %d of %d scores are not "
        "the canonical fp32 bits of their labels (%d query rows)" % (
            what, int((I != Ic).sum()), I.size, bad.size, bad[0] if bad.size else -1, k, int(diff.sum()), diff.size,
            int(diff.any(1).sum())))
    assert np.array_equal(D.view(np.int32), Dc.view(np.int32))
    return Dc, Ic
