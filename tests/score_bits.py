"""Bit-exact checks of the exact search's scores (GPU tests): which calls return the canonical fp32 score (oracle/exactdot_c.c,
csrc/search_common.h canon_part / canon_sum), and the assertion that a result is the canonical top-k, bit for bit."""
import os

import numpy as np

SMALL_MAX_ROWS = 8192         # CAP (csrc/search_common.h): the small path's dense single pass up to here


def rescoring_path(db, q, prefilter=True, storage="f32"):
    """True when search_topk (csrc/search.hip) answers this call through a path whose every score is re-computed in the
    canonical order:
      - the shard keeps fp32 rows AND an fp16 copy, and the pre-filter is on: pfann_db_set_prefilter (csrc/api.hip:685-687)
        hands the copy to search_topk only when it is on; db_load (csrc/api.hip:742-753) makes the copy only for d % 8 == 0
        and a largest row norm below 1e4;
      - and then every path re-scores: nq > 32 (the fp16 scan, search_topk's generic ladder / group-maximum pass), nq <= 32
        with d in {64, 128} (search_small: the fp16 pre-filter for n > CAP, the dense pass + canonical re-scoring for
        n <= CAP).  nq <= 32 with any other d takes the fp32 MFMA ladder (launch_scan + launch_select): MFMA-order scores.
    An empty shard returns no scores at all (False).  Two A/B switches of the library leave the default dispatch:
    PFANN_NO_F16_PREFILTER (db_load makes no fp16 copy: the fp32 MFMA ladder everywhere) and PFANN_SMALL_F32 (nq <= 32 and
    n > CAP stream the fp32 rows with MFMA scores final, search.hip search_topk: small_pre); with either set, the calls it
    touches are not re-scoring paths."""
    n, d = db.shape[0], q.shape[1]
    if storage != "f32" or not prefilter or n == 0 or q.shape[0] == 0 or d % 8 != 0:
        return False
    if os.environ.get("PFANN_NO_F16_PREFILTER") is not None:
        return False
    if os.environ.get("PFANN_SMALL_F32") is not None and q.shape[0] <= 32 and n > SMALL_MAX_ROWS:
        return False
    xmax = float(np.sqrt((np.asarray(db, np.float64) ** 2).sum(1)).max())
    if not xmax < 1e4:
        return False
    return q.shape[0] > 32 or d in (64, 128)


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
