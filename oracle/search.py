"""Oracle a7: exact inner-product top-k (faiss IndexFlatIP.search semantics as used at
reference database.py:121: k largest q.x per query row, scores descending, labels int64,
-1 labels when fewer than k rows exist).  faiss is un-vendored; exact flat IP is
definitional, so this is a restatement of the definition, not of faiss code."""
import numpy as np


def flat_ip_topk(query, db, k):
    query = np.ascontiguousarray(query, dtype=np.float32)
    db = np.ascontiguousarray(db, dtype=np.float32).reshape(-1, query.shape[1])
    nq, n = query.shape[0], db.shape[0]
    D = np.full((nq, k), -np.finfo(np.float32).max, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    if n == 0:
        return D, I
    s = query @ db.T
    kk = min(k, n)
    # stable: ties broken by smaller label
    order = np.argsort(-s, axis=1, kind="stable")[:, :kk]
    D[:, :kk] = np.take_along_axis(s, order, axis=1)
    I[:, :kk] = order
    return D, I


def flat_ip_topk_blas(query, db, k):
    """Same result as flat_ip_topk, via BLAS sgemm + argpartition (the faiss-cpu IndexFlatIP
    stand-in named in BASELINE.md §3 for CPU-baseline timing)."""
    query = np.ascontiguousarray(query, dtype=np.float32)
    nq, n = query.shape[0], db.shape[0]
    D = np.full((nq, k), -np.finfo(np.float32).max, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    if n == 0:
        return D, I
    s = query @ db.T
    kk = min(k, n)
    if kk < n:
        part = np.argpartition(-s, kk - 1, axis=1)[:, :kk]
    else:
        part = np.tile(np.arange(n), (nq, 1))
    ps = np.take_along_axis(s, part, axis=1)
    o = np.lexsort((part, -ps), axis=1)
    D[:, :kk] = np.take_along_axis(ps, o, axis=1)
    I[:, :kk] = np.take_along_axis(part, o, axis=1)
    return D, I


def flat_ip_topk_f16(query, db, k):
    """fp16-storage semantics (faiss GpuMultipleClonerOptions.useFloat16, database.py:101-104): rows and
    queries rounded to IEEE fp16, exact products, wide accumulation -- the k largest
    s16 = sum_i fl16(q_i) * fl16(x_i).  Computed in float64 here (products of two fp16 are exact in fp32, so
    an fp32-accumulating device differs only by summation rounding, ~1e-7 of the norm product)."""
    q16 = np.asarray(query, np.float32).astype(np.float16).astype(np.float64)
    x16 = np.asarray(db, np.float32).reshape(-1, q16.shape[1]).astype(np.float16).astype(np.float64)
    nq, n = q16.shape[0], x16.shape[0]
    D = np.full((nq, k), -np.finfo(np.float32).max, dtype=np.float64)
    I = np.full((nq, k), -1, dtype=np.int64)
    if n == 0:
        return D, I
    kk = min(k, n)
    if nq * n > (1 << 24) and kk < n:
        # big cases: the same list by selection (a stable argsort of 513 x 262,200 scores took 20 s).  Everything above the
        # k-th score, then the LOWEST rows that tie with it -- what the stable sort keeps --, in blocks of query rows
        for m0 in range(0, nq, 64):
            s = q16[m0:m0 + 64] @ x16.T
            kth = -np.partition(-s, kk - 1, axis=1)[:, kk - 1]
            for r in range(s.shape[0]):
                above = np.flatnonzero(s[r] > kth[r])
                rows = np.concatenate([above, np.flatnonzero(s[r] == kth[r])[:kk - above.size]])
                rows = rows[np.lexsort((rows, -s[r, rows]))]
                D[m0 + r, :kk] = s[r, rows]
                I[m0 + r, :kk] = rows
        return D, I
    s = q16 @ x16.T
    order = np.argsort(-s, axis=1, kind="stable")[:, :kk]
    D[:, :kk] = np.take_along_axis(s, order, axis=1)
    I[:, :kk] = order
    return D, I


def canon_window(query, db):
    """Half-width w[m] of the window flat_ip_topk_canonical scores in C: w >= |canon(q_m, x) - s64(q_m, x)| for every
    row x, where s64 is the float64 score.  canon is d/4-term fma chains and two adds, so (Higham's gamma bound, then
    Cauchy-Schwarz) |canon - q.x| <= gamma_(d/4+2) sum_i |q_i x_i| <= (d/4 + 2) 2^-24 (1 + 1e-5) |q| max|x|; the float64
    score adds d 2^-53 |q| max|x|; the absolute term covers products that underflow fp32.  A factor 2 on top."""
    q64 = np.asarray(query, np.float64)
    x64 = np.asarray(db, np.float64).reshape(-1, q64.shape[1])
    d = q64.shape[1]
    xmax = float(np.sqrt((x64 * x64).sum(1)).max()) if x64.shape[0] else 0.0
    rel = (d / 4 + 2) * 2.0 ** -24 + d * 2.0 ** -53
    return 2.0 * (rel * np.sqrt((q64 * q64).sum(1)) * xmax + (d + 2) * 2.0 ** -149)


def flat_ip_topk_canonical(query, db, k, brute=False, chunk=256):
    """Exact top-k under the canonical fp32 score canon(q, x) (oracle/exactdot_c.c, the summation order of every
    re-scoring site of the search): scores descending, ties to the lower row, padding as flat_ip_topk.

    Only a window is scored in C.  With s64 the float64 score, kth64 the k-th largest s64 of a query row and w =
    canon_window(): every row with s64 >= kth64 - 2w is scored.  Proof that no row outside can enter the top k: such
    a row has canon < s64 + w < kth64 - w, while the k rows with s64 >= kth64 have canon >= kth64 - w, so the canonical
    k-th score is >= kth64 - w: strictly above the row's.  brute=True scores every row (a check of the window)."""
    from oracle import native
    query = np.ascontiguousarray(query, dtype=np.float32)
    db = np.ascontiguousarray(db, dtype=np.float32).reshape(-1, query.shape[1])
    nq, n = query.shape[0], db.shape[0]
    D = np.full((nq, k), -np.finfo(np.float32).max, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    if n == 0 or nq == 0:
        return D, I
    kk = min(k, n)
    w = canon_window(query, db)
    x64 = db.astype(np.float64)
    for m0 in range(0, nq, chunk):
        q64 = query[m0:m0 + chunk].astype(np.float64)
        s64 = q64 @ x64.T
        if brute or kk == n:
            keep = np.ones(s64.shape, bool)
        else:
            kth = -np.partition(-s64, kk - 1, axis=1)[:, kk - 1]
            keep = s64 >= (kth - 2.0 * w[m0:m0 + chunk])[:, None]
        mi, xi = np.nonzero(keep)
        sc = native.canon_scores(query, db, mi + m0, xi)
        # per query row: canon descending by the float's total order (+0 above -0, as the device's packed keys), then
        # row ascending
        u = sc.view(np.uint32)
        desc = ~(u ^ np.where(u >> 31 != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000)))
        o = np.lexsort((xi, desc, mi))
        mi, xi, sc = mi[o], xi[o], sc[o]
        start = np.searchsorted(mi, np.arange(q64.shape[0]))
        for r in range(q64.shape[0]):
            s = start[r]
            D[m0 + r, :kk] = sc[s:s + kk]
            I[m0 + r, :kk] = xi[s:s + kk]
    return D, I
