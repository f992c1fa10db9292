"""Adversarial inputs for the fp16 margin (csrc/search_f16.hip, header items 1-4; csrc/nominate.hip, THE MARGIN):

    |s16 - q.x| <= eps = 1.05e-3 ||q|| X + 3.1e-8 sqrt(d) (||q|| + X)

CPU only: numpy builders and references, shared by tests/test_fp16_margin_host.py (the conditions on the inputs) and
tests/test_gpu_fp16_margin.py (the device against them).  Every builder is seeded and returns float32 arrays.

THE ROUNDING PATTERN.  u = 2^-11 is half an ulp of a half in [1, 2).  A component 2^e (1 + 0.98 u) rounds DOWN to 2^e and loses
0.98 u of itself; 2^e (1 + 1.02 u) rounds UP to 2^e (1 + 2 u).  With q and row A both of the first kind and parallel, every
product loses (1 + 0.98 u)^2 - 1 = 1.96 u: s16 = q.A (1 - 0.957e-3), 0.911 of eps's 1.05e-3.  Row B is of the second kind
with its smallest-weight coordinates zeroed (a share gamma of the score): in float64 A beats B by gamma - 0.04 u, in s16 B
beats A by 2 u - gamma.  The pattern lives on the binary grid: it survives a multiplication by a power of two and NO other
factor (30 (1 + 0.98 u) and 30 (1 + 1.02 u) round to the same half).
"""
import numpy as np

U = 2.0 ** -11
DOWN = np.float32(1.0 + 0.98 * U)        # rounds down by 0.98 u (fp32 holds 1 + 4014 / 2^23: 0.97998 u)
UP = np.float32(1.0 + 1.02 * U)          # rounds up by 0.98 u
GAMMA = 4.4e-4                           # the share of the score B gives away; 2 u - GAMMA = 5.4e-4, GAMMA - 0.04 u = 4.2e-4
LABEL_EXP = (-5, -6, -7, -8, -9, -10, -11, -12)      # exponents of the label coordinates: weights 4^e, every subset sum distinct


# ------------------------------------------------------------------------------------------------ references
def f16(x):
    """the round-to-nearest-even fp16 image (subnormals kept), as float64"""
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float64)


def s16_ref(q, X):
    """sum fl16(q_i) fl16(x_i): exact products (22-bit), float64 sums.  q [d] or [nq, d], X [n, d] -> [n] or [nq, n]"""
    return f16(q) @ f16(X).T


def abs16_ref(q, X):
    """sum |fl16(q_i) fl16(x_i)|: what an fp32 accumulation error is relative to"""
    return np.abs(f16(q)) @ np.abs(f16(X)).T


def exact_ref(q, X):
    """q.x of the fp32 inputs in float64"""
    return np.asarray(q, np.float32).astype(np.float64) @ np.asarray(X, np.float32).astype(np.float64).T


def flushed_ref(q, X):
    """s16_ref with every fp16-subnormal half flushed to zero: what a flushing conversion or MFMA input would give"""
    a, b = f16(q), f16(X)
    a = np.where(np.abs(a) < 2.0 ** -14, 0.0, a)
    b = np.where(np.abs(b) < 2.0 ** -14, 0.0, b)
    return a @ b.T


def norm32(rows):
    """||row|| as the kernels form it: fp32 squares, fp32 sum, fp32 sqrt"""
    rows = np.atleast_2d(np.asarray(rows, np.float32))
    return np.sqrt((rows ** 2).sum(1, dtype=np.float32)).astype(np.float32)


def eps_ref(q, xmax, d):
    """q_prep_kernel's eps for every row of q (fp32 steps) -> float64 [nq]"""
    x = np.float32(xmax)
    nrm = norm32(q)
    eps = np.float32(1.05e-3) * nrm * x + np.float32(3.1e-8) * np.sqrt(np.float32(d)) * (nrm + x)
    return eps.astype(np.float64)


def margin_ref(q_rows, d, xmax):
    """E_j as nominate_select_kernel forms it: the fp32 eps_t and norms, the rest in double"""
    n = q_rows.shape[0]
    nrm = norm32(q_rows).astype(np.float64)
    return float(eps_ref(q_rows, xmax, d).sum() + 2.0 ** -22 * (d + n) * float(np.float32(xmax)) * float(nrm.sum()))


# ------------------------------------------------------------------------------------------------ worst-case rows
def label_exponents(S, labels):
    """LABEL_EXP moved by whole exponents so that the heaviest label stays near 2e-5 of a score S (42 at d = 128), whatever d"""
    shift = int(np.clip(np.floor(np.log(S / 42.0) / np.log(4.0)), -1, 2))
    return [x + shift for x in LABEL_EXP[:labels]]


def inverts(d):
    """True where worst_case's B beats A in s16: one dropped coordinate of exponent -3 is a share 1 / (64 S) of the score, and
    S (the sum of 4^e_i) is large enough for that share to stay below 2 u - 1e-4 from d = 64 on.  Below, the exponents -3..0
    do not allow it: only the ratio |s16 - exact| / eps of such a d is used."""
    return d >= 64


def worst_parts(d, seed, labels=0):
    """The pattern behind worst_case -> dict(sign, e, drop, label): signs, exponents -3..0, the coordinates B drops, and
    `labels` further coordinates (of q, A and B alike) with the exponents LABEL_EXP: their weights, 4^e, are a share below
    3.2e-5 of the score and every subset of them has another sum, so copies that keep different subsets have distinct exact
    scores and keep the rounding pattern.  d < 128 draws more exponents 0, so that S allows gamma near GAMMA."""
    rng = np.random.default_rng([seed, d, labels])
    sign = rng.choice(np.asarray([-1.0, 1.0]), d)
    e = rng.integers(-3, 1, d) if d >= 128 else rng.choice(np.asarray([0, 0, 0, -1, -2, -3]), d)
    order = rng.permutation(d)
    label = np.sort(order[:labels])
    e[label] = label_exponents(float((4.0 ** e).sum()), labels)
    rest = order[labels:]
    n_min = min(8, max(1, len(rest) // 4))
    e[rest[:n_min]] = -3                                  # coordinates of the smallest weight exist at every d
    S = float((4.0 ** e).sum())
    m = max(1, int(round(GAMMA * S * 64.0)))
    smallest = rest[e[rest] == -3]
    assert m <= len(smallest), (d, m, len(smallest))
    return {"sign": sign, "e": e, "drop": np.sort(smallest[:m]), "label": label, "S": S, "gamma": m / 64.0 / S}


def split_parts(d, seed, labels=0):
    """The pattern that inverts by MORE than one eps -> the dict of worst_parts.  The coordinates are cut into halves P and N
    with the same exponents.  q rounds DOWN on P and UP on N; A lives on P and rounds down, B lives on N and rounds up:
    s16(A) = q.A (1 - 1.96 u), s16(B) = q.B (1 + 1.96 u) -- the query's own rounding, which worst_case's rows share, now works
    for B and against A.  B gives away a share gamma ~ 2e-4 (coordinates of exponent -4): in float64 A beats B by gamma -
    0.08 u, in s16 B beats A by 4 u - gamma = 1.75e-3 of the score = 1.18 eps (eps = 1.05e-3 sqrt(2) q.A here).  The price:
    |s16 - exact| is 0.64 eps, not 0.91 -- these rows attack the WINDOWS (2 eps in the selects, 2 E in n_close), the
    worst_case rows the bound itself."""
    assert d % 2 == 0 and d >= 64
    rng = np.random.default_rng([seed, d, labels, 7])
    h = d // 2
    order = rng.permutation(d)
    P, N = order[:h], order[h:]
    eh = rng.integers(-3, 1, h) if h >= 64 else rng.choice(np.asarray([0, 0, 0, -1, -2, -3]), h)
    eh[:labels] = label_exponents(float((4.0 ** eh).sum()), labels)
    eh[labels:labels + 6] = -4
    e = np.zeros(d, np.int64)
    e[P], e[N] = eh, eh
    S = float((4.0 ** eh).sum())
    m = max(1, int(round(2.0e-4 * S * 256.0)))
    assert m <= 6, (d, m)
    on_p = np.zeros(d)
    on_p[P] = 1.0
    return {"sign": rng.choice(np.asarray([-1.0, 1.0]), d), "e": e, "qfac": np.where(on_p > 0, float(DOWN), float(UP)), "a_on": on_p,
            "b_on": 1.0 - on_p, "drop": np.sort(N[labels:labels + m]), "label": P[:labels], "label_b": N[:labels],
            "S": S, "gamma": m / 256.0 / S}


def rows_of(parts):
    """-> (q, A, B) float32 of a pattern"""
    mag = parts["sign"] * 2.0 ** parts["e"]
    q = (mag * parts.get("qfac", float(DOWN))).astype(np.float32)
    A = (mag * float(DOWN) * parts.get("a_on", 1.0)).astype(np.float32)
    B = (mag * float(UP) * parts.get("b_on", 1.0)).astype(np.float32)
    B[parts["drop"]] = 0.0
    return q, A, B


def split_case(d, seed):
    """(q, A, B) of split_parts"""
    return rows_of(split_parts(d, seed))


def worst_case(d, seed):
    """(q, A, B): q = A, every component +-2^e (1 + 0.98 u); B = +-2^e (1 + 1.02 u) without its dropped coordinates.
    inverts(d) says whether B beats A in s16 (d >= 64)."""
    return rows_of(worst_parts(d, seed))


def without(row, coords):
    out = np.array(row, np.float32)
    out[np.asarray(coords, np.int64)] = 0.0
    return out


def subsets(label, count):
    """the first `count` subsets of the label coordinates, subset i by the bits of i (subset 0 drops none)"""
    assert count <= 1 << len(label), (count, len(label))
    return [[int(c) for b, c in enumerate(label) if i >> b & 1] for i in range(count)]


# ------------------------------------------------------------------------------------------------ subnormal halves
def subnormal_rows(d, seed, m_max=1023, rows=4):
    """(q, X): q_i = +-1; x_i = +-(m_i + 0.49) 2^-24, m_i in 1..m_max: every half of X is fp16-subnormal and rounds down by
    0.49 of the subnormal spacing.  Row 0 is parallel to q (every product positive: the errors add up), the others have
    random signs."""
    rng = np.random.default_rng([seed, d, m_max])
    q = rng.choice(np.asarray([-1.0, 1.0]), d)
    m = rng.integers(1, m_max + 1, (rows, d)).astype(np.float64)
    sx = rng.choice(np.asarray([-1.0, 1.0]), (rows, d))
    sx[0] = q
    X = sx * (m + 0.49) * 2.0 ** -24
    return q.astype(np.float32), X.astype(np.float32)


def mixed_row(d, seed):
    """(q, x): subnormal_rows' row 0 with one component near 1 of the worst-case kind"""
    q, X = subnormal_rows(d, seed, rows=1)
    x = X[0].copy()
    x[d // 2] = q[d // 2] * DOWN
    return q, x


def grid_subnormal(d, seed, rows=6):
    """(q, X): x_i = +-(m_i + 0.5) 2^-24, m_i in 1..1022: exact ties between two subnormal halves, so the image is the EVEN
    one of m_i, m_i + 1 (truncation, rounding away and a flush all give another); q_i = +-2^p, p in 0..3.  Every product is
    an integer times 2^-24 below 2^13 and every partial sum one below 2^24 (d <= 1024): exact in fp32 in any order, so the
    fp32 s16 has ONE possible bit pattern."""
    assert d <= 1024
    rng = np.random.default_rng([seed, d, 5])
    q = rng.choice(np.asarray([-1.0, 1.0]), d) * 2.0 ** rng.integers(0, 4, d)
    m = rng.integers(1, 1023, (rows, d)).astype(np.float64)
    sx = rng.choice(np.asarray([-1.0, 1.0]), (rows, d))
    sx[0] = np.sign(q)                                    # row 0: no cancellation, the largest sum
    X = sx * (m + 0.5) * 2.0 ** -24
    return q.astype(np.float32), X.astype(np.float32)


# ------------------------------------------------------------------------------------------------ case 1: a world of rows
POW2_SCALES = (1.0, 2.0 ** -7, 32.0)      # the powers of two next to 1e-2 and 30: the pattern survives only these
PLAIN_SCALES = (1e-2, 30.0)               # the issue's own figures: the bound must hold, the pattern is lost


def bound_world(d, seed):
    """(db [64, d], queries [nq, d], tight): one-row songs.  Rows: worst_case A and B at POW2_SCALES and PLAIN_SCALES, then
    random rows of no larger a norm than A at scale 1 (so the largest norm X is that of A x 32 and eps is as small as the
    rows allow).  Queries: q at the same scales and random rows.  tight = [(query, row)] pairs of q and A at power-of-two
    scales with the row at the largest scale: the pairs whose error is 0.911 eps."""
    q, A, B = worst_case(d, seed)
    rng = np.random.default_rng([seed, d, 1])
    rows = [A * np.float32(s) for s in POW2_SCALES] + [B * np.float32(s) for s in POW2_SCALES]
    rows += [(A.astype(np.float64) * s).astype(np.float32) for s in PLAIN_SCALES]
    rows += [(B.astype(np.float64) * s).astype(np.float32) for s in PLAIN_SCALES]
    fill = rng.standard_normal((64 - len(rows), d))
    fill *= (np.linalg.norm(A.astype(np.float64)) * rng.uniform(0.05, 0.95, (fill.shape[0], 1))) / np.linalg.norm(fill, axis=1, keepdims=True)
    db = np.concatenate([np.asarray(rows, np.float32), fill.astype(np.float32)])
    qs = [q * np.float32(s) for s in POW2_SCALES] + [(q.astype(np.float64) * s).astype(np.float32) for s in PLAIN_SCALES]
    rq = rng.standard_normal((4, d)) * rng.uniform(0.01, 30.0, (4, 1)) * np.linalg.norm(q.astype(np.float64)) / np.sqrt(d)
    queries = np.concatenate([np.asarray(qs, np.float32), rq.astype(np.float32)])
    tight = [(j, 2) for j in range(len(POW2_SCALES))]    # row 2: A x 32
    assert db.shape == (64, d) and float(np.linalg.norm(db.astype(np.float64), axis=1).max()) < 1e4
    return db, queries, tight


# ------------------------------------------------------------------------------------------------ case 3: exact top-k
def topk_world(d, n, k, seed, sampled_stride=0, n_adv=3, n_rnd=3, kind="worst"):
    """A shard for the pre-filter -> dict(db, q, adv, a_rows, b_rows).
    Rows: k + 4 copies of A (scale 1: the true top-k of every adversarial query are the k best of them) and k + 20 copies of B
    (scale 1: ranked above every A copy by s16, below by the exact score), each copy without another subset of the label
    coordinates; the same copies at scales 2^-1 and 2^-2 (powers of two: the pattern holds, the scores halve); filler rows of
    0.9 ||A|| in random directions (their scores stay below a third of A's, asserted).  The largest norm is that of the A
    copy that keeps every label, so eps is as small as these rows allow.
    Placement: copy i goes to row (start + i * P) mod n, P a prime near n / 97 -- spread over the shard's tiles, slices and
    owner lanes (sublist_load counts them).  sampled_stride = R > 0 puts the A copies of scale 1 on multiples of R instead:
    the rows the dense level of a survivor ladder of that stride reads, so the exact k-th score of the level IS the k-th
    score of the shard and the full pass runs against tau = exact k-th - eps.
    kind = "split": the rows of split_parts (B copies 1.1 eps above the A copies in s16), and the B copies too on multiples of
    sampled_stride: the sampled passes see them, so the thresholds and windows hang from THEIR s16.
    q: n_adv adversarial rows (q times 1, 2^-3, 4, 2^-7, 32, cycling) followed by n_rnd random rows; adv = n_adv."""
    parts = (worst_parts if kind == "worst" else split_parts)(d, seed, labels=len(LABEL_EXP))
    q, A, B = rows_of(parts)
    rng = np.random.default_rng([seed, d, n, k])
    nA, nB = k + 4, k + 20
    fill = rng.standard_normal((n, d))
    fill *= 0.9 * np.linalg.norm(A.astype(np.float64)) / np.linalg.norm(fill, axis=1, keepdims=True)
    db = fill.astype(np.float32)
    taken = set()

    def place(start, count, grid=1):
        """`count` free rows on multiples of `grid`, a prime number of grid steps apart"""
        slots = n // grid
        step = _prime_near(max(3, slots // 97))
        while slots % step == 0:
            step = _prime_near(step + 2)
        out = []
        p = start % slots
        while len(out) < count:
            if p * grid not in taken:
                taken.add(p * grid)
                out.append(p * grid)
            p = (p + step) % slots
        return np.asarray(out, np.int64)

    # the k best A copies keep label 0 and drop a subset of the others; the four spare copies drop label 0 as well, the
    # heaviest: they trail every one of the k by more than an fp32 score resolves (asserted below), so the float64 top-k
    # and the canonical fp32 top-k are the same SET
    la = parts["label"]
    a_sub = subsets(la[1:], k) + [[int(la[0])] + sub for sub in subsets(la[1:], nA - k)]
    b_sub = subsets(parts.get("label_b", la), nB)
    a_rows = place(7, nA, sampled_stride if sampled_stride else 1)
    for r, sub in zip(a_rows, a_sub):
        db[r] = without(A, sub)
    b_rows = place(3, nB, sampled_stride if sampled_stride and kind == "split" else 1)
    for r, sub in zip(b_rows, b_sub):
        db[r] = without(B, sub)
    for scale in (0.5, 0.25):
        rows = place(11, 8)
        for i, r in enumerate(rows):
            db[r] = (without(A, a_sub[i % nA]) if i % 2 == 0 else without(B, b_sub[i % nA])) * np.float32(scale)
    scales = (1.0, 2.0 ** -3, 4.0, 2.0 ** -7, 32.0)
    adv = np.asarray([q * np.float32(scales[j % len(scales)]) for j in range(n_adv)], np.float32)
    rnd = rng.standard_normal((n_rnd, d))
    rnd *= np.linalg.norm(q.astype(np.float64)) / np.linalg.norm(rnd, axis=1, keepdims=True)
    top = exact_ref(q, A)
    ex_a = exact_ref(q, db[a_rows])
    assert ex_a[:k].min() - ex_a[k:].max() > 64 * 2.0 ** -24 * float(top), "the spare A copies are not clear of the k best"
    others = np.ones(n, bool)
    others[a_rows] = False
    others[b_rows] = False
    assert float(exact_ref(q, db[others]).max()) < 0.51 * float(top), "a filler or scaled row scores half of A's"
    norms = np.linalg.norm(db.astype(np.float64), axis=1)
    assert norms.max() == norms[a_rows[0]], "the A copy that keeps every label has the largest norm"
    return {"db": db, "q": np.concatenate([adv, rnd.astype(np.float32)]), "adv": n_adv, "a_rows": a_rows, "b_rows": b_rows}


def _prime_near(x):
    x = max(3, int(x)) | 1
    while any(x % f == 0 for f in range(3, int(x ** 0.5) + 1, 2)):
        x += 2
    return x


def threshold_distance(world, k, xmax):
    """For every adversarial query of a topk_world, from the references alone: how far the lowest s16_ref among its true
    (float64) top-k rows lies below the float64 k-th best score, in units of eps_ref -> (distances [<= 5], true top-k [<= 5, k])"""
    db, q = world["db"], world["q"][:min(world["adv"], 5)]      # (the adversarial rows cycle through five scales)
    ex = exact_ref(q, db)
    top = np.argsort(-ex, axis=1, kind="stable")[:, :k]
    s16 = s16_ref(q, db)
    eps = eps_ref(q, xmax, db.shape[1])
    out = []
    for j in range(q.shape[0]):
        kth = ex[j, top[j, -1]]
        out.append((kth - s16[j, top[j]].min()) / eps[j])
    return np.asarray(out), top


def small_sublist_load(rows, n):
    """the fullest of the 32 sub-lists of scan_small_kernel's full pass (csrc/search.hip, MODE 0) when `rows` all survive for
    one query row: wave gw of 2048 takes the 32-row tiles gw, gw + 2048, .. of the whole rounds and its share of the rows left
    over; workgroup gw / 4 writes sub-list (gw / 4) mod 32"""
    rows = np.asarray(rows, np.int64)
    W = 2048
    tail0 = (n // 32) // W * W * 32
    bounds = tail0 + np.arange(W + 1, dtype=np.int64) * (n - tail0) // W
    gw = np.where(rows < tail0, (rows // 32) % W, np.searchsorted(bounds, rows, side="right") - 1)
    return int(np.bincount((gw // 4) % 32).max())


def sublist_load(rows, tile_rows, S):
    """the fullest private survivor list of scan_f16_qres_kernel's full pass when `rows` all survive for one query row: tile
    t = row / tile_rows belongs to slice t mod S, and inside the tile rows 4 w + 8 h + .. go to owner (wave w, lane half h)
    (csrc/search_f16.hip, `frag`: tile row = 64 j + 16 g + 8 lhalf + 4 wn + e)"""
    rows = np.asarray(rows, np.int64)
    r = rows % tile_rows
    own = 4 * ((rows // tile_rows) % S) + 2 * ((r >> 2) & 1) + ((r >> 3) & 1)
    return int(np.bincount(own).max())


# ------------------------------------------------------------------------------------------------ case 4: the certificate
def certificate_world(d, n, seed, scale=1.0, kind="worst"):
    """A song world in which the dense winner is NOT the song with the best approximate total
    -> dict(db, pos, q, winner, rival).  The winner's n rows are A-type rows of n different patterns, the query's rows the q
    of those patterns, the rival's rows the B of them: in float64 the winner's total is ahead by gamma - 0.04 u of it, in s16
    the rival's by 2 u - gamma.  kind = "split": the rows of split_parts, the rival ahead by 1.18 eps = 0.57 of 2 E.
    kind = "subnormal": q_i = +-1, the winner's halves (m + 0.49) 2^-24 (m in 1..15: round down),
    the rival's (m + 0.51) 2^-24 (round up) except 0.02 d + 3 coordinates per row one step lower -- the same inversion where only
    the absolute term of eps, 3.1e-8 sqrt(d) (||q|| + X), covers it.
    Around the two: random songs of no larger a row norm, songs of one row and songs of no rows; the winner starts at row 40,
    so its columns in the tile straddle a 64-lane boundary for queries of 19 rows and a tile boundary for 64.  scale
    multiplies the db rows (a power of two: see the module's head)."""
    rng = np.random.default_rng([seed, d, n])
    if kind in ("worst", "split"):
        trip = [(worst_case if kind == "worst" else split_case)(d, seed + 101 * t) for t in range(n)]
        q = np.asarray([t[0] for t in trip])
        W = np.asarray([t[1] for t in trip])
        R = np.asarray([t[2] for t in trip])
    else:
        q = rng.choice(np.asarray([-1.0, 1.0]), (n, d))
        m = rng.integers(1, 16, (n, d)).astype(np.float64)
        W = q * (m + 0.49) * 2.0 ** -24
        low = np.zeros((n, d))
        for t in range(n):
            c = rng.choice(np.flatnonzero(m[t] >= 2), int(0.02 * d) + 3, replace=False)
            low[t, c] = 1.0
        R = q * (m - low + 0.51) * 2.0 ** -24
    row_norm = float(np.linalg.norm(np.asarray(W, np.float64), axis=1).min())

    def noise(rows):
        x = rng.standard_normal((rows, d))
        return x * (row_norm * rng.uniform(0.3, 0.9, (rows, 1))) / np.linalg.norm(x, axis=1, keepdims=True)
    songs = [noise(30)] + [noise(1) for _ in range(5)] + [noise(0), noise(1), noise(0)] + [noise(1) for _ in range(4)]
    winner = len(songs)
    songs += [np.asarray(W, np.float64), noise(0), noise(1)]
    rival = len(songs)
    songs += [np.asarray(R, np.float64), noise(0), noise(1), noise(50)]
    pos = np.pad(np.cumsum([s.shape[0] for s in songs]), (1, 0)).astype(np.int64)
    assert pos[winner] == 40
    db = (np.concatenate(songs) * scale).astype(np.float32)
    return {"db": db, "pos": pos, "q": np.asarray(q, np.float32), "winner": winner, "rival": rival}


def song_totals(world, score):
    """per song the best total over every alignment of the query, from score(q, db) [n, rows] in float64 -> [songs]"""
    q, db, pos = world["q"], world["db"], world["pos"]
    S = score(q, db)
    n = q.shape[0]
    best = np.full(len(pos) - 1, -np.inf)
    for s in range(len(pos) - 1):
        a, b = int(pos[s]), int(pos[s + 1])
        for o in range(-(n - 1), b - a):
            t = np.arange(max(0, -o), min(n, b - a - o))
            best[s] = max(best[s], float(S[t, a + o + t].sum()))
    return best


# ------------------------------------------------------------------------------------------------ the cases of the GPU tests
# (here, so that tests/test_fp16_margin_host.py holds the very inputs of tests/test_gpu_fp16_margin.py to their conditions)
TOPK_SEED = 5
#            name            d     n      adv  rnd  k    path                    sampled stride
TOPK_CASES = [("small_folded", 128, 9001, 3, 2, 20, "small_sampled_folded", 0),
              ("small_d64", 64, 9001, 20, 12, 1, "small_sampled", 0),
              ("gmax_mid", 128, 70000, 100, 100, 100, "gmax", 0),
              ("gmax_1024", 64, 70000, 512, 512, 20, "gmax", 0),
              ("ladder_d96", 96, 20000, 20, 20, 100, "ladder_f16", 16),
              ("ladder_d1024", 1024, 8208, 17, 17, 20, "ladder_f16", 16),
              # split_parts: B copies MORE than one eps above the A copies; both on rows the sampled passes read (every 4th
              # row serves the small path's stride 4 and the group-maximum pass's stride 2, every 16th the ladder)
              ("split_small_folded", 128, 9001, 3, 2, 20, "small_sampled_folded", 4),
              ("split_gmax", 128, 70000, 100, 100, 100, "gmax", 4),
              ("split_ladder_d96", 96, 20000, 20, 20, 100, "ladder_f16", 16)]
POW2_DB_SCALES = (1.0, 32.0, 2.0 ** -7)
CERT_ROWS = (1, 19, 64)
CERT_CASES = ([("worst", d, s) for d in (128, 256) for s in POW2_DB_SCALES] + [("split", 128, s) for s in POW2_DB_SCALES]
              + [("split", 256, 1.0), ("subnormal", 128, 1.0), ("subnormal", 256, 1.0)])
