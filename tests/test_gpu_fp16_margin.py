"""The fp16 margin under attack (tests/fp16_margin_cases.py): the device's s16 against float64 on rows built to come within a
tenth of the bound, subnormal halves bit for bit, the exact top-k where fp16 inverts the ranking, and the certificate of the
dense nomination where it must say no.  tests/test_fp16_margin_host.py holds the inputs to what they claim.

Scales.  The rounding pattern survives only powers of two (30 x A and 30 x B round to the SAME halves), so where a case needs
the pattern the db scales 1e-2 and 30 are taken as 2^-7 and 32; case 1 also runs the plain 1e-2 and 30, on which the bound
must hold like on any row.

Which change of the bound fails which case.  Each line is this file, as it stands, run once on the MI355X against a library
built with that one change (31 cases; the ones not named passed):
  1. `1.05e-3f -> 5.0e-4f` in q_prep_kernel: test_prefilter_keeps_the_exact_topk[ladder_d96], [ladder_d1024], [split_gmax],
     [split_ladder_d96].  The ladders scan against (exact k-th score) - eps and the true rows lie 0.91 eps (split: 0.64 eps,
     under a select window of 0.95 eps with decoys 1.18 eps up) below it; split_gmax scans against a decoy's s16 - 0.95 eps,
     1.13 eps above the true rows.  NOT failed: small_d64, gmax_mid, gmax_1024 -- their thresholds hang from an s16 minus 2 eps
     and the worst_case decoys lead by 0.26 - 0.58 eps only -- and the folded small path, which never runs q_prep_kernel:
  1b. the same in the folded copy of the expression (scan_small_kernel, csrc/search.hip): [split_small_folded].
  2. the same in nominate_prep_kernel: test_certificate_says_no[split-128-1.0], [split-128-32.0], [split-128-0.0078125],
     [split-256-1.0] (n_close = 1: certified although the winner is not listed).  The worst kind's lead, 0.24 of 2 E, stays
     inside the halved margin.
  3. the select windows `2 eps -> 1 eps` (the three `e2` of csrc/search_f16.hip): test_prefilter_keeps_the_exact_topk
     [split_small_folded], [split_gmax], [split_ladder_d96] -- the k-th best s16 is a decoy's, 1.13 - 1.18 eps above every true
     row.  With worst_case rows alone this change survives: a query whose rounding the true row and the decoy SHARE cannot
     separate them by more than ~0.93 eps; split_parts lets the query round down on the true row's coordinates and up on the
     decoy's, which is what takes the lead past 1 eps.
  4. the `3.1e-8f` term removed (q_prep_kernel, its folded copy and nominate_prep_kernel at once): test_certificate_says_no
     [subnormal-128-1.0], [subnormal-256-1.0].  It is the copy in nominate_prep_kernel that these catch; no search case has
     subnormal rows, so the term's absence from the two search copies alone would pass this file.
"""
import os
import re
import shutil

import numpy as np
import pytest

import fp16_margin_cases as fc
import score_bits

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _one_row_songs(torch, db, queries):
    """every row a song, every query one row, n = 64: entry.score IS the device's S16 -> (S [nq, rows] float32, X, index)"""
    from pfann_amd.database import DeviceIndex
    n = db.shape[0]
    assert n <= 64
    idx = DeviceIndex(db.shape[1], 0)
    idx.load(db, np.arange(n + 1, dtype=np.int64))
    nq = queries.shape[0]
    cand, n_found, _ = idx.nominate_songs_dense(torch.as_tensor(queries).cuda(), list(range(nq)), [1] * nq, 64)
    assert (n_found == n).all(), n_found
    S = np.full((nq, n), np.nan, np.float32)
    for j in range(nq):
        S[j, cand["song"][j, :n]] = cand["score"][j, :n].astype(np.float32)
        assert (cand["score"][j, :n] == cand["score"][j, :n].astype(np.float32)).all(), "a total of one row dot is an fp32"
    assert not np.isnan(S).any()
    return S, idx.row_norm_max(), idx


def _half_storage(torch, db, queries, nq):
    """fp16-only storage: D of search is s16 itself -> S [nq, rows] float32 (query row m = queries[m mod len])"""
    from pfann_amd.database import DeviceIndex
    n = db.shape[0]
    idx = DeviceIndex(db.shape[1], 0, storage="f16")
    idx.load(db, np.asarray([0, n], np.int64))
    D, I = idx.search(torch.as_tensor(queries[np.arange(nq) % queries.shape[0]]).cuda(), n)
    D, I = D.cpu().numpy(), I.cpu().numpy()
    assert (np.sort(I, 1) == np.arange(n)[None, :]).all()
    S = np.empty((nq, n), np.float32)
    np.put_along_axis(S, I, D, 1)
    return S


def _hold_to_the_bound(S, queries, db, d, xmax, what, with_totals=True):
    """the two inequalities of every (query, row): |S - exact| <= eps (E of a one-row query where the route has one), and
    |S - s16_ref| <= d 2^-24 sum |fl16(q_i) fl16(x_i)|, the fp32 accumulation alone -> the largest |S - exact| / bound"""
    m = np.arange(S.shape[0]) % queries.shape[0]
    q = queries[m]
    ex, s16, mag = fc.exact_ref(q, db), fc.s16_ref(q, db), fc.abs16_ref(q, db)
    bound = np.asarray([fc.margin_ref(q[j:j + 1], d, xmax) for j in range(q.shape[0])]) if with_totals else fc.eps_ref(q, xmax, d)
    err = np.abs(S.astype(np.float64) - ex)
    acc = np.abs(S.astype(np.float64) - s16)
    j, r = np.unravel_index(np.argmax(err / bound[:, None]), err.shape)
    print("%s: largest |dev - exact| / bound %.4f (query %d row %d), largest accumulation error %.3g of its allowance" % (
        what, err[j, r] / bound[j], j, r, float((acc / np.maximum(d * 2.0 ** -24 * mag, 1e-300)).max())))
    assert (err <= bound[:, None]).all(), (what, "query %d row %d: |dev - exact| %.6g > %.6g" % (j, r, err[j, r], bound[j]))
    bad = np.argwhere(acc > d * 2.0 ** -24 * mag)
    assert bad.size == 0, (what, "query %d row %d: dev %.9g, s16_ref %.9g" % (bad[0][0], bad[0][1], S[tuple(bad[0])], s16[tuple(bad[0])]))
    return float(err[j, r] / bound[j])


# ------------------------------------------------------------------------------------------------ 1. the bound, observed
@pytest.mark.parametrize("d", [8, 24, 64, 128, 136, 256, 1024])
def test_the_bound_on_worst_case_rows(torch_cuda, d):
    """d = 24: a partial MFMA step; 136: the 8-half tail of nominate_tile_kernel's second K block; 256, 1024: whole further
    K blocks.  Printed: the largest |dev - exact| / E, and on the tight pairs (q and A x 32, power-of-two scales) the ratio
    against eps alone -- 0.911 on the CPU (E carries the fp32 allowance 2^-22 (d + 1) ||q|| X on top: 0.23 eps at d = 1024)."""
    db, queries, tight = fc.bound_world(d, 1)
    S, xmax, _ = _one_row_songs(torch_cuda, db, queries)
    assert abs(xmax / float(fc.norm32(db).max()) - 1.0) < 1e-6
    _hold_to_the_bound(S, queries, db, d, xmax, "d %d nominate" % d)
    eps = fc.eps_ref(queries, xmax, d)
    for j, r in tight:
        ratio = abs(float(S[j, r]) - float(fc.exact_ref(queries[j], db[r:r + 1])[0])) / eps[j]
        print("d %d nominate: query %d x row %d: |dev - exact| / eps = %.4f" % (d, j, r, ratio))
        # 0.911 less the fp32 accumulation at its worst (0.058 eps at d = 1024, tests/test_fp16_margin_host.py)
        assert 0.85 <= ratio <= 1.0, (d, j, r, ratio)
    for nq in (1, 40, 1100):
        Sh = _half_storage(torch_cuda, db, queries, nq)
        _hold_to_the_bound(Sh, queries, db, d, xmax, "d %d fp16 storage nq %d" % (d, nq), with_totals=False)
        for j, r in tight:
            if j < nq:
                ratio = abs(float(Sh[j, r]) - float(fc.exact_ref(queries[j], db[r:r + 1])[0])) / eps[j]
                assert 0.85 <= ratio <= 1.0, (d, nq, j, r, ratio)


# ------------------------------------------------------------------------------------------------ 2. subnormal halves
@pytest.mark.parametrize("d", [8, 128, 1024])
def test_subnormal_halves(torch_cuda, d):
    """grid_subnormal: one possible bit pattern.  A flush in rows_to_half_kernel, in either query preparation or in the
    MFMA's A/B inputs gives 0 (or drops the subnormal part), a truncating conversion the odd neighbour."""
    gq, gX = fc.grid_subnormal(d, 3)
    sq, sX = fc.subnormal_rows(d, 2)
    db = np.concatenate([gX, sX])
    queries = np.stack([gq, sq])
    want = fc.s16_ref(gq, gX).astype(np.float32)
    assert (want.astype(np.float64) == fc.s16_ref(gq, gX)).all()
    S, xmax, _ = _one_row_songs(torch_cuda, db, queries)
    print("d %d grid: device %r, reference %r" % (d, S[0, :3].tolist(), want[:3].tolist()))
    assert S[0, :gX.shape[0]].tobytes() == want.tobytes(), (S[0, :gX.shape[0]], want)
    r = _hold_to_the_bound(S, queries, db, d, xmax, "d %d subnormal nominate" % d)
    flushed = float(np.abs(fc.flushed_ref(queries, db) - fc.exact_ref(queries, db)).max() / fc.eps_ref(queries, xmax, d).min())
    assert r <= 1.0 < flushed
    for nq in (1, 40):
        Sh = _half_storage(torch_cuda, db, queries, nq)
        assert Sh[0, :gX.shape[0]].tobytes() == want.tobytes(), (nq, Sh[0, :gX.shape[0]], want)
        _hold_to_the_bound(Sh, queries, db, d, xmax, "d %d subnormal fp16 storage nq %d" % (d, nq), with_totals=False)
    # one component near 1, the rest subnormal: the subnormal part is d - 1 terms of the sum and must not vanish beside it
    mq, mx = fc.mixed_row(d, 2)
    mdb = np.concatenate([mx[None], sX])
    S, xmax, _ = _one_row_songs(torch_cuda, mdb, mq[None])
    _hold_to_the_bound(S, mq[None], mdb, d, xmax, "d %d mixed nominate" % d)
    Sh = _half_storage(torch_cuda, mdb, mq[None], 1)
    _hold_to_the_bound(Sh, mq[None], mdb, d, xmax, "d %d mixed fp16 storage" % d, with_totals=False)
    assert float(S[0, 0]) != float(fc.flushed_ref(mq, mx[None])[0]) and float(Sh[0, 0]) != float(fc.flushed_ref(mq, mx[None])[0])


# ------------------------------------------------------------------------------------------------ 3. the exact top-k
TOPK_CASES = fc.TOPK_CASES


@pytest.mark.parametrize("name,d,n,n_adv,n_rnd,k,path,stride", TOPK_CASES, ids=[c[0] for c in TOPK_CASES])
def test_prefilter_keeps_the_exact_topk(torch_cuda, name, d, n, n_adv, n_rnd, k, path, stride):
    """fc.topk_world: the true top-k of every adversarial query are A copies whose s16 lies 0.91 eps BELOW the exact k-th
    score, under more than k B copies that outrank them in s16.
    The rows the sampled levels read.  ladder_f16 (R = 16, one sampled level): the dense level reads the rows 0, 16, 32, ..;
    every A copy of scale 1 sits on such a row, so that level's k-th exact score is the shard's and the full pass runs
    against tau = exact k-th - eps: the A copies pass it by 0.09 eps.  The small path and the group-maximum plans take their
    threshold from s16 group maxima minus 2 eps (see the module's head): nothing placed anywhere makes that sharp, the copies
    are spread with a prime stride so that no sub-list fills (asserted from the kernels' row -> list maps)."""
    from pfann_amd.database import DeviceIndex
    torch = torch_cuda
    kind = "split" if name.startswith("split") else "worst"
    w = fc.topk_world(d, n, k, fc.TOPK_SEED, stride, n_adv, n_rnd, kind)
    db, q = w["db"], w["q"]
    idx = DeviceIndex(d, 0)
    idx.load(db, np.asarray([0, n], np.int64))
    stages, flags = idx.search_plan(q.shape[0], k)
    assert flags["path"] == path and flags["canonical_scores"] == "1", flags
    copies = np.concatenate([w["a_rows"], w["b_rows"]])
    if path == "gmax":
        full = [s for s in stages if s[0].startswith("scan_f16_qres_kernel") and "false" in s[0]]
        assert len(full) == 1, stages
        # scan_f16_qres_kernel<KS, GMAX, DBR, NBUF>: the db rows per tile are the third template argument
        name_args = re.fullmatch(r"scan_f16_qres_kernel<(\d+), false, (64|128), (2|3)>", full[0][0])
        assert name_args, full[0][0]
        tile_rows = int(name_args.group(2))
        S = full[0][1] // ((q.shape[0] + 127) // 128)
        load, cap = fc.sublist_load(copies, tile_rows, S), 8192 // (4 * S)
    elif path.startswith("small"):
        load, cap = fc.small_sublist_load(copies, n), 8192 // 32
    else:
        load, cap = len(copies), 8192
    assert 4 * load <= cap, "a survivor list fills past a quarter: %d of %d" % (load, cap)
    xmax = idx.row_norm_max()
    dist, top = fc.threshold_distance(w, k, xmax)
    s16 = fc.s16_ref(q[:1], db)[0]
    b_above = (s16[w["b_rows"]].min() - s16[w["a_rows"]].max()) / fc.eps_ref(q[:1], xmax, d)[0]
    print("%s (d %d, n %d, nq %d, k %d, %s): the worst true top-k row's s16 lies %.4f eps below the exact k-th score; "
          "the B copies lie %.3f eps above the A copies in s16; fullest survivor list %d of %d" % (
              name, d, n, q.shape[0], k, path, dist.min(), b_above, load, cap))
    if kind == "worst":
        assert (dist >= 0.85).all() and b_above > 0, (dist, b_above)
    else:                                                # (0.64 eps below the k-th score: these rows attack the windows)
        assert (dist >= 0.6).all() and b_above >= 1.05, (dist, b_above)
    D, I = idx.search(torch.as_tensor(q).cuda(), k)
    D, I = D.cpu().numpy(), I.cpu().numpy()
    for j in range(top.shape[0]):                        # (the adversarial rows cycle through five scales)
        for m in range(j, n_adv, 5):
            lost = sorted(set(top[j].tolist()) - set(I[m].tolist()))
            assert not lost, "query row %d: A copies %r of the float64 top-%d are not returned" % (m, lost[:8], k)
    score_bits.assert_canonical_topk(D, I, q, db, k, what=name)


# ------------------------------------------------------------------------------------------------ 4. the certificate
def _write_world(dirname, w):
    os.makedirs(dirname)
    shutil.copy(os.path.join(REPO, "configs", "default.json"), os.path.join(dirname, "configs.json"))
    lens = np.diff(w["pos"])
    with open(os.path.join(dirname, "songList.txt"), "w") as f:
        f.write("".join("song%02d.wav\n" % s for s in range(len(lens))))
    lens.astype(np.int32).tofile(os.path.join(dirname, "landmarkKey"))
    w["db"].tofile(os.path.join(dirname, "embeddings"))


CERT_CASES = fc.CERT_CASES


@pytest.mark.parametrize("kind,d,scale", CERT_CASES)
def test_certificate_says_no(torch_cuda, tmp_path, kind, d, scale):
    """fc.certificate_world: the dense winner is a song of A-type rows, the rival song of B-type rows has the higher
    approximate total; queries of 1, 19 and 64 rows.  kind = split: the rows of fc.split_parts, the rival ahead by 0.48 - 0.58 of
    2 E (worst: 0.25).  kind = subnormal: the same inversion on subnormal halves, where only
    the absolute term of eps covers it (the rival leads by 0.9 of 2 E there)."""
    from pfann_amd import database as dbm
    from pfann_amd.utils import read_config
    torch = torch_cuda
    for n in fc.CERT_ROWS:
        w = fc.certificate_world(d, n, 9, scale, kind)
        dirname = str(tmp_path / ("n%d" % n))
        _write_world(dirname, w)
        cfg = read_config(os.path.join(dirname, "configs.json"))
        db = dbm.Database(dirname, cfg["indexer"], cfg["hop_size"], d=d)
        idx = db.index
        win, riv = w["winner"], w["rival"]
        xmax = idx.row_norm_max()
        T, A16 = fc.song_totals(w, fc.exact_ref), fc.song_totals(w, fc.s16_ref)
        allowance = 2.0 ** -22 * (d + n) * float(np.float32(xmax)) * float(fc.norm32(w["q"]).astype(np.float64).sum())
        E = fc.margin_ref(w["q"], d, xmax)
        print("%s d %d scale %g, %d rows: float64 lead of the winner %.4g (fp32 allowance %.4g); the rival's lead in s16 %.4g = "
              "%.3f of 2 E" % (kind, d, scale, n, T[win] - T[riv], allowance, A16[riv] - A16[win], (A16[riv] - A16[win]) / (2 * E)))
        assert int(np.argmax(T)) == win and T[win] - np.delete(T, win).max() > allowance
        qd = torch.as_tensor(w["q"]).cuda()
        (ref, ref_found, _), _ = idx.match_windows_dense_topn(qd, [0], [n], 64, 1, 2)
        assert int(ref["song"][0, 0]) == win, ref[0]
        cand, _, n_close = idx.nominate_songs_dense(qd, [0], [n], 1)
        assert int(cand["song"][0, 0]) == riv and int(n_close[0]) >= 2, (cand[0], n_close)
        _, _, certified = db.query_nominate_rescore_batch(qd, [0], [n], 1)
        assert not bool(certified[0]), "certified although the winner is not listed"
        dense_answers, _ = db.query_dense_batch(qd, [0], [n], n=1)
        answers, ranked, certified = db.query_nominate_rescore_batch(qd, [0], [n], 2)
        assert bool(certified[0]) and answers[0][:2] == dense_answers[0][:2]
        raw, _, close = idx.nominate_songs_dense(qd, [0], [n], 2, to_host=False)
        top, _ = idx.match_songs_dense(qd, [0], [n], raw)
        assert int(close.cpu().numpy()[0]) == 2
        assert top[0, 0:1].tobytes() == ref[0, 0:1].tobytes(), (top[0], ref[0])
