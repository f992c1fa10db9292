"""The adversarial inputs of tests/fp16_margin_cases.py, held to what they claim -- on the CPU, from the references alone.
These are conditions on the INPUTS, not measurements of the library: a GPU test of tests/test_gpu_fp16_margin.py that passes
cannot have been fed easy rows.  The last test pins the text of the bound in every place that states it."""
import os
import re

import numpy as np
import pytest

import fp16_margin_cases as fc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_D = (8, 24, 64, 128, 136, 256, 1024)                 # the d of tests/test_gpu_fp16_margin.py's case 1


def _ratio(q, X, d):
    X = np.atleast_2d(X)
    xmax = float(fc.norm32(X).max())
    return np.abs(fc.s16_ref(q, X) - fc.exact_ref(q, X)) / fc.eps_ref(q, xmax, d)[0]


@pytest.mark.parametrize("d", [8, 64, 128, 256, 1024])
def test_worst_case_rows_come_close_to_the_bound(d):
    q, A, B = fc.worst_case(d, 1)
    r = _ratio(q, np.stack([A, B]), d)
    print("d %d: |s16 - exact| / eps = %.4f (A), %.4f (B)" % (d, r[0], r[1]))
    assert r[0] >= 0.85 and (r <= 1.0).all()
    # the fp32 accumulation, at worst d 2^-24 of the sum of the products' magnitudes, still fits under the bound
    acc = d * 2.0 ** -24 * fc.abs16_ref(q, A[None])[0] / fc.eps_ref(q, float(fc.norm32(A)[0]), d)[0]
    assert r[0] + acc <= 1.0, (r[0], acc)


@pytest.mark.parametrize("d", GPU_D)
def test_worst_case_inverts_the_ranking(d):
    q, A, B = fc.worst_case(d, 1)
    ex, s16 = fc.exact_ref(q, np.stack([A, B])), fc.s16_ref(q, np.stack([A, B]))
    a_beats_b, b_beats_a = (ex[0] - ex[1]) / ex[0], (s16[1] - s16[0]) / ex[0]
    print("d %d: A beats B by %.3g in float64, B beats A by %.3g in s16" % (d, a_beats_b, b_beats_a))
    assert a_beats_b >= 1e-4
    assert fc.inverts(d) == (d >= 64)
    if fc.inverts(d):                                    # d < 64: the exponents -3..0 do not allow both (fc.inverts)
        assert b_beats_a >= 1e-4
    assert _ratio(q, A, d)[0] >= 0.85


@pytest.mark.parametrize("d", [8, 128, 1024])
def test_subnormal_rows(d):
    q, X = fc.subnormal_rows(d, 2)
    assert (np.abs(fc.f16(X)) < 2.0 ** -14).all() and (fc.f16(X) != 0).all(), "every half is subnormal"
    r = _ratio(q, X, d)
    xmax = float(fc.norm32(X).max())
    flushed = abs(fc.flushed_ref(q, X)[0] - fc.exact_ref(q, X)[0]) / fc.eps_ref(q, xmax, d)[0]
    print("d %d: |s16 - exact| / eps = %.4f, with every subnormal half flushed %.0f" % (d, r[0], flushed))
    assert r[0] >= 0.35 and (r <= 1.0).all() and flushed > 100.0
    q, x = fc.mixed_row(d, 2)
    assert _ratio(q, x, d)[0] <= 1.0 and (np.abs(fc.f16(x)) < 2.0 ** -14).sum() == d - 1


@pytest.mark.parametrize("d", [8, 128, 1024])
def test_grid_subnormal_has_one_answer(d):
    q, X = fc.grid_subnormal(d, 3)
    m = np.abs(X.astype(np.float64)) * 2.0 ** 24
    assert (m % 1.0 == 0.5).all(), "exact ties"
    h = np.abs(fc.f16(X)) * 2.0 ** 24
    assert (h % 2.0 == 0.0).all() and (np.abs(h - m) == 0.5).all(), "round to even"
    prods = fc.f16(q)[None, :] * fc.f16(X) * 2.0 ** 24
    assert (prods % 1.0 == 0.0).all() and np.abs(prods).sum(1).max() < 2.0 ** 24, "every partial sum is an fp32 integer grid point"
    s = fc.s16_ref(q, X)
    assert (s.astype(np.float32).astype(np.float64) == s).all() and (s != 0).all()
    assert (fc.flushed_ref(q, X) == 0).all() and (s != np.trunc(m) @ fc.f16(q) * 2.0 ** -24).any()


@pytest.mark.parametrize("name,d,n,n_adv,n_rnd,k,path,stride", fc.TOPK_CASES, ids=[c[0] for c in fc.TOPK_CASES])
def test_topk_world_is_adversarial(name, d, n, n_adv, n_rnd, k, path, stride):
    """the shards of test_prefilter_keeps_the_exact_topk (the db does not depend on the number of query rows)"""
    kind = "split" if name.startswith("split") else "worst"
    w = fc.topk_world(d, n, k, fc.TOPK_SEED, stride, 5, 0, kind)
    xmax = float(fc.norm32(w["db"]).max())
    dist, top = fc.threshold_distance(w, k, xmax)
    q = w["q"][:w["adv"]]
    s16, eps = fc.s16_ref(q, w["db"]), fc.eps_ref(q, xmax, d)
    lead = np.asarray([(s16[j, w["b_rows"]].min() - s16[j, w["a_rows"]].max()) / eps[j] for j in range(len(q))])
    print("%s: true top-k %.4f eps below the exact k-th score, B copies %.3f eps above the A copies" % (name, dist.min(), lead.min()))
    assert (dist <= 1.0).all() and (dist >= (0.85 if kind == "worst" else 0.6)).all()
    assert (lead > 0).all() if kind == "worst" else (lead >= 1.05).all()
    assert len(w["b_rows"]) > k
    for j in range(len(q)):
        assert set(top[j].tolist()) == set(w["a_rows"][:k].tolist())
        # the select's cut, (k-th best s16) - window: 2 eps keeps every true row; for the split kind 1 eps would keep none
        kth16 = np.sort(s16[j])[-k]
        assert (s16[j, top[j]] >= kth16 - 2 * eps[j]).all()
        if kind == "split":
            assert (s16[j, top[j]] < kth16 - eps[j]).all()
    ex = fc.exact_ref(q[0], w["db"][w["a_rows"]])
    assert len(set(ex.tolist())) == len(ex), "the A copies' exact scores are distinct"
    if stride:
        assert (w["a_rows"] % stride == 0).all() and (kind == "worst" or (w["b_rows"] % stride == 0).all())


@pytest.mark.parametrize("n", fc.CERT_ROWS)
@pytest.mark.parametrize("kind,d,scale", fc.CERT_CASES)
def test_certificate_world_inverts_the_songs(kind, d, scale, n):
    """the worlds of test_certificate_says_no: the rival leads in s16 by no more than 2 E (n_close must count it), the third
    song is further than 2 E away; split and subnormal: the lead is more than 0.47 of 2 E, the worst kind's a quarter"""
    w = fc.certificate_world(d, n, 9, scale, kind)
    T, A = fc.song_totals(w, fc.exact_ref), fc.song_totals(w, fc.s16_ref)
    xmax = float(fc.norm32(w["db"]).max())
    E = fc.margin_ref(w["q"], d, xmax)
    allowance = 2.0 ** -22 * (d + n) * xmax * float(fc.norm32(w["q"]).astype(np.float64).sum())
    assert int(np.argmax(T)) == w["winner"] and T[w["winner"]] - np.delete(T, w["winner"]).max() > allowance
    assert int(np.argmax(A)) == w["rival"]
    lead = (A[w["rival"]] - A[w["winner"]]) / (2 * E)
    assert 0 < lead <= 1.0 and lead >= {"worst": 0.2, "split": 0.47, "subnormal": 0.85}[kind], lead
    assert np.sort(A)[-3] < A.max() - 2 * E, "only the two are close"


def _function_text(path, name):
    text = open(os.path.join(REPO, path)).read()
    at = text.index(name + "(")
    return text[at:text.index("\n}\n", at)]


def test_the_bound_reads_the_same_wherever_it_stands():
    """one bound: q_prep_kernel, its folded copy at the head of scan_small_kernel's sampled pass, nominate_prep_kernel, and
    the margin of the public header"""
    code = re.compile(r"1\.05e-3f \* nq2 \* (\w+\.)?xnorm_max \+ 3\.1e-8f \* sqrtf\(\(float\)(\w+\.)?[dD]\) \* \(nq2 \+ (\w+\.)?xnorm_max\)")
    assert len(code.findall(_function_text("pfann_amd/csrc/search_f16.hip", "void q_prep_kernel"))) == 1
    assert len(code.findall(_function_text("pfann_amd/csrc/nominate.hip", "void nominate_prep_kernel"))) == 1
    header = open(os.path.join(REPO, "include/pfann_amd.h")).read()
    assert "eps_t = 1.05e-3 ||q_t|| X + 3.1e-8 sqrt(d) (||q_t|| + X)" in header
    for path, name in (("pfann_amd/csrc/search_f16.hip", "void q_prep_kernel"), ("pfann_amd/csrc/search.hip", "void scan_small_kernel"),
                       ("pfann_amd/csrc/nominate.hip", "void nominate_prep_kernel")):
        body = _function_text(path, name)
        assert len(code.findall(body)) == len(re.findall(r"1\.05e-3f", body)) == len(re.findall(r"3\.1e-8f", body)) == 1, path
