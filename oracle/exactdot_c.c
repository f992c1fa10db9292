/* Oracle (TEST INFRASTRUCTURE): the canonical fp32 score of the exact search.
 *
 * Every re-scoring site of the search (search_common.h, canon_dot4) computes q.x for d % 4 == 0 as
 *   for l in 0..3:  p_l = 0;  for e = 4l, 4l + 16, ... < d, t = 0..3 in order:  p_l = fmaf(x[e + t], q[e + t], p_l)
 *   score = (p0 + p1) + (p2 + p3)
 * all in fp32.  This file states that order in plain C, so a test can ask for the bits a correct kernel returns.
 * Built with -O2 -ffp-contract=off and no fast-math (oracle/native.py): no contraction or reassociation of the
 * adds, and fmaf is libm's correctly rounded fused multiply-add whether or not the target has an fma instruction.
 */
#include <math.h>
#include <stdint.h>

static float canon_dot(const float *q, const float *x, int d) {
    float p[4];
    for (int l = 0; l < 4; l++) {
        float acc = 0.0f;
        for (int e = 4 * l; e < d; e += 16)
            for (int t = 0; t < 4; t++) acc = fmaf(x[e + t], q[e + t], acc);
        p[l] = acc;
    }
    const float a = p[0] + p[1];
    const float b = p[2] + p[3];
    return a + b;
}

/* out[i] = canon(query[qi[i]], db[xi[i]]) for i < npairs */
void oracle_canon_scores(const float *query, const float *db, int d, const int64_t *qi, const int64_t *xi,
                         int64_t npairs, float *out) {
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < npairs; i++) out[i] = canon_dot(query + qi[i] * (int64_t)d, db + xi[i] * (int64_t)d, d);
}
