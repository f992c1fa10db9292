// Shared pieces of the exact top-k search (search.hip, search_f16.hip).
#pragma once
#include "kernels.h"
#include "search_plan.h"

namespace pfann {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ unsigned f2ord(float f) {   // monotone float -> uint
    const unsigned u = __float_as_uint(f);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float ord2f(unsigned o) {
    const unsigned u = o ^ ((o >> 31) ? 0x80000000u : 0xFFFFFFFFu);
    return __uint_as_float(u);
}
// ascending sort of packed keys == descending score, ascending row
__device__ __forceinline__ unsigned long long pack_key(float score, unsigned row) {
    return ((unsigned long long)(~f2ord(score)) << 32) | row;
}


struct ScanParams {
    const float *q, *db;
    int64_t nq, nrows;       // nrows = rows scanned at this level = ceil(N / stride)
    int64_t row_stride;      // db row step (level stride)
    int d;
    const float *thr;        // [nq] or nullptr (= emit everything, densely: slot = row index)
    int *cnt;                // [nq]
    unsigned long long *keys;  // [nq][CAP]
    int n_tiles_m;
    int nsub;                // survivor sub-lists per query row (small-batch kernel: 32), else 1
    float *gmax;             // small-batch kernel, group-maximum mode: [nq][gridDim.x * 4]
    // small-batch group-maximum pass with the query preparation folded in (ELT = 2: q32 = the fp32 query rows, p.q unused;
    // what q_prep_kernel does, one launch less): workgroup 0 leaves qh / eps / row_ovf for the launches that follow
    const float *q32 = nullptr;
    float xnorm_max = 0.f;
    void *qh_out = nullptr;  // [nq][d] fp16 query rows
    float *eps = nullptr;    // [nq]
    int *row_ovf = nullptr;
    // the masked twins (EXCL = true; excl_prep_kernel writes both): query row m leaves rows [excl[m].x, excl[m].y) of the
    // shard out (row space, clipped; empty = (0, 0)); excl_tile[m / 128] = the span of the union of a 128-row query tile's
    // ranges ((0xFFFFFFFF, 0) when all are empty): a db tile outside it runs the unmasked epilogue
    const uint2 *excl = nullptr, *excl_tile = nullptr;
};
// row in [lo, hi) of an exclusion range
// (one unsigned compare: row - lo wraps above every length when row < lo; an empty range has length 0)
__device__ __forceinline__ bool excl_hit(uint2 r, unsigned row) { return row - r.x < r.y - r.x; }
// rows [first, last] meet the span of a query tile's ranges
__device__ __forceinline__ bool excl_span_hit(uint2 span, int64_t first, int64_t last) {
    return first < (int64_t)span.y && last >= (int64_t)span.x;
}


// The canonical fp32 score of a row, computed by the four adjacent lanes 4 c .. 4 c + 3 of a candidate:
//   canon_part: lane sub's fma chain, p_sub = fmaf(x[e + t], q[e + t], p_sub) over e = 4 sub, 4 sub + 16, ... < d, t = 0..3
//   canon_sum:  (p0 + p1) + (p2 + p3), in every lane of the four
// Every exact re-scoring site uses it (the select kernels of search_f16.hip, topk_fallback_body), so a row's fp32 score has
// the same bits whichever kernel, shard split or batch produced it; oracle/exactdot_c.c states the same order in C.
// T = float: the fp32 rows; T = _Float16: fp16-only storage (the fallback, where the s16 scores are the result).  xv and qv
// are 16-byte aligned (d % 4 == 0).
template <typename T>
__device__ __forceinline__ float canon_part(const T *__restrict__ xv, const float *qv, int d, int sub) {
    float part = 0.f;
    for (int e = sub * 4; e < d; e += 16) {
        float x0, x1, x2, x3;
        if constexpr (sizeof(T) == 4) {
            const float4 x4 = *reinterpret_cast<const float4 *>(xv + e);
            x0 = x4.x; x1 = x4.y; x2 = x4.z; x3 = x4.w;
        } else {
            typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
            const f16x4 h4 = *reinterpret_cast<const f16x4 *>(xv + e);
            x0 = (float)h4[0]; x1 = (float)h4[1]; x2 = (float)h4[2]; x3 = (float)h4[3];
        }
        const float4 q4 = *reinterpret_cast<const float4 *>(qv + e);
        part = fmaf(x0, q4.x, part); part = fmaf(x1, q4.y, part);
        part = fmaf(x2, q4.z, part); part = fmaf(x3, q4.w, part);
    }
    return part;
}
__device__ __forceinline__ float canon_sum(float part) {
    part += __shfl_xor(part, 1, 64);             // lane 4c: p0 + p1, lane 4c + 2: p2 + p3
    part += __shfl_xor(part, 2, 64);             // (p0 + p1) + (p2 + p3) (fp32 addition commutes: every lane has the same bits)
    return part;
}

__device__ inline void bitonic_sort_u64(unsigned long long *s, int P, int tid, int nt) {
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += nt) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const unsigned long long a = s[i], b = s[ixj];
                    const bool up = (i & k) == 0;
                    if ((a > b) == up) { s[i] = b; s[ixj] = a; }
                }
            }
            __syncthreads();
        }
    }
}

// Exact fallback for a flagged row (body of topk_fallback_kernel; NT threads).  Returns at once when row_ovf[m] == 0.
// EXCL: rows of excl[m] are left out (the masked search: search_plan.h, SearchShape.excl).
template <int ELT, int NT, bool EXCL = false>
__device__ inline void topk_fallback_body(int64_t m, int *row_ovf, const float *__restrict__ q, const void *__restrict__ dbv,
                                          int64_t n, int d, int k, float *D, int64_t *I, int64_t label_base,
                                          const uint2 *__restrict__ excl = nullptr) {
    constexpr int FB = 2048, RPP = NT / 2;        // buffer slots; rows per pass (NT / 4 row groups x 2)
    __shared__ unsigned long long buf[FB];
    __shared__ __attribute__((aligned(16))) float qs[1024];
    __shared__ int s_cnt;
    __shared__ unsigned long long s_T;
    if (row_ovf[m] == 0) return;
    // four lanes per row, the canonical summation order (canon_part / canon_sum): a row's fp32 score has the same bits
    // whether it comes out of a select or out of this fallback (round 6: with eight lanes per row a list overflow on one
    // path of a sharded search moved a score by one ulp against the single-shard run)
    const int tid = threadIdx.x, sub = tid & 3, grp = tid >> 2;
    for (int e = tid; e < d; e += NT) qs[e] = ELT == 4 ? q[m * d + e] : (float)(_Float16)q[m * d + e];
    if (tid == 0) { s_cnt = 0; s_T = ~0ull; }
    uint2 ex = make_uint2(0u, 0u);
    if constexpr (EXCL) ex = excl[m];
    __syncthreads();
    for (int64_t base = 0; base < n; base += RPP) {
        const unsigned long long T = s_T;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int64_t row = base + u * (NT / 4) + grp;
            float part = 0.f;
            if (row < n) {
                if (ELT == 4) part = canon_part(reinterpret_cast<const float *>(dbv) + row * d, qs, d, sub);
                else part = canon_part(reinterpret_cast<const _Float16 *>(dbv) + row * d, qs, d, sub);
            }
            part = canon_sum(part);
            if (sub == 0 && row < n && !(EXCL && excl_hit(ex, (unsigned)row))) {
                const unsigned long long key = pack_key(part, (unsigned)row);
                if (key < T) buf[atomicAdd(&s_cnt, 1)] = key;       // s_cnt <= FB - RPP before the pass
            }
        }
        __syncthreads();
        if (s_cnt > FB - RPP || base + RPP >= n) {                    // block-uniform
            const int c = s_cnt;
            for (int i = c + tid; i < FB; i += NT) buf[i] = ~0ull;
            __syncthreads();
            bitonic_sort_u64(buf, FB, tid, NT);
            if (tid == 0) {
                s_cnt = c < k ? c : k;
                s_T = c >= k ? buf[k - 1] : ~0ull;
            }
            __syncthreads();
        }
    }
    const int c = s_cnt;
    for (int i = tid; i < k; i += NT) {
        if (i < c) {
            D[m * k + i] = ord2f(~(unsigned)(buf[i] >> 32));
            I[m * k + i] = (int64_t)(unsigned)(buf[i] & 0xFFFFFFFFu) + label_base;
        } else {
            D[m * k + i] = -3.4028234663852886e38f;
            I[m * k + i] = -1;
        }
    }
    if (tid == 0) row_ovf[m] = 0;
}

// What the stages of one search_topk call are launched with (search_plan.h says which and how large).
struct StageArgs {
    const float *db; const void *dbh;    // fp32 rows / fp16 rows (either may be absent)
    float xnorm_max;
    int64_t n; int d; int64_t label_base;
    const float *q; int64_t nq; int k;
    float *D; int64_t *I;
    float *lb; int mtop;
    const int64_t *excl_lo, *excl_hi;    // [nq] label ranges of the masked search (nullptr: none)
    SearchWorkspace &ws;
    hipStream_t s;
    // the rows a re-scoring select reads: the fp32 rows where the fp16 ones were only a pre-filter
    const float *db32(const SearchStage &st) const { return st.rescore ? db : nullptr; }
};
// the ScanParams of a scan stage
inline ScanParams scan_params(const SearchStage &st, const StageArgs &a) {
    ScanParams p;
    p.q = st.elt == 2 ? reinterpret_cast<const float *>(a.ws.qh) : a.q;
    p.db = st.elt == 2 ? reinterpret_cast<const float *>(a.dbh) : a.db;
    p.nq = a.nq; p.d = a.d; p.row_stride = st.stride; p.nrows = st.nrows;
    p.thr = st.thr == THR_NONE ? nullptr : (st.thr == THR_ADJ ? a.ws.thr_adj : a.ws.thr);
    p.cnt = a.ws.cnt; p.keys = reinterpret_cast<unsigned long long *>(a.ws.cl);
    p.n_tiles_m = st.n_tiles_m; p.nsub = st.nsub;
    p.gmax = st.gmax ? reinterpret_cast<float *>(a.ws.cl) : nullptr;       // [nq][groups] floats; the keys come after tau is known
    if (st.excl) { p.excl = a.ws.excl; p.excl_tile = a.ws.excl_tile; }
    if (st.fold_prep) { p.q32 = a.q; p.xnorm_max = a.xnorm_max; p.qh_out = a.ws.qh; p.eps = a.ws.eps; p.row_ovf = a.ws.row_ovf; }
    return p;
}

// ---- search_f16.hip ------------------------------------------------------------------------
int launch_rows_to_half(const float *x, int64_t n, int d, void *xh, float *norm_max_dev, hipStream_t s);
// launches the stage if its kernel lives in search_f16.hip (the fp16 scans, query preparation, the re-scoring selects)
int launch_stage_f16(const SearchStage &st, const StageArgs &a);

}  // namespace pfann
