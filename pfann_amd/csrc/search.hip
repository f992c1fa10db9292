// Exact brute-force inner-product top-k for gfx950 (reference database.py:121
// `index.search(query, top_k)` with an IndexFlatIP, i.e. the k largest q.x per query row).
//
// Design (MI355X-first, not faiss' GPU design):
//   * scores are produced by an LDS-tiled fp32-MFMA GEMM tile  q[BM] x db[BN]  (K = d);
//     every db row is streamed from HBM once per pass (query panels come from L2);
//   * NO score matrix is ever written.  Each score is compared in the MFMA epilogue with a
//     per-query threshold tau_q and only survivors are appended (one 8-byte packed key per
//     survivor, one atomic) to a small per-query list;
//   * tau_q is a provable lower bound of the query's k-th best score, obtained from the
//     exact top-k of a strided 1/R, 1/R^2 .. sample of the shard scanned first (the k-th
//     best of a subset can only be <= the k-th best of the whole).  Each level emits
//     ~R*k survivors per query, so the lists stay tiny and the final bitonic select in
//     LDS is exact;
//   * a list overflow on the final level (pathological ties / duplicates) raises tau from
//     the captured survivors and rescans; it never degrades to an approximate answer.
#include <stdlib.h>
#include <algorithm>
#include <utility>
#include <vector>

#include "search_common.h"

namespace pfann {

// One workgroup owns one db tile (BN rows) and a run of QT consecutive query tiles, walked with a
// single software pipeline: tile (q, kt+1) -- or (q+1, 0) -- is prefetched while (q, kt) is on the
// matrix cores, so with K = d = 128 (4 K-tiles) the exposed first load and the pipeline drain are
// paid once per QT*4 K-tiles instead of once per 4.  The db tile is re-read from L1/L2 (64 KB).
// EXCL (the masked search, DESIGN.md "Self-match"): a score of a row inside its query row's range p.excl[m] becomes -inf
// before the filter, on the db tiles that meet the span of the query tile's ranges (p.excl_tile) only; the dense level
// appends like the thresholded ones (its counters start at 0), so an excluded row is absent from the list.
template <int BM, int BN, int WM, int WN, int QT, bool EXCL = false>
__global__ __launch_bounds__(256, 2) void scan_emit_kernel(ScanParams p) {
    constexpr int BK = 32, LDK = BK + 4;
    constexpr int WAVES_N = BN / WN;
    static_assert((BM / WM) * WAVES_N == 4, "4 waves per block");
    constexpr int TM = WM / 32, TN = WN / 32;
    static_assert(BM % 32 == 0 && BN % 32 == 0, "tiles are whole 32-row MFMA blocks");
    constexpr int AR = BM / 32, BR = BN / 32;
    __shared__ __attribute__((aligned(16))) float As[2 * BM * LDK];
    __shared__ __attribute__((aligned(16))) float Bs[2 * BN * LDK];
    __shared__ __attribute__((aligned(16))) float thr_s[QT * BM];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int L = xcd_remap(blockIdx.x, gridDim.x);
    const int n_mg = (p.n_tiles_m + QT - 1) / QT;                // query-tile groups
    const int nt = L / n_mg, mg = L - nt * n_mg;                 // groups fastest: db tile stays in L2
    const int mt0 = mg * QT;
    const int n_q = min(QT, p.n_tiles_m - mt0);                  // query tiles this block really has
    const int64_t n0 = (int64_t)nt * BN;
    const int col4 = tid & 7, rowq = tid >> 3;

    for (int i = tid; i < QT * BM; i += 256) {
        const int64_t m = (int64_t)mt0 * BM + i;
        thr_s[i] = (p.thr != nullptr && m < p.nq) ? p.thr[m] : -INFINITY;
        // masked scores are -inf: never at or above a threshold (fewer than k rows left: the sampled threshold is -inf)
        if (EXCL) thr_s[i] = fmaxf(thr_s[i], -3.4028234663852886e38f);
    }

    // bounds-checked buffer loads (OOB lanes read 0); windows start at this block's first rows
    const int64_t mq0 = (int64_t)mt0 * BM;
    const __amdgpu_buffer_rsrc_t srd_q = make_srd(p.q + mq0 * p.d, (unsigned long long)(p.nq - mq0) * p.d * 4ull);
    // one window per 32-row sub-tile: on a coarse sampling level of a large shard (row_stride up to 65536) the
    // rows of one 128-row tile span more than the 2 GB a buffer offset can address, 32 rows never do
    // (search_plan.h checks 31 * row_stride * d * 4 < 2 GB)
    __amdgpu_buffer_rsrc_t srd_db[BR];
    unsigned doff[BR];
#pragma unroll
    for (int j = 0; j < BR; ++j) {
        const int64_t nj = n0 + 32 * j;                       // first sampled row of the sub-tile
        const int64_t left = p.nrows - nj;                    // sampled rows from there on
        srd_db[j] = make_srd(p.db + (nj < p.nrows ? nj : 0) * p.row_stride * p.d,
                             left > 0 ? (unsigned long long)((left - 1) * p.row_stride + 1) * p.d * 4ull : 0ull);
        doff[j] = nj + rowq < p.nrows ? (unsigned)((unsigned long long)rowq * p.row_stride * p.d * 4ull) : BUF_OOB;
    }
    f32x4 ra[AR], rb[BR];
    // load cursor of the NEXT tile to fetch, all in 32-bit byte offsets inside the two windows
    const int q_rows_left = (int)((p.nq - mq0) < (int64_t)QT * BM ? (p.nq - mq0) : (int64_t)QT * BM);
    const unsigned tile_bytes = (unsigned)BM * (unsigned)p.d * 4u;
    unsigned aoff[AR];
#pragma unroll
    for (int i = 0; i < AR; ++i) aoff[i] = (unsigned)(rowq + 32 * i) * (unsigned)p.d * 4u;
    // lk0: first k of the cursor's K tile.  The cursor moves to the next query tile when the K TILE passes d -- for every
    // thread at once: a thread whose own k (lk0 + 4 col4) passes d sooner, in the last K tile of a d % 32 != 0, loads
    // zeros there and must not run ahead into the next query tile of the run (QT > 1)
    int lk0 = 0, lrow = rowq;                // lrow: row (inside the run) of this thread's first A row
    unsigned lbase = 0;                      // byte offset of the cursor's query tile
    auto load_tile = [&]() {
        const int lkap = lk0 + col4 * 4;
        const bool kok = lkap < p.d;
#pragma unroll
        for (int i = 0; i < AR; ++i)
            ra[i] = buf_load4(srd_q, (kok && lrow + 32 * i < q_rows_left) ? lbase + aoff[i] + (unsigned)lkap * 4u : BUF_OOB);
#pragma unroll
        for (int j = 0; j < BR; ++j)
            rb[j] = buf_load4(srd_db[j], (kok && doff[j] != BUF_OOB) ? doff[j] + (unsigned)lkap * 4u : BUF_OOB);
        lk0 += BK;
        const bool wrap = lk0 >= p.d;
        lk0 = wrap ? 0 : lk0;
        lrow += wrap ? BM : 0;
        lbase += wrap ? tile_bytes : 0u;
    };
    auto store_tile = [&](float *Ad, float *Bd) {
#pragma unroll
        for (int i = 0; i < AR; ++i)
            *reinterpret_cast<f32x4 *>(&Ad[(rowq + 32 * i) * LDK + col4 * 4]) = ra[i];
#pragma unroll
        for (int j = 0; j < BR; ++j)
            *reinterpret_cast<f32x4 *>(&Bd[(rowq + 32 * j) * LDK + col4 * 4]) = rb[j];
    };

    const int nk = (p.d + BK - 1) / BK;
    load_tile();
    store_tile(As, Bs);
    __syncthreads();
    const int l31 = lane & 31, lhalf = lane >> 5;
    int it = 0;                               // running K-tile counter: LDS buffer = it & 1
#pragma unroll 1
    for (int q = 0; q < n_q; ++q) {
        const int64_t m0 = mq0 + (int64_t)q * BM;
        f32x16 acc[TM][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
#pragma unroll 1
        for (int kt = 0; kt < nk; ++kt, ++it) {
            const float *Ac = As + (it & 1) * (BM * LDK), *Bc = Bs + (it & 1) * (BN * LDK);
            float *An = As + ((it + 1) & 1) * (BM * LDK), *Bn = Bs + ((it + 1) & 1) * (BN * LDK);
#pragma unroll
            for (int kk = 0; kk < BK / 8; ++kk) {
                f32x4 a4[TM], b4[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i)
                    a4[i] = *reinterpret_cast<const f32x4 *>(&Ac[(wm * WM + i * 32 + l31) * LDK + kk * 8 + lhalf * 4]);
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    b4[j] = *reinterpret_cast<const f32x4 *>(&Bc[(wn * WN + j * 32 + l31) * LDK + kk * 8 + lhalf * 4]);
                if (kk == 0) {
                    load_tile();
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (kk == BK / 8 - 1) store_tile(An, Bn);
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[i][s], b4[j][s], acc[i][j], 0, 0, 0);
            }
            __syncthreads();
        }
        // epilogue: threshold filter + append.  acc[i][j][r]: query row = (r&3)+8*(r>>2)+4*lhalf,
        // db row = lane&31 of the 32x32 tile.  A wave-level branch costs ~50 cycles and survivors
        // are rare (~1.6e-3 per score), so survival is tested per GROUP of 4 slots (one branch),
        // and only groups with a survivor fall into the per-slot append code.
        const float *thr_c = thr_s + q * BM;
        if constexpr (EXCL) {
            // block-uniform: this db tile meets the ranges of the query tile (in self-match: the tiles of one to three songs)
            if (excl_span_hit(p.excl_tile[m0 >> 7], n0 * p.row_stride, (n0 + BN - 1) * p.row_stride)) {
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int64_t m = m0 + wm * WM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhalf;
                        const uint2 ex = m < p.nq ? p.excl[m] : make_uint2(0u, 0u);
#pragma unroll
                        for (int j = 0; j < TN; ++j)
                            if (excl_hit(ex, (unsigned)((n0 + wn * WN + j * 32 + l31) * p.row_stride))) acc[i][j][r] = -INFINITY;
                    }
            }
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int64_t n = n0 + wn * WN + j * 32 + l31;
            const bool nok = n < p.nrows;
            const unsigned row = (unsigned)(n * p.row_stride);
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                if (!EXCL && p.thr == nullptr) {          // top sampling level: nrows <= CAP, no filter, no atomics
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int64_t m = m0 + wm * WM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhalf;
                        if (nok && m < p.nq) p.keys[m * CAP + n] = pack_key(acc[i][j][r], row);
                    }
                } else {
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        // rows (r&3)+8g+4*lhalf for r&3 = 0..3: four consecutive query rows
                        const int mlg = wm * WM + i * 32 + 8 * g + 4 * lhalf;
                        const f32x4 th = *reinterpret_cast<const f32x4 *>(thr_c + mlg);
                        bool sv[4];
                        bool any = false;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            sv[e] = nok && (m0 + mlg + e) < p.nq && acc[i][j][4 * g + e] >= th[e];
                            any |= sv[e];
                        }
                        if (__any(any)) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                if (sv[e]) {
                                    const int64_t m = m0 + mlg + e;
                                    const int pos = atomicAdd(&p.cnt[m], 1);
                                    if (pos < CAP) p.keys[m * CAP + pos] = pack_key(acc[i][j][4 * g + e], row);
                                }
                            }
                        }
                    }
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// ------------------------------------------------------------------------------------
// Small-batch scan (nq <= 32, d = 128 or 64): the HBM-bound regime (one 10 s query = 19 rows;
// intensity Q/2 flop/byte).  Streaming design:
//   * the query block lives in registers as MFMA A-fragments for the whole kernel;
//   * a persistent grid (2 workgroups per CU) walks the 32-row tiles round-robin -- at any moment the chip reads
//     one moving window of a few tens of MB (2048 far-apart streams measured 20 % slower: TLB reach) -- for as
//     many WHOLE rounds as there are; the rows left over (less than one round) are split row-granularly over
//     all waves, so no wave runs a whole extra tile while the others idle (5 % of a 1 M-row pass);
//   * tiles are read with fully contiguous 1 KB-per-instruction buffer loads (each byte once); the buffer window
//     is rebased per tile (scalar 64-bit math), so shards beyond 2 GB keep this path, and rows past the end of
//     a piece read as zeros through the window's own range check (no per-lane predicates);
//   * the tile is transposed to the MFMA B-fragment layout through a WAVE-PRIVATE padded LDS tile
//     (pitch RB/4+4 dwords: conflict-free ds_write_b128 / ds_read_b128), so there are no workgroup
//     barriers at all; the next tile is already in flight in registers while the current one is
//     on the matrix cores.
// ELT = 4: fp32 rows, v_mfma_f32_32x32x2_f32 (exact fp32; K order: step s of half h uses
//          k = 8*(s>>2) + 4*h + (s&3), same map for both operands);
// ELT = 2: fp16 rows and fp16 query rows, v_mfma_f32_32x32x16_f16 with fp32 accumulation (fp16-only storage).
// Both read 16-byte pieces j*32 + 16*h of a row, so the staging code is shared.
// MODE 0: emit rows with score >= thr[m] into the row's 32 sub-lists.  Survivors (about one per tile) are first
//         collected in a per-workgroup LDS list (wave ballot + one LDS atomic per hit group): a returning GLOBAL
//         atomic per survivor stalled the wave for an L2 round trip per tile and cost 12 us of a 109 us pass
//         (measured by ablation).  When the workgroup has streamed its share it reserves space in the global
//         sub-lists with one atomic per query row and copies its entries out;
// MODE 1: no output but the MAXIMUM score of the wave's range per query row, gmax[m][wave]: the k-th best of
//         these G = 4*gridDim.x group maxima is the score of a real row, hence a lower bound of the k-th best
//         overall, and a sharp one (top rows rarely share a group) -- one sampled pass + a 2048-value select
//         replace the two sampled scan+sort levels of the generic ladder;
// MODE 2: dense (nrows <= CAP): every score is written at slot = row.
// ------------------------------------------------------------------------------------
// EXCL (the masked search, DESIGN.md "Self-match"): on the pieces that meet the span of the ranges (p.excl_tile[0]: one
// query tile) a score of a row inside its query row's range p.excl[m] becomes -inf before it meets the group maximum
// (MODE 1) or the threshold (MODE 0); MODE 2 appends the rows that remain (counters start at 0) instead of writing slot = row.
template <int D, int ELT, int MODE, bool EXCL = false>
__global__ __launch_bounds__(256, 2) void scan_small_kernel(ScanParams p) {
    constexpr int RB = D * ELT;               // bytes per row
    constexpr int NP = RB / 32;               // 32-byte K pieces per row
    constexpr int LD = RB / 4 + 4;            // LDS row pitch (dwords)
    constexpr int RPI = 1024 / RB;            // db rows covered by one 1 KB wave instruction
    constexpr int NI = 32 / RPI;              // load instructions per 32-row tile
    constexpr int CPR = RB / 16;              // 16-byte chunks per row
    typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
    constexpr int NSUB = 32, LCAP = 1024;     // sub-lists per query row; slots of the workgroup's LDS survivor list
    __shared__ __attribute__((aligned(16))) float tile_s[4 * 32 * LD];
    __shared__ __attribute__((aligned(16))) float thr_s[32];
    __shared__ unsigned long long l_key[MODE == 0 ? LCAP : 1];
    __shared__ unsigned short l_m[MODE == 0 ? LCAP : 2];
    __shared__ int l_n, l_hist[32], l_base[32];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, lhalf = lane >> 5;
    const int W = (int)gridDim.x * 4, gw = (int)blockIdx.x * 4 + wave;
    // pieces of this wave: tiles gw, gw + W, ... of the whole rounds, then its share of the left-over rows
    const int64_t rounds = (p.nrows / 32) / W;
    const int64_t tail0 = rounds * W * 32, tail = p.nrows - tail0;
    const int64_t tl_lo = tail0 + (int64_t)gw * tail / W, tl_hi = tail0 + (int64_t)(gw + 1) * tail / W;
    const int64_t n_tl = (tl_hi - tl_lo + 31) / 32;           // tail tiles of this wave (usually 0 or 1)
    const int64_t n_pieces = rounds + n_tl;
    // piece i -> [first row, end row)
    auto piece_lo = [&](int64_t i) { return i < rounds ? ((int64_t)gw + i * W) * 32 : tl_lo + (i - rounds) * 32; };
    auto piece_hi = [&](int64_t i) { return i < rounds ? ((int64_t)gw + i * W) * 32 + 32 : tl_hi; };
    float *ts = tile_s + wave * 32 * LD;
    const char *qb = reinterpret_cast<const char *>(p.q), *dbb = reinterpret_cast<const char *>(p.db);
    const unsigned srow = (unsigned)p.row_stride * RB;      // bytes between two sampled rows
    const int lrow = lane / CPR, lcol = lane % CPR;         // lane -> (row inside the instruction's RPI rows, chunk)
    unsigned loff[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) loff[j] = (unsigned)(j * RPI + lrow) * srow + (unsigned)lcol * 16u;

    f32x4 st[NI];                              // next tile, in flight
    auto load_tile = [&](int64_t i) {
        const int64_t r0 = i < n_pieces ? piece_lo(i) : 0;
        const int64_t left = i < n_pieces ? piece_hi(i) - r0 : 0;   // wave-uniform: rows of the piece from r0 on
        const int nv = left >= 32 ? 32 : (left > 0 ? (int)left : 0);
        const __amdgpu_buffer_rsrc_t srd = make_srd(dbb + (nv > 0 ? r0 : 0) * (int64_t)srow,
                                                    nv > 0 ? (unsigned long long)(nv - 1) * srow + RB : 0ull);
        // streamed once: non-temporal (no L2 / Infinity-Cache allocation): 512 MB in 78 us instead of 90 us in
        // a bare read loop of this shape (tools/ubench/membw.hip)
#pragma unroll
        for (int j = 0; j < NI; ++j)
            st[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srd, (int)loff[j], 0, /*aux: nt*/ 2));
    };
    float mx[16];
    if (MODE == 1) {
#pragma unroll
        for (int r = 0; r < 16; ++r) mx[r] = -INFINITY;
    }
    load_tile(0);                              // the stream starts before anything else is fetched
    if (MODE == 0) {
        // (EXCL: masked scores are -inf and never reach a threshold, also when fewer than k groups were left and it is -inf)
        if (tid < 32) { thr_s[tid] = tid < p.nq ? (EXCL ? fmaxf(p.thr[tid], -3.4028234663852886e38f) : p.thr[tid]) : INFINITY; l_hist[tid] = 0; }
        if (tid == 0) l_n = 0;
        __syncthreads();
    }
    uint2 ex_span = make_uint2(0xFFFFFFFFu, 0u);
    if constexpr (EXCL) ex_span = p.excl_tile[0];
    f32x4 qa[NP];
    if (MODE == 1 && ELT == 2 && p.q32 != nullptr) {
        // query preparation folded in (q_prep_kernel's job, one launch less): fp16 image of the fp32 query rows -- this lane's
        // fragment is elements 16 j + 8 lhalf .. + 7 of row l31 --, the row's error bound eps and the out-of-range flag
        float ss = 0.f;
        f32x4 lo[NP], hi[NP];
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const float *src = p.q32 + (int64_t)l31 * D + j * 16 + lhalf * 8;
            lo[j] = l31 < p.nq ? *reinterpret_cast<const f32x4 *>(src) : f32x4{0.f, 0.f, 0.f, 0.f};
            hi[j] = l31 < p.nq ? *reinterpret_cast<const f32x4 *>(src + 4) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int e = 0; e < 4; ++e) { ss = fmaf(lo[j][e], lo[j][e], ss); ss = fmaf(hi[j][e], hi[j][e], ss); }
        }
        ss += __shfl_xor(ss, 32, 64);
        const bool bad = !(ss < 3.6e9f);                   // ||q|| >= 6e4 or NaN: outside fp16's range
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            f16x8 h8;
#pragma unroll
            for (int e = 0; e < 4; ++e) { h8[e] = bad ? (_Float16)0.f : (_Float16)lo[j][e]; h8[4 + e] = bad ? (_Float16)0.f : (_Float16)hi[j][e]; }
            qa[j] = __builtin_bit_cast(f32x4, h8);
            if (gw == 0 && l31 < p.nq)
                *reinterpret_cast<f32x4 *>(reinterpret_cast<char *>(p.qh_out) + (int64_t)l31 * RB + j * 32 + lhalf * 16) = qa[j];
        }
        if (gw == 0 && lhalf == 0 && l31 < p.nq) {
            const float nq2 = sqrtf(ss);
            p.eps[l31] = 1.05e-3f * nq2 * p.xnorm_max + 3.1e-8f * sqrtf((float)D) * (nq2 + p.xnorm_max);
            if (bad) p.row_ovf[l31] = 1;                   // recomputed exactly by the fallback
        }
    } else {
#pragma unroll
        for (int j = 0; j < NP; ++j)
            qa[j] = l31 < p.nq ? *reinterpret_cast<const f32x4 *>(qb + (int64_t)l31 * RB + j * 32 + lhalf * 16)
                               : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int64_t pi = 0; pi < n_pieces; ++pi) {
        const int64_t r0 = piece_lo(pi), r_hi = piece_hi(pi);
        // registers -> wave-private LDS tile (the previous tile's fragment reads are complete: their
        // results fed MFMAs already issued), then put the next tile in flight
#pragma unroll
        for (int j = 0; j < NI; ++j)
            *reinterpret_cast<f32x4 *>(&ts[(j * RPI + lrow) * LD + lcol * 4]) = st[j];
        load_tile(pi + 1);                     // past the last piece: empty window, reads zeros, no traffic
        __builtin_amdgcn_sched_barrier(0);
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const f32x4 xb = *reinterpret_cast<const f32x4 *>(&ts[l31 * LD + 8 * j + 4 * lhalf]);
            if (ELT == 4) {
#pragma unroll
                for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[j][e], xb[e], acc, 0, 0, 0);
            } else {
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, qa[j]), __builtin_bit_cast(f16x8, xb),
                                                             acc, 0, 0, 0);
            }
        }
        // acc[r]: query row (r&3)+8*(r>>2)+4*lhalf, sampled row r0 + l31
        const int64_t n = r0 + l31;
        const bool nok = n < r_hi;
        const unsigned row = (unsigned)(n * p.row_stride);
        unsigned masked = 0u;                  // EXCL: bit r = acc[r] is an excluded row's score
        if constexpr (EXCL) {
            if (excl_span_hit(ex_span, r0 * p.row_stride, (r_hi - 1) * p.row_stride)) {        // wave-uniform, rare
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = (r & 3) + 8 * (r >> 2) + 4 * lhalf;
                    const uint2 ex = m < p.nq ? p.excl[m] : make_uint2(0u, 0u);
                    if (excl_hit(ex, row)) { acc[r] = -INFINITY; masked |= 1u << r; }
                    __builtin_amdgcn_sched_barrier(0);     // one range in flight at a time: the branch is rare, registers are not
                }
            }
        }
        if (MODE == 2) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = (r & 3) + 8 * (r >> 2) + 4 * lhalf;
                if (EXCL) {
                    if (nok && m < p.nq && !((masked >> r) & 1u)) p.keys[(int64_t)m * CAP + atomicAdd(&p.cnt[m], 1)] = pack_key(acc[r], row);
                } else if (nok && m < p.nq) p.keys[(int64_t)m * CAP + n] = pack_key(acc[r], row);
            }
        } else if (MODE == 1) {
#pragma unroll
            for (int r = 0; r < 16; ++r) mx[r] = fmaxf(mx[r], nok ? acc[r] : -INFINITY);
        } else {
            bool any = false;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 th = *reinterpret_cast<const f32x4 *>(thr_s + 8 * g + 4 * lhalf);
#pragma unroll
                for (int e = 0; e < 4; ++e) any |= acc[4 * g + e] >= th[e];
            }
            if (__any(any && nok)) {
                const int sub = (int)blockIdx.x & (NSUB - 1);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = (r & 3) + 8 * (r >> 2) + 4 * lhalf;
                    const bool sv = nok && acc[r] >= thr_s[m];
                    const unsigned long long mask = __ballot(sv);
                    if (mask != 0ull) {                                     // wave-uniform
                        int base = 0;
                        if (lane == (int)__builtin_ctzll(mask)) base = atomicAdd(&l_n, (int)__builtin_popcountll(mask));
                        base = __builtin_amdgcn_readlane(base, (int)__builtin_ctzll(mask));
                        const int pos = base + (int)__builtin_popcountll(mask & ((1ull << lane) - 1ull));
                        if (sv) {
                            const unsigned long long key = pack_key(acc[r], row);
                            if (pos < LCAP) {
                                l_key[pos] = key;
                                l_m[pos] = (unsigned short)m;
                            } else {                                        // LDS list full (pathological): straight out
                                const int gp = atomicAdd(&p.cnt[m * NSUB + sub], 1);
                                if (gp < CAP / NSUB) p.keys[(int64_t)m * CAP + sub * (CAP / NSUB) + gp] = key;
                            }
                        }
                    }
                }
            }
        }
    }
    if (MODE == 0) {
        // the workgroup's survivors -> the global sub-lists: one reservation per query row
        __syncthreads();
        const int sub = (int)blockIdx.x & (NSUB - 1);
        const int n_l = l_n < LCAP ? l_n : LCAP;
        for (int i = tid; i < n_l; i += 256) atomicAdd(&l_hist[l_m[i]], 1);
        __syncthreads();
        if (tid < 32) {
            const int c = l_hist[tid];
            l_base[tid] = c > 0 ? atomicAdd(&p.cnt[tid * NSUB + sub], c) : 0;
            l_hist[tid] = 0;                                               // reused as the per-row cursor
        }
        __syncthreads();
        for (int i = tid; i < n_l; i += 256) {
            const int m = l_m[i];
            const int gp = l_base[m] + atomicAdd(&l_hist[m], 1);
            if (gp < CAP / NSUB) p.keys[(int64_t)m * CAP + sub * (CAP / NSUB) + gp] = l_key[i];
        }
    }
    if (MODE == 1) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v = mx[r];
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));     // the half's 32 lanes
            const int m = (r & 3) + 8 * (r >> 2) + 4 * lhalf;
            if (l31 == 0 && m < p.nq) p.gmax[(int64_t)m * W + gw] = v;
        }
    }
}

// k-th largest of the G group maxima of every query row (MSB radix select, 4 x 8 bits, LDS histogram) ->
// thr[m]; also zeroes the row's survivor counters for the pass that follows.
// eps != nullptr (fp16 pre-filter): the maxima are approximate scores; thr_adj[m] = tau - margin * eps[m] (floored at
// -1000 eps: finite, below every possible score), margin = 2 with exact re-scoring downstream, 0 when the s16 scores are final.
__global__ __launch_bounds__(256) void group_max_select_kernel(const float *__restrict__ gmax, int G, int k,
                                                               float *__restrict__ thr, int *__restrict__ cnt, int ncnt,
                                                               const float *__restrict__ eps, float *__restrict__ thr_adj,
                                                               float margin, float *__restrict__ topm, int mtop, float margin_out,
                                                               int *zero_me) {
    constexpr int GMAX = 4096;
    __shared__ unsigned sv[GMAX];
    __shared__ int s_n;
    const int64_t m = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (zero_me != nullptr && m == 0 && tid == 0) *zero_me = 0;      // the select's overflow counter (one memset less)
    for (int i = tid; i < ncnt; i += 256) cnt[m * ncnt + i] = 0;
    for (int i = tid; i < G; i += 256) sv[i] = ~f2ord(gmax[m * G + i]);          // ascending = descending score
    __syncthreads();
    // keys of the kA-th and the kB-th smallest entry of sv (= kA-th / kB-th best score) in ONE sweep: MSB radix select,
    // 4 x 8 bits, two histograms per pass (wave 0 resolves rank A, wave 1 rank B).  kB <= 0: only A.  Phase 1 of a
    // sharded search needs both the row's k-th best group maximum and its mtop-th: two separate selects cost the kernel
    // twice (0.85 vs 0.47 ms per 77,824 rows).
    __shared__ int hist2[2][256];
    __shared__ int s_bin2[2], s_kk2[2];
    auto kth2 = [&](int kA, int kB, unsigned &outA, unsigned &outB) {
        unsigned pA = 0, pB = 0;
        const bool two = kB > 0;
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            hist2[0][tid] = 0;
            hist2[1][tid] = 0;
            __syncthreads();
            for (int i = tid; i < G; i += 256) {
                const unsigned hi = sv[i];
                if (pass == 0 || (hi >> (shift + 8)) == (pA >> (shift + 8))) atomicAdd(&hist2[0][(hi >> shift) & 255], 1);
                if (two && (pass == 0 || (hi >> (shift + 8)) == (pB >> (shift + 8)))) atomicAdd(&hist2[1][(hi >> shift) & 255], 1);
            }
            __syncthreads();
            if (wave < (two ? 2 : 1)) {
                const int *h = hist2[wave];
                const int kk = wave == 0 ? kA : kB;
                const int c0 = h[4 * lane], c1 = h[4 * lane + 1], c2 = h[4 * lane + 2], c3 = h[4 * lane + 3];
                const int sum4 = c0 + c1 + c2 + c3;
                int incl = sum4;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int v = __shfl_up(incl, o, 64);
                    if (lane >= o) incl += v;
                }
                const int excl = incl - sum4;
                if (excl < kk && kk <= incl) {          // exactly one lane
                    int rem = kk - excl, bin = 4 * lane;
                    if (rem > c0) { rem -= c0; ++bin; if (rem > c1) { rem -= c1; ++bin; if (rem > c2) { rem -= c2; ++bin; } } }
                    s_bin2[wave] = bin;
                    s_kk2[wave] = rem;
                }
            }
            __syncthreads();
            pA |= (unsigned)s_bin2[0] << shift;
            kA = s_kk2[0];
            if (two) { pB |= (unsigned)s_bin2[1] << shift; kB = s_kk2[1]; }
        }
        outA = pA;
        outB = pB;
    };
    // topm[m][0..mtop): the mtop best group maxima minus margin_out * eps -- each the score of a DIFFERENT real row of
    // this shard, lowered to a bound of its true score -- for the cross-shard bound (search_topk phase 1); -inf padded
    const int mm = topm != nullptr ? (mtop < G ? mtop : G) : 0;
    unsigned prefix = 0, tm = 0;
    if (G >= k) kth2(k, mm, prefix, tm);
    else if (mm > 0) kth2(mm, 0, tm, prefix);
    if (topm != nullptr) {
        const float e = eps != nullptr ? margin_out * eps[m] : 0.f;
        for (int i = mm + tid; i < mtop; i += 256) topm[m * mtop + i] = -INFINITY;
        if (mm > 0) {
            if (tid == 0) s_n = 0;
            __syncthreads();
            for (int i = tid; i < G; i += 256)
                if (sv[i] < tm) topm[m * mtop + atomicAdd(&s_n, 1)] = ord2f(~sv[i]) - e;       // strictly better: < mm of them
            __syncthreads();
            for (int i = s_n + tid; i < mm; i += 256) topm[m * mtop + i] = ord2f(~tm) - e;     // the mm-th best and its ties
            __syncthreads();
        }
    }
    if (G < k) {
        if (tid == 0) { thr[m] = -INFINITY; if (eps != nullptr) thr_adj[m] = -1000.f * eps[m]; }
        return;
    }
    if (tid == 0) {
        const float t = ord2f(~prefix);
        thr[m] = t;
        if (eps != nullptr) thr_adj[m] = fmaxf(t - margin * eps[m], -1000.f * eps[m]);
    }
}

// The same selection with ONE WAVEFRONT per query row (round 5), for G <= 64 * VPL group maxima: the workgroup form above
// spends its time in barriers -- four radix passes of three __syncthreads each for ~500-800 values -- and costs a rank of
// an 8-way sharded search 0.47 of its 4.8 ms of scan kernels per 77,824-row step (the work per query row does not shrink
// with the shard: tools/ubench/sharded_scan_model.py).  Here a lane keeps VPL values in registers and the k-th (and
// mtop-th) largest comes from an MSB-first bisection on the orderable bit patterns, one ballot + popcount per value and
// bit, no LDS, no barrier (the scheme of bound_reduce_kernel).  Same outputs: thr / thr_adj, the zeroed counters, topm.
template <int VPL>
__global__ __launch_bounds__(256) void group_max_select_wave_kernel(const float *__restrict__ gmax, int G, int k,
                                                                    float *__restrict__ thr, int *__restrict__ cnt, int ncnt,
                                                                    const float *__restrict__ eps, float *__restrict__ thr_adj,
                                                                    float margin, float *__restrict__ topm, int mtop,
                                                                    float margin_out, int *zero_me, int64_t nq) {
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= nq) return;
    if (zero_me != nullptr && m == 0 && lane == 0) *zero_me = 0;
    for (int i = lane; i < ncnt; i += 64) cnt[m * ncnt + i] = 0;
    unsigned key[VPL];
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int i = lane + 64 * j;
        key[j] = i < G ? f2ord(gmax[m * G + i]) : 0u;           // 0: below every value (f2ord(x) > 0 for every non-NaN x)
    }
    // the bits every value shares need no bisection: scores of one query row lie in a narrow band (sign, exponent and the
    // first mantissa bits agree)
    unsigned diff = 0u;
    const unsigned key0 = __shfl(key[0], 0, 64);
#pragma unroll
    for (int j = 0; j < VPL; ++j) diff |= (lane + 64 * j < G) ? (key[j] ^ key0) : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) diff |= __shfl_xor(diff, o, 64);
    const int top_bit = diff ? 31 - __clz(diff) : -1;            // highest bit in which two values differ
    const unsigned common = top_bit >= 31 ? 0u : (top_bit < 0 ? key0 : (key0 & ~((2u << top_bit) - 1u)));
    // key of the kk-th largest of the G values, 1 <= kk <= G; stop_bit > 0 leaves the lowest bits zero: a value BELOW the
    // kk-th largest by less than 2^stop_bit ulps -- fine for a threshold (any lower value is a valid bound), not for topm
    auto kth_largest = [&](int kk, int stop_bit) {
        unsigned prefix = common;
        for (int bit = top_bit; bit >= stop_bit; --bit) {
            const unsigned cand = prefix | (1u << bit);
            int c = 0;
#pragma unroll
            for (int j = 0; j < VPL; ++j) c += __popcll(__ballot(key[j] >= cand));
            if (c >= kk) prefix = cand;
        }
        return prefix;
    };
    const int mm = topm != nullptr ? (mtop < G ? mtop : G) : 0;
    if (topm != nullptr) {
        const float e = eps != nullptr ? margin_out * eps[m] : 0.f;
        for (int i = mm + lane; i < mtop; i += 64) topm[m * mtop + i] = -INFINITY;
        if (mm > 0) {
            const unsigned tm = kth_largest(mm, 0);
            int base = 0;                                        // strictly better than the mm-th best: fewer than mm of them
#pragma unroll
            for (int j = 0; j < VPL; ++j) {
                const bool take = key[j] > tm;
                const unsigned long long mask = __ballot(take);
                if (take) topm[m * mtop + base + __popcll(mask & ((1ull << lane) - 1ull))] = ord2f(key[j]) - e;
                base += __popcll(mask);
            }
            for (int i = base + lane; i < mm; i += 64) topm[m * mtop + i] = ord2f(tm) - e;      // the mm-th best and its ties
        }
    }
    if (G < k) {
        if (lane == 0) { thr[m] = -INFINITY; if (eps != nullptr) thr_adj[m] = -1000.f * eps[m]; }
        return;
    }
    // the threshold: 16 bits below the first differing one are plenty, and never more than the last 8 bits are dropped
    // (2^-16 of a float's value: the survivor count is steep in the threshold; a sign or exponent difference among the
    // maxima must not eat the precision)
    const unsigned pk = kth_largest(k, top_bit > 16 ? (top_bit - 16 < 8 ? top_bit - 16 : 8) : 0);
    if (lane == 0) {
        const float t = ord2f(pk);
        thr[m] = t;
        if (eps != nullptr) thr_adj[m] = fmaxf(t - margin * eps[m], -1000.f * eps[m]);
    }
}

// ------------------------------------------------------------------------------------
// Exact fallback for rows whose survivor lists overflowed (row_ovf[m] != 0): thousands of rows tying at the
// k-th score, or hundreds of near-duplicates landing in one sub-list.  ONE workgroup per flagged row streams the
// whole shard and keeps a running top-k (LDS buffer of FB keys; when it fills, sort, keep the best k, raise the
// cut to the k-th key).  Keys order by (score desc, row asc), so ties cannot stall it.  Slow (one workgroup reads
// N*d bytes) but it only ever runs for pathological rows, it is exact, and it keeps the host out of the loop:
// pfann_search_topk never synchronises, never retries and cannot fail with "lists keep overflowing".
// Unflagged rows cost one 4-byte read.  ELT = 4: fp32 rows; ELT = 2: fp16 rows, query rounded to fp16.
// ------------------------------------------------------------------------------------
template <int ELT, bool EXCL = false>
__global__ __launch_bounds__(256) void topk_fallback_kernel(int *__restrict__ row_ovf, const float *__restrict__ q,
                                                            const void *__restrict__ dbv, int64_t n, int d, int k,
                                                            float *__restrict__ D, int64_t *__restrict__ I,
                                                            int64_t label_base, const uint2 *__restrict__ excl) {
    topk_fallback_body<ELT, 256, EXCL>(blockIdx.x, row_ovf, q, dbv, n, d, k, D, I, label_base, excl);
}

// The masked search's ranges, once per call: label ranges [lo[m], hi[m]) -> rows of this shard (clipped; lo >= hi: nothing;
// nullptr: nothing), and per 128-row query tile the span of the union of its ranges -- what the masked scans test a db tile
// against before they look at single rows.  One workgroup of 128 threads per query tile.
__global__ __launch_bounds__(128) void excl_prep_kernel(const int64_t *__restrict__ lo, const int64_t *__restrict__ hi, int64_t nq,
                                                        int64_t n, int64_t label_base, uint2 *__restrict__ excl,
                                                        uint2 *__restrict__ excl_tile) {
    __shared__ unsigned s_lo[2], s_hi[2];
    const int tid = threadIdx.x;
    const int64_t m = (int64_t)blockIdx.x * 128 + tid;
    unsigned a = 0u, b = 0u;
    if (m < nq && lo != nullptr && hi != nullptr) {
        const int64_t l = lo[m] <= label_base ? 0 : (lo[m] - label_base < n ? lo[m] - label_base : n);
        const int64_t h = hi[m] <= label_base ? 0 : (hi[m] - label_base < n ? hi[m] - label_base : n);
        if (l < h) { a = (unsigned)l; b = (unsigned)h; }             // (n < 2^32: search_plan.h)
    }
    if (m < nq) excl[m] = make_uint2(a, b);
    unsigned ulo = a < b ? a : 0xFFFFFFFFu, uhi = b;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ulo = min(ulo, (unsigned)__shfl_xor((int)ulo, o, 64));
        uhi = max(uhi, (unsigned)__shfl_xor((int)uhi, o, 64));
    }
    if ((tid & 63) == 0) { s_lo[tid >> 6] = ulo; s_hi[tid >> 6] = uhi; }
    __syncthreads();
    if (tid == 0) excl_tile[blockIdx.x] = make_uint2(min(s_lo[0], s_lo[1]), max(s_hi[0], s_hi[1]));
}

// ------------------------------------------------------------------------------------
// Per-query exact select: bitonic sort of the (<= CAP) packed survivors in LDS.
//   mode 0: write thr[m] = k-th best score (or -inf when fewer than k survivors)
//   mode 1: write D[m][k], I[m][k] (+label_base); pad with -FLT_MAX / -1
// row_ovf[m] is set when a final-level list of row m overflowed.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void select_kernel(const unsigned long long *__restrict__ keys,
                                                      const int *__restrict__ cnt, int k, int mode,
                                                      float *__restrict__ thr, float *__restrict__ D,
                                                      int64_t *__restrict__ I, int64_t label_base,
                                                      int *row_ovf, int nsub) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long skeys[];
    __shared__ int s_off[130];
    const int64_t m = blockIdx.x;
    const int tid = threadIdx.x;
    const int subcap = CAP / nsub;
    bool over = false;
    if (tid == 0) {
        int run = 0;
        for (int g = 0; g < nsub; ++g) {
            int c = cnt[m * nsub + g];
            if (c > subcap) { c = subcap; over = true; }
            s_off[g] = run;
            run += c;
        }
        s_off[nsub] = run;
        s_off[129] = over ? 1 : 0;
        if (over && mode == 1) row_ovf[m] = 1;      // topk_fallback_kernel recomputes this row
    }
    __syncthreads();
    const int n = s_off[nsub];
    over = s_off[129] != 0;
    int P = 1;
    while (P < n) P <<= 1;
    for (int g = 0; g < nsub; ++g) {
        const int o = s_off[g], c = s_off[g + 1] - o;
        for (int i = tid; i < c; i += 1024) skeys[o + i] = keys[m * CAP + g * subcap + i];
    }
    for (int i = n + tid; i < P; i += 1024) skeys[i] = ~0ull;
    __syncthreads();
    bitonic_sort_u64(skeys, P, tid, 1024);
    if (mode == 0) {
        if (tid == 0) thr[m] = n >= k ? ord2f(~(unsigned)(skeys[k - 1] >> 32)) : -INFINITY;
    } else {
        for (int i = tid; i < k; i += 1024) {
            if (i < n) {
                const unsigned long long key = skeys[i];
                D[m * k + i] = ord2f(~(unsigned)(key >> 32));
                I[m * k + i] = (int64_t)(unsigned)(key & 0xFFFFFFFFu) + label_base;
            } else {
                D[m * k + i] = -3.4028234663852886e38f;
                I[m * k + i] = -1;
            }
        }
    }
}


__global__ void fill_int_kernel(int *p, int v, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per device: remember (kernel, device) pairs already done
int ensure_dyn_lds(const void *func, int bytes) {
    static std::vector<std::pair<const void *, int>> done;       // callers hold the API's single-thread contract
    int dev = 0;
    PF_HIP(hipGetDevice(&dev));
    for (auto &e : done) if (e.first == func && e.second == dev) return 0;
    PF_HIP(hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    done.emplace_back(func, dev);
    return 0;
}

static int ensure_ws(SearchWorkspace &ws, int64_t nq) {
    if (ws.cap_q >= nq) return 0;
    if (ws.thr) { (void)hipFree(ws.thr); (void)hipFree(ws.cnt); (void)hipFree(ws.cl); (void)hipFree(ws.row_ovf); (void)hipFree(ws.left); }
    if (!ws.overflow) PF_HIP(hipMalloc(&ws.overflow, 4 * sizeof(int)));    // [1] rows left to the big select kernel
    const int64_t cap = nq < 64 ? 64 : nq;
    if (ws.thr_adj) { (void)hipFree(ws.thr_adj); (void)hipFree(ws.eps); }
    PF_HIP(hipMalloc(&ws.thr_adj, sizeof(float) * cap));
    PF_HIP(hipMalloc(&ws.eps, sizeof(float) * cap));
    PF_HIP(hipMalloc(&ws.thr, sizeof(float) * cap));
    PF_HIP(hipMalloc(&ws.cnt, sizeof(int) * cap * 256));     // up to 256 sub-lists per row
    PF_HIP(hipMalloc(&ws.cl, sizeof(unsigned long long) * cap * CAP));
    PF_HIP(hipMalloc(&ws.left, sizeof(int) * cap));
    PF_HIP(hipMalloc(&ws.row_ovf, sizeof(int) * cap));
    PF_HIP(hipMemset(ws.row_ovf, 0, sizeof(int) * cap));     // kept zero by topk_fallback_kernel afterwards
    ws.cap_q = cap;
    return 0;
}

__global__ void fill_empty_kernel(float *D, int64_t *I, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) { D[i] = -3.4028234663852886e38f; I[i] = -1; }
}

// phase 1 on a path without a sampled threshold: no information
__global__ void bound_none_kernel(float *lb, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) lb[i] = -INFINITY;
}
// phase 2: rows of this shard whose true score reaches the global bound have s16 >= lb - eps
__global__ void bound_in_kernel(float *__restrict__ thr_adj, const float *__restrict__ eps, float margin, const float *__restrict__ lb,
                                int64_t nq) {
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m < nq) thr_adj[m] = fmaxf(thr_adj[m], lb[m] - margin * eps[m]);
}

// One stage of the plan: the kernel it names with the arguments the stage and the call give it.
static int launch_stage(const SearchStage &st, const StageArgs &a) {
    SearchWorkspace &ws = a.ws;
    hipStream_t s = a.s;
    const dim3 grid(st.grid), block(st.block);
    const float *gm = reinterpret_cast<const float *>(ws.cl), *ep = st.with_eps ? ws.eps : nullptr;
    float *topm = st.topm ? a.lb : nullptr;
    const int mtop = st.topm ? a.mtop : 0;
    int *zero_me = st.zero_me ? ws.overflow + 1 : nullptr;       // the select's overflow counter (one memset less)
    switch (st.kernel) {
#define X(id, ...) case K_##id: PF_LAUNCH((__VA_ARGS__), grid, block, st.lds, s, scan_params(st, a)); break;
    PF_SCAN_KERNELS(X) PF_SCAN_EXCL_KERNELS(X)
#undef X
    case K_EXCL_PREP:
        PF_LAUNCH(excl_prep_kernel, grid, block, 0, s, a.excl_lo, a.excl_hi, a.nq, a.n, a.label_base, ws.excl, ws.excl_tile);
        break;
    case K_FILL_EMPTY: PF_LAUNCH(fill_empty_kernel, grid, block, 0, s, a.D, a.I, a.nq * a.k); break;
    case K_BOUND_NONE: PF_LAUNCH(bound_none_kernel, grid, block, 0, s, a.lb, a.nq * a.mtop); break;
    case K_BOUND_IN: PF_LAUNCH(bound_in_kernel, grid, block, 0, s, ws.thr_adj, ws.eps, st.margin, a.lb, a.nq); break;
    case K_FILL_INT: PF_LAUNCH(fill_int_kernel, grid, block, 0, s, ws.cnt, st.fill, a.nq); break;
    case K_GROUP_SELECT:
        PF_LAUNCH(group_max_select_kernel, grid, block, 0, s, gm, st.G, a.k, ws.thr, ws.cnt, st.ncnt, ep, ws.thr_adj, st.margin, topm, mtop,
                  st.margin_out, zero_me);
        break;
    case K_GROUP_SELECT_WAVE_8:
        PF_LAUNCH(group_max_select_wave_kernel<8>, grid, block, 0, s, gm, st.G, a.k, ws.thr, ws.cnt, st.ncnt, ep, ws.thr_adj, st.margin, topm,
                  mtop, st.margin_out, zero_me, a.nq);
        break;
    case K_GROUP_SELECT_WAVE_16:
        PF_LAUNCH(group_max_select_wave_kernel<16>, grid, block, 0, s, gm, st.G, a.k, ws.thr, ws.cnt, st.ncnt, ep, ws.thr_adj, st.margin, topm,
                  mtop, st.margin_out, zero_me, a.nq);
        break;
    case K_SELECT:
        if (ensure_dyn_lds((const void *)select_kernel, CAP * 8)) return -1;
        PF_LAUNCH(select_kernel, grid, block, st.lds, s, reinterpret_cast<const unsigned long long *>(ws.cl), ws.cnt, a.k, st.mode, ws.thr,
                  a.D, a.I, a.label_base, ws.row_ovf, st.nsub);
        break;
    case K_FALLBACK_4:
        PF_LAUNCH(topk_fallback_kernel<4>, grid, block, 0, s, ws.row_ovf, a.q, (const void *)a.db, a.n, a.d, a.k, a.D, a.I, a.label_base,
                  (const uint2 *)nullptr);
        break;
    case K_FALLBACK_4_EXCL:
        PF_LAUNCH((topk_fallback_kernel<4, true>), grid, block, 0, s, ws.row_ovf, a.q, (const void *)a.db, a.n, a.d, a.k, a.D, a.I,
                  a.label_base, (const uint2 *)ws.excl);
        break;
    case K_FALLBACK_2_EXCL:
        PF_LAUNCH((topk_fallback_kernel<2, true>), grid, block, 0, s, ws.row_ovf, a.q, a.dbh, a.n, a.d, a.k, a.D, a.I, a.label_base,
                  (const uint2 *)ws.excl);
        break;
    case K_FALLBACK_2:
        PF_LAUNCH(topk_fallback_kernel<2>, grid, block, 0, s, ws.row_ovf, a.q, a.dbh, a.n, a.d, a.k, a.D, a.I, a.label_base,
                  (const uint2 *)nullptr);
        break;
    default: return launch_stage_f16(st, a);
    }
    PF_HIP(hipGetLastError());
    return 0;
}

// Validate, size the workspace, plan (search_plan.h: every choice of kernel, grid and threshold is made there), run the stages.
int search_topk(const float *db, const void *dbh, float xnorm_max, int64_t n, int d, int64_t label_base,
                const float *q, int64_t nq, int k, float *D, int64_t *I, SearchWorkspace &ws, hipStream_t s,
                int phase, float *lb, int mtop, const int64_t *excl_lo, const int64_t *excl_hi) {
    if (nq <= 0) return 0;
    SearchShape sh;
    sh.n = n; sh.d = d; sh.nq = nq; sh.k = k; sh.phase = phase; sh.mtop = mtop;
    sh.storage = db == nullptr ? STORE_F16 : (dbh != nullptr ? STORE_F32_COPY : STORE_F32);
    sh.resume = phase == 2 && ws.bound_valid && ws.bound_q == q && ws.bound_nq == nq && ws.bound_k == k;
    sh.has_lb = lb != nullptr;
    sh.excl = excl_lo != nullptr && excl_hi != nullptr;
    if (!sh.resume) ws.bound_valid = false;
    const SearchPlan plan = plan_search(sh, search_tuning());
    if (plan.error != PLAN_OK) { set_error("%s", plan.error_msg); return -1; }
    if (n > 0) {
        if (db == nullptr && dbh == nullptr) { set_error("search_topk: no rows"); return -1; }
        if (ensure_ws(ws, nq)) return -1;
        if (plan.need_qh && ws.qh_elems < nq * d) {
            if (ws.qh) { PF_HIP(hipStreamSynchronize(s)); (void)hipFree(ws.qh); }
            ws.qh = nullptr; ws.qh_elems = 0;
            PF_HIP(hipMalloc(&ws.qh, (size_t)nq * d * 2));
            ws.qh_elems = nq * d;
        }
        if (sh.excl && ws.excl_cap < nq) {
            // (grows like ws.qh above: the one place this call waits for the stream, and only when the batch got larger)
            if (ws.excl) { PF_HIP(hipStreamSynchronize(s)); (void)hipFree(ws.excl); }
            ws.excl = ws.excl_tile = nullptr; ws.excl_cap = 0;
            const int64_t cap = nq < 64 ? 64 : nq;
            // one allocation for both: the ranges, and behind them the spans of the query tiles
            PF_HIP(hipMalloc(&ws.excl, sizeof(uint2) * (cap + cap / 128 + 1)));
            ws.excl_tile = ws.excl + cap;
            ws.excl_cap = cap;
        }
    }
    const StageArgs a{db, dbh, xnorm_max, n, d, label_base, q, nq, k, D, I, lb, mtop, excl_lo, excl_hi, ws, s};
    for (int i = 0; i < plan.n_stages;) {
        const SearchStage &st = plan.stages[i];
        if (st.zero_cnt) PF_HIP(hipMemsetAsync(ws.cnt, 0, sizeof(int) * nq, s));
        if (st.tag == nullptr) {
            if (launch_stage(st, a)) return -1;
            ++i;
            continue;
        }
        ProfScope ps(st.tag, s, st.work);
        if (st.zero_overflow) PF_HIP(hipMemsetAsync(ws.overflow + 1, 0, 2 * sizeof(int), s));
        for (const int end = i + st.scope; i < end; ++i)
            if (launch_stage(plan.stages[i], a)) return -1;
    }
    // the hand-over between the two phases of a sharded search, valid for exactly this (q, nq, k)
    if (plan.leaves_bound) { ws.bound_valid = true; ws.bound_q = q; ws.bound_nq = nq; ws.bound_k = k; ws.bound_G = plan.G; }
    if (plan.consumes_bound) ws.bound_valid = false;
    return 0;
}

// ------------------------------------------------------------------------------------
// Merge of per-shard top-k lists (after the RCCL all-gather): exact top-k of S/L[nq][m].
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void merge_kernel(const float *__restrict__ S, const int64_t *__restrict__ Lb,
                                                     int m, int k, float *__restrict__ D,
                                                     int64_t *__restrict__ I) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long skeys[];
    const int64_t qi = blockIdx.x;
    const int tid = threadIdx.x;
    int P = 1;
    while (P < m) P <<= 1;
    for (int i = tid; i < P; i += 1024) {
        unsigned long long key = ~0ull;
        if (i < m && Lb[qi * m + i] >= 0) key = pack_key(S[qi * m + i], (unsigned)i);
        skeys[i] = key;
    }
    __syncthreads();
    bitonic_sort_u64(skeys, P, tid, 1024);
    for (int i = tid; i < k; i += 1024) {
        const unsigned long long key = i < P ? skeys[i] : ~0ull;
        if (key != ~0ull) {
            D[qi * k + i] = ord2f(~(unsigned)(key >> 32));
            I[qi * k + i] = Lb[qi * m + (unsigned)(key & 0xFFFFFFFFu)];
        } else {
            D[qi * k + i] = -3.4028234663852886e38f;
            I[qi * k + i] = -1;
        }
    }
}

int topk_merge(const float *S, const int64_t *L, int64_t nq, int m, int k, float *D, int64_t *I,
               hipStream_t s) {
    if (nq <= 0) return 0;
    if (m > 16384) { set_error("topk_merge: m=%d > 16384", m); return -1; }
    int P = 1;
    while (P < m) P <<= 1;
    if (ensure_dyn_lds((const void *)merge_kernel, 16384 * 8)) return -1;
    ProfScope ps("topk_merge", s);
    PF_LAUNCH(merge_kernel, dim3((unsigned)nq), dim3(1024), (size_t)P * 8, s, S, L, m, k, D, I);
    PF_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------
// The sharded search's two small reductions, one WAVEFRONT per query row (round 4).  Both used to go through merge_kernel
// -- a 1024-thread workgroup and a full bitonic sort in LDS per row -- and were, at 8 shards, the second largest item of
// a rank's scan time (2.1 of 7.4 ms per 77,824-row step: tools/ubench/sharded_scan_model.py).
//   bound_reduce_kernel : cands[G][nq][m] (the all-gathered pfann_search_bound outputs, as gathered: no transposed copy)
//                         -> lb[nq] = the k-th largest of the row's G*m values (-inf entries are absent); fewer than k
//                         present: -FLT_MAX.  A selection, not a sort: MSB-first bisection on the orderable bit patterns,
//                         one ballot + popcount per value and bit.
//   merge_lists_kernel  : Dl/Il[G][nq][k] (every shard's list for this rank's query slice, as the all-to-all delivers
//                         them) -> the exact top-k of the union, sorted by (score descending, shard-major position
//                         ascending) exactly like merge_kernel: k-th smallest packed key by bisection, ballot compaction
//                         of the k winners into LDS, rank sort (k <= 128: every lane counts the keys below its two).
// Rows of at most 64 * 16 = 1024 values; larger unions keep merge_kernel.
// ------------------------------------------------------------------------------------
constexpr int WPR_VPL = 16;       // values per lane

template <int VPL>
__global__ __launch_bounds__(256) void bound_reduce_kernel(const float *__restrict__ cands, int G, int64_t nq, int m, int k,
                                                           float *__restrict__ lb) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= nq) return;
    const int n = G * m;
    unsigned key[VPL];
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int i = lane + 64 * j;
        key[j] = 0u;                                            // absent: below every real value (f2ord(x) > 0 for finite x)
        if (i < n) {
            const int g = i / m, c = i - g * m;
            const float v = cands[((int64_t)g * nq + row) * m + c];
            if (v > -3.0e38f) key[j] = f2ord(v);                    // -inf / -FLT_MAX padding = absent
        }
    }
    int total = 0;
#pragma unroll
    for (int j = 0; j < VPL; ++j) total += __popcll(__ballot(key[j] != 0u));
    if (total < k) { if (lane == 0) lb[row] = -3.4028234663852886e38f; return; }
    unsigned prefix = 0u;
    for (int bit = 31; bit >= 0; --bit) {
        const unsigned cand = prefix | (1u << bit);
        int c = 0;
#pragma unroll
        for (int j = 0; j < VPL; ++j) c += __popcll(__ballot(key[j] >= cand));
        if (c >= k) prefix = cand;                               // at least k values reach cand: the k-th largest does too
    }
    if (lane == 0) lb[row] = ord2f(prefix);
}

__global__ __launch_bounds__(256) void merge_lists_kernel(const float *__restrict__ Dl, const int64_t *__restrict__ Il, int G,
                                                          int64_t nq, int k, float *__restrict__ D, int64_t *__restrict__ I) {
    __shared__ unsigned long long win[4][128];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * 4 + w;
    if (row >= nq) return;
    const int n = G * k;
    unsigned long long key[WPR_VPL];
    int nvalid = 0;
#pragma unroll
    for (int j = 0; j < WPR_VPL; ++j) {
        const int i = lane + 64 * j;
        key[j] = ~0ull;
        if (i < n) {
            const int g = i / k, c = i - g * k;
            const int64_t at = ((int64_t)g * nq + row) * k + c;
            if (Il[at] >= 0) key[j] = pack_key(Dl[at], (unsigned)i);   // i = shard-major position: ascending labels on ties
        }
        nvalid += __popcll(__ballot(key[j] != ~0ull));
    }
    const int kk = nvalid < k ? nvalid : k;
    // the kk-th smallest key (keys of valid entries are unique: the position is part of them)
    unsigned long long prefix = 0ull;
    if (kk > 0) {
        // largest P with count(key < P) < kk  <=>  P is the kk-th smallest: build P bit by bit
        for (int bit = 63; bit >= 0; --bit) {
            const unsigned long long cand = prefix | (1ull << bit);
            int c = 0;
#pragma unroll
            for (int j = 0; j < WPR_VPL; ++j) c += __popcll(__ballot(key[j] < cand));
            if (c < kk) prefix = cand;
        }
    }
    // winners (key <= prefix) -> LDS, in any order
    int base = 0;
#pragma unroll
    for (int j = 0; j < WPR_VPL; ++j) {
        const bool take = kk > 0 && key[j] <= prefix && key[j] != ~0ull;
        const unsigned long long mask = __ballot(take);
        if (take) win[w][base + __popcll(mask & ((1ull << lane) - 1ull))] = key[j];
        base += __popcll(mask);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");       // one wave: its LDS writes are visible to its own lanes
    // rank sort of the kk winners: lane owns winners lane and lane + 64
    for (int e = lane; e < k; e += 64) {
        float dv = -3.4028234663852886e38f;
        int64_t iv = -1;
        int pos = e;
        if (e < kk) {
            const unsigned long long me = win[w][e];
            int r = 0;
            for (int o = 0; o < kk; ++o) r += win[w][o] < me ? 1 : 0;
            const unsigned i = (unsigned)(me & 0xFFFFFFFFull);
            const int g = (int)i / k, c = (int)i - g * k;
            dv = ord2f(~(unsigned)(me >> 32));
            iv = Il[((int64_t)g * nq + row) * k + c];
            pos = r;
        }
        D[row * k + pos] = dv;
        I[row * k + pos] = iv;
    }
}

int bound_reduce(const float *cands, int G, int64_t nq, int m, int k, float *lb, hipStream_t s) {
    if (nq <= 0) return 0;
    if (G < 1 || m < 1 || (int64_t)G * m > 64 * WPR_VPL) { set_error("bound_reduce: %d x %d values per row > %d", G, m, 64 * WPR_VPL); return -1; }
    ProfScope ps("topk_bound_reduce", s);
    const int n = G * m;                      // values per lane: 5 covers dist.py's G * (2k/G + 8) at k = 100 up to G = 8
    if (n <= 64 * 5) PF_LAUNCH(bound_reduce_kernel<5>, dim3((unsigned)cdiv(nq, 4)), dim3(256), 0, s, cands, G, nq, m, k, lb);
    else if (n <= 64 * 8) PF_LAUNCH(bound_reduce_kernel<8>, dim3((unsigned)cdiv(nq, 4)), dim3(256), 0, s, cands, G, nq, m, k, lb);
    else PF_LAUNCH(bound_reduce_kernel<WPR_VPL>, dim3((unsigned)cdiv(nq, 4)), dim3(256), 0, s, cands, G, nq, m, k, lb);
    PF_HIP(hipGetLastError());
    return 0;
}

int merge_lists(const float *Dl, const int64_t *Il, int G, int64_t nq, int k, float *D, int64_t *I, hipStream_t s) {
    if (nq <= 0) return 0;
    if (G < 1 || k < 1 || k > 128 || (int64_t)G * k > 64 * WPR_VPL) { set_error("merge_lists: %d lists of %d outside the wave kernel's range", G, k); return -1; }
    ProfScope ps("topk_merge_lists", s);
    PF_LAUNCH(merge_lists_kernel, dim3((unsigned)cdiv(nq, 4)), dim3(256), 0, s, Dl, Il, G, nq, k, D, I);
    PF_HIP(hipGetLastError());
    return 0;
}

// pfann_prewarm: one empty launch per translation unit makes the runtime load this unit's code object now
__global__ void noop_search_kernel() {}
int prewarm_search() {
    hipLaunchKernelGGL(noop_search_kernel, dim3(1), dim3(1), 0, 0);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace pfann
