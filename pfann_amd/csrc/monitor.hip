// Monitor mode: the sequence matcher over every window of a long recording (pfann_match_windows).
//
// The answer for the window that starts at row w0 of a recording is what match_kernel (rerank.hip) gives for the query
// (qstart = rstart + w0, qlen = window), mode 0: candidates = the alignments (song, offset) that a top-k label of one of
// THAT window's rows nominates, in np.unique order, score = sum of the window's row dots / sub_len, strict-> first-wins
// argmax (reference database.py:129-163 applied to emb[w0:w0+window]).  Matching the windows one by one computes every
// (alignment, row) inner product once per window that contains the row -- up to `window` times -- and sorts candidate
// lists that are 95 % the same.  Here one workgroup owns a CHUNK of up to C consecutive window starts of one recording:
//
//   labels of the chunk's S = (n-1)*hop + window rows -> keys (song, diagonal, row), diagonal = row-in-song - row-in-chunk,
//      so one alignment is one diagonal whichever window looks at it (its offset in window i is diagonal + i*hop)
//   -> bitonic sort in LDS: unique alignments are runs of equal (song, diagonal), in np.unique order, each run holding
//      the rows that nominated it in ascending order
//   -> one wave per alignment: the dots of the rows that some candidate window of the chunk contains, each computed ONCE
//      into a per-wave LDS line; then lane i forms the sum of window i if one of its own rows nominated the alignment,
//      and keeps its first maximum
//   -> the 16 waves' per-window maxima are merged (ties: the smaller alignment index, i.e. np.unique order).
//
// SUMMATION ORDER (a window's score bits depend on the window's rows and the candidate only, not on hop, chunking, the
// other windows / recordings of the call or the storage plan):
//   row dot  : lane c holds float4 chunk c (c + 64 m) of the row, four fmaf chains p0..p3 from +0 in ascending m,
//              s = (p0 + p1) + (p2 + p3), then wave_sum's xor butterfly (32, 16, .., 1).  For d <= 128 a row has at most 32
//              chunks and two rows share a wave, one per half: lanes 32..63 of the one-row form hold +0 and s is never
//              -0, so the butterfly's first step is the identity and the 16..1 steps inside a half give the same bits.
//   window   : tot = 0; tot += dot[row] for the window's rows in ascending order, fp32 (rows outside the song: +0)
//   score    : (double)tot / (double)sub_len, as mode 0 of match_kernel.
#include "kernels.h"
#include "match_common.h"
#include <algorithm>
#include <type_traits>

namespace pfann {

static constexpr int WIN_NT = 1024;
static constexpr int WIN_ROW_BITS = 8;                 // row-in-chunk field of a key: S <= WIN_SMAX = 256
static constexpr int WIN_DIAG_BITS = 28;               // diagonal + WIN_SMAX; the song takes the 28 bits above
static constexpr int WIN_GRID = 1024;                  // workgroups; each walks the chunk slots blockIdx.x, + gridDim.x, ..

__device__ __forceinline__ int windows_of(int L, int window, int hop) {
    return L <= 0 ? 0 : (L < window ? 1 : (L - window) / hop + 1);
}

template <bool F16>
__global__ __launch_bounds__(WIN_NT) void match_windows_kernel(WindowsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long sk[];    // [P] keys, then [P + 1] run heads (ushort)
    __shared__ long long s_cpos[1024];
    __shared__ float s_dot[WIN_NT / 64][WIN_SMAX];       // per wave: the row dots of the alignment in hand
    __shared__ float s_bt[WIN_NT / 64][64];              // per wave and window: best total, its alignment, candidates seen
    __shared__ int s_ba[WIN_NT / 64][64];
    __shared__ int s_bn[WIN_NT / 64][64];
    __shared__ int s_wtot[WIN_NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nchr = a.d >> 2;

    const int64_t nW = a.wfirst[a.nR];
    // few windows in the whole call: smaller chunks, so that more than a handful of compute units take part
    const int C = min(a.C, max(4, (int)((nW + 255) / 256)));
    // chunk slots: recording r owns the slots [wfirst[r] / C + r, wfirst[r + 1] / C + r + 1), at least ceil(its windows / C)
    const int64_t n_slots = nW / C + a.nR;
    int cshift, n_coarse;
    load_coarse_song_pos<WIN_NT>(a.song_pos, a.n_songs, s_cpos, tid, cshift, n_coarse);

    for (int64_t slot = blockIdx.x; slot < n_slots; slot += gridDim.x) {
        int64_t lo = 0, hi = a.nR;                       // first recording whose slots start after `slot`
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (a.wfirst[mid] / C + mid <= slot) lo = mid + 1; else hi = mid;
        }
        const int64_t r = lo - 1;
        const int L = a.rlen[r];
        const int64_t nw = min((int64_t)windows_of(L, a.window, a.hop), a.wfirst[r + 1] - a.wfirst[r]);
        const int64_t c0 = (slot - (a.wfirst[r] / C + r)) * C;       // first window of the chunk
        if (c0 >= nw) continue;                          // (the whole workgroup: a spare slot)
        const int nwc = (int)min((int64_t)C, nw - c0);
        const int wl = min(a.window, L);                 // rows of a window: `window`, or all rows of a shorter recording
        const int S = (nwc - 1) * a.hop + wl;            // rows the chunk spans (<= WIN_SMAX, S * k <= MAXC: the host's C)
        const int64_t q0 = a.rstart[r] + c0 * a.hop;
        const int ntot = S * a.k;
        int P = 1;
        while (P < ntot) P <<= 1;
        unsigned short *heads = reinterpret_cast<unsigned short *>(sk + P);

        // ---- keys (song, diagonal, row)
        for (int i = tid; i < P; i += WIN_NT) {
            unsigned long long key = SENT;
            if (i < ntot) {
                const int tr = i / a.k;
                const int64_t lab = a.labels[(q0 + tr) * a.k + (i - tr * a.k)];
                if (lab >= 0) {
                    const int song = song_of_label(a.song_pos, a.n_songs, s_cpos, cshift, n_coarse, lab);
                    const int64_t p = song >= 0 ? lab - a.song_pos[song] : 0;
                    // (p beyond the field: a label past the last row -- the search never returns one)
                    if (song >= 0 && p < (1ll << WIN_DIAG_BITS) - 2 * WIN_SMAX)
                        key = ((unsigned long long)song << (WIN_DIAG_BITS + WIN_ROW_BITS)) |
                              ((unsigned long long)(unsigned)((int)p - tr + WIN_SMAX) << WIN_ROW_BITS) | (unsigned long long)tr;
                }
            }
            sk[i] = key;
        }
        __syncthreads();
        bitonic_sort_keys<WIN_NT>(sk, P, tid);

        // ---- run heads: heads[a] = first key of alignment a, heads[n] = end of the last run
        {
            const int ept = P >= WIN_NT ? P / WIN_NT : 1;
            int cnt = 0;
            unsigned hm = 0;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int i = tid * ept + e;
                if (e < ept && i < P && (i == 0 || (sk[i] >> WIN_ROW_BITS) != (sk[i - 1] >> WIN_ROW_BITS))) { hm |= 1u << e; ++cnt; }
            }
            int incl = cnt;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int v = __shfl_up(incl, o, 64);
                if (lane >= o) incl += v;
            }
            if (lane == 63) s_wtot[wave] = incl;
            __syncthreads();
            int base = 0, total = 0;
            for (int w = 0; w < WIN_NT / 64; ++w) { const int v = s_wtot[w]; if (w < wave) base += v; total += v; }
            int pos = base + incl - cnt;
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (hm & (1u << e)) heads[pos++] = (unsigned short)(tid * ept + e);
            if (tid == 0) heads[total] = (unsigned short)P;        // P <= 8192
            __syncthreads();
            // the padding / dropped labels sort last as one run of SENT: not an alignment
            const int nalign = total - (sk[P - 1] == SENT ? 1 : 0);

            // ---- one wave per alignment
            float best = -INFINITY;
            int besta = 0x7FFFFFFF, ncand = 0;
            const int ws = lane * a.hop;
            const bool wlive = lane < nwc;
            float *dot = s_dot[wave];
            const float4 *qb = reinterpret_cast<const float4 *>(a.q + q0 * a.d);
            for (int al = wave; al < nalign; al += WIN_NT / 64) {
                const int h0 = heads[al], h1 = heads[al + 1];
                const unsigned long long key0 = sk[h0];
                const int song = (int)(key0 >> (WIN_DIAG_BITS + WIN_ROW_BITS));
                const int diag = (int)((key0 >> WIN_ROW_BITS) & ((1ull << WIN_DIAG_BITS) - 1)) - WIN_SMAX;
                const int tmin = (int)(key0 & (WIN_SMAX - 1)), tmax = (int)(sk[h1 - 1] & (WIN_SMAX - 1));
                // windows that can hold a nominating row: i*hop <= row < i*hop + wl
                const int i_lo = tmin - wl + 1 <= 0 ? 0 : (tmin - wl + a.hop) / a.hop;
                const int i_hi = min(nwc - 1, tmax / a.hop);
                if (i_lo > i_hi) continue;               // nominated only by rows between two windows (hop > window)
                const int r_lo = i_lo * a.hop, r_hi = i_hi * a.hop + wl;     // their rows, inside [0, S)
                const int64_t start = a.song_pos[song];
                const int slen = (int)(a.song_pos[song + 1] - start);
                const int a_lo = max(r_lo, -diag), a_hi = min(r_hi, slen - diag);   // the rows that lie inside the song
                for (int tr = r_lo + lane; tr < r_hi; tr += 64)
                    if (tr < a_lo || tr >= a_hi) dot[tr] = 0.f;
                if (nchr <= 32) {
                    // two rows per step (one per half wave), four steps in flight: the gather lives on memory-level parallelism
                    const int half = lane >> 5, hl = lane & 31;
                    for (int t0 = a_lo; t0 < a_hi; t0 += 8) {
                        float s[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const int tr = t0 + 2 * u + half;
                            s[u] = 0.f;
                            if (tr < a_hi && hl < nchr) {
                                const float4 w = qb[(int64_t)tr * nchr + hl];
                                const int64_t ro = (start + diag + tr) * (int64_t)nchr + hl;
                                float4 v;
                                if (F16) {
                                    typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
                                    const f16x4 h = reinterpret_cast<const f16x4 *>(a.dbh)[ro];
                                    v = make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]);
                                } else {
                                    v = reinterpret_cast<const float4 *>(a.db)[ro];
                                }
                                const float p0 = fmaf(v.x, w.x, 0.f), p1 = fmaf(v.y, w.y, 0.f);
                                const float p2 = fmaf(v.z, w.z, 0.f), p3 = fmaf(v.w, w.w, 0.f);
                                s[u] = (p0 + p1) + (p2 + p3);
                            }
                        }
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const float v = wave_sum_half(s[u]);
                            const int tr = t0 + 2 * u + half;
                            if (hl == 0 && tr < a_hi) dot[tr] = v;
                        }
                    }
                } else {
                    for (int tr = a_lo; tr < a_hi; ++tr) {
                        const float4 *wq = qb + (int64_t)tr * nchr;
                        const int64_t ro = (start + diag + tr) * (int64_t)nchr;
                        float p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f;
                        for (int ch = lane; ch < nchr; ch += 64) {
                            const float4 w = wq[ch];
                            float4 v;
                            if (F16) {
                                typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
                                const f16x4 h = reinterpret_cast<const f16x4 *>(a.dbh)[ro + ch];
                                v = make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]);
                            } else {
                                v = reinterpret_cast<const float4 *>(a.db)[ro + ch];
                            }
                            p0 = fmaf(v.x, w.x, p0); p1 = fmaf(v.y, w.y, p1); p2 = fmaf(v.z, w.z, p2); p3 = fmaf(v.w, w.w, p3);
                        }
                        const float v = wave_sum((p0 + p1) + (p2 + p3));
                        if (lane == 0) dot[tr] = v;
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the line is written: every lane may read it
                __builtin_amdgcn_wave_barrier();
                // lane i = window i: a candidate there only if one of the window's OWN rows nominated the alignment
                bool mine = false;
                for (int e = h0; e < h1; ++e) {
                    const int n = (int)(sk[e] & (WIN_SMAX - 1));
                    mine |= n >= ws && n < ws + wl;
                }
                if (wlive && mine) {
                    float tot = 0.f;
                    for (int j = 0; j < wl; ++j) tot += dot[ws + j];
                    ++ncand;
                    if (tot > best) { best = tot; besta = al; }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // all read before the next alignment overwrites
                __builtin_amdgcn_wave_barrier();
            }
            s_bt[wave][lane] = best;
            s_ba[wave][lane] = besta;
            s_bn[wave][lane] = ncand;
            __syncthreads();
            // ---- per window: first maximum in alignment (= np.unique) order over the waves
            if (tid < nwc) {
                float b = -INFINITY;
                int ba = 0x7FFFFFFF, n = 0;
                for (int w = 0; w < WIN_NT / 64; ++w) {
                    const float t = s_bt[w][tid];
                    const int ta = s_ba[w][tid];
                    n += s_bn[w][tid];
                    if (ta != 0x7FFFFFFF && (t > b || (t == b && ta < ba))) { b = t; ba = ta; }
                }
                pfann_match_result res;
                res.n_cand = n;
                if (ba != 0x7FFFFFFF) {
                    const unsigned long long key = sk[heads[ba]];
                    res.song = (int)(key >> (WIN_DIAG_BITS + WIN_ROW_BITS));
                    res.offset = (int)((key >> WIN_ROW_BITS) & ((1ull << WIN_DIAG_BITS) - 1)) - WIN_SMAX + tid * a.hop;
                    res.shift = 0;
                    res.score = (double)b / (double)wl;
                } else {
                    res.song = -1; res.offset = 0; res.shift = 0; res.score = -INFINITY;
                }
                a.results[a.wfirst[r] + c0 + tid] = res;
            }
            __syncthreads();                             // the lists are free for the next slot
        }
    }
}

// ---- ranked windows (pfann_match_windows_topn): the n best songs of every window --------------------------------------
// Keys, sort, run heads, row dots and window totals are those of match_windows_kernel above -- same summation order, so a
// total has the same bits here and there.  The sorted keys put a song's alignments next to each other, in candidate order,
// so instead of striding over the alignments the 16 waves take contiguous blocks of them, cut at song boundaries: a wave
// sees whole songs, and lane i (window i) keeps the song's first maximum and its number of candidates in registers.  When
// the song ends, every lane that had a candidate packs (total, alignment, count) into one 64-bit word that compares as
// (total descending, alignment ascending) and pushes it into the window's list of n words in LDS: slot j takes the word
// with atomicMax and hands the smaller of the two on to slot j + 1.  Every word passes slot 0, which therefore ends with
// the largest; every other word passes slot 1; and so on: whatever the order in which the waves arrive, the list ends as
// the n largest words in descending order.  Slot values never decrease and never exceed the slot before, so a word that
// is not above slot n - 1 can be dropped at once, which is what happens to nearly every song once the lists are warm.
// LDS: the kernel above's lists without its three per-wave [16][64] arrays, plus [64 slots][64 windows] words = 32 KB
// and 64 counters: 139.6 KB of the 160 KB of a compute unit; no scratch in HBM.
static constexpr int WTOP_AL_BITS = 13, WTOP_CNT_BITS = 14;          // alignment < MAXC = 2^13, candidates <= MAXC

__device__ __forceinline__ unsigned ordered_bits(float t) {         // a > b  <=>  ordered_bits(a) > ordered_bits(b)
    const unsigned u = __float_as_uint(t);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ordered_float(unsigned u) {
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}

// the row dots of one alignment for the chunk rows [r_lo, r_hi) into the wave's line: match_windows_kernel's, to the bit
template <bool F16>
__device__ __forceinline__ void alignment_row_dots(const WindowsArgs &a, const float4 *qb, float *dot, int64_t start, int diag,
                                                   int r_lo, int r_hi, int a_lo, int a_hi, int nchr, int lane) {
    for (int tr = r_lo + lane; tr < r_hi; tr += 64)
        if (tr < a_lo || tr >= a_hi) dot[tr] = 0.f;
    if (nchr <= 32) {
        const int half = lane >> 5, hl = lane & 31;
        for (int t0 = a_lo; t0 < a_hi; t0 += 8) {
            float s[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int tr = t0 + 2 * u + half;
                s[u] = 0.f;
                if (tr < a_hi && hl < nchr) {
                    const float4 w = qb[(int64_t)tr * nchr + hl];
                    const int64_t ro = (start + diag + tr) * (int64_t)nchr + hl;
                    float4 v;
                    if (F16) {
                        typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
                        const f16x4 h = reinterpret_cast<const f16x4 *>(a.dbh)[ro];
                        v = make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]);
                    } else {
                        v = reinterpret_cast<const float4 *>(a.db)[ro];
                    }
                    const float p0 = fmaf(v.x, w.x, 0.f), p1 = fmaf(v.y, w.y, 0.f);
                    const float p2 = fmaf(v.z, w.z, 0.f), p3 = fmaf(v.w, w.w, 0.f);
                    s[u] = (p0 + p1) + (p2 + p3);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float v = wave_sum_half(s[u]);
                const int tr = t0 + 2 * u + half;
                if (hl == 0 && tr < a_hi) dot[tr] = v;
            }
        }
    } else {
        for (int tr = a_lo; tr < a_hi; ++tr) {
            const float4 *wq = qb + (int64_t)tr * nchr;
            const int64_t ro = (start + diag + tr) * (int64_t)nchr;
            float p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f;
            for (int ch = lane; ch < nchr; ch += 64) {
                const float4 w = wq[ch];
                float4 v;
                if (F16) {
                    typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
                    const f16x4 h = reinterpret_cast<const f16x4 *>(a.dbh)[ro + ch];
                    v = make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]);
                } else {
                    v = reinterpret_cast<const float4 *>(a.db)[ro + ch];
                }
                p0 = fmaf(v.x, w.x, p0); p1 = fmaf(v.y, w.y, p1); p2 = fmaf(v.z, w.z, p2); p3 = fmaf(v.w, w.w, p3);
            }
            const float v = wave_sum((p0 + p1) + (p2 + p3));
            if (lane == 0) dot[tr] = v;
        }
    }
}

template <bool F16>
__global__ __launch_bounds__(WIN_NT) void match_windows_topn_kernel(WindowsTopnArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long sk[];    // [P] keys, then [P + 1] run heads (ushort)
    __shared__ long long s_cpos[1024];
    __shared__ float s_dot[WIN_NT / 64][WIN_SMAX];       // per wave: the row dots of the alignment in hand
    __shared__ unsigned long long s_top[WIN_TOPN_FAST * 64];     // [slot][window]: the ranked words, 0 = empty
    __shared__ int s_nf[64];                             // per window: songs with a candidate
    __shared__ int s_wtot[WIN_NT / 64];
    constexpr int NWV = WIN_NT / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nchr = a.d >> 2;

    const int64_t nW = a.wfirst[a.nR];
    const int C = min(a.C, max(4, (int)((nW + 255) / 256)));         // chunks and slots as in match_windows_kernel
    const int64_t n_slots = nW / C + a.nR;
    int cshift, n_coarse;
    load_coarse_song_pos<WIN_NT>(a.song_pos, a.n_songs, s_cpos, tid, cshift, n_coarse);
    for (int e = tid; e < a.n * 64; e += WIN_NT) s_top[e] = 0;
    if (tid < 64) s_nf[tid] = 0;
    // (the first barrier of the first slot orders these stores before any use)

    for (int64_t slot = blockIdx.x; slot < n_slots; slot += gridDim.x) {
        int64_t lo = 0, hi = a.nR;                       // first recording whose slots start after `slot`
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (a.wfirst[mid] / C + mid <= slot) lo = mid + 1; else hi = mid;
        }
        const int64_t r = lo - 1;
        const int L = a.rlen[r];
        const int64_t nw = min((int64_t)windows_of(L, a.window, a.hop), a.wfirst[r + 1] - a.wfirst[r]);
        const int64_t c0 = (slot - (a.wfirst[r] / C + r)) * C;       // first window of the chunk
        if (c0 >= nw) continue;                          // (the whole workgroup: a spare slot)
        const int nwc = (int)min((int64_t)C, nw - c0);
        const int wl = min(a.window, L);                 // rows of a window: `window`, or all rows of a shorter recording
        const int S = (nwc - 1) * a.hop + wl;            // rows the chunk spans (<= WIN_SMAX, S * k <= MAXC: the host's C)
        const int64_t q0 = a.rstart[r] + c0 * a.hop;
        const int ntot = S * a.k;
        int P = 1;
        while (P < ntot) P <<= 1;
        unsigned short *heads = reinterpret_cast<unsigned short *>(sk + P);

        // ---- keys (song, diagonal, row)
        for (int i = tid; i < P; i += WIN_NT) {
            unsigned long long key = SENT;
            if (i < ntot) {
                const int tr = i / a.k;
                const int64_t lab = a.labels[(q0 + tr) * a.k + (i - tr * a.k)];
                if (lab >= 0) {
                    const int song = song_of_label(a.song_pos, a.n_songs, s_cpos, cshift, n_coarse, lab);
                    const int64_t p = song >= 0 ? lab - a.song_pos[song] : 0;
                    if (song >= 0 && p < (1ll << WIN_DIAG_BITS) - 2 * WIN_SMAX)
                        key = ((unsigned long long)song << (WIN_DIAG_BITS + WIN_ROW_BITS)) |
                              ((unsigned long long)(unsigned)((int)p - tr + WIN_SMAX) << WIN_ROW_BITS) | (unsigned long long)tr;
                }
            }
            sk[i] = key;
        }
        __syncthreads();
        bitonic_sort_keys<WIN_NT>(sk, P, tid);

        // ---- run heads: heads[a] = first key of alignment a, heads[n] = end of the last run
        const int ept = P >= WIN_NT ? P / WIN_NT : 1;
        int cnt = 0;
        unsigned hm = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int i = tid * ept + e;
            if (e < ept && i < P && (i == 0 || (sk[i] >> WIN_ROW_BITS) != (sk[i - 1] >> WIN_ROW_BITS))) { hm |= 1u << e; ++cnt; }
        }
        int incl = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o, 64);
            if (lane >= o) incl += v;
        }
        if (lane == 63) s_wtot[wave] = incl;
        __syncthreads();
        int base = 0, total = 0;
        for (int w = 0; w < NWV; ++w) { const int v = s_wtot[w]; if (w < wave) base += v; total += v; }
        int pos = base + incl - cnt;
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (hm & (1u << e)) heads[pos++] = (unsigned short)(tid * ept + e);
        if (tid == 0) heads[total] = (unsigned short)P;
        __syncthreads();
        const int nalign = total - (sk[P - 1] == SENT ? 1 : 0);

        // ---- the wave's block of alignments [blk0, blk1): from the first song boundary at or after wave * nalign / 16 to
        // the next wave's (a song that spans several nominal cuts leaves the waves between them an empty block)
        int blk[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            int b = wave + e >= NWV ? nalign : (wave + e) * nalign / NWV;
            while (b > 0 && b < nalign) {                // (wave-uniform)
                const int al = b + lane;
                const bool edge = al >= nalign || (sk[heads[al]] >> (WIN_DIAG_BITS + WIN_ROW_BITS)) !=
                                                  (sk[heads[al - 1]] >> (WIN_DIAG_BITS + WIN_ROW_BITS));
                const unsigned long long m = __ballot(edge);
                if (m) { b += __ffsll(m) - 1; break; }
                b += 64;
            }
            blk[e] = b;
        }

        // ---- whole songs: lane i = window i keeps the song's first maximum and its candidates, then ranks the song
        float best = -INFINITY;
        int besta = -1, ncand = 0, nsongs = 0, cur = -1;
        const int ws = lane * a.hop;
        const bool wlive = lane < nwc;
        float *dot = s_dot[wave];
        const float4 *qb = reinterpret_cast<const float4 *>(a.q + q0 * a.d);
        for (int al = blk[0]; al <= blk[1]; ++al) {
            int song = -1, h0 = 0, h1 = 0;
            unsigned long long key0 = 0;
            if (al < blk[1]) {
                h0 = heads[al]; h1 = heads[al + 1];
                key0 = sk[h0];
                song = (int)(key0 >> (WIN_DIAG_BITS + WIN_ROW_BITS));
            }
            if (song != cur) {                           // the song in hand is complete (al == blk1: the block's last one)
                if (ncand > 0) {
                    ++nsongs;
                    if (besta >= 0) {                    // (a song whose totals are all NaN or -inf counts but never ranks)
                        unsigned long long x = ((unsigned long long)ordered_bits(best) << 32) |
                                               ((unsigned long long)(MAXC - 1 - besta) << WTOP_CNT_BITS) | (unsigned long long)ncand;
                        unsigned long long *col = s_top + lane;
                        if (x > __atomic_load_n(col + (a.n - 1) * 64, __ATOMIC_RELAXED))
                            for (int j = 0; j < a.n && x != 0; ++j) {
                                const unsigned long long old = atomicMax(col + j * 64, x);
                                if (old < x) x = old;
                            }
                    }
                }
                cur = song; best = -INFINITY; besta = -1; ncand = 0;
            }
            if (al == blk[1]) break;
            const int diag = (int)((key0 >> WIN_ROW_BITS) & ((1ull << WIN_DIAG_BITS) - 1)) - WIN_SMAX;
            const int tmin = (int)(key0 & (WIN_SMAX - 1)), tmax = (int)(sk[h1 - 1] & (WIN_SMAX - 1));
            const int i_lo = tmin - wl + 1 <= 0 ? 0 : (tmin - wl + a.hop) / a.hop;
            const int i_hi = min(nwc - 1, tmax / a.hop);
            if (i_lo > i_hi) continue;                   // nominated only by rows between two windows (hop > window)
            const int r_lo = i_lo * a.hop, r_hi = i_hi * a.hop + wl;
            const int64_t start = a.song_pos[song];
            const int slen = (int)(a.song_pos[song + 1] - start);
            const int a_lo = max(r_lo, -diag), a_hi = min(r_hi, slen - diag);
            alignment_row_dots<F16>(a, qb, dot, start, diag, r_lo, r_hi, a_lo, a_hi, nchr, lane);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the line is written: every lane may read it
            __builtin_amdgcn_wave_barrier();
            bool mine = false;
            for (int e = h0; e < h1; ++e) {
                const int n = (int)(sk[e] & (WIN_SMAX - 1));
                mine |= n >= ws && n < ws + wl;
            }
            if (wlive && mine) {
                float tot = 0.f;
                for (int j = 0; j < wl; ++j) tot += dot[ws + j];
                ++ncand;
                if (tot > best) { best = tot; besta = al; }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // all read before the next alignment overwrites
            __builtin_amdgcn_wave_barrier();
        }
        if (nsongs) atomicAdd(&s_nf[lane], nsongs);
        __syncthreads();

        // ---- the lists leave, and are empty again for the next slot (every thread clears what it read)
        const int64_t wbase = a.wfirst[r] + c0;
        for (int e = tid; e < a.n * 64; e += WIN_NT) {
            const int w = e & 63, j = e >> 6;
            const unsigned long long x = s_top[e];
            s_top[e] = 0;
            if (w >= nwc) continue;
            pfann_match_result res;
            if (x != 0) {
                const unsigned long long key = sk[heads[MAXC - 1 - (int)((x >> WTOP_CNT_BITS) & ((1u << WTOP_AL_BITS) - 1))]];
                res.song = (int)(key >> (WIN_DIAG_BITS + WIN_ROW_BITS));
                res.offset = (int)((key >> WIN_ROW_BITS) & ((1ull << WIN_DIAG_BITS) - 1)) - WIN_SMAX + w * a.hop;
                res.shift = 0;
                res.n_cand = (int)(x & ((1u << WTOP_CNT_BITS) - 1));
                res.score = (double)ordered_float((unsigned)(x >> 32)) / (double)wl;
            } else {
                res.song = -1; res.offset = 0; res.shift = 0; res.n_cand = 0; res.score = -INFINITY;
            }
            a.top[(wbase + w) * a.n + j] = res;
        }
        if (tid < 64) {
            if (tid < nwc && a.n_found != nullptr) a.n_found[wbase + tid] = s_nf[tid];
            s_nf[tid] = 0;
        }
        __syncthreads();                                 // the lists are free for the next slot
    }
}

// windows -> (qstart, qlen) of the general path: window g of the call is window g - wfirst[r] of its recording r
__global__ void expand_windows_kernel(const int64_t *__restrict__ rstart, const int32_t *__restrict__ rlen, int64_t nR, int window,
                                      int hop, const int64_t *__restrict__ wfirst, int64_t nW, int64_t *__restrict__ qstart,
                                      int32_t *__restrict__ qlen) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nW) return;
    int64_t lo = 0, hi = nR - 1;                         // first recording whose windows end after g
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (wfirst[mid + 1] <= g) lo = mid + 1; else hi = mid;
    }
    const int64_t w0 = (g - wfirst[lo]) * hop;
    const int64_t L = rlen[lo];
    qstart[g] = rstart[lo] + w0;
    const int64_t left = L - w0;
    qlen[g] = (int32_t)(left <= 0 ? 0 : (left < window ? left : window));
}

int launch_expand_windows(const int64_t *rstart, const int32_t *rlen, int64_t nR, int window, int hop, const int64_t *wfirst,
                          int64_t nW, int64_t *qstart, int32_t *qlen, hipStream_t s) {
    if (nW <= 0) return 0;
    PF_LAUNCH(expand_windows_kernel, dim3((unsigned)cdiv(nW, 256)), dim3(256), 0, s, rstart, rlen, nR, window, hop, wfirst, nW,
              qstart, qlen);
    PF_HIP(hipGetLastError());
    return 0;
}

int match_windows_chunk(int k, int window, int hop) {
    if (k < 1 || window < 1 || hop < 1 || window > WIN_SMAX) return 0;
    int64_t c = ((int64_t)(MAXC / k) - window + 1) / hop;           // (C * hop + window - 1) * k <= MAXC
    c = std::min<int64_t>(c, (WIN_SMAX - window) / hop + 1);        // (C - 1) * hop + window <= WIN_SMAX
    return (int)std::max<int64_t>(0, std::min<int64_t>(c, 64));     // one lane per window
}

// what the two windowed launches share: the chunk and song bounds, the LDS opt-in and size, the fp32 / fp16 instantiation
// (and the ranked launch's own argument check); `what` names the call in a refusal, `tag` is its ProfScope tag
template <class Args>
static int launch_windows(const char *what, const char *tag, void (*k32)(Args), void (*k16)(Args), const Args &a, hipStream_t s) {
    if (a.nR <= 0) return 0;
    if (a.C < 1 || a.C > match_windows_chunk(a.k, a.window, a.hop)) { set_error("%s: chunk of %d windows does not fit", what, a.C); return -1; }
    if (a.n_songs >= (1 << 28) - 1) { set_error("%s: too many songs", what); return -1; }
    if constexpr (std::is_same<Args, WindowsTopnArgs>::value)
        if (a.n < 1 || a.n > WIN_TOPN_FAST || a.top == nullptr) { set_error("%s: top-N arguments (n=%d)", what, a.n); return -1; }
    const int lds_max = MAXC * 8 + (MAXC + 8) * 2;
    void (*fn)(Args) = a.db != nullptr ? k32 : k16;
    if (ensure_dyn_lds((const void *)fn, lds_max)) return -1;
    int P = 1;
    while (P < ((a.C - 1) * a.hop + a.window) * a.k) P <<= 1;
    const size_t lds = (size_t)P * 8 + (size_t)(P + 8) * 2;
    ProfScope ps(tag, s);
    PF_LAUNCH(fn, dim3(WIN_GRID), dim3(WIN_NT), lds, s, a);
    PF_HIP(hipGetLastError());
    return 0;
}

int launch_match_windows(const WindowsArgs &a, hipStream_t s) {
    return launch_windows("match_windows", "seq_match_windows", match_windows_kernel<false>, match_windows_kernel<true>, a, s);
}

int launch_match_windows_topn(const WindowsTopnArgs &a, hipStream_t s) {
    static_assert(MAXC <= (1 << WTOP_AL_BITS) && MAXC < (1 << WTOP_CNT_BITS), "a ranked word holds an alignment index and a count");
    return launch_windows("match_windows_topn", "seq_match_windows_topn", match_windows_topn_kernel<false>,
                          match_windows_topn_kernel<true>, a, s);
}

__global__ void noop_monitor_kernel() {}
int prewarm_monitor() {
    hipLaunchKernelGGL(noop_monitor_kernel, dim3(1), dim3(1), 0, 0);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace pfann
