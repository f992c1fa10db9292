// Windowed dense nomination on the fp16 MFMA (pfann_nominate_windows_dense): pfann_nominate_songs_dense for every window of long
// recordings, over tiles that neighbouring windows SHARE.  Window w of recording r is the query of rows
// [rstart[r] + w * hop, .. + wl), wl = min(window, rlen[r]); its cand row, n_found and n_close are byte for byte what
// pfann_nominate_songs_dense (nominate.hip) writes for that query: tot16, A, eps_t, E and the ranking are defined there and
// keep their definitions and their summation order.  With an excluded song for the recording, that song's candidates are no
// candidates: it is not ranked and not counted, and the certificate speaks about the dense matcher called with the same exclusion.
//
// WHY ANOTHER TILING.  nominate.hip packs disjoint queries into a 128-row tile, 128 / max_qlen slots; windows of a recording
// overlap, so as queries their row dots are computed once per window.  dense.hip's geometry computes them once per tile: a tile
// is NW_T consecutive recording rows x NW_T consecutive database rows with a halo of window-1 rows both ways, and owns the
// SI = NW_T - (window-1) window starts i < SI and the alignments whose window row 0 meets its columns j < SI.  At window 19
// and hop 2 that is 55 windows per tile product instead of 6.
//
// ROWS.  nominate_windows_prep_kernel, one wave per row, writes ONE fp16 image of the call's recording rows, unpacked
// [rows][d] halves, with q_prep_kernel's arithmetic exactly as nominate_prep_kernel does, and per row eps_t, ||q_t|| and a flag
// (norm >= 6e4 or a NaN: the row's image is zeros).  Row i of recording r lies at nw_row_base(r) + i: the recording's first
// row-tile slot times SI plus r halos, so every recording has room for the rows its windows of the call read and the host can
// size the image from n_windows and nR alone (the row counts live on the device).
// TILES.  Items, slots, recordings, spare slots, the coarse song_pos table, s_song and s_head, the per-song segmented shuffle
// maximum and the ws_row0 indexing are match_windows_dense_kernel<RANKED>'s; the staging, the product and S16 laid over the
// staging are nominate_tile_kernel's: 128-half K blocks of both operands behind one barrier, v_mfma_f32_32x32x16_f16 over the
// k-blocks of 16 in ascending order.  The words are 32-bit ordered bits (no id: the offset is not tracked), one atomicMax per
// non-empty (window, song in the tile) into ws[window of the chunk][song].  Pieces of the excluded song are dropped here.
//   The walk is the summation order: tot = +0; tot += S16[i + t][j + t] in ascending t.  No sliding or prefix sums.
//   The k-th LIVE window start of a tile goes to half k & 1 of the workgroup (dense.hip hands start ib + h to half h, so at
//   hop 2 one half idles); which half walks a window cannot change a byte.
// SELECT.  nominate_windows_select_kernel, one workgroup per window of the chunk, is nominate_select_kernel with the window's
// rows located through the slot, the flag OR-ed over the window's rows and the excluded song skipped.
//
// BYTE CONTRACT.  A window's outputs are a function of its rows, the database and the excluded song: not of hop, the window's
// position, its neighbours, the chunking, the grid or the run.
//
// The pieces are copies, the accepted precedent: dense.hip's and nominate.hip's code must not move (kernels.h).
#include "kernels.h"
#include "match_common.h"
#include <algorithm>

namespace pfann {

static constexpr int NW_T = 128;            // tile edge: recording rows and db rows
static constexpr int NW_NT = 256;           // 4 waves, 2 x 2, each 64 x 64 of the tile
static constexpr int NW_BK = 128;           // K (halves) per staging step
static constexpr int NW_LDK = NW_BK + 8;    // staging pitch (halves): 272 bytes, conflict-free b128 reads
static constexpr int NW_LDS = NW_T + 8;     // pitch of S (dwords)
static constexpr int NW_GRID = 2048;
static constexpr int NW_S_BYTES = NW_T * NW_LDS * 4;
static_assert(2 * NW_T * NW_LDK * 2 <= NW_S_BYTES, "the K tiles fit under S");

typedef _Float16 nw_f16x8 __attribute__((ext_vector_type(8)));
typedef float nw_f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ unsigned nw_ordered_bits(float t) {      // a > b  <=>  bits(a) > bits(b); never 0 for a number
    const unsigned u = __float_as_uint(t);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float nw_ordered_float(unsigned u) {
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}
__device__ __forceinline__ int nw_windows_of(int L, int window, int hop) {
    return L <= 0 ? 0 : (L < window ? 1 : (L - window) / hop + 1);
}
// first row of recording r in the call's row image: its first slot's rows, behind one halo per earlier recording
__device__ __forceinline__ int64_t nw_row_base(const NominateWindowsArgs &a, int64_t r, int SI) {
    return (a.wfirst[r] * a.hop / SI + r) * SI + r * (a.window - 1);
}
// what the call knows of recording r: its windows of the call, the rows of a window, the rows those windows read
__device__ __forceinline__ void nw_recording(const NominateWindowsArgs &a, int64_t r, int &nw, int &wl, int &used) {
    const int L = a.rlen[r];
    nw = (int)min((int64_t)nw_windows_of(L, a.window, a.hop), a.wfirst[r + 1] - a.wfirst[r]);
    wl = min(a.window, L);
    used = nw > 0 ? (nw - 1) * a.hop + wl : 0;           // <= L, and <= the room behind nw_row_base (kernels.h)
}

// One wave per row of the image: q_prep_kernel's arithmetic for a row that a window of the call reads, nothing for the spare
// rows behind a recording (no tile reads them).
__global__ void nominate_windows_prep_kernel(NominateWindowsArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= a.n_rows) return;
    const int SI = NW_T - (a.window - 1);
    int64_t lo = 0, hi = a.nR;                           // first recording whose rows start after `row`
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (nw_row_base(a, mid, SI) <= row) lo = mid + 1; else hi = mid;
    }
    const int64_t r = lo - 1;
    int nw, wl, used;
    nw_recording(a, r, nw, wl, used);
    const int64_t i = row - nw_row_base(a, r, SI);
    if (i >= used) return;
    const float *q = a.q + (a.rstart[r] + i) * (int64_t)a.d;
    _Float16 *qh = reinterpret_cast<_Float16 *>(a.qh) + row * a.d;
    float ss = 0.f;
    for (int e = lane; e < a.d; e += 64) {
        const float v = q[e];
        ss = fmaf(v, v, ss);
    }
    ss = wave_sum(ss);
    const bool bad = !(ss < 3.6e9f);                       // ||q|| >= 6e4 or NaN: outside fp16's range
    for (int e = lane; e < a.d; e += 64) qh[e] = bad ? (_Float16)0.f : (_Float16)q[e];
    if (lane == 0) {
        const float nq2 = sqrtf(ss);
        a.eps[row] = 1.05e-3f * nq2 * a.xnorm_max + 3.1e-8f * sqrtf((float)a.d) * (nq2 + a.xnorm_max);
        a.norm[row] = nq2;
        a.bad[row] = bad ? 1 : 0;
    }
}

__global__ __launch_bounds__(NW_NT) void nominate_windows_tile_kernel(NominateWindowsArgs a) {
    // S[NW_T][NW_LDS]; while the product runs its first bytes are the two K tiles As, Bs [NW_T][NW_LDK] of halves
    extern __shared__ __attribute__((aligned(16))) float s_S[];          // NW_S_BYTES, dynamic: past the static 64 KB
    __shared__ long long s_cpos[1024];
    __shared__ int s_song[NW_T];
    __shared__ int s_head[NW_T];
    __shared__ unsigned s_best[2 * NW_T];
    _Float16 *As = reinterpret_cast<_Float16 *>(s_S), *Bs = As + NW_T * NW_LDK;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, lhalf = lane >> 5;
    const int SI = NW_T - (a.window - 1);                // window starts / alignments a tile owns per edge
    const int64_t NJ = (a.ntotal + a.window - 1 + SI - 1) / SI;
    const int64_t n_items = a.slot_n * NJ;
    const _Float16 *qh = reinterpret_cast<const _Float16 *>(a.qh), *dbh = reinterpret_cast<const _Float16 *>(a.dbh);
    int cshift, n_coarse;
    load_coarse_song_pos<NW_NT>(a.song_pos, a.n_songs, s_cpos, tid, cshift, n_coarse);

    for (int64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int64_t jt = item / a.slot_n, slot = a.slot_lo + (item - jt * a.slot_n);   // neighbouring workgroups share the db tile
        int64_t lo = 0, hi = a.nR;                       // first recording whose slots start after `slot`
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (a.wfirst[mid] * a.hop / SI + mid <= slot) lo = mid + 1; else hi = mid;
        }
        const int64_t r = lo - 1;
        int nw, wl, used;
        nw_recording(a, r, nw, wl, used);
        const int64_t I0 = (slot - (a.wfirst[r] * a.hop / SI + r)) * SI;     // first recording row of the tile
        if (nw <= 0 || I0 > (int64_t)(nw - 1) * a.hop) continue;         // (the whole workgroup: a spare slot)
        const int64_t J0 = jt * SI - (a.window - 1);     // db row of the tile's column 0 (before the rows in the first tile)
        const int64_t Q0 = nw_row_base(a, r, SI) + I0;   // image row of the tile's row 0
        const int excl = a.excl != nullptr ? a.excl[r] : -1;
        const int i0 = (int)I0;

        if (tid < NW_T) {
            const int64_t g = J0 + tid;
            const int sg = g >= 0 && g < a.ntotal ? song_of_label(a.song_pos, a.n_songs, s_cpos, cshift, n_coarse, g) : -1;
            s_song[tid] = sg;
            // the song's first column in the tile (a column without a song: itself)
            s_head[tid] = sg >= 0 ? (int)max((int64_t)0, a.song_pos[sg] - J0) : tid;
            s_best[tid] = 0;
            s_best[NW_T + tid] = 0;
        }

        // ---- S = recording tile x db tile^T.  A row of a K block is 16 chunks of eight halves; thread tid stages chunk tid & 15
        // of the rows (tid >> 4) + 16 i, i < 8, of both operands
        nw_f32x16 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
        const int sc = tid & 15, sr = tid >> 4;
#pragma unroll 1
        for (int k0 = 0; k0 < a.d; k0 += NW_BK) {
            const int k = k0 + sc * 8;
            u32x4_t ra[8], rb[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int row = sr + 16 * i;
                const u32x4_t z = {0u, 0u, 0u, 0u};
                ra[i] = i0 + row < used && k < a.d ? *reinterpret_cast<const u32x4_t *>(qh + (Q0 + row) * a.d + k) : z;
                const int64_t g = J0 + row;
                rb[i] = g >= 0 && g < a.ntotal && k < a.d ? *reinterpret_cast<const u32x4_t *>(dbh + g * a.d + k) : z;
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int o = (sr + 16 * i) * NW_LDK + sc * 8;
                *reinterpret_cast<u32x4_t *>(&As[o]) = ra[i];
                *reinterpret_cast<u32x4_t *>(&Bs[o]) = rb[i];
            }
            __syncthreads();
            const int nkk = min(NW_BK / 16, (a.d - k0 + 15) / 16);       // MFMA steps of 16 k; lane half h holds k = 8h..8h+7
            for (int kk = 0; kk < nkk; ++kk) {
                nw_f16x8 a8[2], b8[2];
#pragma unroll
                for (int i = 0; i < 2; ++i)
                    a8[i] = *reinterpret_cast<const nw_f16x8 *>(&As[(wm * 64 + i * 32 + l31) * NW_LDK + kk * 16 + lhalf * 8]);
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    b8[j] = *reinterpret_cast<const nw_f16x8 *>(&Bs[(wn * 64 + j * 32 + l31) * NW_LDK + kk * 16 + lhalf * 8]);
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a8[i], b8[j], acc[i][j], 0, 0, 0);
            }
            __syncthreads();                             // the K tiles are read: the next block, or S, may overwrite them
        }
        // acc[i][j][e]: recording row (e & 3) + 8 * (e >> 2) + 4 * lhalf, db row l31 of the 32 x 32 block
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    s_S[(wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lhalf) * NW_LDS + wn * 64 + j * 32 + l31] = acc[i][j][e];
        __syncthreads();

        // ---- diagonals, per song: thread = column j, half h of the workgroup takes the (kb + h)-th live window start.  A
        // thread's FIRST piece (the song of column j) is reduced over the lanes of the same song by a segmented shuffle maximum
        // -- songs are contiguous in column order --, and the first lane of every run updates the half's table; later pieces
        // (the stretch crossed a song boundary) update it directly.  Then one global atomicMax per non-empty entry.
        {
            const int j = tid & (NW_T - 1), half = tid >> 7;
            unsigned *tab = s_best + half * NW_T;
            const int head0 = s_head[j];
            const int first_w = (i0 + a.hop - 1) / a.hop;            // the tile's first window start, in windows
            const int64_t ws_row0 = (slot - a.slot_lo) * a.wps;      // the chunk's workspace row of that window
            // live starts: windows first_w + k with (first_w + k) * hop < i0 + SI and first_w + k < nw
            const int n_live = max(0, min(nw - first_w, (i0 + SI - 1) / a.hop - first_w + 1));
            auto bits = [&](int cur, float tot) -> unsigned { return cur < 0 || cur == excl ? 0u : nw_ordered_bits(tot); };
            for (int kb = 0; kb < n_live; kb += NW_NT / NW_T) {
                const int k = kb + half;
                if (k < n_live) {                                    // (whole waves)
                    const int i = (first_w + k) * a.hop - i0;        // the window's first row in the tile, < SI
                    unsigned x0 = 0;
                    if (j < SI) {
                        int cur = s_song[j], head = head0;
                        bool first = true;
                        float tot = 0.f;
                        const float *Sp = s_S + i * NW_LDS + j;
                        for (int t = 0; t < wl; ++t) {
                            const int sg = s_song[j + t];
                            if (sg != cur) {
                                const unsigned x = bits(cur, tot);
                                if (first) x0 = x; else if (x != 0) atomicMax(&tab[head], x);
                                first = false;
                                cur = sg;
                                head = s_head[j + t];
                                tot = 0.f;
                            }
                            tot += Sp[t * (NW_LDS + 1)];
                        }
                        const unsigned x = bits(cur, tot);
                        if (first) x0 = x; else if (x != 0) atomicMax(&tab[head], x);
                    }
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) {               // lane l: the maximum of lanes l .. l + 2 o - 1 of its run
                        const unsigned v = __shfl_down(x0, o, 64);
                        const int hv = __shfl_down(head0, o, 64);
                        if (lane + o < 64 && hv == head0 && v > x0) x0 = v;
                    }
                    const int hp = __shfl_up(head0, 1, 64);
                    if ((lane == 0 || hp != head0) && x0 != 0) atomicMax(&tab[head0], x0);
                }
                __syncthreads();
                {
                    const unsigned x = tab[j];                       // entry j: the song whose first column is j
                    if (x != 0) {                                    // (only a half with a window start has any)
                        tab[j] = 0;
                        atomicMax(&a.ws[(ws_row0 + k) * a.n_songs + s_song[j]], x);
                    }
                }
                __syncthreads();                                     // the tables are empty again
            }
        }
        __syncthreads();                                 // S, the songs and the tables are free for the next tile
    }
}

// ---- ws -> the n best songs of every window of the chunk, n_found, n_close -------------------------------------------------
// One workgroup per (slot of the chunk, window start of the slot), located as dense_select_kernel locates it; a pair that is no
// window of the call ends at once.  The rest is nominate_select_kernel: key = (bits of A) << 32 | 0xFFFFFFFF - song, key
// order IS the ranking and keys are distinct, so the list is selected by comparing keys, never by arrival.
static constexpr int NW_SEL_NT = 256;

__global__ __launch_bounds__(NW_SEL_NT) void nominate_windows_select_kernel(NominateWindowsArgs a) {
    __shared__ unsigned long long s_max[2][NW_SEL_NT / 64];
    __shared__ unsigned long long s_first[NW_SEL_NT / 64];
    __shared__ int s_cnt[NW_SEL_NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int SI = NW_T - (a.window - 1);
    const int64_t slot = a.slot_lo + blockIdx.x / a.wps;
    const int kw = blockIdx.x % a.wps;
    int64_t lo = 0, hi = a.nR;                           // the recording of the slot, as in the tile kernel
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a.wfirst[mid] * a.hop / SI + mid <= slot) lo = mid + 1; else hi = mid;
    }
    const int64_t r = lo - 1;
    int nw, n, used;
    nw_recording(a, r, nw, n, used);
    const int64_t I0 = (slot - (a.wfirst[r] * a.hop / SI + r)) * SI;
    if (nw <= 0 || I0 > (int64_t)(nw - 1) * a.hop) return;               // (the whole workgroup, here and below)
    const int64_t wi = (I0 + a.hop - 1) / a.hop + kw;    // window of the recording
    if (wi * a.hop >= I0 + SI || wi >= nw) return;
    const int64_t w = a.wfirst[r] + wi;
    const int64_t row0 = nw_row_base(a, r, SI) + wi * a.hop;             // image row of the window's row 0
    const int excl = a.excl != nullptr ? a.excl[r] : -1;
    pfann_match_result *top = a.cand + w * a.n;
    pfann_match_result pad;
    pad.song = -1; pad.offset = 0; pad.shift = 0; pad.n_cand = 0; pad.score = -INFINITY;
    auto all_padding = [&](int code) {
        for (int i = tid; i < a.n; i += NW_SEL_NT) top[i] = pad;
        if (tid == 0) {
            if (a.n_found != nullptr) a.n_found[w] = code;
            if (a.n_close != nullptr) a.n_close[w] = code;
        }
    };
    int bad = 0;                                         // (every thread: a few broadcast loads)
    for (int t = 0; t < n; ++t) bad |= a.bad[row0 + t];
    if (bad != 0) { all_padding(-1); return; }
    const unsigned *row = a.ws + (int64_t)blockIdx.x * a.n_songs;
    auto word_of = [&](int s) -> unsigned { return s == excl ? 0u : row[s]; };   // (the tile kernel left the excluded song empty)
    auto key_of = [](unsigned x, int s) { return ((unsigned long long)x << 32) | (0xFFFFFFFFu - (unsigned)s); };

    unsigned long long mine = 0;                         // the largest key of this thread's songs not yet listed
    int cnt = 0;
    for (int s = tid; s < a.n_songs; s += NW_SEL_NT) {
        const unsigned x = word_of(s);
        if (x != 0) {
            ++cnt;
            const unsigned long long key = key_of(x, s);
            mine = key > mine ? key : mine;
        }
    }
    {
        unsigned long long best = mine;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long v = __shfl_xor(best, o, 64);
            best = v > best ? v : best;
            cnt += __shfl_xor(cnt, o, 64);
        }
        if (lane == 0) { s_first[wave] = best; s_cnt[wave] = cnt; }
    }
    __syncthreads();
    unsigned long long first = 0;
    int found = 0;
#pragma unroll
    for (int i = 0; i < NW_SEL_NT / 64; ++i) { first = s_first[i] > first ? s_first[i] : first; found += s_cnt[i]; }
    if (found == 0) { all_padding(0); return; }
    // the margin, in double from the fp32 values of the window's rows, in ascending t
    double se = 0.0, sn = 0.0;
    for (int t = 0; t < n; ++t) { se += (double)a.eps[row0 + t]; sn += (double)a.norm[row0 + t]; }
    const double E = se + 2.384185791015625e-07 * (double)(a.d + n) * ((double)a.xnorm_max * sn);        // 2^-22
    const double thr = (double)nw_ordered_float((unsigned)(first >> 32)) - 2.0 * E;
    int close = 0;
    for (int s = tid; s < a.n_songs; s += NW_SEL_NT) {
        const unsigned x = word_of(s);
        close += x != 0 && (double)nw_ordered_float(x) >= thr;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) close += __shfl_xor(close, o, 64);
    __syncthreads();                                     // s_cnt is read
    if (lane == 0) s_cnt[wave] = close;
    __syncthreads();
    if (tid == 0) {
        int c = 0;
        for (int i = 0; i < NW_SEL_NT / 64; ++i) c += s_cnt[i];
        if (a.n_found != nullptr) a.n_found[w] = found;
        if (a.n_close != nullptr) a.n_close[w] = c;
    }

    for (int e = 0; e < a.n; ++e) {
        unsigned long long best = mine;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long v = __shfl_xor(best, o, 64);
            best = v > best ? v : best;
        }
        if (lane == 0) s_max[e & 1][wave] = best;
        __syncthreads();                                 // (one per entry: the next entry writes the other row)
#pragma unroll
        for (int i = 0; i < NW_SEL_NT / 64; ++i) best = s_max[e & 1][i] > best ? s_max[e & 1][i] : best;
        if (best == 0) {                                 // no song left: padding
            for (int i = e + tid; i < a.n; i += NW_SEL_NT) top[i] = pad;
            return;
        }
        if (mine == best) {                              // keys are distinct: exactly one thread
            const int sg = (int)(0xFFFFFFFFu - (unsigned)best);
            pfann_match_result res;
            res.song = sg;
            res.offset = 0;
            res.shift = 0;
            res.n_cand = (int)(a.song_pos[sg + 1] - a.song_pos[sg]) + n - 1;
            res.score = (double)nw_ordered_float((unsigned)(best >> 32)) / (double)n;
            top[e] = res;
            mine = 0;
            if (e + 1 < a.n)
                for (int s = tid; s < a.n_songs; s += NW_SEL_NT) {
                    const unsigned x = word_of(s);
                    if (x == 0) continue;
                    const unsigned long long key = key_of(x, s);
                    if (key < best && key > mine) mine = key;
                }
        }
    }
}

// rows of the call's image: every slot's SI rows and one halo per recording (nw_row_base)
int64_t nominate_windows_rows(int64_t nW, int64_t nR, int window, int hop) {
    return dense_topn_slots(nW, nR, window, hop) * (NW_T - (window - 1)) + nR * (window - 1);
}
// bytes of the image with eps_t, ||q_t|| and the flags, 256-byte aligned: the chunk's ws lies behind them
size_t nominate_windows_image_bytes(int64_t n_rows, int d) {
    return (((size_t)n_rows * d * 2 + 15) / 16 * 16 + (size_t)n_rows * 12 + 255) / 256 * 256;
}
void nominate_windows_scratch_layout(NominateWindowsArgs &a, void *base) {
    char *p = reinterpret_cast<char *>(base);            // (256-byte aligned: fp16 rows are read 16 bytes at a time)
    a.qh = p;
    p += ((size_t)a.n_rows * a.d * 2 + 15) / 16 * 16;
    a.eps = reinterpret_cast<float *>(p);
    a.norm = a.eps + a.n_rows;
    a.bad = reinterpret_cast<int *>(a.norm + a.n_rows);
    a.ws = reinterpret_cast<unsigned *>(reinterpret_cast<char *>(base) + nominate_windows_image_bytes(a.n_rows, a.d));
}

// once per call, before its first chunk
int launch_nominate_windows_prep(const NominateWindowsArgs &a, hipStream_t s) {
    if (a.nR <= 0 || a.nW <= 0 || a.n_rows <= 0) return 0;
    ProfScope ps("seq_nominate_windows_prep", s, (double)a.n_rows * a.d * 6.0);
    PF_LAUNCH(nominate_windows_prep_kernel, dim3((unsigned)cdiv(a.n_rows, 4)), dim3(256), 0, s, a);
    PF_HIP(hipGetLastError());
    return 0;
}

// one chunk: the row-tile slots [slot_lo, slot_lo + slot_n) of the call
int launch_nominate_windows_dense(const NominateWindowsArgs &a, hipStream_t s) {
    if (a.nR <= 0 || a.nW <= 0 || a.slot_n <= 0) return 0;
    const int64_t rows = a.slot_n * a.wps;               // windows the chunk's slots can hold
    // every song's running best starts empty (0: no number has the ordered bits 0)
    if (a.n_songs > 0) PF_HIP(hipMemsetAsync(a.ws, 0, (size_t)rows * a.n_songs * sizeof(unsigned), s));
    if (a.ntotal > 0) {                                  // a database without rows: no tile
        const int SI = NW_T - (a.window - 1);
        const int64_t NJ = (a.ntotal + a.window - 1 + SI - 1) / SI;
        const int64_t n_items = a.slot_n * NJ;
        if (ensure_dyn_lds((const void *)nominate_windows_tile_kernel, NW_S_BYTES)) return -1;
        ProfScope ps("seq_nominate_windows_tiles", s, 2.0 * NW_T * NW_T * (double)n_items * a.d);
        PF_LAUNCH(nominate_windows_tile_kernel, dim3((unsigned)std::min<int64_t>(n_items, NW_GRID)), dim3(NW_NT), NW_S_BYTES, s, a);
        PF_HIP(hipGetLastError());
    }
    ProfScope ps("seq_nominate_windows_select", s, (double)rows * a.n_songs * 4.0);
    PF_LAUNCH(nominate_windows_select_kernel, dim3((unsigned)rows), dim3(NW_SEL_NT), 0, s, a);
    PF_HIP(hipGetLastError());
    return 0;
}

}  // namespace pfann
