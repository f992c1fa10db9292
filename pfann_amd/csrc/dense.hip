// Dense matcher: every alignment of every window, no top-k nomination (pfann_match_windows_dense).
//
// The dense answer of a window of n rows Q[0..n) is what pfann_match (mode 0, frame_shift_mul 1, score_alpha 0) returns
// for that slice when every row's label list is the whole database: candidates = every (song s with rows, offset o) with
// -(n-1) <= o <= len_s - 1, total(s, o) = sum over t with 0 <= o + t < len_s of dot(Q[t], db[song_pos[s] + o + t]),
// score = (double)total / (double)n, strict-> first-wins argmax in (song, offset) ascending order.
//
// One workgroup owns a TILE of DN_T consecutive rows of one recording x DN_T consecutive database rows:
//   -> S[i][j] = dot(recording row I0 + i, db row J0 + j) on v_mfma_f32_32x32x2_f32, K ascending; the tile stays in LDS
//   -> the tile owns the window starts i < DN_T - (window-1) and the alignments whose window row 0 meets db row J0 + j,
//      j < DN_T - (window-1): neighbouring tiles overlap by window-1 rows in both directions (the halo), so the whole
//      diagonal stretch S[i + t][j + t], t < n, of every owned (window, alignment) lies inside its tile.  db tiles start
//      at row -(window-1); rows outside the recording or the database are read as zeros and belong to no song
//   -> a stretch is cut where the song of db row J0 + j + t changes (song ids of the tile's columns: one lookup per column
//      in song_pos); every piece is the total of ONE candidate, (that song, o = J0 + j - song_pos[song]), and every
//      candidate of a window is one piece of exactly one stretch.  Songs shorter than the window put several pieces on
//      one stretch.  Pieces of the recording's excluded song are dropped here
//   -> per window start the largest packed word of the tile, then one 64-bit atomicMax into the window's result slot
//      (its 8-byte score field; the call zeroes it first), and a last small kernel decodes the words in place.
// Packed word: high half = the order-preserving bits of the fp32 total, low half = 0xFFFFFFFF - id with
//   id(s, o) = song_pos[s] + s * (n-1) + o + (n-1) = (db row of window row 0) + (s + 1) * (n-1),
// monotone in (song, offset): equal totals resolve to the first candidate in order, whichever tile arrives first.
// Comparing totals inside one window is comparing scores (one divisor, monotone), as in the ranked monitor kernel.
//
// SUMMATION ORDER.  A row dot is the MFMA's fmaf chain from +0 over k = 0, 1, .., d-1 (the K tile is stored in LDS so that
// step s of a group of eight reads k = 2 s and k = 2 s + 1); a total is tot = +0; tot += S[i + t][j + t] in ascending t,
// fp32; no sliding or prefix sums.
// BYTE CONTRACT.  A window's 24 result bytes are a function of the window's rows, the database and its recording's
// excluded song alone: not of hop, the other windows or recordings of the call, the tiling or the run.
//
// SONG-SHARDED (pfann_match_windows_dense_part / _merge, _topn_part / _topn_merge).  A candidate is (song, offset) and songs are
// never split, so it belongs to exactly one shard; its total adds rows of its own song only, so the shard computes the very
// float; and the id is formed from the GLOBAL song_pos, which every handle carries, so words of different shards compare as they
// do inside one handle: the maximum over the shards' words is the word the whole database leaves, ties included, and the sum of
// the shards' integer statistics is the whole sum.  N handles give the bytes of one (kernel: SHARD below; merges further down).
#include "kernels.h"
#include "match_common.h"
#include <algorithm>

namespace pfann {

static constexpr int DN_T = 128;            // tile edge: recording rows and db rows
static constexpr int DN_NT = 256;           // 4 waves, 2 x 2, each 64 x 64 of the tile
static constexpr int DN_BK = 32;            // K per staging step
static constexpr int DN_LDK = DN_BK + 4;    // staging pitch (dwords): conflict-free b128 reads
static constexpr int DN_LDS = DN_T + 8;     // pitch of S: the two half waves of an accumulator store hit disjoint banks
static constexpr int DN_GRID = 2048;
static constexpr int DN_S_BYTES = DN_T * DN_LDS * 4;

typedef float dn_f32x4 __attribute__((ext_vector_type(4)));
typedef float dn_f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ unsigned dn_ordered_bits(float t) {      // a > b  <=>  bits(a) > bits(b); never 0 for a number
    const unsigned u = __float_as_uint(t);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float dn_ordered_float(unsigned u) {
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}
__device__ __forceinline__ int dn_windows_of(int L, int window, int hop) {
    return L <= 0 ? 0 : (L < window ? 1 : (L - window) / hop + 1);
}

// RANKED (pfann_match_windows_dense_topn): the same tiles over the row-tile slots of one chunk; the pieces of a window start
// are reduced per SONG inside the tile -- s_best is then one table per half of the workgroup, indexed by the song's first
// column in the tile (s_head) -- and every non-empty entry goes out with one atomicMax into ws[window of the chunk][song].
//
// STATS (pfann_match_windows_dense_stats; with RANKED pfann_match_windows_dense_topn_stats): beside the maximum, the first two moments of the window's FULL pieces --
// stretches that no song boundary cuts, of a song that is not the excluded one: the candidates 0 <= o <= len_s - n.  A piece
// with fp32 total tot adds the integers 1, rint((double)tot * 2^24) and rint((double)tot * (double)tot * 2^18); both products
// are exact in double, so the rounding is the only rounding, and everything after it -- wave shuffles, one LDS entry per
// window start, one global 64-bit atomicAdd per non-zero entry -- is integer addition: the three sums of a window are, like
// its result bytes, a function of its rows, the database and the excluded song alone.  RANKED + STATS: a thread's stretch is a
// full piece exactly when the ranked walk never cut it (the unranked form's !cut), from the very tot that is packed into the
// word; only the window starts ib, ib + 1 are live at a time, so the LDS entries are one per half of the workgroup, and the
// global add goes to stats[wf + (i0 + i) / hop] -- the window of the CALL, not the chunk's workspace row: every (window, tile)
// pair belongs to one chunk, the call zeroes stats once before its first chunk.  Whole handles only.
//
// SHARD (pfann_match_windows_dense_part / _topn_part): the handle holds the global rows [row_lo, row_lo + nrows) of a song-sharded
// database, whole songs only, and the global song_pos.  The db tiles run over that range -- tile jt starts at global row
// row_lo + jt * SI - (window-1) --, rows outside it are zeros without a song (what a tile of the whole database reads past
// either end), and the song lookup, s_head and the id stay global: a candidate belongs to exactly one shard and gets there the
// word it gets from the whole database.  The unranked form leaves the raw words (no decode), the ranked form indexes its
// workspace by song - song_lo.  No new LDS; the instantiations without SHARD are the code they were before it existed.
//
// All seven instantiations take the one DenseArgs (kernels.h) and read only the groups of their form; launch_dense_unranked and
// launch_dense_ranked, further down, pick the instantiation from (shard, stats != nullptr).
template <bool RANKED, bool STATS = false, bool SHARD = false>
__global__ __launch_bounds__(DN_NT) void match_windows_dense_kernel(DenseArgs a) {
    static_assert(!(RANKED && STATS && SHARD), "the ranked moments are kept by whole handles");
    // S[DN_T][DN_LDS]; while the product runs its first bytes are the two K tiles As, Bs [DN_T][DN_LDK]
    extern __shared__ __attribute__((aligned(16))) float s_S[];          // DN_S_BYTES, dynamic: past the static 64 KB
    __shared__ long long s_cpos[1024];
    __shared__ int s_song[DN_T];
    __shared__ int s_head[RANKED ? DN_T : 1];
    __shared__ unsigned long long s_best[RANKED ? 2 * DN_T : DN_T];
    // per window start of the tile: sum_q, sumsq_q and the number of full pieces (at most DN_T: 20 bytes per start); RANKED: per
    // half of the workgroup (its one live window start)
    __shared__ unsigned long long s_sum[STATS ? (RANKED ? 2 * (DN_NT / DN_T) : 2 * DN_T) : 1];
    __shared__ int s_full[STATS ? (RANKED ? DN_NT / DN_T : DN_T) : 1];
    static_assert(2 * DN_T * DN_LDK <= DN_T * DN_LDS, "the K tiles fit under S");
    float *As = s_S, *Bs = s_S + DN_T * DN_LDK;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, lhalf = lane >> 5;
    const int SI = DN_T - (a.window - 1);                // window starts / alignments a tile owns per edge
    const int64_t n_slots = a.nW * a.hop / SI + a.nR;    // recording r owns the row-tile slots from wfirst[r] * hop / SI + r
    int64_t row_lo = 0, row_n = a.ntotal;                // the global rows this handle holds
    if constexpr (SHARD) { row_lo = a.row_lo; row_n = a.nrows; }
    const int64_t NJ = (row_n + a.window - 1 + SI - 1) / SI;
    int64_t slot_lo = 0, slot_n = n_slots;
    if constexpr (RANKED) { slot_lo = a.slot_lo; slot_n = a.slot_n; }
    const int64_t n_items = slot_n * NJ;
    int cshift, n_coarse;
    load_coarse_song_pos<DN_NT>(a.song_pos, a.n_songs, s_cpos, tid, cshift, n_coarse);

    for (int64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int64_t jt = item / slot_n, slot = slot_lo + (item - jt * slot_n);   // neighbouring workgroups share the db tile
        int64_t lo = 0, hi = a.nR;                       // first recording whose slots start after `slot`
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (a.wfirst[mid] * a.hop / SI + mid <= slot) lo = mid + 1; else hi = mid;
        }
        const int64_t r = lo - 1;
        const int L = a.rlen[r];
        const int64_t wf = a.wfirst[r];
        const int nw = (int)min((int64_t)dn_windows_of(L, a.window, a.hop), a.wfirst[r + 1] - wf);
        const int64_t I0 = (slot - (wf * a.hop / SI + r)) * SI;          // first recording row of the tile
        if (nw <= 0 || I0 > (int64_t)(nw - 1) * a.hop) continue;         // (the whole workgroup: a spare slot)
        const int wl = min(a.window, L);                 // rows of a window: `window`, or all rows of a shorter recording
        const int64_t J0 = row_lo + jt * SI - (a.window - 1);   // db row of the tile's column 0 (before the rows in the first tile)
        const int excl = a.excl != nullptr ? a.excl[r] : -1;
        const int i0 = (int)I0;

        if (tid < DN_T) {
            const int64_t g = J0 + tid;
            s_song[tid] = g >= row_lo && g < row_lo + row_n ? song_of_label(a.song_pos, a.n_songs, s_cpos, cshift, n_coarse, g) : -1;
            s_best[tid] = 0;
            if constexpr (RANKED) {                      // the song's first column in the tile (a column without a song: itself)
                const int sg = s_song[tid];
                s_head[tid] = sg >= 0 ? (int)max((int64_t)0, a.song_pos[sg] - J0) : tid;
                s_best[DN_T + tid] = 0;
            }
            if constexpr (STATS && !RANKED) { s_sum[2 * tid] = 0; s_sum[2 * tid + 1] = 0; s_full[tid] = 0; }
            if constexpr (STATS && RANKED) {
                if (tid < DN_NT / DN_T) { s_sum[2 * tid] = 0; s_sum[2 * tid + 1] = 0; s_full[tid] = 0; }
            }
        }

        // ---- S = Q tile x db tile^T.  Thread tid stages rows (tid >> 2) and (tid >> 2) + 64 of both operands, eight
        // consecutive k (two float4) at 8 * (tid & 3) of every K step
        const int srow = tid >> 2, sk8 = (tid & 3) * 8;
        const float *qp[2], *dp[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int row = srow + 64 * u;
            qp[u] = i0 + row < L ? a.q + (a.rstart[r] + i0 + row) * (int64_t)a.d : nullptr;
            const int64_t g = J0 + row;
            dp[u] = g >= row_lo && g < row_lo + row_n ? a.db + (g - row_lo) * (int64_t)a.d : nullptr;
        }
        dn_f32x4 ra[2][2], rb[2][2];
        auto load_tile = [&](int k0) {
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int k = k0 + sk8 + 4 * h;
                    const dn_f32x4 z = {0.f, 0.f, 0.f, 0.f};
                    ra[u][h] = qp[u] != nullptr && k < a.d ? *reinterpret_cast<const dn_f32x4 *>(qp[u] + k) : z;
                    rb[u][h] = dp[u] != nullptr && k < a.d ? *reinterpret_cast<const dn_f32x4 *>(dp[u] + k) : z;
                }
        };
        // position 4 * half + s of a group of eight holds k = 2 * s + half: the half wave that supplies the MFMA's k = half
        // reads one b128 and steps s = 0..3 walk k in ascending order
        auto store_tile = [&]() {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int o = (srow + 64 * u) * DN_LDK + sk8;
                const dn_f32x4 ae = {ra[u][0][0], ra[u][0][2], ra[u][1][0], ra[u][1][2]};
                const dn_f32x4 ao = {ra[u][0][1], ra[u][0][3], ra[u][1][1], ra[u][1][3]};
                const dn_f32x4 be = {rb[u][0][0], rb[u][0][2], rb[u][1][0], rb[u][1][2]};
                const dn_f32x4 bo = {rb[u][0][1], rb[u][0][3], rb[u][1][1], rb[u][1][3]};
                *reinterpret_cast<dn_f32x4 *>(&As[o]) = ae;
                *reinterpret_cast<dn_f32x4 *>(&As[o + 4]) = ao;
                *reinterpret_cast<dn_f32x4 *>(&Bs[o]) = be;
                *reinterpret_cast<dn_f32x4 *>(&Bs[o + 4]) = bo;
            }
        };
        dn_f32x16 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
        const int nk = (a.d + DN_BK - 1) / DN_BK;
        load_tile(0);
#pragma unroll 1
        for (int kt = 0; kt < nk; ++kt) {
            store_tile();
            __syncthreads();
            if (kt + 1 < nk) load_tile((kt + 1) * DN_BK);
#pragma unroll
            for (int kk = 0; kk < DN_BK / 8; ++kk) {
                dn_f32x4 a4[2], b4[2];
#pragma unroll
                for (int i = 0; i < 2; ++i)
                    a4[i] = *reinterpret_cast<const dn_f32x4 *>(&As[(wm * 64 + i * 32 + l31) * DN_LDK + kk * 8 + lhalf * 4]);
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    b4[j] = *reinterpret_cast<const dn_f32x4 *>(&Bs[(wn * 64 + j * 32 + l31) * DN_LDK + kk * 8 + lhalf * 4]);
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < 2; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[i][s], b4[j][s], acc[i][j], 0, 0, 0);
            }
            __syncthreads();                             // the K tiles are read: the next step, or S, may overwrite them
        }
        // acc[i][j][e]: recording row (e & 3) + 8 * (e >> 2) + 4 * lhalf, db row l31 of the 32 x 32 block
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    s_S[(wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lhalf) * DN_LDS + wn * 64 + j * 32 + l31] = acc[i][j][e];
        __syncthreads();

        if constexpr (RANKED) {
            // ---- diagonals, per song: thread = column j, half h of the workgroup takes window start ib + h.  A thread's FIRST
            // piece (the song of column j) is reduced over the lanes of the same song by a segmented shuffle maximum -- songs
            // are contiguous in column order --, and the first lane of every run updates the half's table; later pieces
            // (the stretch crossed a song boundary) update it directly.  Then one global atomicMax per non-empty entry.
            const int j = tid & (DN_T - 1), half = tid >> 7;
            const int64_t g = J0 + j;
            unsigned long long *tab = s_best + half * DN_T;
            const int head0 = s_head[j];
            const int first_w = (i0 + a.hop - 1) / a.hop;            // the tile's first window start, in windows
            const int64_t ws_row0 = (slot - slot_lo) * a.wps - first_w;
            auto starts = [&](int i) { const int w0 = i0 + i; return i < SI && w0 % a.hop == 0 && w0 / a.hop < nw; };
            auto packed = [&](int cur, float tot) -> unsigned long long {
                if (cur < 0 || cur == excl) return 0;
                const unsigned id = (unsigned)(g + (int64_t)(cur + 1) * (wl - 1));
                return ((unsigned long long)dn_ordered_bits(tot) << 32) | (0xFFFFFFFFu - id);
            };
            for (int ib = 0; ib < SI; ib += DN_NT / DN_T) {
                const bool act0 = starts(ib), act1 = starts(ib + 1);
                if (!act0 && !act1) continue;                        // (the whole workgroup)
                const int i = ib + half;
                if (half ? act1 : act0) {                            // (whole waves)
                    unsigned long long x0 = 0;
                    [[maybe_unused]] int full = 0;                   // STATS: this thread's stretch is a full piece
                    [[maybe_unused]] long long sum = 0, sumsq = 0;
                    if (j < SI) {
                        int cur = s_song[j], head = head0;
                        bool first = true;
                        float tot = 0.f;
                        for (int t = 0; t < wl; ++t) {
                            const int sg = s_song[j + t];
                            if (sg != cur) {
                                const unsigned long long x = packed(cur, tot);
                                if (first) x0 = x; else if (x != 0) atomicMax(&tab[head], x);
                                first = false;
                                cur = sg;
                                head = s_head[j + t];
                                tot = 0.f;
                            }
                            tot += s_S[(i + t) * DN_LDS + j + t];
                        }
                        const unsigned long long x = packed(cur, tot);
                        if (first) x0 = x; else if (x != 0) atomicMax(&tab[head], x);
                        if constexpr (STATS) {
                            if (first && x != 0) {                   // never cut, a song, not the excluded one
                                const double td = (double)tot;
                                full = 1;
                                sum = __double2ll_rn(td * 16777216.0);           // 2^PFANN_DENSE_STATS_SUM_SHIFT
                                sumsq = __double2ll_rn(td * td * 262144.0);      // 2^PFANN_DENSE_STATS_SQ_SHIFT
                            }
                        }
                    }
                    if constexpr (STATS) {
#pragma unroll
                        for (int o = 32; o > 0; o >>= 1) {
                            full += __shfl_xor(full, o, 64);
                            sum += __shfl_xor(sum, o, 64);
                            sumsq += __shfl_xor(sumsq, o, 64);
                        }
                        if (lane == 0 && full != 0) {
                            atomicAdd(&s_full[half], full);
                            atomicAdd(&s_sum[2 * half], (unsigned long long)sum);
                            atomicAdd(&s_sum[2 * half + 1], (unsigned long long)sumsq);
                        }
                    }
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) {               // lane l: the maximum of lanes l .. l + 2 o - 1 of its run
                        const unsigned long long v = __shfl_down(x0, o, 64);
                        const int hv = __shfl_down(head0, o, 64);
                        if (lane + o < 64 && hv == head0 && v > x0) x0 = v;
                    }
                    const int hp = __shfl_up(head0, 1, 64);
                    if ((lane == 0 || hp != head0) && x0 != 0) atomicMax(&tab[head0], x0);
                }
                __syncthreads();
                {
                    const unsigned long long x = tab[j];             // entry j: the song whose first column is j
                    if (x != 0) {                                    // (only a half with a window start has any)
                        tab[j] = 0;
                        if constexpr (SHARD) atomicMax(&a.ws[(ws_row0 + (i0 + i) / a.hop) * a.n_owned + (s_song[j] - a.song_lo)], x);
                        else atomicMax(&a.ws[(ws_row0 + (i0 + i) / a.hop) * a.n_songs + s_song[j]], x);
                    }
                }
                if constexpr (STATS) {
                    if (j == 0) {                                    // the half's entry: the window of the CALL, wf + (i0 + i) / hop
                        const int nf = s_full[half];
                        if (nf != 0) {                               // (only a half with a window start has any)
                            unsigned long long *st = reinterpret_cast<unsigned long long *>(&a.stats[wf + (i0 + i) / a.hop]);
                            atomicAdd(&st[0], (unsigned long long)nf);
                            if (s_sum[2 * half] != 0) atomicAdd(&st[1], s_sum[2 * half]);
                            if (s_sum[2 * half + 1] != 0) atomicAdd(&st[2], s_sum[2 * half + 1]);
                            s_full[half] = 0; s_sum[2 * half] = 0; s_sum[2 * half + 1] = 0;
                        }
                    }
                }
                __syncthreads();                                     // the tables are empty again
            }
        } else {
            // ---- diagonals: thread = column j, the two halves of the workgroup take the window starts in turn (wave-uniform i)
            {
                const int j = tid & (DN_T - 1);
                const int64_t g = J0 + j;
                for (int i = tid >> 7; i < SI; i += DN_NT / DN_T) {
                    const int w0 = i0 + i;
                    if (w0 % a.hop != 0 || w0 / a.hop >= nw) continue;       // not a window start of this recording
                    unsigned long long best = 0;
                    [[maybe_unused]] int full = 0;                           // STATS: this thread's stretch is a full piece
                    [[maybe_unused]] long long sum = 0, sumsq = 0;
                    if (j < SI) {
                        int cur = s_song[j];
                        [[maybe_unused]] bool cut = false;
                        float tot = 0.f;
                        for (int t = 0; t < wl; ++t) {
                            const int sg = s_song[j + t];
                            if (sg != cur) {
                                if (cur >= 0 && cur != excl) {
                                    const unsigned id = (unsigned)(g + (int64_t)(cur + 1) * (wl - 1));
                                    const unsigned long long x = ((unsigned long long)dn_ordered_bits(tot) << 32) | (0xFFFFFFFFu - id);
                                    best = x > best ? x : best;
                                }
                                cur = sg;
                                tot = 0.f;
                                if constexpr (STATS) cut = true;
                            }
                            tot += s_S[(i + t) * DN_LDS + j + t];
                        }
                        if (cur >= 0 && cur != excl) {
                            const unsigned id = (unsigned)(g + (int64_t)(cur + 1) * (wl - 1));
                            const unsigned long long x = ((unsigned long long)dn_ordered_bits(tot) << 32) | (0xFFFFFFFFu - id);
                            best = x > best ? x : best;
                            if constexpr (STATS) {
                                if (!cut) {
                                    const double td = (double)tot;
                                    full = 1;
                                    sum = __double2ll_rn(td * 16777216.0);           // 2^PFANN_DENSE_STATS_SUM_SHIFT
                                    sumsq = __double2ll_rn(td * td * 262144.0);      // 2^PFANN_DENSE_STATS_SQ_SHIFT
                                }
                            }
                        }
                    }
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) {
                        const unsigned long long v = __shfl_xor(best, o, 64);
                        best = v > best ? v : best;
                        if constexpr (STATS) {
                            full += __shfl_xor(full, o, 64);
                            sum += __shfl_xor(sum, o, 64);
                            sumsq += __shfl_xor(sumsq, o, 64);
                        }
                    }
                    if (lane == 0 && best != 0) atomicMax(&s_best[i], best);
                    if constexpr (STATS) {
                        if (lane == 0 && full != 0) {
                            atomicAdd(&s_full[i], full);
                            atomicAdd(&s_sum[2 * i], (unsigned long long)sum);
                            atomicAdd(&s_sum[2 * i + 1], (unsigned long long)sumsq);
                        }
                    }
                }
            }
            __syncthreads();
            if (tid < SI) {
                const unsigned long long x = s_best[tid];
                if (x != 0) {                                // (only window starts of the recording ever get a word)
                    const int64_t w = wf + (i0 + tid) / a.hop;
                    if constexpr (SHARD) atomicMax(&a.words[w], x);
                    else atomicMax(reinterpret_cast<unsigned long long *>(&a.results[w].score), x);
                    if constexpr (STATS) {
                        const int nf = s_full[tid];
                        if (nf != 0) {                       // (a full piece is a candidate: x != 0 wherever there is one)
                            unsigned long long *st = reinterpret_cast<unsigned long long *>(&a.stats[w]);
                            atomicAdd(&st[0], (unsigned long long)nf);
                            if (s_sum[2 * tid] != 0) atomicAdd(&st[1], s_sum[2 * tid]);
                            if (s_sum[2 * tid + 1] != 0) atomicAdd(&st[2], s_sum[2 * tid + 1]);
                        }
                    }
                }
            }
        }
        __syncthreads();                                 // S, the songs and the maxima are free for the next tile
    }
}

// the recording of window w, the rows n of its windows and its excluded song (Args: anything with nR, wfirst, rlen, window, excl)
template <class Args>
__device__ __forceinline__ void dn_window_of(const Args &a, int64_t w, int &n, int &excl) {
    int64_t lo = 0, hi = a.nR - 1;                       // first recording whose windows end after w
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a.wfirst[mid + 1] <= w) lo = mid + 1; else hi = mid;
    }
    n = min(a.window, a.rlen[lo]);
    excl = a.excl != nullptr ? a.excl[lo] : -1;
}

// a window's packed word -> its result.  n_cand = sum over songs with rows (without the excluded one) of len_s + n - 1; ntotal,
// song_pos and songs_with_rows are those of the WHOLE database
__device__ __forceinline__ pfann_match_result dn_decode_word(unsigned long long x, int n, int excl, const int64_t *song_pos,
                                                             int n_songs, int64_t ntotal, int64_t songs_with_rows) {
    int64_t ncand = ntotal + songs_with_rows * (n - 1);
    if (excl >= 0 && excl < n_songs) {
        const int64_t len = song_pos[excl + 1] - song_pos[excl];
        if (len > 0) ncand -= len + n - 1;
    }
    pfann_match_result res;
    if (x != 0) {
        const int64_t id = (int64_t)(0xFFFFFFFFu - (unsigned)x);
        int sl = 0, sh = n_songs;                        // largest s with song_pos[s] + s * (n-1) <= id
        while (sl < sh) {
            const int mid = (sl + sh) >> 1;
            if (song_pos[mid] + (int64_t)mid * (n - 1) <= id) sl = mid + 1; else sh = mid;
        }
        const int s = sl - 1;
        res.song = s;
        res.offset = (int)(id - song_pos[s] - (int64_t)(s + 1) * (n - 1));
        res.shift = 0;
        res.n_cand = (int)ncand;
        res.score = (double)dn_ordered_float((unsigned)(x >> 32)) / (double)n;
    } else {
        res.song = -1; res.offset = 0; res.shift = 0; res.n_cand = 0; res.score = -INFINITY;
    }
    return res;
}

// packed words -> results, in place
__global__ void dense_decode_kernel(DenseArgs a, int64_t songs_with_rows) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= a.nW) return;
    int n, excl;
    dn_window_of(a, w, n, excl);
    const unsigned long long x = *reinterpret_cast<const unsigned long long *>(&a.results[w].score);
    a.results[w] = dn_decode_word(x, n, excl, a.song_pos, a.n_songs, a.ntotal, songs_with_rows);
}

// pfann_match_windows_dense_merge, one thread per window: the largest word of the parts (ids are global, so it is the word the
// whole database leaves in the slot, ties included), the sum of the parts' integers (every full candidate is in exactly one
// part), and dense_decode_kernel's decode
__global__ void dense_merge_kernel(DenseMergeArgs a) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= a.nW) return;
    int n, excl;
    dn_window_of(a, w, n, excl);
    unsigned long long x = 0;
    for (int p = 0; p < a.n_parts; ++p) {
        const unsigned long long v = a.words[(int64_t)p * a.nW + w];
        x = v > x ? v : x;
    }
    a.results[w] = dn_decode_word(x, n, excl, a.song_pos, a.n_songs, a.ntotal, a.songs_with_rows);
    if (a.stats != nullptr) {
        unsigned long long nf = 0, sum = 0, sumsq = 0;   // two's complement: unsigned addition
        for (int p = 0; p < a.n_parts; ++p) {
            const pfann_dense_stats st = a.part_stats[(int64_t)p * a.nW + w];
            nf += (unsigned long long)st.n_full; sum += (unsigned long long)st.sum_q; sumsq += (unsigned long long)st.sumsq_q;
        }
        pfann_dense_stats out;
        out.n_full = (int64_t)nf; out.sum_q = (int64_t)sum; out.sumsq_q = (int64_t)sumsq;
        a.stats[w] = out;
    }
}

int launch_dense_merge(const DenseMergeArgs &a, hipStream_t s) {
    if (a.nR <= 0 || a.nW <= 0) return 0;
    ProfScope ps("seq_dense_merge", s, (double)a.nW * a.n_parts * (a.stats != nullptr ? 32.0 : 8.0));
    PF_LAUNCH(dense_merge_kernel, dim3((unsigned)cdiv(a.nW, 256)), dim3(256), 0, s, a);
    PF_HIP(hipGetLastError());
    return 0;
}

// the tile kernel of one form over the rows this handle holds; work_rows: the recording rows of the profile's figure
template <bool RANKED, bool STATS, bool SHARD>
static int launch_dense_tiles(const DenseArgs &a, int64_t slot_n, const char *tag, double work_rows, hipStream_t s) {
    const int64_t rows = SHARD ? a.nrows : a.ntotal;
    if (rows <= 0) return 0;                             // a database or a shard without rows: no tile
    const int SI = DN_T - (a.window - 1);
    const int64_t NJ = (rows + a.window - 1 + SI - 1) / SI;
    const int64_t n_items = slot_n * NJ;
    const auto kernel = match_windows_dense_kernel<RANKED, STATS, SHARD>;
    if (ensure_dyn_lds((const void *)kernel, DN_S_BYTES)) return -1;
    ProfScope ps(tag, s, 2.0 * work_rows * (double)rows * a.d);
    PF_LAUNCH(kernel, dim3((unsigned)std::min<int64_t>(n_items, DN_GRID)), dim3(DN_NT), DN_S_BYTES, s, a);
    PF_HIP(hipGetLastError());
    return 0;
}

// the unranked forms.  A whole handle's words are decoded in place; a shard's stay raw: pfann_match_windows_dense_merge decodes
// the maximum over all parts
int launch_dense_unranked(const DenseArgs &a, bool shard, int64_t songs_with_rows, hipStream_t s) {
    if (a.nR <= 0 || a.nW <= 0) return 0;
    // every slot's running best starts empty (word 0: no number has the ordered bits 0)
    if (shard) PF_HIP(hipMemsetAsync(a.words, 0, (size_t)a.nW * sizeof(unsigned long long), s));
    else PF_HIP(hipMemsetAsync(a.results, 0, (size_t)a.nW * sizeof(pfann_match_result), s));
    const bool stats = a.stats != nullptr;
    if (stats) PF_HIP(hipMemsetAsync(a.stats, 0, (size_t)a.nW * sizeof(pfann_dense_stats), s));
    const int64_t n_slots = dense_topn_slots(a.nW, a.nR, a.window, a.hop);
    const double work = (double)a.nW * a.hop + (double)a.nR * a.window;
    int rc;
    if (shard) rc = stats ? launch_dense_tiles<false, true, true>(a, n_slots, "seq_match_windows_dense_part", work, s)
                          : launch_dense_tiles<false, false, true>(a, n_slots, "seq_match_windows_dense_part", work, s);
    else rc = stats ? launch_dense_tiles<false, true, false>(a, n_slots, "seq_match_windows_dense_stats", work, s)
                    : launch_dense_tiles<false, false, false>(a, n_slots, "seq_match_windows_dense", work, s);
    if (rc || shard) return rc;
    PF_LAUNCH(dense_decode_kernel, dim3((unsigned)cdiv(a.nW, 256)), dim3(256), 0, s, a, songs_with_rows);
    PF_HIP(hipGetLastError());
    return 0;
}

// ---- ranked: ws -> the n best songs of every window of the chunk (pfann_match_windows_dense_topn) --------------------------
// One workgroup per (slot of the chunk, window start of the slot); a pair that is no window of the call ends at once.  A
// song's word holds its best candidate; word order IS the ranking (higher total first, equal totals to the smaller id: the
// lower song), and words are distinct, so the lists are selected by comparing words, never by arrival: every thread keeps
// the largest word of its strided share of the songs, the workgroup's maximum is the next entry, and the thread that held
// it looks for its next largest word below it.
static constexpr int DN_SEL_NT = 256;

// SHARD: the words of the handle's owned songs, ws[..][song - song_lo]; entries carry the global song; no per-song block.
template <bool SHARD>
__global__ __launch_bounds__(DN_SEL_NT) void dense_select_kernel(DenseArgs a) {
    __shared__ unsigned long long s_max[2][DN_SEL_NT / 64];
    __shared__ int s_cnt[DN_SEL_NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int SI = DN_T - (a.window - 1);
    const int64_t slot = a.slot_lo + blockIdx.x / a.wps;
    const int kw = blockIdx.x % a.wps;
    int64_t lo = 0, hi = a.nR;                           // the recording of the slot, as in the tile kernel
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a.wfirst[mid] * a.hop / SI + mid <= slot) lo = mid + 1; else hi = mid;
    }
    const int64_t r = lo - 1;
    const int L = a.rlen[r];
    const int64_t wf = a.wfirst[r];
    const int nw = (int)min((int64_t)dn_windows_of(L, a.window, a.hop), a.wfirst[r + 1] - wf);
    const int64_t I0 = (slot - (wf * a.hop / SI + r)) * SI;
    if (nw <= 0 || I0 > (int64_t)(nw - 1) * a.hop) return;
    const int64_t wi = (I0 + a.hop - 1) / a.hop + kw;    // window of the recording
    if (wi * a.hop >= I0 + SI || wi >= nw) return;
    const int64_t w = wf + wi;
    const int n = min(a.window, L);
    int s_base = 0, n_sel = a.n_songs;                   // the songs of the workspace: mine_s and s below are song - s_base
    if constexpr (SHARD) { s_base = a.song_lo; n_sel = a.n_owned; }
    const unsigned long long *row = a.ws + (int64_t)blockIdx.x * n_sel;
    pfann_match_result *top = a.top + w * a.n;
    auto offset_of = [&](unsigned long long x, int s) {
        return (int)((int64_t)(0xFFFFFFFFu - (unsigned)x) - a.song_pos[s] - (int64_t)(s + 1) * (n - 1));
    };
    auto score_of = [&](unsigned long long x) { return (double)dn_ordered_float((unsigned)(x >> 32)) / (double)n; };

    unsigned long long mine = 0;                         // the largest word of this thread's songs not yet listed
    int mine_s = -1, cnt = 0;
    for (int s = tid; s < n_sel; s += DN_SEL_NT) {
        const unsigned long long x = row[s];
        cnt += x != 0;
        if (x > mine) { mine = x; mine_s = s; }
        if constexpr (!SHARD) {
            if (a.song_scores != nullptr) {              // the reference's block records only scores above its zeros
                const float f = x != 0 ? (float)score_of(x) : 0.f;
                float2 v = {0.f, 0.f};
                if (f > 0.f) { v.x = f; v.y = (float)offset_of(x, s); }
                reinterpret_cast<float2 *>(a.song_scores)[w * a.n_songs + s] = v;
            }
        }
    }
    if (a.n_found != nullptr) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
        if (lane == 0) s_cnt[wave] = cnt;
        __syncthreads();
        if (tid == 0) {
            int c = 0;
            for (int i = 0; i < DN_SEL_NT / 64; ++i) c += s_cnt[i];
            a.n_found[w] = c;
        }
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
        for (int i = 0; i < DN_SEL_NT / 64; ++i) best = s_max[e & 1][i] > best ? s_max[e & 1][i] : best;
        if (best == 0) {                                 // no song left: padding
            for (int i = e + tid; i < a.n; i += DN_SEL_NT) {
                pfann_match_result res;
                res.song = -1; res.offset = 0; res.shift = 0; res.n_cand = 0; res.score = -INFINITY;
                top[i] = res;
            }
            return;
        }
        if (mine == best) {                              // words are distinct: exactly one thread
            pfann_match_result res;
            const int sg = s_base + mine_s;
            res.song = sg;
            res.offset = offset_of(best, sg);
            res.shift = 0;
            res.n_cand = (int)(a.song_pos[sg + 1] - a.song_pos[sg]) + n - 1;
            res.score = score_of(best);
            top[e] = res;
            mine = 0; mine_s = -1;
            if (e + 1 < a.n)
                for (int s = tid; s < n_sel; s += DN_SEL_NT) {
                    const unsigned long long x = row[s];
                    if (x < best && x > mine) { mine = x; mine_s = s; }
                }
        }
    }
}

int dense_topn_wps(int window, int hop) { return (DN_T - (window - 1) + hop - 1) / hop; }
int64_t dense_topn_slots(int64_t nW, int64_t nR, int window, int hop) { return nW * hop / (DN_T - (window - 1)) + nR; }

int launch_dense_ranked(const DenseArgs &a, bool shard, hipStream_t s) {
    if (a.nR <= 0 || a.nW <= 0 || a.slot_n <= 0) return 0;
    const int64_t rows = a.slot_n * a.wps;               // windows the chunk's slots can hold
    const int songs = shard ? a.n_owned : a.n_songs;
    if (songs > 0) PF_HIP(hipMemsetAsync(a.ws, 0, (size_t)rows * songs * sizeof(unsigned long long), s));
    const double work = (double)a.slot_n * DN_T;
    int rc;
    if (shard) rc = launch_dense_tiles<true, false, true>(a, a.slot_n, "seq_match_windows_dense_topn_part", work, s);
    else rc = a.stats != nullptr ? launch_dense_tiles<true, true, false>(a, a.slot_n, "seq_match_windows_dense_topn_stats", work, s)
                                 : launch_dense_tiles<true, false, false>(a, a.slot_n, "seq_match_windows_dense_topn", work, s);
    if (rc) return -1;
    ProfScope ps("seq_dense_select", s, (double)rows * songs * 8.0);
    if (shard) PF_LAUNCH(dense_select_kernel<true>, dim3((unsigned)rows), dim3(DN_SEL_NT), 0, s, a);
    else PF_LAUNCH(dense_select_kernel<false>, dim3((unsigned)rows), dim3(DN_SEL_NT), 0, s, a);
    PF_HIP(hipGetLastError());
    return 0;
}

// pfann_match_windows_dense_topn_merge, one wave per window: the n best of the parts' n_parts * n entries by score descending,
// then song ascending, padding last.  This IS the word order of the whole database's select: (double)total / (double)n_rows is
// injective on fp32 totals for n_rows <= 64 (the quotient of two different floats by a divisor below 2^7 keeps more than the 24
// bits that tell them apart), so equal scores are equal totals, and between different songs the smaller id is the lower song;
// the songs of different parts are disjoint, so every (score, song) is there once.  Entry e = the best entry after entry e-1.
static constexpr int DN_MRG_NT = 256;

__global__ __launch_bounds__(DN_MRG_NT) void dense_topn_merge_kernel(const pfann_match_result *tops, const int32_t *nf_parts,
                                                                     int n_parts, int64_t nW, int n, pfann_match_result *top,
                                                                     int32_t *n_found) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * (DN_MRG_NT / 64) + (threadIdx.x >> 6);
    if (w >= nW) return;                                 // (whole waves; no barrier below)
    const int E = n_parts * n;
    auto entry = [&](int i) -> const pfann_match_result & {
        const int p = i / n;
        return tops[((int64_t)p * nW + w) * n + (i - p * n)];
    };
    auto before = [](double sa, int ga, double sb, int gb) { return sa > sb || (sa == sb && ga < gb); };
    if (n_found != nullptr) {
        int c = 0;
        for (int p = lane; p < n_parts; p += 64) c += nf_parts[(int64_t)p * nW + w];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
        if (lane == 0) n_found[w] = c;
    }
    double last_sc = 0.0;
    int last_sg = -1;                                    // the entry listed last (-1: none yet)
    for (int e = 0; e < n; ++e) {
        double bs = 0.0;
        int bg = -1, bi = -1;
        for (int i = lane; i < E; i += 64) {
            const pfann_match_result &r = entry(i);
            if (r.song < 0) continue;
            if (last_sg >= 0 && !before(last_sc, last_sg, r.score, r.song)) continue;
            if (bi < 0 || before(r.score, r.song, bs, bg)) { bs = r.score; bg = r.song; bi = i; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double vs = __shfl_xor(bs, o, 64);
            const int vg = __shfl_xor(bg, o, 64), vi = __shfl_xor(bi, o, 64);
            if (vi >= 0 && (bi < 0 || before(vs, vg, bs, bg))) { bs = vs; bg = vg; bi = vi; }
        }
        if (bi < 0) {                                    // nothing left: padding
            for (int i = e + lane; i < n; i += 64) {
                pfann_match_result res;
                res.song = -1; res.offset = 0; res.shift = 0; res.n_cand = 0; res.score = -INFINITY;
                top[w * n + i] = res;
            }
            return;
        }
        if (lane == 0) top[w * n + e] = entry(bi);
        last_sc = bs; last_sg = bg;
    }
}

int launch_dense_topn_merge(const pfann_match_result *tops, const int32_t *nf_parts, int n_parts, int64_t nW, int n,
                            pfann_match_result *top, int32_t *n_found, hipStream_t s) {
    if (nW <= 0) return 0;
    ProfScope ps("seq_dense_topn_merge", s, (double)nW * n_parts * n * 24.0);
    PF_LAUNCH(dense_topn_merge_kernel, dim3((unsigned)cdiv(nW, DN_MRG_NT / 64)), dim3(DN_MRG_NT), 0, s, tops, nf_parts, n_parts, nW, n,
              top, n_found);
    PF_HIP(hipGetLastError());
    return 0;
}

// one launch loads the code object of this translation unit: every instantiation of the tile kernel (the SHARD ones included),
// both selects, the decode and the two merges
__global__ void noop_dense_kernel() {}
int prewarm_dense() {
    hipLaunchKernelGGL(noop_dense_kernel, dim3(1), dim3(1), 0, 0);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace pfann
