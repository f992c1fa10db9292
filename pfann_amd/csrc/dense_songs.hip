// Rescoring stage (pfann_match_songs_dense): every alignment of the few songs a query's list names, nothing else.
//
// For a query of n rows Q[0..n) (1 <= n <= 64) and a listed song s of len_s rows the entry is the one the ranked dense matcher
// (dense.hip, pfann_match_windows_dense_topn) gives song s for a window of those n rows: candidates -(n-1) <= o <= len_s - 1,
// total(s, o) = +0 plus, in ascending t, every dot(Q[t], db[song_pos[s] + o + t]) with 0 <= o + t < len_s, fp32; the largest
// total wins, equal totals go to the smaller offset; score = (double)total / (double)n.
//
// One workgroup owns a (query, list slot) PAIR at a time (grid-stride).  The slot is dropped when its song id is out of range,
// has no rows, or stands in an earlier slot of the same list; otherwise the workgroup walks the song in column tiles:
//   -> S[t][c] = dot(Q[t], song row C0 + c), 64 x SD_TN, on v_mfma_f32_32x32x2_f32 with K ascending, through the LDS layout of
//      dense.hip (position 4 h + s of a group of eight holds k = 2 s + h): a row dot is the fmaf chain from +0 over k = 0..d-1,
//      the very float the dense kernel forms.  Query rows t >= n and song rows outside [0, len_s) are staged as ZEROS -- never
//      the neighbouring song's rows --, their dots are +0, and x + (+0) keeps the bits of x: the total of an alignment that
//      hangs over either end of the song needs no cutting
//   -> tile ct starts at song row C0 = ct * SI - (n-1), SI = SD_TN - (n-1), and owns the alignments o = C0 + c, c < SI:
//      neighbouring tiles overlap by n-1 columns, so the diagonal S[t][c + t], t < n, of every owned alignment is in its tile
//   -> thread c adds its diagonal in ascending t (no sliding or prefix sums) and keeps the largest packed word it has seen over
//      all tiles: high half = the order-preserving bits of the total, low half = 0xFFFFFFFF - (o + n-1).
// The workgroup's largest word goes, by a plain store, into the 8-byte score field of top[query][slot] (0: a dropped slot), and
// songs_dense_rank_kernel, one wave per query, ranks the at most 64 words of a list by (total descending, song ascending) --
// the ranked dense matcher's order -- and writes entries and padding in place.
//
// BYTE CONTRACT.  A (query, song) entry is a function of the query's rows, the song's rows and n: one workgroup forms it from
// those alone, with one fixed tiling; m, the slot, the other songs and queries, the grid and the run have no part in it.
//
// The staging and MFMA steps are dense.hip's, copied for a 64-row left operand rather than shared through a header:
// match_windows_dense_kernel's code must not move (kernels.h).
#include "kernels.h"
#include <algorithm>

namespace pfann {

static constexpr int SD_TM = 64;            // query rows of the product (PFANN_SONGS_DENSE_MAX_ROWS)
static constexpr int SD_TN = 128;           // song columns of a tile
static constexpr int SD_NT = 256;           // 4 waves, each 64 x 32 of the tile
static constexpr int SD_BK = 32;            // K per staging step
static constexpr int SD_LDK = SD_BK + 4;    // staging pitch (dwords): conflict-free b128 reads
static constexpr int SD_LDS = SD_TN + 8;    // pitch of S
static constexpr int SD_GRID = 2048;
static_assert(SD_TM == PFANN_SONGS_DENSE_MAX_ROWS, "the product holds the longest query");

typedef float sd_f32x4 __attribute__((ext_vector_type(4)));
typedef float sd_f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ unsigned sd_ordered_bits(float t) {      // a > b  <=>  bits(a) > bits(b); never 0 for a number
    const unsigned u = __float_as_uint(t);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sd_ordered_float(unsigned u) {
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}

__global__ __launch_bounds__(SD_NT) void match_songs_dense_kernel(SongsDenseArgs a) {
    // S[SD_TM][SD_LDS]; while the product runs its first bytes are the two K tiles As [SD_TM][SD_LDK], Bs [SD_TN][SD_LDK]
    __shared__ __attribute__((aligned(16))) float s_S[SD_TM * SD_LDS];
    __shared__ unsigned long long s_red[SD_NT / 64];
    static_assert((SD_TM + SD_TN) * SD_LDK <= SD_TM * SD_LDS, "the K tiles fit under S");
    float *As = s_S, *Bs = s_S + SD_TM * SD_LDK;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lhalf = lane >> 5;
    const int64_t n_items = a.nQ * a.m;

    for (int64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int64_t j = item / a.m;
        const int slot = (int)(item - j * a.m);
        const int n = a.qlen[j];
        if (n < 1 || n > SD_TM) continue;                // (the whole workgroup) the rank kernel writes these queries
        const int s = a.cand[item].song;
        int len = 0;
        int64_t pos = 0;
        if (s >= 0 && s < a.n_songs) { pos = a.song_pos[s]; len = (int)(a.song_pos[s + 1] - pos); }
        // a song counts once, in its first slot
        const int dup = __syncthreads_or(tid < slot && a.cand[j * a.m + tid].song == s);
        unsigned long long *word = reinterpret_cast<unsigned long long *>(&a.top[item].score);
        if (len <= 0 || dup) {
            if (tid == 0) *word = 0;
            continue;
        }
        const int SI = SD_TN - (n - 1);
        const int n_tiles = (len + n - 1 + SI - 1) / SI;
        const float *qrows = a.q + a.qstart[j] * (int64_t)a.d;
        const float *srows = a.db + pos * (int64_t)a.d;
        unsigned long long best = 0;

        for (int ct = 0; ct < n_tiles; ++ct) {
            const int C0 = ct * SI - (n - 1);            // song row of the tile's column 0
            // ---- S = Q x tile^T.  Thread tid stages query row tid >> 2 and tile rows tid >> 2, (tid >> 2) + 64, eight
            // consecutive k (two float4) at 8 * (tid & 3) of every K step
            const int srow = tid >> 2, sk8 = (tid & 3) * 8;
            const float *qp = srow < n ? qrows + srow * (int64_t)a.d : nullptr;
            const float *dp[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int g = C0 + srow + 64 * u;
                dp[u] = g >= 0 && g < len ? srows + g * (int64_t)a.d : nullptr;
            }
            sd_f32x4 ra[2], rb[2][2];
            auto load_tile = [&](int k0) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int k = k0 + sk8 + 4 * h;
                    const sd_f32x4 z = {0.f, 0.f, 0.f, 0.f};
                    ra[h] = qp != nullptr && k < a.d ? *reinterpret_cast<const sd_f32x4 *>(qp + k) : z;
#pragma unroll
                    for (int u = 0; u < 2; ++u)
                        rb[u][h] = dp[u] != nullptr && k < a.d ? *reinterpret_cast<const sd_f32x4 *>(dp[u] + k) : z;
                }
            };
            // position 4 * half + s of a group of eight holds k = 2 * s + half: the half wave that supplies the MFMA's k = half
            // reads one b128 and steps s = 0..3 walk k in ascending order
            auto store_tile = [&]() {
                const sd_f32x4 ae = {ra[0][0], ra[0][2], ra[1][0], ra[1][2]};
                const sd_f32x4 ao = {ra[0][1], ra[0][3], ra[1][1], ra[1][3]};
                *reinterpret_cast<sd_f32x4 *>(&As[srow * SD_LDK + sk8]) = ae;
                *reinterpret_cast<sd_f32x4 *>(&As[srow * SD_LDK + sk8 + 4]) = ao;
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int o = (srow + 64 * u) * SD_LDK + sk8;
                    const sd_f32x4 be = {rb[u][0][0], rb[u][0][2], rb[u][1][0], rb[u][1][2]};
                    const sd_f32x4 bo = {rb[u][0][1], rb[u][0][3], rb[u][1][1], rb[u][1][3]};
                    *reinterpret_cast<sd_f32x4 *>(&Bs[o]) = be;
                    *reinterpret_cast<sd_f32x4 *>(&Bs[o + 4]) = bo;
                }
            };
            sd_f32x16 acc[2];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
            const int nk = (a.d + SD_BK - 1) / SD_BK;
            load_tile(0);
#pragma unroll 1
            for (int kt = 0; kt < nk; ++kt) {
                store_tile();
                __syncthreads();
                if (kt + 1 < nk) load_tile((kt + 1) * SD_BK);
#pragma unroll
                for (int kk = 0; kk < SD_BK / 8; ++kk) {
                    sd_f32x4 a4[2];
#pragma unroll
                    for (int i = 0; i < 2; ++i)
                        a4[i] = *reinterpret_cast<const sd_f32x4 *>(&As[(i * 32 + l31) * SD_LDK + kk * 8 + lhalf * 4]);
                    const sd_f32x4 b4 = *reinterpret_cast<const sd_f32x4 *>(&Bs[(wave * 32 + l31) * SD_LDK + kk * 8 + lhalf * 4]);
#pragma unroll
                    for (int st = 0; st < 4; ++st)
#pragma unroll
                        for (int i = 0; i < 2; ++i)
                            acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[i][st], b4[st], acc[i], 0, 0, 0);
                }
                __syncthreads();                         // the K tiles are read: the next step, or S, may overwrite them
            }
            // acc[i][e]: query row 32 i + (e & 3) + 8 * (e >> 2) + 4 * lhalf, column 32 wave + l31
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    s_S[(i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lhalf) * SD_LDS + wave * 32 + l31] = acc[i][e];
            __syncthreads();

            // ---- diagonals: thread = column c, alignment o = C0 + c
            if (tid < SI && C0 + tid <= len - 1) {
                float tot = 0.f;
                for (int t = 0; t < n; ++t) tot += s_S[t * SD_LDS + tid + t];
                const unsigned id = (unsigned)(C0 + tid + (n - 1));
                const unsigned long long x = ((unsigned long long)sd_ordered_bits(tot) << 32) | (0xFFFFFFFFu - id);
                best = x > best ? x : best;
            }
            __syncthreads();                             // S is free for the next tile
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long v = __shfl_xor(best, o, 64);
            best = v > best ? v : best;
        }
        if (lane == 0) s_red[wave] = best;
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int i = 1; i < SD_NT / 64; ++i) best = s_red[i] > best ? s_red[i] : best;
            *word = best;
        }
        __syncthreads();                                 // s_red is free for the next pair
    }
}

// One wave per query, lane = list slot.  Every lane reads its slot's word before any lane writes an entry (the ranks below need
// every lane's word), so the words may lie in the entries they become.
static constexpr int SD_RANK_NT = 256;

__global__ __launch_bounds__(SD_RANK_NT) void songs_dense_rank_kernel(SongsDenseArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t j = (int64_t)blockIdx.x * (SD_RANK_NT / 64) + (threadIdx.x >> 6);
    if (j >= a.nQ) return;                               // (whole waves; no barrier below)
    const int n = a.qlen[j];
    pfann_match_result *top = a.top + j * a.m;
    pfann_match_result pad;
    pad.song = -1; pad.offset = 0; pad.shift = 0; pad.n_cand = 0; pad.score = -INFINITY;
    if (n > SD_TM) {                                     // not rescored: the list as it came
        if (lane < a.m) top[lane] = a.cand[j * a.m + lane];
        if (lane == 0 && a.n_found != nullptr) a.n_found[j] = -1;
        return;
    }
    if (n < 1) {
        if (lane < a.m) top[lane] = pad;
        if (lane == 0 && a.n_found != nullptr) a.n_found[j] = 0;
        return;
    }
    unsigned long long x = 0;
    int s = -1;
    if (lane < a.m) {
        x = *reinterpret_cast<const unsigned long long *>(&top[lane].score);
        s = a.cand[j * a.m + lane].song;
    }
    const unsigned tb = (unsigned)(x >> 32);             // listed songs are distinct: (total, song) is a strict order
    int rank = 0;
    for (int i = 0; i < a.m; ++i) {
        const unsigned long long xi = __shfl(x, i, 64);
        const int si = __shfl(s, i, 64);
        const unsigned ti = (unsigned)(xi >> 32);
        rank += xi != 0 && (ti > tb || (ti == tb && si < s));
    }
    const int found = __popcll(__ballot(x != 0));
    if (x != 0) {
        pfann_match_result res;
        res.song = s;
        res.offset = (int)(0xFFFFFFFFu - (unsigned)x) - (n - 1);
        res.shift = 0;
        res.n_cand = (int)(a.song_pos[s + 1] - a.song_pos[s]) + n - 1;
        res.score = (double)sd_ordered_float(tb) / (double)n;
        top[rank] = res;
    }
    if (lane >= found && lane < a.m) top[lane] = pad;
    if (lane == 0 && a.n_found != nullptr) a.n_found[j] = found;
}

int launch_match_songs_dense(const SongsDenseArgs &a, hipStream_t s) {
    if (a.nQ <= 0) return 0;
    const int64_t n_items = a.nQ * a.m;
    {
        ProfScope ps("seq_match_songs_dense", s, 2.0 * SD_TM * SD_TN * (double)n_items * a.d);   // one tile per pair: most songs fit one
        PF_LAUNCH(match_songs_dense_kernel, dim3((unsigned)std::min<int64_t>(n_items, SD_GRID)), dim3(SD_NT), 0, s, a);
        PF_HIP(hipGetLastError());
    }
    ProfScope ps("seq_songs_dense_rank", s, (double)n_items * 24.0);
    PF_LAUNCH(songs_dense_rank_kernel, dim3((unsigned)cdiv(a.nQ, SD_RANK_NT / 64)), dim3(SD_RANK_NT), 0, s, a);
    PF_HIP(hipGetLastError());
    return 0;
}

// one launch loads the code object of this translation unit
__global__ void noop_dense_songs_kernel() {}
int prewarm_dense_songs() {
    hipLaunchKernelGGL(noop_dense_songs_kernel, dim3(1), dim3(1), 0, 0);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace pfann
