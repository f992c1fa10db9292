// Database updates (pfann_db_append / pfann_db_remove_songs, api.hip): the two kernels an update of a loaded handle needs.
//
//   song_norm_max_kernel  per-song maxima of the row norms, with the per-row arithmetic of rows_to_half_kernel
//                         (search_f16.hip): the largest of them is the xnorm_max a fresh pfann_db_load of the same rows
//                         computes, bit for bit, and it can be taken again after a song has left -- also with fp16-only
//                         storage, where no fp32 row is left to recompute from.
//   gather_rows_kernel    the move of a removal.  The kept rows are runs (src, dst, len) with dst <= src, ascending; the
//                         matrix is walked in ascending chunks of destination rows: ONE gather launch per chunk into a
//                         bounded staging buffer, then one copy down to the destination, in stream order.  Correct by
//                         construction: a chunk with destination rows [r0, r1) overwrites only rows below r1, and every
//                         row a LATER chunk reads has src >= dst >= r1; inside a chunk nothing is written to the matrix
//                         before the whole chunk has been read.  No launch depends on what another workgroup has done.
//
// Both are plain bandwidth-bound copies / reductions: no LDS, no scratch; 16-byte loads and stores where the row allows.
#include <algorithm>

#include "kernels.h"

namespace pfann {

// song of global row g: the s with song_pos[s] <= g < song_pos[s + 1] (songs without rows are stepped over)
__device__ __forceinline__ int song_of_row(const int64_t *__restrict__ song_pos, int n_songs, int64_t g) {
    int lo = 0, hi = n_songs;             // invariant: song_pos[lo] <= g < song_pos[hi]
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (song_pos[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ void song_norm_max_kernel(const float *__restrict__ x, int64_t n, int d, int64_t row0_global,
                                     const int64_t *__restrict__ song_pos, int n_songs, int song_base,
                                     float *__restrict__ song_max) {
    // one wave per row, the summation order of rows_to_half_kernel: lane e, e + 64, ... by fmaf, then wave_sum
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= n) return;
    float ss = 0.f;
    for (int e = lane; e < d; e += 64) {
        const float v = x[row * d + e];
        ss = fmaf(v, v, ss);
    }
    ss = wave_sum(ss);
    if (lane == 0) {
        const int s = song_of_row(song_pos, n_songs, row0_global + row);
        // non-negative floats (and NaN above them) order like their bit patterns: the maximum does not depend on arrival order
        atomicMax(reinterpret_cast<unsigned *>(song_max) + (s - song_base), __float_as_uint(sqrtf(ss)));
    }
}

int launch_song_norm_max(const float *x, int64_t n, int d, int64_t row0_global, const int64_t *song_pos, int n_songs,
                         int song_base, float *song_max, hipStream_t s) {
    if (n <= 0) return 0;
    PF_LAUNCH(song_norm_max_kernel, dim3((unsigned)cdiv(n, 4)), dim3(256), 0, s, x, n, d, row0_global, song_pos, n_songs,
              song_base, song_max);
    PF_HIP(hipGetLastError());
    return 0;
}

// V: uint4 (rows of a multiple of 16 bytes) or unsigned (any fp32 row)
template <typename V>
__global__ void gather_rows_kernel(const V *__restrict__ src, V *__restrict__ stage, const DbRun *__restrict__ runs, int n_runs,
                                   int64_t dst0, int total, FastDiv vpr) {
    // total = rows of the chunk * vpr < 2^31 (the host bounds the chunk): the row of a vector is one multiply-high
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int r = fastdiv(i, vpr);
        const int v = i - r * vpr.d;
        const int64_t dst = dst0 + r;
        int lo = 0, hi = n_runs;          // invariant: runs[lo].dst <= dst < runs[hi].dst (the host checked runs[0].dst <= dst0)
        while (hi - lo > 1) {
            const int mid = lo + ((hi - lo) >> 1);
            if (runs[mid].dst <= dst) lo = mid; else hi = mid;
        }
        const int64_t s = runs[lo].src + (dst - runs[lo].dst);
        stage[i] = src[s * vpr.d + v];
    }
}

int launch_gather_rows(const void *src, void *stage, const DbRun *runs_dev, int n_runs, int64_t dst0, int64_t n_rows,
                       int64_t row_bytes, hipStream_t s) {
    if (n_rows <= 0) return 0;
    const bool wide = row_bytes % 16 == 0;
    const int vpr = (int)(row_bytes / (wide ? 16 : 4));
    const int64_t total = n_rows * vpr;
    if (total >= (1ll << 31) - 2048 * 256) { set_error("db move: a chunk of %lld rows is too large", (long long)n_rows); return -1; }
    const unsigned grid = (unsigned)std::min<int64_t>(cdiv(total, 256), 2048);
    ProfScope ps("db_move_gather", s, 2.0 * (double)n_rows * (double)row_bytes);
    if (wide)
        PF_LAUNCH(gather_rows_kernel<uint4>, dim3(grid), dim3(256), 0, s, reinterpret_cast<const uint4 *>(src),
                  reinterpret_cast<uint4 *>(stage), runs_dev, n_runs, dst0, (int)total, make_fastdiv(vpr));
    else
        PF_LAUNCH(gather_rows_kernel<unsigned>, dim3(grid), dim3(256), 0, s, reinterpret_cast<const unsigned *>(src),
                  reinterpret_cast<unsigned *>(stage), runs_dev, n_runs, dst0, (int)total, make_fastdiv(vpr));
    PF_HIP(hipGetLastError());
    return 0;
}

// Kept runs of a removal, from the host's song_pos: gone[s] != 0 marks a song that loses its rows.  Only what lies behind
// the first removed row is listed (rows before it are not touched); neighbouring kept songs form one run.
// -> rows left; *first = first destination row the move writes (= rows left when nothing moves)
int64_t db_kept_runs(const std::vector<int64_t> &song_pos, const std::vector<char> &gone, std::vector<DbRun> &runs,
                     int64_t *first) {
    runs.clear();
    const int n_songs = (int)song_pos.size() - 1;
    int64_t dst = 0;
    bool moved = false;
    int64_t first_dst = -1;
    for (int s = 0; s < n_songs; ++s) {
        const int64_t lo = song_pos[s], len = song_pos[s + 1] - song_pos[s];
        if (len <= 0) continue;
        if (gone[s]) { moved = true; continue; }
        if (moved) {
            if (first_dst < 0) first_dst = dst;
            if (!runs.empty() && runs.back().src + runs.back().len == lo) runs.back().len += len;
            else runs.push_back(DbRun{lo, dst, len});
        }
        dst += len;
    }
    *first = first_dst < 0 ? dst : first_dst;
    return dst;
}

__global__ void noop_dbstore_kernel() {}
int prewarm_dbstore() {
    hipLaunchKernelGGL(noop_dbstore_kernel, dim3(1), dim3(1), 0, 0);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace pfann
