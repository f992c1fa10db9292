// Device helpers shared by the sequence matcher (rerank.hip) and the windowed matcher (monitor.hip): the in-LDS key list,
// its bitonic sort and the label -> song lookup.
#pragma once
#include "common.h"

namespace pfann {

static constexpr int MAXC = 8192;       // candidate slots of the in-LDS key list (rows * top_k)
static constexpr unsigned long long SENT = ~0ull;

// Thread tid owns the positions i = tid + m*NT.  A compare-exchange distance j < 64 pairs positions of the same 64-aligned
// group, i.e. two lanes of ONE wave: those steps need no workgroup barrier (a wave's LDS operations execute in order, and
// within one instruction all 64 lanes read before any of them writes), only the steps with j >= 64 and the hand-over
// between the two kinds do.  For P = 2048 that is 21 barriers instead of 66 (the one-query matcher spent 30 us of its
// 74 us candidate phase in them).
template <int NT>
__device__ void bitonic_sort_keys(unsigned long long *sk, int P, int tid) {
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            if (j >= 32 || j == (k >> 1)) __syncthreads();     // positions written by other waves are read from here on
            else __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            for (int i = tid; i < P; i += NT) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const unsigned long long x = sk[i], y = sk[ixj];
                    const bool up = (i & k) == 0;
                    if ((x > y) == up) { sk[i] = y; sk[ixj] = x; }
                }
            }
        }
    }
    __syncthreads();
}

// song of a label = upper_bound over song_pos: 15+ dependent global loads per label when searched directly
// (a third of the candidate phase for one query); the first ~10 levels run on a coarse copy in LDS instead:
// s_cpos[i] = song_pos[i << cshift], n_coarse entries (<= 1024).  Ends with a barrier.
template <int NT>
__device__ __forceinline__ void load_coarse_song_pos(const int64_t *song_pos, int n_songs, long long *s_cpos, int tid,
                                                     int &cshift, int &n_coarse) {
    cshift = 0;
    while ((n_songs >> cshift) > 1023) ++cshift;
    n_coarse = (n_songs >> cshift) + 1;
    for (int i = tid; i < n_coarse; i += NT) s_cpos[i] = song_pos[(int64_t)i << cshift];
    __syncthreads();
}
// largest s with song_pos[s] <= lab  (searchsorted side='right' - 1); -1 when there is none
__device__ __forceinline__ int song_of_label(const int64_t *song_pos, int n_songs, const long long *s_cpos, int cshift,
                                             int n_coarse, int64_t lab) {
    int cl = 0, ch = n_coarse;    // coarse: entries before cl are <= lab, from ch on > lab
    while (cl < ch) {
        const int mid = (cl + ch) >> 1;
        if (s_cpos[mid] <= lab) cl = mid + 1; else ch = mid;
    }
    // song_pos[(cl-1) << cshift] <= lab < song_pos[cl << cshift] (when those exist): the same predicate
    // on the narrowed range gives the same answer as on [0, n_songs)
    int lo = cl > 0 ? (cl - 1) << cshift : 0;
    int hi = min(n_songs, cl << cshift);   // song_pos has n_songs+1 entries; search [0, n_songs)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (song_pos[mid] <= lab) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

}  // namespace pfann
