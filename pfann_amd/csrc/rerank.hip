// Candidate generation + sequence score + argmax on the GPU, one workgroup per query
// (reference database.py:129-163 `query_embeddings_base`, mode 0; and the native scorer
// cpp/seqscore.cpp:49-135 `seq_score`, mode 1).
//
//   labels[t][i] -> (song, offset = label - song_pos[song] - t/fsm, shift = t%fsm)
//   -> 64-bit packed keys, bitonic sort + dedup in LDS (= np.unique / std::sort+unique)
//   -> one wave per unique candidate gathers the <= qlen consecutive db rows of that
//      alignment (coalesced 512-byte rows, L2-resident after the scan) and accumulates the
//      inner products; out-of-song rows contribute 0; the divisor is always sub_len
//   -> first-wins strict-> argmax in the reference's own candidate order, so ties resolve
//      to the smallest (song, offset) exactly as the reference does.
#include "kernels.h"
#include "match_common.h"
#include <algorithm>

namespace pfann {

static constexpr int OFF_BIAS = 1 << 27;

struct Cand { int song, off, shift; };

__device__ __forceinline__ unsigned long long pack_cand(int mode, int song, int off, int shift) {
    const unsigned long long ob = (unsigned long long)(unsigned)(off + OFF_BIAS);
    if (mode == 0) return ((unsigned long long)shift << 58) | ((unsigned long long)song << 28) | ob;
    return ((unsigned long long)song << 34) | (ob << 6) | (unsigned long long)shift;
}
__device__ __forceinline__ Cand unpack_cand(int mode, unsigned long long key) {
    Cand c;
    if (mode == 0) {
        c.shift = (int)(key >> 58);
        c.song = (int)((key >> 28) & 0x3FFFFFFFull);
        c.off = (int)(key & 0xFFFFFFFull) - OFF_BIAS;
    } else {
        c.song = (int)(key >> 34);
        c.off = (int)((key >> 6) & 0xFFFFFFFull) - OFF_BIAS;
        c.shift = (int)(key & 63ull);
    }
    return c;
}

// ---- candidates (database.py:133-138 / seqscore.cpp:49-60): labels[t][i] -> packed (song, offset, shift) keys in sk[0..P)
// (SENT for label -1, songs of other shards under only_owned, and the padding up to P).  No trailing barrier.
template <int NT>
__device__ void make_candidate_keys(const RerankArgs &a, int64_t q0, int ntot, int P, unsigned long long *sk, long long *s_cpos, int tid) {
        int cshift, n_coarse;
        load_coarse_song_pos<NT>(a.song_pos, a.n_songs, s_cpos, tid, cshift, n_coarse);
        for (int i = tid; i < P; i += NT) {
            unsigned long long key = SENT;
            if (i < ntot) {
                const int t = i / a.k;
                const int64_t lab = a.labels[(q0 + t) * a.k + (i - t * a.k)];
                if (lab >= 0) {
                    const int song = song_of_label(a.song_pos, a.n_songs, s_cpos, cshift, n_coarse, lab);
                    const int tim = t / a.fsm, shift = t - tim * a.fsm;
                    const int off = (int)(lab - a.song_pos[song] - tim);
                    const bool owned = song >= a.song_lo && song < a.song_hi;
                    if (song >= 0 && (owned || !a.only_owned)) key = pack_cand(a.mode, song, off, shift);
                }
            }
            sk[i] = key;
        }
}

// Phase 1 of the phased launch for a handful of queries, spread over the chip: a bitonic sort of one query's 2048 keys
// inside ONE workgroup is 66 dependent LDS round trips (53 us of the one-query matcher's 70 us candidate phase, measured
// by ablation).  A RANK sort has no dependent steps and parallelises over workgroups: each of the gridDim.y workgroups
// builds all P keys in its LDS (redundantly, in parallel), then ranks its own slice of P / gridDim.y keys against all of
// them -- rank = #{keys smaller} + #{equal keys at a lower index}, a permutation -- and stores them at their rank in
// gkeys.  Duplicates are NOT removed here: equal candidates score equal, so the first-wins argmax, the per-song replay
// and (counted in phase 3) n_cand come out the same.  ncand = number of real (non-sentinel) keys.
template <int NT>
__global__ __launch_bounds__(NT) void match_rank_kernel(RerankArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long sk_lds[];   // [P] keys
    __shared__ long long s_cpos[1024];
    __shared__ int s_rank[128];
    __shared__ int s_cnt;
    const int64_t qi = blockIdx.x;
    const int tid = threadIdx.x;
    const int64_t q0 = a.qstart[qi];
    const int qlen = a.qlen[qi];
    const int ntot = qlen * a.k;
    int P = 1;
    while (P < ntot) P <<= 1;
    const int G = (int)gridDim.y;
    const int SL = a.pmax / G;                    // slice length when P == pmax; shorter queries use fewer slices
    if (P > a.pmax) {
        if (tid == 0 && blockIdx.y == 0) {
            if (a.results != nullptr) {           // (a top-N call has none: its phase 3 writes the refusal)
                pfann_match_result r; r.song = -2; r.offset = 0; r.shift = 0; r.n_cand = -1; r.score = -INFINITY; a.results[qi] = r;
            }
            a.ncand[qi] = -1;
        }
        return;
    }
    const int slice0 = (int)blockIdx.y * SL;
    if (slice0 >= P) return;
    if (tid < 128) s_rank[tid] = 0;
    if (tid == 0) s_cnt = 0;
    make_candidate_keys<NT>(a, q0, ntot, P, sk_lds, s_cpos, tid);
    __syncthreads();
    if (blockIdx.y == 0) {                        // number of real keys
        int c = 0;
        for (int i = tid; i < P; i += NT) c += sk_lds[i] != SENT ? 1 : 0;
        c = (int)wave_sum((float)c);              // <= 16 per lane, <= 1024 per wave: exact in fp32
        if ((tid & 63) == 0) atomicAdd(&s_cnt, c);
    }
    // thread = (slice key s, partition of the j range): SL <= 128 keys x NT / SL partitions of P * SL / NT positions
    const int s = tid % SL, part = tid / SL, nparts = NT / SL;
    const int gi = slice0 + s;
    const bool live = gi < P;                     // a short query among longer ones: P < SL
    const unsigned long long K = live ? sk_lds[gi] : SENT;
    int cnt = 0;
    if (live)
        for (int j = part; j < P; j += nparts) {  // every lane of a wave reads the same j: an LDS broadcast
            const unsigned long long kj = sk_lds[j];
            cnt += (kj < K || (kj == K && j < gi)) ? 1 : 0;
        }
    if (live) atomicAdd(&s_rank[s], cnt);
    __syncthreads();
    unsigned long long *gk = a.gkeys + qi * (int64_t)a.pmax;
    if (tid < SL && slice0 + tid < P) gk[s_rank[tid]] = sk_lds[slice0 + tid];
    if (blockIdx.y == 0 && tid == 0) a.ncand[qi] = s_cnt;
}

// ---- ranked top-N songs (pfann_match_topn): the selection stage that replaces the argmax ------------------------------
// Same list, same scores, same candidate order as the argmax below.  Entry r is found by pass r of a block-wide first-wins
// strict-> argmax (score as double, list index) over the candidates whose song no earlier pass selected: that candidate is
// its song's best by the argmax's own rule, and a tie between two songs goes to the one whose best candidate comes first.
// Pass r + 1 retires every candidate of the song pass r selected (a marker in its score slot -- a thread only ever reads and
// writes the slots of its own candidates) and counts the distinct ones: the entry's n_cand.  A song that recurs once per
// shift (mode 0, frame_shift_mul > 1) needs nothing extra: its runs are retired by song id, in parallel.  One barrier per
// pass; n + 1 passes at most, fewer when the songs run out.  Pass 0's spare count is n_found (distinct songs).
static constexpr unsigned TOPN_RETIRED = 0xFFFFFFFFu;      // a NaN: a slot that holds it by itself never wins either

__device__ __forceinline__ int song_of_key(int mode, unsigned long long key) {
    return mode == 0 ? (int)((key >> 28) & 0x3FFFFFFFull) : (int)(key >> 34);
}
__device__ __forceinline__ pfann_match_result topn_padding() {
    pfann_match_result r; r.song = -1; r.offset = 0; r.shift = 0; r.n_cand = 0; r.score = -INFINITY;
    return r;
}
template <int NT>
__device__ void topn_refuse(const RerankArgs &a, int64_t qi, int tid) {
    pfann_match_result *top = a.top + qi * a.topn;
    for (int i = tid; i < a.topn; i += NT) {
        pfann_match_result r = topn_padding();
        if (i == 0) { r.song = -2; r.n_cand = -1; }       // entry 0 is pfann_match's refusal
        top[i] = r;
    }
    if (tid == 0 && a.n_found != nullptr) a.n_found[qi] = -1;
}
// is list position c the first one of its song?  (sorted list sk[0..nc), possibly with repeated keys)
__device__ __forceinline__ bool first_of_song(const RerankArgs &a, const unsigned long long *sk, int nc, int c, unsigned long long key) {
    const int pre = a.mode == 0 ? 28 : 34;                  // key >> pre = (shift, song) / song: one run of the list
    if (c > 0 && (sk[c - 1] >> pre) == (key >> pre)) return false;
    if (a.mode != 0 || a.fsm == 1) return true;
    // mode 0 orders by (shift, song, offset): the song may have a run under every smaller shift
    const unsigned long long song = (key >> 28) & 0x3FFFFFFFull;
    const int shift = (int)(key >> 58);
    for (int s = 0; s < shift; ++s) {
        const unsigned long long want = ((unsigned long long)s << 30) | song;       // (shift, song) of that run
        int lo = 0, hi = nc;                                 // first position whose (shift, song) is >= want
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((sk[mid] >> 28) < want) lo = mid + 1; else hi = mid;
        }
        if (lo < nc && (sk[lo] >> 28) == want) return false;
    }
    return true;
}
template <int NT>
__device__ void select_topn(const RerankArgs &a, int64_t qi, int qlen, const unsigned long long *sk, float *score, int nc, int tid) {
    constexpr int NW = NT / 64;
    __shared__ double s_best[2][NW];
    __shared__ int s_besti[2][NW], s_cnt[2][NW];
    const int lane = tid & 63, wave = tid >> 6;
    pfann_match_result *top = a.top + qi * a.topn;
    int last_song = -1, r = 0;
    for (;; ++r) {
        const bool want = r < a.topn;
        double best = -INFINITY;
        int besti = 0x7FFFFFFF, cnt = 0;
        for (int c = tid; c < nc; c += NT) {
            const unsigned long long key = sk[c];
            const bool distinct = c == 0 || sk[c - 1] != key;       // (the rank-sorted list keeps its repeats)
            if (r == 0) {
                cnt += (distinct && first_of_song(a, sk, nc, c, key)) ? 1 : 0;
            } else if (song_of_key(a.mode, key) == last_song) {
                cnt += distinct ? 1 : 0;
                score[c] = __uint_as_float(TOPN_RETIRED);
                continue;
            }
            if (!want) continue;
            const float sc = score[c];
            if (__float_as_uint(sc) == TOPN_RETIRED) continue;
            double sco;
            if (a.mode == 0) {
                const int shift = (int)(key >> 58);
                const int sub_len = (qlen - shift + a.fsm - 1) / a.fsm;
                sco = (double)sc / (double)sub_len;
            } else {
                sco = (double)sc;
            }
            if (sco > best) { best = sco; besti = c; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ob = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(besti, o, 64);
            cnt += __shfl_xor(cnt, o, 64);
            if (ob > best || (ob == best && oi < besti)) { best = ob; besti = oi; }
        }
        const int b = r & 1;         // two buffers: pass r + 1 may write while a slow wave still reads pass r
        if (lane == 0) { s_best[b][wave] = best; s_besti[b][wave] = besti; s_cnt[b][wave] = cnt; }
        __syncthreads();
        best = s_best[b][0]; besti = s_besti[b][0]; cnt = s_cnt[b][0];
#pragma unroll
        for (int w = 1; w < NW; ++w) {
            const double ob = s_best[b][w];
            const int oi = s_besti[b][w];
            cnt += s_cnt[b][w];
            if (ob > best || (ob == best && oi < besti)) { best = ob; besti = oi; }
        }
        if (tid == 0) {
            if (r > 0) top[r - 1].n_cand = cnt;
            else if (a.n_found != nullptr) a.n_found[qi] = cnt;
        }
        if (!want || besti == 0x7FFFFFFF) break;
        const Cand cd = unpack_cand(a.mode, sk[besti]);
        if (tid == 0) {
            pfann_match_result e;
            e.song = cd.song; e.offset = cd.off; e.shift = cd.shift; e.n_cand = 0; e.score = best;
            top[r] = e;
        }
        last_song = cd.song;
    }
    for (int i = r + tid; i < a.topn; i += NT) top[i] = topn_padding();
}

template <int NT, bool TOPN>
__global__ __launch_bounds__(NT) void match_kernel(RerankArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long sk_lds[];   // [P] keys
    __shared__ int s_nc;
    __shared__ long long s_cpos[1024];     // every 2^cshift-th entry of song_pos: the first levels of the song lookup
    const int64_t qi = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t q0 = a.qstart[qi];
    const int qlen = a.qlen[qi];
    const int ntot = qlen * a.k;
    int P = 1;
    while (P < ntot) P <<= 1;
    if (P > a.pmax) {   // host sized the buffers for max_qlen: refuse rather than overrun
        if constexpr (TOPN) {
            if (a.phase != 2) topn_refuse<NT>(a, qi, tid);    // (phase 3 too: the rank-sorted phase 1 has no results[] to write)
            if (tid == 0 && a.phase == 1) a.ncand[qi] = -1;
        } else
        if (tid == 0 && a.phase <= 1) {
            pfann_match_result r; r.song = -2; r.offset = 0; r.shift = 0; r.n_cand = -1; r.score = -INFINITY; a.results[qi] = r;
            if (a.phase == 1) a.ncand[qi] = -1;
        }
        return;
    }
    // candidate keys + sums live in LDS for ordinary queries and in an HBM scratch slab for very
    // long ones (same code: a workgroup's global stores are visible to it after __syncthreads)
    // (phase 1 of the phased launch sorts in LDS when the list fits and only publishes the result)
    const bool in_lds = a.gkeys == nullptr || (a.phase == 1 && a.pmax <= MAXC);
    unsigned long long *sk = in_lds ? sk_lds : a.gkeys + qi * (int64_t)a.pmax;
    float *score = in_lds ? reinterpret_cast<float *>(sk_lds + P) : a.gscore + qi * (int64_t)a.pmax;

    int nc;
    if (a.phase <= 1) {
        make_candidate_keys<NT>(a, q0, ntot, P, sk, s_cpos, tid);
        __syncthreads();
        // ---- sort ascending (== lexicographic candidate order of the reference)
        bitonic_sort_keys<NT>(sk, P, tid);
        // ---- dedup (np.unique / std::unique).  Lists of <= 8 keys per thread: order-preserving compaction (each thread
        // takes a run of consecutive keys into registers, a block-wide exclusive scan of the unique counts gives the
        // destinations) instead of blanking the repeats and sorting a second time; longer lists keep the second sort.
        if (P <= 8 * NT) {
            __shared__ int s_wtot[NT / 64];
            const int ept = P >= NT ? P / NT : 1;
            unsigned long long kreg[8];
            int cnt_u = 0;
            unsigned umask = 0;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int i = tid * ept + e;
                kreg[e] = SENT;
                if (e < ept && i < P) {
                    kreg[e] = sk[i];
                    const bool u = kreg[e] != SENT && (i == 0 || kreg[e] != sk[i - 1]);
                    if (u) { umask |= 1u << e; ++cnt_u; }
                }
            }
            int incl = cnt_u;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int v = __shfl_up(incl, o, 64);
                if (lane >= o) incl += v;
            }
            if (lane == 63) s_wtot[wave] = incl;
            __syncthreads();                      // every key is in registers: the list may be overwritten
            int base = 0, total = 0;
            for (int w = 0; w < NT / 64; ++w) { const int v = s_wtot[w]; if (w < wave) base += v; total += v; }
            int pos = base + incl - cnt_u;
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (umask & (1u << e)) sk[pos++] = kreg[e];
            if (tid == 0) s_nc = total;
            __syncthreads();
        } else {
        int *dupf = reinterpret_cast<int *>(score);
        for (int i = tid; i < P; i += NT) dupf[i] = (i > 0 && sk[i] == sk[i - 1]) ? 1 : 0;
        __syncthreads();
        for (int i = tid; i < P; i += NT) if (dupf[i]) sk[i] = SENT;
        if (tid == 0) s_nc = 0;
        __syncthreads();
        bitonic_sort_keys<NT>(sk, P, tid);
        for (int i = tid; i < P; i += NT)
            if (sk[i] != SENT && (i + 1 == P || sk[i + 1] == SENT)) s_nc = i + 1;
        __syncthreads();
        }
        nc = s_nc;
        if (a.phase == 1) {          // phased launch: the sorted unique keys go to / stay in gkeys
            if (in_lds) {
                unsigned long long *gk = a.gkeys + qi * (int64_t)a.pmax;
                for (int i = tid; i < nc; i += NT) gk[i] = sk[i];
            }
            if (tid == 0) a.ncand[qi] = nc;
            return;
        }
    } else {
        nc = a.ncand[qi];
        if (nc < 0) return;
    }

    // ---- score every unique candidate: one wave each (phase 2: the candidates of a query are spread over
    // gridDim.y workgroups, so a single query uses the whole GPU instead of one CU)
    const int c_first = a.phase == 2 ? (int)blockIdx.y * (NT / 64) + wave : wave;
    const int c_step = a.phase == 2 ? (int)gridDim.y * (NT / 64) : NT / 64;
    if (a.phase != 3)
    for (int c = c_first; c < nc; c += c_step) {
        const Cand cd = unpack_cand(a.mode, sk[c]);
        const int64_t start = a.song_pos[cd.song];
        const int slen = (int)(a.song_pos[cd.song + 1] - start);
        const int sub_len = (qlen - cd.shift + a.fsm - 1) / a.fsm;
        float tot = 0.f;         // mode 0: lane-partial of the whole dot; mode 1: running sco
        if (a.fsm == 1 && (a.mode == 0 || a.alpha == 0.0f)) {
            // The rows of one alignment are ONE contiguous block of the db (and of the query): a single long dot
            // product read with independent 16-byte loads, four chunks in flight per lane, instead of qlen
            // row-by-row round trips -- the matcher is a random 10 KB gather per candidate and lives on memory-level
            // parallelism.  Fixed, data-independent summation order: duplicated songs still tie bit-exactly.
            const int j_lo = cd.off < 0 ? -cd.off : 0;
            const int j_hi = min(sub_len, slen - cd.off);
            const int nch = j_hi > j_lo ? (j_hi - j_lo) * (a.d >> 2) : 0;
            const int64_t ro = (start + cd.off + j_lo - a.label_base) * a.d;
            const float4 *qb = reinterpret_cast<const float4 *>(a.q + (q0 + j_lo) * a.d);
            float p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f;
            if (a.db != nullptr) {
                const float4 *vb = reinterpret_cast<const float4 *>(a.db + ro);
#pragma unroll 4
                for (int ch = lane; ch < nch; ch += 64) {
                    const float4 v = vb[ch], w = qb[ch];
                    p0 = fmaf(v.x, w.x, p0); p1 = fmaf(v.y, w.y, p1); p2 = fmaf(v.z, w.z, p2); p3 = fmaf(v.w, w.w, p3);
                }
            } else {
                typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
                const f16x4 *vb = reinterpret_cast<const f16x4 *>(reinterpret_cast<const _Float16 *>(a.dbh) + ro);
#pragma unroll 4
                for (int ch = lane; ch < nch; ch += 64) {
                    const f16x4 v = vb[ch];
                    const float4 w = qb[ch];
                    p0 = fmaf((float)v[0], w.x, p0); p1 = fmaf((float)v[1], w.y, p1);
                    p2 = fmaf((float)v[2], w.z, p2); p3 = fmaf((float)v[3], w.w, p3);
                }
            }
            tot = wave_sum((p0 + p1) + (p2 + p3));
            if (a.mode != 0) tot = tot / (float)max(sub_len, 1);
            if (lane == 0) score[c] = tot;
            continue;
        }
        for (int j = 0; j < sub_len; ++j) {
            const int r = cd.off + j;
            if (r < 0 || r >= slen) continue;
            const int64_t ro = (start + r - a.label_base) * a.d;
            const float *qv = a.q + (q0 + (int64_t)j * a.fsm + cd.shift) * a.d;
            float part = 0.f;
            if (a.db != nullptr) {
                const float *v = a.db + ro;
                for (int e = lane; e < a.d; e += 64) part = fmaf(v[e], qv[e], part);
            } else {                      // fp16-only storage: ONLY fp16 rows exist, so the sequence score is fp16-grade too
                                          // (in the reference useFloat16 touches the GPU search index alone; its rerank
                                          // reconstructs fp32 rows from the CPU index, database.py:148-152)
                const _Float16 *v = reinterpret_cast<const _Float16 *>(a.dbh) + ro;
                for (int e = lane; e < a.d; e += 64) part = fmaf((float)v[e], qv[e], part);
            }
            if (a.mode == 0) {
                tot += part;
            } else {
                const float ip = wave_sum(part);
                if (a.alpha == 0.0f) tot += ip;
                else if (a.alpha > 0.0f) { const float l2 = 1.0f - ip; tot += expf(-a.alpha * l2 * l2); }
            }
        }
        if (a.mode == 0) tot = wave_sum(tot);
        else tot = tot / (float)max(sub_len, 1);
        if (lane == 0) score[c] = tot;
    }
    if (a.phase == 2) return;
    __syncthreads();
    if constexpr (TOPN) {
        select_topn<NT>(a, qi, qlen, sk, score, nc, tid);
        return;
    }
    int n_unique = nc;
    if (a.phase == 3) {                  // the rank-sorted list of the phased launch keeps its duplicates: count the distinct keys
        if (tid == 0) s_nc = 0;
        __syncthreads();
        int u = 0;
        for (int c = tid; c < nc; c += NT) u += (c == 0 || sk[c] != sk[c - 1]) ? 1 : 0;
        u = (int)wave_sum((float)u);
        if (lane == 0 && u) atomicAdd(&s_nc, u);
        __syncthreads();
        n_unique = s_nc;
    }

    // ---- argmax, first-wins in candidate order (database.py:158-163 / seqscore.cpp:115-124)
    if (tid < 64) {
        double best = -INFINITY;
        int besti = 0x7FFFFFFF;
        for (int c = lane; c < nc; c += 64) {
            double sco;
            if (a.mode == 0) {
                const int shift = (int)(sk[c] >> 58);
                const int sub_len = (qlen - shift + a.fsm - 1) / a.fsm;
                sco = (double)score[c] / (double)sub_len;
            } else {
                sco = (double)score[c];
            }
            if (sco > best) { best = sco; besti = c; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ob = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(besti, o, 64);
            if (ob > best || (ob == best && oi < besti)) { best = ob; besti = oi; }
        }
        if (lane == 0) {
            pfann_match_result r;
            r.n_cand = n_unique;
            if (nc > 0 && besti != 0x7FFFFFFF) {
                const Cand cd = unpack_cand(a.mode, sk[besti]);
                r.song = cd.song; r.offset = cd.off; r.shift = cd.shift; r.score = best;
            } else {
                r.song = -1; r.offset = 0; r.shift = 0; r.score = -INFINITY;
            }
            a.results[qi] = r;
        }
    }
    // ---- per-song best (only recorded when > the zero-initialised slot)
    if (a.song_scores != nullptr) {
        float *ss = a.song_scores + ((int64_t)qi * a.ss_n - a.ss_lo) * 2;       // indexed by GLOBAL song id below
        if (a.mode == 1 || a.fsm == 1) {
            // one song = one contiguous run of the sorted list: the run's first max wins
            for (int c = tid; c < nc; c += NT) {
                const Cand cd = unpack_cand(a.mode, sk[c]);
                if (c > 0 && unpack_cand(a.mode, sk[c - 1]).song == cd.song) continue;   // not a run head
                float best = 0.f;    // slots start at 0: only scores > 0 are recorded
                int besto = 0;
                bool any = false;
                for (int e = c; e < nc; ++e) {
                    const Cand ce = unpack_cand(a.mode, sk[e]);
                    if (ce.song != cd.song) break;
                    float sco;
                    if (a.mode == 0) sco = (float)((double)score[e] / (double)qlen);   // fsm == 1: sub_len == qlen
                    else sco = score[e];
                    // the stored slot is float32 and numpy compares a Python float with it IN float32 (the score is rounded
                    // first): a later candidate of the song whose score rounds to the slot's value does not replace it
                    if (sco > best) {
                        best = sco; any = true;
                        besto = a.mode == 0 ? ce.off : ce.off * a.fsm - ce.shift;
                    }
                }
                if (any) { ss[cd.song * 2] = best; ss[cd.song * 2 + 1] = (float)besto; }
            }
        } else if (tid == 0) {
            // python path with frame_shift_mul > 1: songs recur once per shift; replay serially
            for (int c = 0; c < nc; ++c) {
                const Cand cd = unpack_cand(0, sk[c]);
                const int sub_len = (qlen - cd.shift + a.fsm - 1) / a.fsm;
                const float sco = (float)((double)score[c] / (double)sub_len);    // compared in float32, as above
                if (sco > ss[cd.song * 2]) {
                    ss[cd.song * 2] = sco;
                    ss[cd.song * 2 + 1] = (float)(cd.off * a.fsm - cd.shift);
                }
            }
        }
    }
}

// ---- multi-GPU winner selection ----------------------------------------------------------------------
// One 128-bit key per (rank, query) whose UNSIGNED lexicographic order (hi, lo) is the reference's preference:
// higher score first, ties -> the candidate that comes first in its sorted candidate list, i.e. the smallest
// (shift, song, offset) (database.py:129,140,158-163: strict '>' over np.unique-sorted candidates).
//   hi = ~orderable(score as fp64)      lo = shift << 58 | song << 28 | (offset + 2^27)      (no candidate: all ones)
__device__ __forceinline__ unsigned long long ord64(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return u ^ ((u >> 63) ? ~0ull : 0x8000000000000000ull);
}
__global__ void match_pack_kernel(const pfann_match_result *__restrict__ res, int64_t nQ, unsigned long long *__restrict__ keys) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nQ) return;
    const pfann_match_result r = res[j];
    unsigned long long hi = ~0ull, lo = ~0ull;
    if (r.song >= 0) { hi = ~ord64(r.score + 0.0); lo = pack_cand(0, r.song, r.offset, r.shift); }   // -0.0 + 0.0 = +0.0: equal scores, equal bits
    // a REFUSED query (song == -2: candidate buffer sizing error on this rank) must not read as "no candidate": the
    // all-zero key beats every real key (hi == 0 would need a NaN score), and the pick hands -2 on to the host
    if (r.song == -2) { hi = 0ull; lo = 0ull; }
    keys[2 * j] = hi;
    keys[2 * j + 1] = lo;
}
__global__ void match_pick_kernel(const unsigned long long *__restrict__ keys, int G, int64_t nQ, pfann_match_result *__restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nQ) return;
    unsigned long long bh = ~0ull, bl = ~0ull;
    for (int g = 0; g < G; ++g) {
        const unsigned long long h = keys[((int64_t)g * nQ + j) * 2], l = keys[((int64_t)g * nQ + j) * 2 + 1];
        if (h < bh || (h == bh && l < bl)) { bh = h; bl = l; }
    }
    pfann_match_result r;
    r.n_cand = 0;
    if (bh == ~0ull && bl == ~0ull) {
        r.song = -1; r.offset = 0; r.shift = 0; r.score = -INFINITY;
    } else if (bh == 0ull && bl == 0ull) {          // some rank refused this query
        r.song = -2; r.offset = 0; r.shift = 0; r.score = -INFINITY;
    } else {
        const Cand c = unpack_cand(0, bl);
        r.song = c.song; r.offset = c.off; r.shift = c.shift;
        const unsigned long long o = ~bh;
        r.score = __longlong_as_double((long long)(o ^ ((o >> 63) ? 0x8000000000000000ull : ~0ull)));
    }
    out[j] = r;
}
// per-song slot 1: alignment in fine frames (t * fsm - shift) -> seconds, (t - shift / fsm) * hop_size, computed in double
// like the reference's Python floats (database.py:148,193) and stored as float32; slots never written hold 0 -> 0 s
__global__ void song_scores_to_seconds_kernel(float *__restrict__ ss, int64_t n_pairs, int fsm, double hop_size, int native_path) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pairs) return;
    if (native_path) {      // database.py:193: song_score[:, 1] *= hop_size / frame_shift_mul, a float32 multiply
        ss[2 * i + 1] = ss[2 * i + 1] * (float)(hop_size / (double)fsm);
        return;
    }
    const long long fine = (long long)ss[2 * i + 1];
    long long shift = (-fine) % fsm;
    if (shift < 0) shift += fsm;
    const long long t = (fine + shift) / fsm;
    ss[2 * i + 1] = (float)(((double)t - (double)shift / (double)fsm) * hop_size);
}
int launch_song_scores_to_seconds(float *ss, int64_t n_pairs, int fsm, double hop_size, int native_path, hipStream_t s) {
    if (n_pairs <= 0) return 0;
    if (fsm < 1) { set_error("song_scores_to_seconds: frame_shift_mul=%d", fsm); return -1; }
    ProfScope ps("song_scores_to_seconds", s);
    PF_LAUNCH(song_scores_to_seconds_kernel, dim3((unsigned)cdiv(n_pairs, 256)), dim3(256), 0, s, ss, n_pairs, fsm, hop_size, native_path);
    PF_HIP(hipGetLastError());
    return 0;
}

int launch_match_pack(const pfann_match_result *res, int64_t nQ, unsigned long long *keys, hipStream_t s) {
    if (nQ <= 0) return 0;
    PF_LAUNCH(match_pack_kernel, dim3((unsigned)cdiv(nQ, 256)), dim3(256), 0, s, res, nQ, keys);
    PF_HIP(hipGetLastError());
    return 0;
}
int launch_match_pick(const unsigned long long *keys, int G, int64_t nQ, pfann_match_result *out, hipStream_t s) {
    if (nQ <= 0) return 0;
    PF_LAUNCH(match_pick_kernel, dim3((unsigned)cdiv(nQ, 256)), dim3(256), 0, s, keys, G, nQ, out);
    PF_HIP(hipGetLastError());
    return 0;
}

template <bool TOPN>
static int launch_match_as(const RerankArgs &a, hipStream_t s) {
    if (a.nQ <= 0) return 0;
    if (TOPN != (a.topn > 0) || (TOPN && (a.top == nullptr || a.topn > 64))) { set_error("match: top-N arguments (n=%d)", a.topn); return -1; }
    if (a.fsm < 1 || a.fsm > 32) { set_error("match: frame_shift_mul=%d outside 1..32", a.fsm); return -1; }
    if (a.n_songs >= (1 << 30)) { set_error("match: too many songs"); return -1; }
    constexpr auto kern = match_kernel<1024, TOPN>;
    if (ensure_dyn_lds((const void *)kern, MAXC * 12)) return -1;
    if (a.pmax > MAXC && a.gkeys == nullptr) {
        set_error("match: max_qlen*top_k needs %d candidate slots > %d and no scratch was given", a.pmax, MAXC);
        return -1;
    }
    static const bool per_phase = getenv("PFANN_PROF_LAYERS") != nullptr;
    static const bool no_rank = getenv("PFANN_NO_RANK_SORT") != nullptr;
    // rank-sorted phase 1 (match_rank_kernel): 32 workgroups per query, slices of pmax / 32 <= 128 keys
    const bool rank_p1 = a.phase == 1 && !no_rank && a.pmax >= 1024 && a.pmax <= 4096;
    if (a.phase == 1 && per_phase) {     // tuning aid: one profiling tag per phase
        RerankArgs b = a;
        { ProfScope p1("seq_match p1 candidates", s);
          if (rank_p1) PF_LAUNCH(match_rank_kernel<1024>, dim3((unsigned)a.nQ, 32), dim3(1024), (size_t)a.pmax * 8, s, b);
          else PF_LAUNCH(kern, dim3((unsigned)a.nQ), dim3(1024), a.pmax <= MAXC ? (size_t)a.pmax * 12 : 64, s, b); }
        b.phase = 2;
        const unsigned chunks = (unsigned)std::min<int64_t>((a.pmax + 15) / 16, std::max<int64_t>(1, 2048 / a.nQ));
        { ProfScope p2("seq_match p2 scores", s);
          PF_LAUNCH(kern, dim3((unsigned)a.nQ, chunks), dim3(1024), 64, s, b); }
        b.phase = 3;
        { ProfScope p3("seq_match p3 argmax", s);
          PF_LAUNCH(kern, dim3((unsigned)a.nQ), dim3(1024), 64, s, b); }
        PF_HIP(hipGetLastError());
        return 0;
    }
    ProfScope ps("seq_match", s);
    if (a.phase == 1) {
        // few queries: candidates (one workgroup per query) -> scores (all CUs) -> argmax
        RerankArgs b = a;
        if (rank_p1) PF_LAUNCH(match_rank_kernel<1024>, dim3((unsigned)a.nQ, 32), dim3(1024), (size_t)a.pmax * 8, s, b);
        else
        PF_LAUNCH(kern, dim3((unsigned)a.nQ), dim3(1024), a.pmax <= MAXC ? (size_t)a.pmax * 12 : 64, s, b);
        b.phase = 2;
        const unsigned chunks = (unsigned)std::min<int64_t>((a.pmax + 15) / 16, std::max<int64_t>(1, 2048 / a.nQ));
        PF_LAUNCH(kern, dim3((unsigned)a.nQ, chunks), dim3(1024), 64, s, b);
        b.phase = 3;
        PF_LAUNCH(kern, dim3((unsigned)a.nQ), dim3(1024), 64, s, b);
        PF_HIP(hipGetLastError());
        return 0;
    }
    if (a.gkeys != nullptr) {
        PF_LAUNCH(kern, dim3((unsigned)a.nQ), dim3(1024), 64, s, a);
        PF_HIP(hipGetLastError());
        return 0;
    }
    // 16 waves per query: candidate scoring is a latency-bound gather (<= 19 dependent-free row loads
    // per candidate), so more waves in flight per query is what shortens it
    PF_LAUNCH(kern, dim3((unsigned)a.nQ), dim3(1024), (size_t)a.pmax * 12, s, a);
    PF_HIP(hipGetLastError());
    return 0;
}

int launch_match(const RerankArgs &a, hipStream_t s) {
    return a.topn > 0 ? launch_match_as<true>(a, s) : launch_match_as<false>(a, s);
}

// pfann_prewarm: one empty launch per translation unit makes the runtime load this unit's code object now
__global__ void noop_rerank_kernel() {}
int prewarm_rerank() {
    hipLaunchKernelGGL(noop_rerank_kernel, dim3(1), dim3(1), 0, 0);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace pfann
