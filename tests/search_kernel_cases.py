"""Every shape a GPU test holds against an exact reference of the search, in one place (no torch, no GPU).

The GPU tests parametrize over, or read their sizes from, the objects below; tests/test_search_kernel_coverage.py puts the
same objects through the launch plan (csrc/search_plan.h) on the CPU and asserts that every kernel instantiation the search
can launch is reached by at least one of them.  A new instantiation gets its exact-answer case HERE, with the kernel it
was added for in `kernels`, and its GPU test in tests/test_gpu_search_kernel_cases.py.

Case fields:
  name     unique
  n, d     rows and width of the shard the call runs against
  nq, k    query rows of the call (above 16384 the library walks chunks of 16384) and list length
  storage  "f32" fp32 rows, pre-filter off; "copy" fp32 rows, pre-filter on (the fp16 copy exists for d % 8 == 0 and
           n > 0: elsewhere the call is an "f32" one, as pfann_db_load decides); "f16" fp16-only storage
  phase    0 pfann_search_topk (excl: pfann_search_topk_excl), 1 pfann_search_bound (mtop = its m), "2-resume"
           pfann_search_topk_bounded behind the pfann_search_bound of the same rows (a resume only where that left a bound)
  excl     one row range left out per query row
  test     "<module>::<test function>" that runs the shape
  kernels  kernels the plan of the shape must hold: what the case was added for
Shapes drawn at random (test_search_topk_random_shapes) are not listed."""
from collections import namedtuple

Case = namedtuple("Case", "name n d nq k storage phase excl test kernels mtop")
CASES = []
CHUNK = 16384                 # query rows per launch plan (csrc/api.hip walks larger batches in chunks)


def _add(name, n, d, nq, k, storage, test, phase=0, excl=False, kernels=(), mtop=1):
    assert storage in ("f32", "copy", "f16") and phase in (0, 1, "2-resume")
    assert name not in {c.name for c in CASES}, name
    CASES.append(Case(name, n, d, nq, k, storage, phase, excl, test, tuple(kernels), mtop))
    return CASES[-1]


def case(name):
    (c,) = [c for c in CASES if c.name == name]
    return c


def cases_of(test):
    """the cases of one test function ("module::function"), in registry order"""
    out = [c for c in CASES if c.test == test]
    assert out, test
    return out


def plan_storage(c):
    """the storage argument of pfann_search_plan for the case's handle: what pfann_db_load / pfann_db_set_prefilter hand to
    the search (csrc/api.hip) -- 0 fp32 rows only, 1 fp32 rows + fp16 copy, 2 fp16-only"""
    if c.storage == "f16":
        return 2
    return 1 if c.storage == "copy" and c.d % 8 == 0 and c.n > 0 else 0


def bound_m(k, shards):
    """values per query row a rank hands to the bound reduction (pfann_amd/dist.py)"""
    return min(k, 2 * k // shards + 8)


def _two_phase(prefix, test, cuts, d, nq, k, storage, ms, whole=True):
    """the calls of a two-phase sharded search: every shard's bound (one entry per m), its bounded pass and its plain search,
    and the unsplit search"""
    n = cuts[-1] - cuts[0]
    if whole:
        _add("%s_whole" % prefix, n, d, nq, k, storage, test)
    for j, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
        for m in ms:
            _add("%s_shard%d_bound_m%d" % (prefix, j, m), hi - lo, d, nq, k, storage, test, phase=1, mtop=m)
        _add("%s_shard%d_bounded" % (prefix, j), hi - lo, d, nq, k, storage, test, phase="2-resume")
        _add("%s_shard%d_plain" % (prefix, j), hi - lo, d, nq, k, storage, test)


# ------------------------------------------------------------------------------------------------ tests/test_gpu_parity.py
P = "test_gpu_parity::"
PREFILTER_STORAGE = {True: "copy", False: "f32"}

EXACT_SHAPES = [
    (0, 128, 3, 10), (7, 128, 19, 100), (5000, 128, 19, 100), (8192, 64, 5, 1), (8193, 16, 33, 20),
    (100000, 128, 19, 100), (300000, 128, 130, 100), (140000, 128, 64, 300), (200000, 64, 40, 1000),
]
EXACT_PREFILTER = [True, False]
for _pf in EXACT_PREFILTER:
    for _n, _d, _nq, _k in EXACT_SHAPES:
        _add("exact_%d_%d_%d_%d_%s" % (_n, _d, _nq, _k, PREFILTER_STORAGE[_pf]), _n, _d, _nq, _k, PREFILTER_STORAGE[_pf],
             P + "test_search_topk_exact")

CLUSTERED = [
    _add("clustered_nq19", 120000, 128, 19, 100, "copy", P + "test_search_topk_clustered_and_duplicate_rows"),
    _add("clustered_nq139_copy", 120000, 128, 139, 100, "copy", P + "test_search_topk_clustered_and_duplicate_rows"),
    _add("clustered_nq139_f32", 120000, 128, 139, 100, "f32", P + "test_search_topk_clustered_and_duplicate_rows"),
]

LARGE_BATCH_SHAPES = [(40000, 128, 1100, 100), (70001, 64, 1030, 20), (150000, 128, 2100, 300)]
for _n, _d, _nq, _k in LARGE_BATCH_SHAPES:
    _add("large_batch_%d_%d_%d_%d" % (_n, _d, _nq, _k), _n, _d, _nq, _k, "copy", P + "test_search_topk_large_batch_sublists")

MID_BATCH_SHAPES = [(250007, 128, 33), (250007, 128, 76), (250007, 128, 304), (250007, 128, 1000), (130001, 64, 200)]
MID_BATCH_K = 100
for _n, _d, _nq in MID_BATCH_SHAPES:
    _add("mid_batch_%d_%d_%d" % (_n, _d, _nq), _n, _d, _nq, MID_BATCH_K, "copy",
         P + "test_search_topk_mid_batch_takes_the_query_stationary_kernels")

PRIVATE_LISTS_NQ = [130, 2100]
PRIVATE_LISTS = [_add("private_lists_nq%d" % _nq, 150000, 128, _nq, 100, "copy", P + "test_search_topk_private_lists_take_whole_songs")
                 for _nq in PRIVATE_LISTS_NQ]

SUBLIST_OVERFLOW = _add("sublist_overflow", 60000, 128, 1100, 300, "copy", P + "test_search_topk_sublist_overflow_falls_back")

BIG_CLUSTER_NQ = [80, 1100]
BIG_CLUSTER = [_add("big_cluster_nq%d" % _nq, 100000, 128, _nq, 100, "copy", P + "test_search_topk_more_than_4096_survivors")
               for _nq in BIG_CLUSTER_NQ]

NEAR_TIES = _add("near_ties", 60000, 128, 96, 100, "copy", P + "test_search_prefilter_near_ties_stay_exact")

SMALL_OVERFLOW = [
    _add("small_overflow_d64", 1000000, 64, 19, 300, "copy", P + "test_search_small_batch_sublist_overflow_device_fallback"),
    _add("small_overflow_d64_again", 1000000, 64, 17, 100, "copy", P + "test_search_small_batch_sublist_overflow_device_fallback"),
]

TAIL_LAUNCH_PREFILTER = [True, False]
TAIL_LAUNCH = {_pf: [
    _add("tail_launch_%s" % PREFILTER_STORAGE[_pf], 600000, 128, 19, 300, PREFILTER_STORAGE[_pf], P + "test_search_small_batch_d128_tail_launch"),
    _add("tail_launch_%s_again" % PREFILTER_STORAGE[_pf], 600000, 128, 16, 100, PREFILTER_STORAGE[_pf], P + "test_search_small_batch_d128_tail_launch"),
] for _pf in TAIL_LAUNCH_PREFILTER}

F16_FALLBACK_D128 = _add("f16_fallback_d128", 300000, 128, 7, 300, "f16", P + "test_search_small_batch_fp16_storage_fallback_d128")

ZERO_QUERY_NQ = (3, 100)
ZERO_QUERY = [_add("zero_query_nq%d" % _nq, 30000, 128, _nq, 50, "copy", P + "test_search_all_scores_tie_zero_query")
              for _nq in ZERO_QUERY_NQ]

MARGIN_NORMS = _add("margin_norms", 60000, 128, 96, 100, "copy", P + "test_search_prefilter_margin_scales_with_norms")

F16_STORAGE_SHAPES = [(7, 128, 19, 100), (5000, 128, 19, 100), (100000, 128, 19, 100),
                      (90000, 64, 1, 20), (150000, 128, 130, 100), (70001, 64, 1100, 100),
                      (40000, 128, 40, 300)]
for _n, _d, _nq, _k in F16_STORAGE_SHAPES:
    _add("f16_storage_%d_%d_%d_%d" % (_n, _d, _nq, _k), _n, _d, _nq, _k, "f16", P + "test_search_fp16_storage")

QUERY_CHUNKS = _add("query_chunks", 3000, 16, CHUNK + 700, 5, "copy", P + "test_search_chunks_large_query_batches")

# the storage argument of the test -> the registry's: a default handle keeps its fp16 copy and the pre-filter on
TWO_PHASE_STORAGE = ["f32", "f16"]
TWO_PHASE_REGISTRY_STORAGE = {"f32": "copy", "f16": "f16"}
TWO_PHASE = dict(d=128, nq=2100, k=100, cuts=[0, 50000, 90000, 150000])
for _st in TWO_PHASE_STORAGE:
    _two_phase("two_phase_%s" % _st, P + "test_two_phase_sharded_search_is_the_exact_global_topk", TWO_PHASE["cuts"], TWO_PHASE["d"],
               TWO_PHASE["nq"], TWO_PHASE["k"], TWO_PHASE_REGISTRY_STORAGE[_st], (TWO_PHASE["k"], bound_m(TWO_PHASE["k"], 3)))

# -------------------------------------------------------------------------------------------- tests/test_gpu_score_bits.py
S = "test_gpu_score_bits::"
QS_D = [64, 128]
QS_NQ = [33, 76, 304, 1000, 2100]
QS_N, QS_K = 60001, 100
for _nq in QS_NQ:
    for _d in QS_D:
        _add("bits_query_stationary_nq%d_d%d" % (_nq, _d), QS_N, _d, _nq, QS_K, "copy", S + "test_query_stationary_batches_select_small")

BITS_BIG_CLUSTER_NQ = [80, 1100]
BITS_BIG_CLUSTER = [_add("bits_big_cluster_nq%d" % _nq, 100000, 128, _nq, 100, "copy", S + "test_more_than_4096_survivors_select_body")
                    for _nq in BITS_BIG_CLUSTER_NQ]
BITS_SUBLIST_OVERFLOW = _add("bits_sublist_overflow", 60000, 128, 1100, 300, "copy", S + "test_sublist_overflow_fallback_fp32_rows")
BITS_FOLDED = _add("bits_folded_small_d128", 600000, 128, 20, 300, "copy", S + "test_folded_small_path_d128")
BITS_UNFOLDED = _add("bits_unfolded_small_d64", 1000000, 64, 19, 300, "copy", S + "test_unfolded_small_path_d64")

GENERIC_LADDER_N = 50000
GENERIC_LADDER = [(128, 40, 300), (128, 70, 1000), (96, 100, 100), (96, 33, 20)]          # d, nq, k
for _d, _nq, _k in GENERIC_LADDER:
    _add("bits_generic_ladder_%d_%d_%d" % (_d, _nq, _k), GENERIC_LADDER_N, _d, _nq, _k, "copy", S + "test_generic_ladder")

DENSE_SMALL = [(128, 7, 19, 100), (128, 5000, 19, 100), (64, 8192, 5, 1), (128, 8192, 32, 1000), (64, 3000, 1, 20)]   # d, n, nq, k
for _d, _n, _nq, _k in DENSE_SMALL:
    _add("bits_dense_small_%d_%d_%d_%d" % (_d, _n, _nq, _k), _n, _d, _nq, _k, "copy", S + "test_dense_small_shard")

BITS_MARGIN = _add("bits_margin_non_unit", 60000, 128, 96, 100, "copy", S + "test_margin_non_unit_norms")

BOUNDED = dict(d=128, nq=300, k=100, cuts=[0, 50000, 90000, 150000])
_two_phase("bits_bounded", S + "test_bounded_second_phase", BOUNDED["cuts"], BOUNDED["d"], BOUNDED["nq"], BOUNDED["k"], "copy",
           (bound_m(BOUNDED["k"], 3),))

# one query row on every path: searched alone, in two batches, and as a two-phase search over two cuts of the database
ONE_ROW = dict(d=128, n=60000, k=100, batches=(100, 2100), small_batches=(1, 19),
               cuts=[0, 20000, 40000, 60000], cuts_dense=[0, 8000, 40000, 60000])
_T = S + "test_one_row_same_bits_on_every_path"
_add("bits_one_row_alone", ONE_ROW["n"], ONE_ROW["d"], 1, ONE_ROW["k"], "copy", _T)
for _nq in ONE_ROW["batches"]:
    _add("bits_one_row_batch%d" % _nq, ONE_ROW["n"], ONE_ROW["d"], _nq, ONE_ROW["k"], "copy", _T)


def _one_row_two_phase(prefix, cuts, nq):
    for j, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
        _add("%s_shard%d_bound" % (prefix, j), hi - lo, ONE_ROW["d"], nq, ONE_ROW["k"], "copy", _T, phase=1, mtop=bound_m(ONE_ROW["k"], 3))
        _add("%s_shard%d_bounded" % (prefix, j), hi - lo, ONE_ROW["d"], nq, ONE_ROW["k"], "copy", _T, phase="2-resume")


for _nq in ONE_ROW["batches"]:
    _one_row_two_phase("bits_one_row_two_phase_batch%d" % _nq, ONE_ROW["cuts"], _nq)
for _nq in ONE_ROW["small_batches"]:                         # (the rows under test are two: a batch of "1" holds 2 rows)
    _one_row_two_phase("bits_one_row_two_phase_dense_batch%d" % _nq, ONE_ROW["cuts_dense"], max(_nq, 2))
    _one_row_two_phase("bits_one_row_two_phase_batch%d" % _nq, ONE_ROW["cuts"], max(_nq, 2))

# ------------------------------------------------------------------------------------------ tests/test_gpu_search_excl.py
X = "test_gpu_search_excl::"
EXCL_CASES = [
    # name, n, d, nq, k, storage, path, a masked kernel the plan must hold
    ("small_dense", 300, 128, 5, 10, "copy", "small_dense", "scan_small_kernel<128, 4, 2, true>"),
    ("small_dense_d64", 300, 64, 5, 10, "copy", "small_dense", "scan_small_kernel<64, 4, 2, true>"),
    ("folded_nq1", 12288, 128, 1, 100, "copy", "small_sampled_folded", "scan_small_kernel<128, 2, 0, true>"),
    ("folded_nq19", 12288, 128, 19, 100, "copy", "small_sampled_folded", "select_tail_kernel<4, true>"),
    ("sampled_d64_nq1", 12288, 64, 1, 100, "copy", "small_sampled", "scan_small_kernel<64, 2, 1, true>"),
    ("sampled_d64_nq19", 12288, 64, 19, 100, "copy", "small_sampled", "scan_small_kernel<64, 2, 0, true>"),
    ("gmax_nq33", 40000, 128, 33, 100, "copy", "gmax", "scan_f16_qres_kernel<8, true, 128, 3, true>"),
    ("gmax_nq130", 40000, 128, 130, 100, "copy", "gmax", "scan_f16_qres_kernel<8, false, 64, 3, true>"),
    ("gmax_d64", 40000, 64, 130, 100, "copy", "gmax", "scan_f16_qres_kernel<4, true, 128, 2, true>"),
    ("ladder_f16", 20000, 128, 130, 100, "copy", "ladder_f16", "scan_f16_kernel<1, true>"),
    ("ladder_f16_k200", 20000, 128, 130, 200, "copy", "ladder_f16", "scan_f16_qres_kernel<8, false, 128, 2, true>"),
    # fp32 rows only.  nq = 19 at d = 128 is the small path on the fp32 streaming kernels (the plan says so); the ladder
    # itself takes <= 32 query rows only at another d
    ("f32_nq19", 20000, 128, 19, 100, "f32", "small_sampled_folded", "scan_small_kernel<128, 4, 0, true>"),
    ("ladder_f32_nq19", 20000, 96, 19, 100, "f32", "ladder_f32", "scan_emit_kernel<32, 128, 32, 32, 1, true>"),
    ("ladder_f32_nq50", 20000, 128, 50, 100, "f32", "ladder_f32", "scan_emit_kernel<64, 64, 32, 32, 1, true>"),
    ("ladder_f32_nq130", 20000, 128, 130, 100, "f32", "ladder_f32", "scan_emit_kernel<128, 128, 64, 64, 1, true>"),
    ("f16_small", 300, 128, 5, 10, "f16", "small_dense", "scan_small_kernel<128, 2, 2, true>"),
    ("f16_sampled", 12288, 128, 19, 100, "f16", "small_sampled_folded", "select_tail_kernel<2, true>"),
    ("f16_batched", 40000, 128, 130, 100, "f16", "gmax", "topk_fallback_kernel<2, true>"),
    ("f16_ladder", 20000, 128, 130, 200, "f16", "ladder_f16", "scan_f16_kernel<1, true>"),
]
for _c in EXCL_CASES:
    _add("excl_" + _c[0], _c[1], _c[2], _c[3], _c[4], _c[5], X + "test_own_song_excluded", excl=True, kernels=(_c[7],))

# The group-maximum pass samples every gs-th row, gs = the coarsest of 4, 2, 1 that leaves 4 tiles of 128 sampled rows per
# slice (search_plan.h).  With one to five query tiles there are 64 slices, so gs = 4 from n = 131,072 rows, gs = 2 from
# 65,536, and the 40,000-row shapes above all run at gs = 1.  The plan text does not print the stride, so these shapes
# come from that rule; what the text does show, the kernel, is asserted.  A million-row database runs at gs = 4.
EXCL_STRIDED = [
    # name, n, d, nq, modes, the masked sampled pass
    ("stride2_nbuf3", 70000, 128, 130, ("run",), "scan_f16_qres_kernel<8, true, 128, 3, true>"),
    ("stride2_d64", 70000, 64, 130, ("run",), "scan_f16_qres_kernel<4, true, 128, 2, true>"),
    ("stride4_nbuf2", 140000, 128, 600, ("run",), "scan_f16_qres_kernel<8, true, 128, 2, true>"),
]
EXCL_STRIDED_K = 100
for _c in EXCL_STRIDED:
    _add("excl_" + _c[0], _c[1], _c[2], _c[3], EXCL_STRIDED_K, "copy", X + "test_sampled_pass_with_a_row_stride", excl=True, kernels=(_c[5],))

# ---------------------------------------------------------------------------------- tests/test_gpu_search_kernel_cases.py
# The smallest shapes that reach, under default tuning, the kernel instantiations no older test held against an exact
# answer.  `kernels` is what each was added for: the GPU test asserts it from the handle's plan, the coverage test from
# the shape's.
N = "test_gpu_search_kernel_cases::"


def _twin(kernel):
    return kernel[:-1] + ", true>"


def _new(name, n, d, nq, k, storage, test, kernels, excl=False, **kw):
    c = _add(name, n, d, nq, k, storage, N + test, kernels=kernels, **kw)
    if excl:
        _add(name + "_excl", n, d, nq, k, storage, N + test, excl=True, kernels=[_twin(kn) for kn in kernels], **kw)
    return c


# d = 64, <= 32 query rows, fp32 rows without the pre-filter: the sampled and the full streaming pass in fp32 (and, through
# one row whose sub-list overflows, the fp32 fallback)
_new("small64_f32", 12288, 64, 19, 100, "f32", "test_small_d64_fp32_streaming",
     ["scan_small_kernel<64, 4, 1>", "scan_small_kernel<64, 4, 0>", "topk_fallback_kernel<4>"], excl=True)
# <= 32 query rows at a d the small path does not take: the fp32 ladder on 32-row query tiles (found by the coverage test:
# the masked twin had a case, tests/test_gpu_search_excl.py ladder_f32_nq19, the unmasked kernel none)
_new("emit32_f32", 20000, 96, 19, 100, "f32", "test_fp32_ladder_small_batch", ["scan_emit_kernel<32, 128, 32, 32, 1>"])
# d = 64, fp16-only storage, n <= 8192: the dense pass
_new("small64_f16_dense", 5000, 64, 5, 10, "f16", "test_small_d64_fp16_dense", ["scan_small_kernel<64, 2, 2>"], excl=True)
_new("small64_f16_dense_n8192", 8192, 64, 5, 1, "f16", "test_small_d64_fp16_dense", ["scan_small_kernel<64, 2, 2>"], excl=True)
# 2049 db tiles x ceil(5 / 4) groups of query tiles = 4098 >= 4096 workgroups: the long-run forms of the generic scans.
# Five query tiles: one full group of four, and a group of ONE tile whose only row is query 512.
QT4_N, QT4_NQ = 262200, 513
_new("emit_qt4", QT4_N, 128, QT4_NQ, 100, "f32", "test_long_query_tile_runs", ["scan_emit_kernel<128, 128, 64, 64, 4>"], excl=True)
_new("emit_qt4_d36", QT4_N, 36, QT4_NQ, 100, "f32", "test_long_query_tile_runs", ["scan_emit_kernel<128, 128, 64, 64, 4>"])
_new("f16_qt4", QT4_N, 96, QT4_NQ, 100, "copy", "test_long_query_tile_runs", ["scan_f16_kernel<4>"], excl=True)
_new("f16_qt4_half", QT4_N, 96, QT4_NQ, 100, "f16", "test_long_query_tile_runs", ["scan_f16_kernel<4>"])
# masked full pass on two tile buffers: 12 query tiles x 64 slices = 768 workgroups
_add("dbr64_nbuf2_excl", 40000, 128, 1500, 100, "copy", N + "test_masked_full_pass_on_two_tile_buffers", excl=True,
     kernels=["scan_f16_qres_kernel<8, false, 64, 2, true>"])
# the wave-per-row group select with 16 values per lane: G = 1024 (all 16) and G = 832 (13, the benchmark's launch group)
WAVE16 = ["group_max_select_wave_kernel<16>"]
_add("wave16_full", 8320, 128, 8065, 100, "copy", N + "test_wave_group_select_16", kernels=WAVE16)
_add("wave16_full_excl", 8320, 128, 8065, 100, "copy", N + "test_wave_group_select_16", excl=True, kernels=WAVE16)
for _d in (128, 64):
    for _st in ("copy", "f16"):
        _add("wave16_bench_d%d_%s" % (_d, _st), 8320, _d, 9728, 100, _st, N + "test_wave_group_select_16", kernels=WAVE16)
# phase 1 of the sharded search on the wave selects (topm)
WAVE_TOPM = dict(d=128, nq=9728, k=100, cuts=[0, 8320, 17320, 25020])
WAVE_TOPM_STORAGE = ["copy", "f16"]
WAVE8_TOPM = dict(d=128, nq=16384, k=100, cuts=[0, 8320])


def _topm(prefix, spec, storage, kernel):
    k, cuts, m = spec["k"], spec["cuts"], bound_m(spec["k"], 3)
    T = N + "test_wave_group_select_topm"
    _add("%s_whole" % prefix, cuts[-1], spec["d"], spec["nq"], k, storage, T)
    for j, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
        _add("%s_shard%d_bound" % (prefix, j), hi - lo, spec["d"], spec["nq"], k, storage, T, phase=1, mtop=m, kernels=[kernel])
        _add("%s_shard%d_bounded" % (prefix, j), hi - lo, spec["d"], spec["nq"], k, storage, T, phase="2-resume", kernels=["bound_in_kernel"])


for _st in WAVE_TOPM_STORAGE:
    _topm("wave_topm_%s" % _st, WAVE_TOPM, _st, "group_max_select_wave_kernel<16>")
_topm("wave8_topm", WAVE8_TOPM, "copy", "group_max_select_wave_kernel<8>")
# pfann_search_bound where no sampled threshold exists: small batch, k > 128, fp32 rows only, empty shard
BOUND_NONE_SHAPES = [(20000, 128, 19, 100, "copy"), (20000, 128, 130, 200, "copy"), (20000, 128, 130, 100, "f32"), (0, 128, 130, 100, "copy")]
for _n, _d, _nq, _k, _st in BOUND_NONE_SHAPES:
    _nm = "bound_none_%d_%d_%d_%s" % (_n, _nq, _k, _st)
    _add(_nm, _n, _d, _nq, _k, _st, N + "test_bound_without_a_sampled_threshold", phase=1, mtop=bound_m(_k, 3), kernels=["bound_none_kernel"])
    _add(_nm + "_bounded", _n, _d, _nq, _k, _st, N + "test_bound_without_a_sampled_threshold", phase="2-resume")
    _add(_nm + "_plain", _n, _d, _nq, _k, _st, N + "test_bound_without_a_sampled_threshold")
