"""Host mirror of the reference's retrieval interface (database.py:74-195):
`Database(dir_for_db, indexer_params, hop_size)` and
`Database.query_embeddings(query) -> (score, (song_id, time_s), song_score[n_songs,2])`.

The fingerprints live in HBM; search (exact flat inner-product top-k) and the sequence
matcher run as HIP kernels (csrc/search.hip, csrc/rerank.hip).  `query_batch` exposes the
batched form the CLIs and bench use; `query_embeddings` keeps the reference's per-query
contract, python-path semantics (cpp_accelerate=False, database.py:12).
"""
import contextlib
import ctypes
import itertools
import json
import os
import struct
import time

import numpy as np
import torch

from . import faissio
from . import lib as _l
from .utils import read_file_list


def song_pos_from_key(landmark_key):
    return np.pad(np.cumsum(np.asarray(landmark_key), dtype=np.int64), (1, 0))      # database.py:86


def search_plan(n, d, nq, k, storage, phase=0, resume_with_lb=False, mtop=1, excl=False):
    """pfann_search_plan parsed: storage 0 = fp32 rows only, 1 = fp32 rows + fp16 copy, 2 = fp16-only -> (stages, flags).
    excl: the plan of the search with a row range left out per query row (pfann_search_plan_excl; phase 0 only)."""
    lib = _l.load()
    buf = ctypes.create_string_buffer(16384)
    if excl:
        if phase != 0:
            raise ValueError("search_plan: the masked search has no sharded halves (phase %r)" % (phase,))
        _l.check(lib.pfann_search_plan_excl(n, d, nq, k, storage, buf, len(buf)), "pfann_search_plan_excl")
    else:
        _l.check(lib.pfann_search_plan(n, d, nq, k, storage, phase, 1 if resume_with_lb else 0, mtop, buf, len(buf)),
                 "pfann_search_plan")
    lines = buf.value.decode().splitlines()
    stages = []
    for ln in lines[:-1]:
        name, rest = ln.rsplit(" grid=", 1)
        g, b, l = (int(x.split("=")[-1]) for x in rest.replace("grid=", "").split(" "))
        stages.append((name, g, b, l))
    assert lines[-1].startswith("flags "), lines[-1]
    return stages, dict(kv.split("=", 1) for kv in lines[-1].split(" ")[1:])


class DeviceIndex:
    """One shard of fingerprints on one GPU + its search / match kernels."""

    def __init__(self, d, device=0, storage="f32"):
        """storage "f32" (default; exact fp32 results) or "f16": only fp16 rows are kept and searched on the fp16
        matrix cores without fp32 re-scoring (half the footprint and scan bytes; approximate like faiss'
        useFloat16, database.py:101-104)."""
        _l.require_gpu()
        self.lib = _l.load()
        self.d = d
        self.device = torch.device("cuda", device)
        self.handle = self.lib.pfann_db_create(d, device)
        if not self.handle:
            raise _l.PfannError("pfann_db_create failed: " + _l.last_error())
        self.storage = storage
        _l.check(self.lib.pfann_db_set_storage(self.handle, {"f32": 0, "f16": 1}[storage]), "pfann_db_set_storage")
        self.ntotal = 0
        self.label_base = 0
        self.n_songs = 0
        self._small_args = {}
        self._prefilter = True
        self._host_res = None

    def __del__(self):
        h, self.handle = getattr(self, "handle", None), None
        if h:
            self.lib.pfann_db_destroy(h)

    def load(self, emb, song_pos, label_base=0, song_range=None):
        """emb: float32 [n, d] numpy (host) or torch cuda tensor; song_pos: GLOBAL int64 prefix sums.  song_range: the
        caller's own cut (song_lo, song_hi) of the song list when it made one (dist.shard_songs) -- songs without rows at
        a shard boundary belong to the side the cut says; by default the library derives the songs from the rows."""
        song_pos = np.ascontiguousarray(song_pos, dtype=np.int64)
        self.song_pos = song_pos
        self.n_songs = song_pos.shape[0] - 1
        if isinstance(emb, torch.Tensor) and emb.is_cuda:
            e = emb.to(torch.float32).contiguous()
            ptr, is_dev, n = e.data_ptr(), 1, e.shape[0]
        else:
            e = np.ascontiguousarray(emb.cpu().numpy() if isinstance(emb, torch.Tensor) else emb, np.float32)
            e = e.reshape(-1, self.d)
            ptr, is_dev, n = e.ctypes.data, 0, e.shape[0]
        _l.check(self.lib.pfann_db_load(self.handle, ptr, is_dev, n,
                                        song_pos.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                        self.n_songs, label_base), "pfann_db_load")
        self.ntotal = n
        self.label_base = label_base
        if song_range is not None:
            _l.check(self.lib.pfann_db_set_owned_songs(self.handle, int(song_range[0]), int(song_range[1])),
                     "pfann_db_set_owned_songs")

    # ---- updates (include/pfann_amd.h: "Database updates"): blocking maintenance calls, never beside a query on this index
    def reserve(self, rows, songs=0):
        """room for `rows` rows and `songs` songs without reallocation (never shrinks) -> capacity in rows"""
        _l.check(self.lib.pfann_db_reserve(self.handle, int(rows), int(songs)), "pfann_db_reserve")
        return self.capacity()

    def capacity(self):
        return int(self.lib.pfann_db_capacity(self.handle))

    def row_norm_max(self):
        return float(self.lib.pfann_db_row_norm_max(self.handle))

    def append(self, emb, rows_per_song):
        """New songs behind the last one: emb float32 [sum(rows_per_song), d] (numpy, or a torch cuda tensor), one entry of
        rows_per_song per song (0 allowed) -> the id of the first new song.  A refused call leaves the index as it was."""
        rps = np.ascontiguousarray(rows_per_song, dtype=np.int32).reshape(-1)
        if isinstance(emb, torch.Tensor) and emb.is_cuda:
            e = emb.to(torch.float32).contiguous().reshape(-1, self.d)
            ptr, is_dev, n = e.data_ptr(), 1, e.shape[0]
        else:
            e = np.ascontiguousarray(emb.cpu().numpy() if isinstance(emb, torch.Tensor) else emb, np.float32).reshape(-1, self.d)
            ptr, is_dev, n = e.ctypes.data, 0, e.shape[0]
        _l.check(self.lib.pfann_db_append(self.handle, ptr, is_dev, n, rps.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                          rps.shape[0]), "pfann_db_append")
        first = self.n_songs
        base = getattr(self, "song_pos", np.zeros(1, np.int64))
        self.song_pos = np.concatenate([base, base[-1] + np.cumsum(rps, dtype=np.int64)])
        self.n_songs += rps.shape[0]
        self.ntotal += n
        return first

    def remove_songs(self, songs):
        """The songs (ids, any order) lose their rows and keep their ids; later rows move down."""
        ids = np.ascontiguousarray(songs, dtype=np.int32).reshape(-1)
        _l.check(self.lib.pfann_db_remove_songs(self.handle, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ids.shape[0]),
                 "pfann_db_remove_songs")
        lens = np.diff(self.song_pos)
        lens[ids] = 0
        self.song_pos = np.pad(np.cumsum(lens, dtype=np.int64), (1, 0))
        self.ntotal = int(self.song_pos[-1])

    def set_prefilter(self, on=True):
        """fp16 pre-filter of the batched scan (exact result either way) -> True if in use."""
        self._prefilter = bool(on)
        return bool(self.lib.pfann_db_set_prefilter(self.handle, 1 if on else 0))

    def search_plan(self, nq, k, phase=0, resume_with_lb=False, mtop=1, excl=False):
        """What search (phase 0), search_bound (1, mtop = its m) or search_bounded (2; resume_with_lb: behind the
        search_bound of the same q) launches for nq query rows against this shard, from pfann_search_plan: ->
        (stages, flags), stages = [(kernel, grid, block, dynamic LDS bytes)] in launch order, flags = the dict of the last
        line (path, q_prep, fallback, canonical_scores, ...).  No GPU work."""
        if self.storage == "f16":
            storage = 2
        else:
            storage = 1 if self.lib.pfann_db_set_prefilter(self.handle, 1 if self._prefilter else 0) else 0
        return search_plan(self.ntotal, self.d, nq, k, storage, phase, resume_with_lb, mtop, excl)

    def _stream(self):
        return _l.current_stream_ptr(self.device)

    def search(self, q, k, exclude=None):
        """index.search(q, k): q torch cuda [nq, d] -> (D [nq,k] f32 desc, I [nq,k] int64) on device.
        exclude = (lo, hi), two int64 tensors or arrays of length nq: query row m is answered over the rows whose label is
        not in [lo[m], hi[m]) (pfann_search_topk_excl: exact, not a post-filter; lo >= hi excludes nothing)."""
        q = q.to(self.device, torch.float32).contiguous()
        nq = q.shape[0]
        D = torch.empty((nq, k), device=self.device, dtype=torch.float32)
        I = torch.empty((nq, k), device=self.device, dtype=torch.int64)
        if exclude is not None:
            lo, hi = (x.to(self.device, torch.int64).contiguous() if isinstance(x, torch.Tensor)
                      else _l.upload_async(np.asarray(x), self.device, np.int64) for x in exclude)
            if lo.shape != (nq,) or hi.shape != (nq,):
                raise ValueError("search: exclude wants two arrays of %d rows (got %r, %r)" % (nq, tuple(lo.shape), tuple(hi.shape)))
            if nq:
                _l.check(self.lib.pfann_search_topk_excl(self.handle, q.data_ptr(), nq, k, lo.data_ptr(), hi.data_ptr(),
                                                         D.data_ptr(), I.data_ptr(), self._stream()), "pfann_search_topk_excl")
            return D, I
        if nq:
            _l.check(self.lib.pfann_search_topk(self.handle, q.data_ptr(), nq, k, D.data_ptr(), I.data_ptr(),
                                                self._stream()), "pfann_search_topk")
        return D, I

    BOUND_CHUNK = 16384        # query rows per pfann_search_bound / pfann_search_topk_bounded call

    def search_bound(self, q, k, m=1):
        """First half of a sharded search (<= BOUND_CHUNK rows): -> [nq, m] f32 on the device: per query row the m best
        sampled scores of THIS shard (m different real rows), each lowered to a bound of its exact score; -inf padded (all
        -inf where no sampled threshold exists).  reduce_bound over the ranks' tensors gives what search_bounded wants."""
        nq = q.shape[0]
        lb = torch.empty((nq, m), device=self.device, dtype=torch.float32)
        if nq:
            _l.check(self.lib.pfann_search_bound(self.handle, q.data_ptr(), nq, k, m, lb.data_ptr(), self._stream()),
                     "pfann_search_bound")
        return lb

    def reduce_bound(self, cands, k):
        """cands [n_ranks, nq, m] (all-gathered search_bound outputs) -> [nq]: the k-th largest of every row's union, a lower
        bound of the row's k-th best score over all shards (>= k different real rows reach it); -FLT_MAX when the union
        holds fewer than k finite values."""
        G, nq, m = cands.shape
        if G * m <= 1024 and nq:
            # one wavefront per row straight from the gathered layout (pfann_bound_reduce): a selection, not a sort
            c = cands.to(self.device, torch.float32).contiguous()
            lb = torch.empty((nq,), device=self.device, dtype=torch.float32)
            _l.check(self.lib.pfann_bound_reduce(self.handle, c.data_ptr(), G, nq, m, k, lb.data_ptr(), self._stream()),
                     "pfann_bound_reduce")
            return lb
        vals = cands.to(self.device).permute(1, 0, 2).reshape(nq, G * m).contiguous()
        if G * m < k:
            return torch.full((nq,), -3.4028234663852886e38, device=self.device, dtype=torch.float32)
        labels = torch.where(torch.isfinite(vals), torch.arange(G * m, device=self.device, dtype=torch.int64).expand(nq, -1),
                             torch.full_like(vals, -1, dtype=torch.int64)).contiguous()
        D, _ = self.merge_topk(vals, labels, k)
        return D[:, k - 1].contiguous()

    def search_bounded(self, q, k, lb):
        """Second half: (D, I) of this shard restricted to rows that can be in the global top-k (padded with
        -FLT_MAX / -1); q must be the very tensor search_bound was given."""
        nq = q.shape[0]
        D = torch.empty((nq, k), device=self.device, dtype=torch.float32)
        I = torch.empty((nq, k), device=self.device, dtype=torch.int64)
        if nq:
            _l.check(self.lib.pfann_search_topk_bounded(self.handle, q.data_ptr(), nq, k, lb.contiguous().data_ptr(),
                                                        D.data_ptr(), I.data_ptr(), self._stream()),
                     "pfann_search_topk_bounded")
        return D, I

    def merge_lists(self, Dl, Il, k):
        """Dl / Il [G, nq, k] (every shard's list for these query rows, as the all-to-all delivers them) -> exact top-k of
        the union (D [nq, k] descending, I), ties to the lower shard: the merge of ShardedIndex.search_global."""
        G, nq, kk = Dl.shape
        if kk == k and k <= 128 and G * k <= 1024:
            Dl, Il = Dl.to(self.device, torch.float32).contiguous(), Il.to(self.device, torch.int64).contiguous()
            D = torch.empty((nq, k), device=self.device, dtype=torch.float32)
            I = torch.empty((nq, k), device=self.device, dtype=torch.int64)
            if nq:
                _l.check(self.lib.pfann_topk_merge_lists(self.handle, Dl.data_ptr(), Il.data_ptr(), G, nq, k, D.data_ptr(),
                                                         I.data_ptr(), self._stream()), "pfann_topk_merge_lists")
            return D, I
        S = Dl.permute(1, 0, 2).reshape(nq, G * kk).contiguous()            # shard-major: ascending labels on ties
        L = Il.permute(1, 0, 2).reshape(nq, G * kk).contiguous()
        return self.merge_topk(S, L, k)

    def merge_topk(self, S, L, k):
        nq, m = S.shape
        D = torch.empty((nq, k), device=self.device, dtype=torch.float32)
        I = torch.empty((nq, k), device=self.device, dtype=torch.int64)
        if nq:
            _l.check(self.lib.pfann_topk_merge(self.handle, S.contiguous().data_ptr(), L.contiguous().data_ptr(),
                                               nq, m, k, D.data_ptr(), I.data_ptr(), self._stream()),
                     "pfann_topk_merge")
        return D, I

    RESULT_DTYPE = np.dtype([("song", "<i4"), ("offset", "<i4"), ("shift", "<i4"), ("n_cand", "<i4"), ("score", "<f8")])

    @classmethod
    def decode_results(cls, raw, shape=-1):
        """Result bytes -> RESULT_DTYPE array, the ONE place that reads them: a tensor of 24-byte results ([..., 24] uint8, on
        the device -- then this is the one device-to-host copy of a step -- or the pinned buffer the kernel wrote into) gives
        the shape of its leading dimensions, host bytes give `shape`.  A song of -2 is the matcher's refusal."""
        if isinstance(raw, torch.Tensor):
            raw, shape = raw.cpu().numpy().tobytes(), tuple(raw.shape[:-1])
        out = np.frombuffer(raw, dtype=cls.RESULT_DTYPE).reshape(shape)
        if (out["song"] == -2).any():
            raise _l.PfannError("matcher refused a query (candidate buffer sizing error)")
        return out

    def results_to_host(self, res_dev):
        """device results (uint8 [nQ, 24]) -> structured numpy array: the ONE device-to-host copy of a step."""
        return self.decode_results(res_dev)

    def pack_winner_keys(self, res_dev):
        """-> int64 [nQ, 2] device tensor of 128-bit keys (bit patterns of two uint64), see pfann_match_pack."""
        nQ = res_dev.shape[0]
        keys = torch.empty((nQ, 2), device=self.device, dtype=torch.int64)
        _l.check(self.lib.pfann_match_pack(self.handle, res_dev.data_ptr(), nQ, keys.data_ptr(), self._stream()), "pfann_match_pack")
        return keys

    def pick_winner(self, all_keys, to_host=True):
        """all_keys int64 [G, nQ, 2] (all-gathered) -> structured array of the winners (one D2H), or with to_host=False
        the device tensor of results (results_to_host turns it into the array later)."""
        all_keys = all_keys.to(self.device).contiguous()
        G, nQ = all_keys.shape[0], all_keys.shape[1]
        out = torch.empty((nQ, ctypes.sizeof(_l.MatchResult)), device=self.device, dtype=torch.uint8)
        _l.check(self.lib.pfann_match_pick(self.handle, all_keys.data_ptr(), G, nQ, out.data_ptr(), self._stream()), "pfann_match_pick")
        return self.results_to_host(out) if to_host else out

    def owned_songs(self):
        """-> (song_lo, song_hi): the songs whose rows all live in this shard"""
        lo, hi = ctypes.c_int(0), ctypes.c_int(0)
        self.lib.pfann_db_owned_songs(self.handle, ctypes.byref(lo), ctypes.byref(hi))
        return lo.value, hi.value

    def song_scores_to_seconds(self, ss, fsm, hop_size, native_path=False):
        """in place: the alignment slot of every (score, alignment) pair of a song_scores block, fine frames -> seconds"""
        if ss is not None and ss.numel():
            _l.check(self.lib.pfann_song_scores_to_seconds(self.handle, ss.data_ptr(), ss.numel() // 2, int(fsm), float(hop_size),
                                                           1 if native_path else 0, self._stream()),
                     "pfann_song_scores_to_seconds")
        return ss

    def _match_args(self, q, labels, start, length):
        """the matchers' shared arguments -> (q float32, labels int64 on the device; start int64, length int32 host arrays)"""
        return (q.to(self.device, torch.float32).contiguous(), labels.to(self.device, torch.int64).contiguous(),
                np.ascontiguousarray(start, dtype=np.int64), np.ascontiguousarray(length, dtype=np.int32))

    def _upload_ranges(self, start_np, length_np):
        return _l.upload_async(start_np, self.device, np.int64), _l.upload_async(length_np, self.device, np.int32)

    def match(self, q, labels, qstart, qlen, fsm=1, alpha=0.0, mode=0, only_owned=False, want_song_scores=False,
              to_host=True, owned_block=False):
        """Sequence matcher for nQ queries.  Returns (results structured array -- or, with to_host=False, the device
        tensor of results --, song_scores or None).  owned_block (with only_owned): song_scores is [nQ, owned songs, 2],
        this shard's columns of the score matrix, instead of [nQ, n_songs, 2]."""
        q, labels, qs_np, ql_np = self._match_args(q, labels, qstart, qlen)
        nQ = int(ql_np.shape[0])
        if nQ <= 4:
            # the one-query regime calls with the same tiny (qstart, qlen) over and over: keep their device copies
            key = (qs_np.tobytes(), ql_np.tobytes())
            hit = self._small_args.get(key)
            if hit is None:
                if len(self._small_args) > 64:
                    self._small_args.clear()
                hit = self._small_args[key] = self._upload_ranges(qs_np, ql_np)
            qs, ql = hit
        else:
            qs, ql = self._upload_ranges(qs_np, ql_np)
        k = labels.shape[1]
        rsz = ctypes.sizeof(_l.MatchResult)
        host_res = None
        if to_host and 0 < nQ <= 64:
            # few queries: the kernel writes its 24-byte results straight into pinned (device-mapped) host memory, so the
            # answer is on the host when the stream has drained -- no device-to-host copy call on the latency path
            if self._host_res is None:
                self._host_res = torch.empty((64, rsz), dtype=torch.uint8, pin_memory=True)
            host_res = self._host_res[:nQ]
            res = host_res
        else:
            res = torch.empty((nQ, rsz), device=self.device, dtype=torch.uint8)
        ss = None
        if want_song_scores:
            lo, hi = self.owned_songs() if owned_block else (0, self.n_songs)
            ss = torch.zeros((nQ, hi - lo, 2), device=self.device, dtype=torch.float32)
        if nQ:
            _l.check(self.lib.pfann_match(self.handle, q.data_ptr(), labels.data_ptr(), k, qs.data_ptr(),
                                          ql.data_ptr(), nQ, int(ql_np.max()), fsm, float(alpha), mode,
                                          (1 if only_owned else 0) | (2 if owned_block else 0), res.data_ptr(),
                                          ss.data_ptr() if ss is not None else None, self._stream()),
                     "pfann_match")
        if not to_host:
            return res, ss
        if host_res is not None:
            torch.cuda.current_stream(self.device).synchronize()
            return self.decode_results(host_res), ss
        return self.results_to_host(res), ss

    def topn_to_host(self, top_dev, n_found_dev):
        """device top-N lists (uint8 [nQ, n, 24]) and counts -> (structured array [nQ, n], int32 [nQ])"""
        return self.decode_results(top_dev), n_found_dev.cpu().numpy()

    def match_topn(self, q, labels, qstart, qlen, n, fsm=1, alpha=0.0, mode=0, only_owned=False, to_host=True):
        """Ranked answers (pfann_match_topn): the n best songs of each of nQ queries, selected on the device -- no per-song
        block.  -> (structured array [nQ, n] of RESULT_DTYPE, n_found int32 [nQ]); entry [j, 0] is `match`'s answer,
        entries past the candidate songs are song -1 / score -inf; with to_host=False the two device tensors (uint8
        [nQ, n, 24], int32 [nQ]) that topn_to_host turns into the arrays later."""
        q, labels, qs_np, ql_np = self._match_args(q, labels, qstart, qlen)
        nQ, n = int(ql_np.shape[0]), self._check_n("match_topn", n)
        qs, ql = self._upload_ranges(qs_np, ql_np)
        top = torch.empty((nQ, n, ctypes.sizeof(_l.MatchResult)), device=self.device, dtype=torch.uint8)
        n_found = torch.empty((nQ,), device=self.device, dtype=torch.int32)
        if nQ:
            _l.check(self.lib.pfann_match_topn(self.handle, q.data_ptr(), labels.data_ptr(), labels.shape[1], qs.data_ptr(),
                                               ql.data_ptr(), nQ, int(ql_np.max()), int(fsm), float(alpha), int(mode),
                                               1 if only_owned else 0, n, top.data_ptr(), n_found.data_ptr(), self._stream()),
                     "pfann_match_topn")
        if not to_host:
            return top, n_found
        return self.topn_to_host(top, n_found)

    @staticmethod
    def _check_n(what, n):
        """-> n as an int, or the refusal of a ranked list that is not 1..64 long"""
        n = int(n)
        if not 1 <= n <= 64:
            raise _l.PfannError("%s: n=%d outside 1..64" % (what, n))
        return n

    @staticmethod
    def _window_hop(what, window, hop):
        """-> (window, hop) as ints, or the ValueError every windowed call raises first"""
        window, hop = int(window), int(hop)
        if window < 1 or hop < 1:
            raise ValueError("%s: window and hop are positive numbers of segments (got %r, %r)" % (what, window, hop))
        return window, hop

    def _alloc_outputs(self, nW, n, kinds):
        """the outputs of a windowed call, by kind, in the order of the C arguments (None stays None: a null pointer)"""
        rsz = ctypes.sizeof(_l.MatchResult)
        form = {"res": ((nW, rsz), torch.uint8), "top": ((nW, n, rsz), torch.uint8), "n_found": ((nW,), torch.int32),
                "stats": ((nW, 3), torch.int64), "ss": ((nW, self.n_songs, 2), torch.float32), "words": ((nW,), torch.int64)}
        return tuple(None if kd is None else torch.empty(form[kd][0], device=self.device, dtype=form[kd][1]) for kd in kinds)

    def _windows_lib_call(self, what, head, n, out):
        """pfann_<what>(handle, *head, [n,] the outputs, stream)"""
        _l.check(getattr(self.lib, "pfann_" + what)(self.handle, *head, *(() if n is None else (n,)),
                                                    *(None if t is None else t.data_ptr() for t in out), self._stream()),
                 "pfann_" + what)

    def _match_windows(self, what, q, labels, rstart, rlen, window, hop, fsm, alpha, mode, n=None):
        """match_windows (n None) and match_windows_topn: the outputs on the device -> ((res,) or (top, n_found), wfirst).
        Order of refusals: window / hop, n, the assertion."""
        window, hop = self._window_hop(what, window, hop)
        if n is not None:
            n = self._check_n(what, n)
        q, labels, rs_np, rl_np = self._match_args(q, labels, rstart, rlen)
        nR = int(rl_np.shape[0])
        assert rs_np.shape[0] == nR and (nR == 0 or int((rs_np + rl_np).max()) <= q.shape[0]), "recordings exceed the rows given"
        wfirst = np.pad(np.cumsum(window_counts(rl_np, window, hop)), (1, 0)).astype(np.int64)
        nW = int(wfirst[-1])
        out = self._alloc_outputs(nW, n, ("res",) if n is None else ("top", "n_found"))
        if nW:
            rs, rl = self._upload_ranges(rs_np, rl_np)
            wf = _l.upload_async(wfirst, self.device, np.int64)
            self._windows_lib_call(what, (q.data_ptr(), labels.data_ptr(), labels.shape[1], rs.data_ptr(), rl.data_ptr(), nR, window,
                                          hop, int(fsm), float(alpha), int(mode), wf.data_ptr()), n, out)
        return out, wfirst

    def match_windows(self, q, labels, rstart, rlen, window, hop, fsm=1, alpha=0.0, mode=0, to_host=True):
        """Sequence matcher over every window of nR recordings (pfann_match_windows): recording r owns rows
        [rstart[r], rstart[r] + rlen[r]) of q / labels.  -> (results, wfirst): window i of recording r -- rows
        [i * hop, i * hop + window) of it -- is results[wfirst[r] + i], field for field what `match` returns for that
        slice; results is the structured array, or with to_host=False the device tensor."""
        (res,), wfirst = self._match_windows("match_windows", q, labels, rstart, rlen, window, hop, fsm, alpha, mode)
        return (self.results_to_host(res) if to_host else res), wfirst

    def match_windows_topn(self, q, labels, rstart, rlen, window, hop, n, fsm=1, alpha=0.0, mode=0, to_host=True):
        """Ranked answers for every window (pfann_match_windows_topn): recordings and windows as in match_windows.
        -> ((top [nW, n] of RESULT_DTYPE, n_found int32 [nW]), wfirst): row wfirst[r] + i is, field for field, what
        `match_topn` returns for window i of recording r, and its entry 0 is match_windows' answer; with to_host=False
        the two device tensors (uint8 [nW, n, 24], int32 [nW]) that topn_to_host turns into the arrays later."""
        out, wfirst = self._match_windows("match_windows_topn", q, labels, rstart, rlen, window, hop, fsm, alpha, mode, n)
        return (self.topn_to_host(*out) if to_host else out), wfirst

    def _dense_args(self, what, rstart, rlen, window, hop, exclude_song, q_rows=None):
        """the windowed arguments every dense call shares -> (window, hop, nR, nW, wfirst, device rstart, rlen, wfirst,
        exclude_song or None).  q_rows: the rows of q that the recordings must lie in (None for dense_merge, which reads no q).
        Order of refusals: window / hop, the two assertions, exclude_song's shape; the three arrays are uploaded even when
        there is no window (the caller then makes no library call)."""
        window, hop = self._window_hop(what, window, hop)
        rs_np, rl_np = np.ascontiguousarray(rstart, dtype=np.int64), np.ascontiguousarray(rlen, dtype=np.int32)
        nR = int(rl_np.shape[0])
        assert rs_np.shape[0] == nR, "one start per recording"
        assert q_rows is None or nR == 0 or int((rs_np + rl_np).max()) <= q_rows, "recordings exceed the rows given"
        wfirst = np.pad(np.cumsum(window_counts(rl_np, window, hop)), (1, 0)).astype(np.int64)
        ex = None
        if exclude_song is not None:
            ex_np = np.ascontiguousarray(exclude_song, dtype=np.int32)
            if ex_np.shape != (nR,):
                raise ValueError("%s: exclude_song wants one song id per recording (%d), got %r" % (what, nR, ex_np.shape))
            ex = _l.upload_async(ex_np, self.device, np.int32)
        rs, rl = self._upload_ranges(rs_np, rl_np)
        return window, hop, nR, int(wfirst[-1]), wfirst, rs, rl, _l.upload_async(wfirst, self.device, np.int64), ex

    def _dense_call(self, what, q, rstart, rlen, window, hop, exclude_song, kinds, n=None):
        """The six dense calls over q (pfann_<what>): kinds names the form's outputs in the order of its C arguments (_alloc_outputs),
        n is the list length of a ranked form -> (the outputs on the device, wfirst); no library call without a window.
        Order of refusals: window / hop, n, then _dense_args'."""
        if n is not None:
            self._window_hop(what, window, hop)
            n = self._check_n(what, n)
        window, hop, nR, nW, wfirst, rs, rl, wf, ex = self._dense_args(what, rstart, rlen, window, hop, exclude_song, q.shape[0])
        q = q.to(self.device, torch.float32).contiguous()
        out = self._alloc_outputs(nW, n, kinds)
        if nW:
            self._windows_lib_call(what, (q.data_ptr(), rs.data_ptr(), rl.data_ptr(), nR, window, hop, wf.data_ptr(), nW,
                                          ex.data_ptr() if ex is not None else None), n, out)
        return out, wfirst

    def match_windows_dense(self, q, rstart, rlen, window, hop, exclude_song=None, to_host=True):
        """Dense matcher over every window of nR recordings (pfann_match_windows_dense): no labels -- every alignment of
        every song is a candidate of every window, so the answer is what `match` gives for the slice when each row's label
        list is the whole database.  Recordings, windows and the return value (results, wfirst) are match_windows'.
        exclude_song: one song id per recording (-1: none) whose alignments are no candidates.  window <= 64, fp32 rows."""
        (res,), wfirst = self._dense_call("match_windows_dense", q, rstart, rlen, window, hop, exclude_song, ("res",))
        return (self.results_to_host(res) if to_host else res), wfirst

    def match_windows_dense_stats(self, q, rstart, rlen, window, hop, exclude_song=None, to_host=True):
        """match_windows_dense with the background statistics of every window (pfann_match_windows_dense_stats): the count and
        the two fixed-point sums of the totals of its full candidates, significance.STATS_DTYPE, from the same pass.
        -> ((results, stats), wfirst): results byte for byte match_windows_dense's; with to_host=False the device tensors
        (uint8 [nW, 24], int64 [nW, 3])."""
        (res, stats), wfirst = self._dense_call("match_windows_dense_stats", q, rstart, rlen, window, hop, exclude_song, ("res", "stats"))
        if not to_host:
            return (res, stats), wfirst
        return (self.results_to_host(res), self.stats_to_host(stats)), wfirst

    @staticmethod
    def stats_to_host(stats_dev):
        """device statistics (int64 [nW, 3]) -> significance.STATS_DTYPE array"""
        from .significance import STATS_DTYPE
        return np.ascontiguousarray(stats_dev.cpu().numpy()).view(STATS_DTYPE).reshape(-1)

    def _dense_ranked_to_host(self, top, n_found, ss, *stats):
        return self.topn_to_host(top, n_found) + (ss.cpu().numpy() if ss is not None else None,) + tuple(map(self.stats_to_host, stats))

    def match_windows_dense_topn(self, q, rstart, rlen, window, hop, n, exclude_song=None, want_song_scores=False, to_host=True):
        """Ranked dense answers (pfann_match_windows_dense_topn): the n best songs of every window over EVERY alignment, and
        with want_song_scores the per-song block [nW, n_songs, 2] of (float32 score, best offset in frames; zeros where the
        score is not > 0).  Recordings, windows and exclude_song as in match_windows_dense.
        -> ((top [nW, n] of RESULT_DTYPE, n_found int32 [nW], block or None), wfirst): entry 0 of a window is
        match_windows_dense's answer; with to_host=False the device tensors (uint8 [nW, n, 24], int32 [nW], float32 block)."""
        out, wfirst = self._dense_call("match_windows_dense_topn", q, rstart, rlen, window, hop, exclude_song,
                                       ("top", "n_found", "ss" if want_song_scores else None), n)
        return (self._dense_ranked_to_host(*out) if to_host else out), wfirst

    def match_windows_dense_topn_stats(self, q, rstart, rlen, window, hop, n, exclude_song=None, want_song_scores=False, to_host=True):
        """match_windows_dense_topn with the background statistics of every window from the same pass
        (pfann_match_windows_dense_topn_stats): the ranked outputs byte for byte match_windows_dense_topn's, the statistics byte
        for byte match_windows_dense_stats'.  Whole handles only.
        -> ((top, n_found, block or None, stats), wfirst); with to_host=False the device tensors (.., int64 [nW, 3])."""
        out, wfirst = self._dense_call("match_windows_dense_topn_stats", q, rstart, rlen, window, hop, exclude_song,
                                       ("top", "n_found", "ss" if want_song_scores else None, "stats"), n)
        return (self._dense_ranked_to_host(*out) if to_host else out), wfirst

    def match_songs_dense(self, q, qstart, qlen, cand, to_host=True):
        """Rescoring stage (pfann_match_songs_dense): every alignment of the songs `cand` lists for each of nQ queries, scored
        as the dense matcher scores them.  cand: a device tensor in match_topn's raw layout (uint8 [nQ, m, 24]; only the song
        fields are read), or a host int array [nQ, m] of song ids (-1: padding).  -> (structured array [nQ, m] of RESULT_DTYPE
        ranked by score, n_found int32 [nQ]); entries past the listed songs are song -1 / score -inf; a query of more than 64
        rows gets its input entries back and n_found -1.  With to_host=False the two device tensors, as match_topn."""
        q = q.to(self.device, torch.float32).contiguous()
        qs_np, ql_np = np.ascontiguousarray(qstart, dtype=np.int64), np.ascontiguousarray(qlen, dtype=np.int32)
        nQ = int(ql_np.shape[0])
        assert qs_np.shape[0] == nQ and (nQ == 0 or int((qs_np + ql_np).max()) <= q.shape[0]), "queries exceed the rows given"
        rsz = ctypes.sizeof(_l.MatchResult)
        if not torch.is_tensor(cand):
            ids = np.asarray(cand)
            if ids.ndim != 2 or ids.shape[0] != nQ:
                raise ValueError("match_songs_dense: cand wants one row of song ids per query (%d), got %r" % (nQ, ids.shape))
            host = np.zeros(ids.shape, dtype=self.RESULT_DTYPE)
            host["song"] = ids
            cand = torch.from_numpy(host.view(np.uint8).reshape(ids.shape + (rsz,))).to(self.device)
        if cand.dtype != torch.uint8 or cand.dim() != 3 or cand.shape[0] != nQ or cand.shape[2] != rsz:
            raise ValueError("match_songs_dense: cand wants uint8 [%d, m, %d], got %s %r" % (nQ, rsz, cand.dtype, tuple(cand.shape)))
        cand = cand.to(self.device).contiguous()
        m = int(cand.shape[1])
        top = torch.empty((nQ, m, rsz), device=self.device, dtype=torch.uint8)
        n_found = torch.empty((nQ,), device=self.device, dtype=torch.int32)
        if nQ:
            qs, ql = self._upload_ranges(qs_np, ql_np)
            _l.check(self.lib.pfann_match_songs_dense(self.handle, q.data_ptr(), qs.data_ptr(), ql.data_ptr(), nQ, cand.data_ptr(), m,
                                                      top.data_ptr(), n_found.data_ptr(), self._stream()),
                     "pfann_match_songs_dense")
        if not to_host:
            return top, n_found
        return self.topn_to_host(top, n_found)

    def nominate_songs_dense(self, q, qstart, qlen, n, to_host=True, max_qlen=None):
        """Dense song nomination on the fp16 MFMA (pfann_nominate_songs_dense): for each of nQ queries the n songs with the
        best approximate dense score, in match_topn's layout -- what match_songs_dense takes as `cand` --, and the certificate.
        -> (cand structured array [nQ, n], n_found int32 [nQ], n_close int32 [nQ]); n_close[j] <= n proves that the dense
        matcher's best song of query j is listed (-1: a query over 64 rows, or with a row outside fp16's range: not
        nominated).  With to_host=False the three device tensors (uint8 [nQ, n, 24], int32 [nQ], int32 [nQ]).  max_qlen: the
        rows of a query's slot in a tile (default: the longest query, at most 64); it has no part in a query's bytes."""
        q = q.to(self.device, torch.float32).contiguous()
        qs_np, ql_np = np.ascontiguousarray(qstart, dtype=np.int64), np.ascontiguousarray(qlen, dtype=np.int32)
        nQ, n = int(ql_np.shape[0]), int(n)
        assert qs_np.shape[0] == nQ and (nQ == 0 or int((qs_np + ql_np).max()) <= q.shape[0]), "queries exceed the rows given"
        # the longest query the tiles take: longer ones are not nominated (n_close -1)
        max_qlen = int(min(max(int(ql_np.max()) if nQ else 1, 1), 64)) if max_qlen is None else int(max_qlen)
        cand = torch.empty((nQ, max(n, 0), ctypes.sizeof(_l.MatchResult)), device=self.device, dtype=torch.uint8)
        n_found = torch.empty((nQ,), device=self.device, dtype=torch.int32)
        n_close = torch.empty((nQ,), device=self.device, dtype=torch.int32)
        qs, ql = self._upload_ranges(qs_np, ql_np)
        _l.check(self.lib.pfann_nominate_songs_dense(self.handle, q.data_ptr(), qs.data_ptr(), ql.data_ptr(), nQ, max_qlen, n,
                                                     cand.data_ptr(), n_found.data_ptr(), n_close.data_ptr(), self._stream()),
                 "pfann_nominate_songs_dense")
        if not to_host:
            return cand, n_found, n_close
        return self.topn_to_host(cand, n_found) + (n_close.cpu().numpy(),)

    def nominate_windows_dense(self, q, rstart, rlen, window, hop, n, exclude_song=None, to_host=True):
        """Windowed dense nomination (pfann_nominate_windows_dense): nominate_songs_dense for every window of nR recordings, over
        tiles that neighbouring windows share.  Recordings, windows and exclude_song as in match_windows_dense.
        -> ((cand [nW, n] of RESULT_DTYPE, n_found int32 [nW], n_close int32 [nW]), wfirst): row wfirst[r] + i is byte for byte
        what nominate_songs_dense gives the query window_queries names for window i of recording r (without that recording's
        excluded song); with to_host=False the three device tensors (uint8 [nW, n, 24], int32 [nW], int32 [nW])."""
        what = "nominate_windows_dense"
        self._window_hop(what, window, hop)
        n = self._check_n(what, n)
        window, hop, nR, nW, wfirst, rs, rl, wf, ex = self._dense_args(what, rstart, rlen, window, hop, exclude_song, q.shape[0])
        q = q.to(self.device, torch.float32).contiguous()
        cand = torch.empty((nW, n, ctypes.sizeof(_l.MatchResult)), device=self.device, dtype=torch.uint8)
        n_found = torch.empty((nW,), device=self.device, dtype=torch.int32)
        n_close = torch.empty((nW,), device=self.device, dtype=torch.int32)
        if nW:
            self._windows_lib_call(what, (q.data_ptr(), rs.data_ptr(), rl.data_ptr(), nR, window, hop, wf.data_ptr(), nW,
                                          ex.data_ptr() if ex is not None else None), n, (cand, n_found, n_close))
        if not to_host:
            return (cand, n_found, n_close), wfirst
        return self.topn_to_host(cand, n_found) + (n_close.cpu().numpy(),), wfirst

    # ---- the dense matcher over song-sharded handles: a part per handle, one merge (include/pfann_amd.h) ----------------
    def match_windows_dense_part(self, q, rstart, rlen, window, hop, exclude_song=None, stats=False):
        """This handle's part of match_windows_dense / _stats (pfann_match_windows_dense_part): the handle may hold a shard.
        -> ((words int64 [nW]: the bit patterns of the windows' raw running-best words, 0 where this handle has no candidate;
        the statistics int64 [nW, 3] over this handle's full candidates, or None), wfirst); device tensors for dense_merge."""
        return self._dense_call("match_windows_dense_part", q, rstart, rlen, window, hop, exclude_song,
                                ("words", "stats" if stats else None))

    def dense_merge(self, words, part_stats, rlen, window, hop, exclude_song=None):
        """words int64 [parts, nW] (and part_stats int64 [parts, nW, 3] or None) of match_windows_dense_part over handles that cut
        the song list, in any order -> (results uint8 [nW, 24], statistics int64 [nW, 3] or None): byte for byte what
        match_windows_dense / _stats give on one handle of the whole database (pfann_match_windows_dense_merge).  Any handle of
        the database can merge."""
        window, hop, nR, nW, wfirst, _, rl, wf, ex = self._dense_args("dense_merge", np.zeros(len(rlen), dtype=np.int64), rlen,
                                                                      window, hop, exclude_song)
        words = words.to(self.device, torch.int64).contiguous()
        parts = int(words.shape[0])
        assert tuple(words.shape) == (parts, nW), "words is [parts, windows]"
        if part_stats is not None:
            part_stats = part_stats.to(self.device, torch.int64).contiguous()
            assert tuple(part_stats.shape) == (parts, nW, 3), "part_stats is [parts, windows, 3]"
        res = torch.empty((nW, ctypes.sizeof(_l.MatchResult)), device=self.device, dtype=torch.uint8)
        st = torch.empty((nW, 3), device=self.device, dtype=torch.int64) if part_stats is not None else None
        if nW:
            _l.check(self.lib.pfann_match_windows_dense_merge(self.handle, words.data_ptr(),
                                                              part_stats.data_ptr() if part_stats is not None else None, parts,
                                                              rl.data_ptr(), nR, window, wf.data_ptr(), nW,
                                                              ex.data_ptr() if ex is not None else None, res.data_ptr(),
                                                              st.data_ptr() if st is not None else None, self._stream()),
                     "pfann_match_windows_dense_merge")
        return res, st

    def match_windows_dense_topn_part(self, q, rstart, rlen, window, hop, n, exclude_song=None):
        """This handle's part of match_windows_dense_topn (pfann_match_windows_dense_topn_part): the n best of its owned songs for
        every window, no per-song block.  -> ((top uint8 [nW, n, 24], n_found int32 [nW]), wfirst); device tensors."""
        n = self._check_n("match_windows_dense_topn_part", n)       # (this form refuses n before window and hop)
        return self._dense_call("match_windows_dense_topn_part", q, rstart, rlen, window, hop, exclude_song, ("top", "n_found"), n)

    def dense_topn_merge(self, tops, n_found_parts):
        """tops uint8 [parts, nW, n, 24] and n_found_parts int32 [parts, nW] of match_windows_dense_topn_part, parts in any order
        -> (top uint8 [nW, n, 24], n_found int32 [nW]): byte for byte match_windows_dense_topn on one handle of the whole
        database (pfann_match_windows_dense_topn_merge)."""
        tops = tops.to(self.device, torch.uint8).contiguous()
        n_found_parts = n_found_parts.to(self.device, torch.int32).contiguous()
        parts, nW, n = int(tops.shape[0]), int(tops.shape[1]), int(tops.shape[2])
        assert tops.shape[3] == ctypes.sizeof(_l.MatchResult) and tuple(n_found_parts.shape) == (parts, nW)
        top = torch.empty((nW, n, ctypes.sizeof(_l.MatchResult)), device=self.device, dtype=torch.uint8)
        n_found = torch.empty((nW,), device=self.device, dtype=torch.int32)
        if nW:
            _l.check(self.lib.pfann_match_windows_dense_topn_merge(self.handle, tops.data_ptr(), n_found_parts.data_ptr(), parts, nW,
                                                                   n, top.data_ptr(), n_found.data_ptr(), self._stream()),
                     "pfann_match_windows_dense_topn_merge")
        return top, n_found


def window_counts(rlen, window, hop):
    """windows per recording (include/pfann_amd.h, pfann_match_windows): starts 0, hop, 2*hop, .. while w0 + window <= L;
    one window over all rows when 0 < L < window; none when L == 0"""
    L = np.asarray(rlen, dtype=np.int64)
    return np.where(L <= 0, 0, np.where(L < window, 1, (L - window) // hop + 1)).astype(np.int64)


def window_queries(rstart, rlen, window, hop):
    """the windows of window_counts as queries -> (qstart int64 [nW], qlen int32 [nW], wfirst int64 [nR + 1]): window i of
    recording r is query wfirst[r] + i, rows [rstart[r] + i * hop, .. + min(window, rlen[r])) of the rows the recordings lie in"""
    rs, L = np.asarray(rstart, dtype=np.int64).reshape(-1), np.asarray(rlen, dtype=np.int64).reshape(-1)
    counts = window_counts(L, window, hop)
    wfirst = np.pad(np.cumsum(counts), (1, 0)).astype(np.int64)
    rec = np.repeat(np.arange(L.shape[0], dtype=np.int64), counts)
    qstart = rs[rec] + (np.arange(int(wfirst[-1]), dtype=np.int64) - wfirst[rec]) * int(hop)
    return qstart.astype(np.int64), np.minimum(L[rec], int(window)).astype(np.int32), wfirst


def self_match_ranges(song_pos, song_lo, song_hi):
    """Self-match of the songs [song_lo, song_hi) -> (rstart, rlen, lo, hi): song s is recording s - song_lo, rows
    [rstart, rstart + rlen) of the group's rows (rstart counts from the group's first row); lo / hi [rows]: the label
    range every row leaves out, its own song's [song_pos[s], song_pos[s + 1]).  Songs without rows have rlen 0."""
    pos = np.asarray(song_pos, dtype=np.int64)[song_lo:song_hi + 1]
    rlen = np.diff(pos)
    return (pos[:-1] - pos[0]).astype(np.int64), rlen.astype(np.int32), np.repeat(pos[:-1], rlen), np.repeat(pos[1:], rlen)


def self_match_groups(song_pos, song_lo, song_hi, max_rows):
    """[(a, b)]: consecutive song ranges covering [song_lo, song_hi), each with at most max_rows rows unless it is one song"""
    pos = np.asarray(song_pos, dtype=np.int64)
    out, a = [], song_lo
    while a < song_hi:
        b = a + 1
        while b < song_hi and pos[b + 1] - pos[a] <= max_rows:
            b += 1
        out.append((a, b))
        a = b
    return out


def _fine_to_time(fine, fsm, hop_size):
    """fine = t*fsm - shift  ->  (t - shift/fsm) * hop_size, as database.py:148 computes it."""
    fine = np.asarray(fine, dtype=np.int64)
    shift = (-fine) % fsm
    t = (fine + shift) // fsm
    return (t - shift / fsm) * hop_size


# The reference's module-level switch (database.py:12): False = the Python-path semantics of query_embeddings_base (the
# default), True = those of query_embeddings_cpp / cpp/seqscore.cpp (fp32 divide, score_alpha honoured, score and time read
# back from the per-song block).  PFANN_CPP_ACCELERATE=1 sets it for the CLIs.  Either way the work runs in the HIP kernels.
cpp_accelerate = os.environ.get("PFANN_CPP_ACCELERATE", "0") not in ("0", "")


def default_mode(mode=None):
    """the matcher mode of a launch that names none: the module switch above"""
    return (1 if cpp_accelerate else 0) if mode is None else mode


MONITOR_DTYPE = np.dtype([("w0", "<i8"), ("score", "<f8"), ("song", "<i8"), ("time_s", "<f8")])


def format_results(res, mode, fsm, hop_size, empty_db=False):
    """RESULT_DTYPE array of any shape -> (score float64, song int64, time_s float64) of that shape: the ONE statement of
    how a 24-byte match result becomes an answer, for every query form.
    mode 0, query_embeddings_base (database.py:148): (score, song, (offset - shift / fsm) * hop_size); no candidate
    (song < 0) or an empty database: (-inf, -1, 0).
    mode 1, query_embeddings_cpp (database.py:166-195), reads score and time back from the per-song block, which holds
    float32 and only ever records scores > 0: (float32 score, song, float32(offset * fsm - shift) * hop_size / fsm); no
    candidate or a float32 score that is not > 0: (0, song or -1, 0)."""
    song = res["song"].astype(np.int64)
    off, shift = res["offset"].astype(np.int64), res["shift"].astype(np.int64)
    if mode == 1:
        sc = res["score"].astype(np.float32)
        ok = (song >= 0) & (sc > 0)
        fine = (off * fsm - shift).astype(np.float32).astype(np.float64)
        return np.where(ok, sc.astype(np.float64), 0.0), np.where(song >= 0, song, -1), np.where(ok, fine * hop_size / fsm, 0.0)
    ok = (song >= 0) & (not empty_db)
    return np.where(ok, res["score"], -np.inf), np.where(ok, song, -1), np.where(ok, (off - shift / fsm) * hop_size, 0.0)


def _as_tuples(score, song, time_s, mode):
    """flat format_results arrays as the reference's Python objects: [(score, (song, time_s))], floats and ints; the mode-0
    answer without a candidate is (-1e999, (-1, 0)) with the reference's int 0"""
    times = time_s.tolist()
    if mode != 1:
        for j in np.flatnonzero(song < 0):
            times[j] = 0
    return list(zip(score.tolist(), zip(song.tolist(), times)))


def result_tuples(res, mode, fsm, hop_size, empty_db=False):
    """RESULT_DTYPE [n] -> [(score, (song, time_s))]: what query_finish answers per query, before the per-song block"""
    return _as_tuples(*format_results(res, mode, fsm, hop_size, empty_db), mode)


def topn_tuples(top, mode, fsm, hop_size, empty_db=False):
    """RESULT_DTYPE [nQ, n] ranked lists -> per query the list of result_tuples entries that count: entry 0 always (it is
    the query's answer, also without a candidate), later entries up to the first song < 0, and in mode 1 only those with
    a float32 score > 0 -- the reference's per-song block never records the others."""
    nq, n = top.shape
    score, song, time_s = format_results(top, mode, fsm, hop_size, empty_db)
    keep = np.ones((nq, n), dtype=bool)
    keep[:, 1:] = np.logical_and.accumulate(top["song"][:, 1:] >= 0, axis=1)
    if mode == 1:
        keep[:, 1:] &= score[:, 1:] > 0
    flat = _as_tuples(score.ravel(), song.ravel(), time_s.ravel(), mode)
    return [[flat[i] for i in np.flatnonzero(row) + j * n] for j, row in enumerate(keep)]


def monitor_rows(res, wfirst, hop, mode, fsm, hop_size):
    """windowed results -> per recording a MONITOR_DTYPE array (w0, score, song, time_s): recording r's windows are
    res[wfirst[r]:wfirst[r + 1]], `hop` rows apart"""
    score, song, time_s = format_results(res, mode, fsm, hop_size)
    out = []
    for a, b in zip(wfirst[:-1], wfirst[1:]):
        rows = np.zeros(b - a, dtype=MONITOR_DTYPE)
        rows["w0"] = np.arange(b - a, dtype=np.int64) * hop
        rows["score"], rows["song"], rows["time_s"] = score[a:b], song[a:b], time_s[a:b]
        out.append(rows)
    return out


MONITOR_TOPN_DTYPE = np.dtype(MONITOR_DTYPE.descr + [("votes", "<i4")])


def monitor_topn_rows(top, wfirst, hop, mode, fsm, hop_size):
    """ranked windowed results [nW, n] -> per recording a MONITOR_TOPN_DTYPE array [windows, n]: column j is monitor_rows of
    the rank-j entries (padding entries: -inf, -1, 0 like a window without a candidate), votes = the entry's n_cand"""
    cols = [monitor_rows(top[:, j], wfirst, hop, mode, fsm, hop_size) for j in range(top.shape[1])]
    out = []
    for r, (a, b) in enumerate(zip(wfirst[:-1], wfirst[1:])):
        rows = np.zeros((b - a, top.shape[1]), dtype=MONITOR_TOPN_DTYPE)
        for j, col in enumerate(cols):
            for f in MONITOR_DTYPE.names:
                rows[f][:, j] = col[r][f]
        rows["votes"] = top["n_cand"][a:b]
        out.append(rows)
    return out


def launch_ahead(items, launch):
    """-> iterator of launch(item) in order, one launch ahead of its consumer: the first launch is made at once, and item
    g + 1 is launched before item g's launch is handed out to be read back, so the GPU has work while the host reads."""
    items = iter(items)

    def hand_out(cur):
        while cur:
            nxt = [launch(x) for x in itertools.islice(items, 1)]
            yield cur[0]
            cur = nxt
    return hand_out([launch(x) for x in itertools.islice(items, 1)])


class LazyLaunches:
    """[(j0, j1)] cuts + launch(j0, j1) -> iterable of (j0, j1, launch result) with the first launch made at once and
    every later one made when its predecessor is handed out (launch_ahead)."""

    def __init__(self, cuts, launch):
        self._cuts = list(cuts)
        self._it = launch_ahead(self._cuts, lambda c: (c[0], c[1], launch(*c)))
        self.max_in_flight = 0                       # (for the tests: the one handed out + its successor, when it has one)

    def __len__(self):
        return len(self._cuts)

    def __iter__(self):
        for g, cur in enumerate(self._it, 1):
            self.max_in_flight = max(self.max_in_flight, 1 + (g < len(self._cuts)))
            yield cur


class Database:
    def __init__(self, dir_for_db, indexer_params, hop_size, device=0, d=None, storage=None, ranks=None):
        """ranks: a pfann_amd.dist.Ranks (one process per GPU).  With more than one rank (or PFANN_FORCE_SHARDED=1) the
        database is sharded by whole songs: this process reads and holds only its contiguous song range, every query
        method is then COLLECTIVE (all ranks call it with the same arguments and get the same answers), and the
        batched form hands back this shard's columns of the per-song score matrix (song_range)."""
        self.ranks = ranks if (ranks is not None and ranks.sharded) else None
        if ranks is not None:
            device = ranks.device
        self.dir_for_db = dir_for_db
        self.params = indexer_params
        self.top_k = self.params["top_k"]
        self.frame_shift_mul = self.params.get("frame_shift_mul", 1)
        self.hop_size = hop_size
        self.score_alpha = self.params.get("score_alpha", 0)
        self.timer = None          # a utils.StageTimer: query_batch then reports 'search' and 'rerank' separately
        self._copy_stream = None   # the side stream results are read back on (_read_back makes it at the first read)
        self._pin = {}             # pinned landing buffers of _pinned, by dtype

        if os.path.exists(os.path.join(dir_for_db, "dbupdate.journal")):
            raise _l.PfannError("%s holds the journal of an interrupted update: run `python dbupdate.py check %s --repair` "
                                "first (pfann_amd/dbfiles.py)" % (dir_for_db, dir_for_db))
        self.songList = read_file_list(os.path.join(dir_for_db, "songList.txt"))
        key = np.fromfile(os.path.join(dir_for_db, "landmarkKey"), dtype=np.int32)
        assert len(self.songList) == key.shape[0]
        self.song_pos = song_pos_from_key(key)

        n_songs, n_rows = len(self.songList), int(self.song_pos[-1])
        self.song_range = (0, n_songs)                           # songs whose score columns this process holds
        r_lo, r_hi = 0, n_rows
        if self.ranks is not None:
            from .dist import shard_songs
            ranges = shard_songs(self.song_pos, self.ranks.world)
            self.song_range = ranges[self.ranks.rank]
            # (query_launch_chunks must cut alike on every rank -- its launches are collective: the widest shard decides)
            self._widest_shard = max(hi - lo for lo, hi in ranges)
            r_lo, r_hi = int(self.song_pos[self.song_range[0]]), int(self.song_pos[self.song_range[1]])
        emb = None
        lv = os.path.join(dir_for_db, "landmarkValue")
        if os.path.exists(lv):
            try:
                emb, _, n_all = faissio.read_index_flat(lv, rows=(r_lo, r_hi))
                assert n_all == n_rows, "landmarkValue rows != sum(landmarkKey)"
            except (ValueError, struct.error, OSError, IndexError) as x:   # not a flat index / truncated file
                print("landmarkValue unusable (%s): falling back to the raw embeddings file" % x)
                emb = None
        if emb is None:                                         # database.py:96-97 fallback
            if d is None:
                cfg = os.path.join(dir_for_db, "configs.json")
                d = json.load(open(cfg))["model"]["d"]
            path = os.path.join(dir_for_db, "embeddings")
            assert os.path.getsize(path) == n_rows * d * 4, "embeddings rows != sum(landmarkKey)"
            emb = np.fromfile(path, dtype=np.float32, count=(r_hi - r_lo) * d, offset=r_lo * d * 4).reshape(-1, d)
        self.d = emb.shape[1] if emb.ndim == 2 and emb.shape[0] else (d or emb.shape[-1])
        assert emb.shape[0] == r_hi - r_lo, "embeddings rows != sum(landmarkKey)"
        # "use_float16" in the indexer params (or PFANN_DB_STORAGE=f16) selects fp16-only storage: the knob the
        # reference hard-codes as co.useFloat16 = True for its GPU index (database.py:101-104)
        if storage is None:
            storage = os.environ.get("PFANN_DB_STORAGE") or ("f16" if self.params.get("use_float16", False) else "f32")
        self.index = DeviceIndex(self.d, device, storage)
        # ONE statement of which songs this process owns: the cut made above (0-row songs at a shard boundary cannot be
        # told from the row range), handed to the library and read back
        self.index.load(emb, self.song_pos, r_lo, song_range=self.song_range if self.ranks is not None else None)
        if self.ranks is not None:
            assert self.index.owned_songs() == tuple(self.song_range), (self.index.owned_songs(), self.song_range)
        self.sharded = None
        if self.ranks is not None:
            from .dist import ShardedIndex
            self.sharded = ShardedIndex(self.index, self.song_pos, self.top_k, self.frame_shift_mul, self.score_alpha,
                                        group=self.ranks.group, always_exchange=self.ranks.world == 1)
        # per-song score blocks of one launch: at most this many (score, alignment) pairs in HBM (and as many in the
        # pinned landing buffer); the CLIs split a launch group's queries accordingly (query_launch_chunks)
        self.max_score_pairs = int(float(os.environ.get("PFANN_SCORE_BLOCK_MB", "1024")) * (1 << 20)) // 8

    def attach_engine(self, engine):
        """The tools call this with the Engine that embeds their queries: with the exchange stream on, the engine's front
        end then starts behind the shard scan of the exchange in flight (dist.ShardedIndex.hold_front_end)."""
        if self.sharded is not None and self.sharded.xs is not None:
            engine.before_front_end = self.sharded.hold_front_end

    def warmup(self, rows=19 * 64, want_song_scores=True, topn=0):
        """throw-away queries through search + match: kernel code objects and scratch buffers exist afterwards.  rows: the
        largest number of query rows one launch group will bring (the matcher: PFANN_MAX_BATCH) -- the search workspace is
        sized by it, and growing it later means a hipFree, which waits for everything in flight: the first full group of
        a matcher run used to stall 30 ms behind its own encoder there (profiles/r3/NOTES.md)."""
        if int(self.song_pos[-1]):                   # (the WHOLE database: under ranks every rank must come along)
            q = torch.zeros((19, self.d), device=self.index.device)
            q[:, 0] = 1.0
            self.query_finish(self.query_launch(q, [0], [19], want_song_scores=want_song_scores))
            nq = max(1, int(rows) // 19)
            big = torch.cat([q] * nq)                # (also loads torch's concatenation kernel, which the CLIs use per group)
            self.query_finish(self.query_launch(big, np.arange(nq) * 19, [19] * nq, want_song_scores=want_song_scores),
                              reuse_buffers=True)
            if topn:                                 # (matcher.py --top: the top-N instantiation of the matcher, both plans)
                self.query_topn_batch(q, [0], [19], topn)
                self.query_topn_batch(big, np.arange(nq) * 19, [19] * nq, topn)

    # ---- batched form ------------------------------------------------------------------
    def query_launch(self, emb, qstart, qlen, want_song_scores=False, mode=None):
        """First half of query_batch: search + sequence match launched asynchronously, nothing read back.  The CLIs launch
        group g+1 before they finish group g, so the GPU never idles while the host formats and writes results."""
        mode = default_mode(mode)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] + [torch.cuda.Event()]
        # song-sharded, PFANN_EXCHANGE_STREAM=1: search, collectives, matcher and winner pick run on the exchange stream
        # (dist.ShardedIndex.exchange), so the next group's encoder does not queue behind the collectives
        with (self.sharded.exchange(emb) if self.sharded is not None else contextlib.nullcontext()):
            ev[0].record()
            if self.sharded is not None:
                # two-phase shard search + all-to-all merge (`search`), owner-side match + 128-bit key all-gather +
                # device pick (`rerank`); `res` are the winners over ALL shards, `ss` this shard's columns
                D, I = self.sharded.search_global(emb)
                ev[1].record()
                res, ss = self.sharded.match_global(emb, I, qstart, qlen, want_song_scores, mode)
            else:
                D, I = self.index.search(emb, self.top_k)
                ev[1].record()
                res, ss = self.index.match(emb, I, qstart, qlen, self.frame_shift_mul, self.score_alpha, mode,
                                           False, want_song_scores, to_host=False)
            ev[2].record()
            # frames -> seconds where the block lives (database.py:148,193 do it on the host): (t - shift/fsm) * hop_size
            # with fine = t*fsm - shift, in double like the reference's Python floats, stored as float32
            self.index.song_scores_to_seconds(ss, self.frame_shift_mul, self.hop_size, native_path=mode == 1)
            ev[3].record()              # (the block is complete HERE, not at ev[2]: query_finish copies it after this one)
        return {"res": res, "ss": ss, "ev": ev, "keep": (emb, I), "mode": mode}

    def query_launch_chunks(self, emb, qstart, qlen, want_song_scores=False, mode=None):
        """query_launch over as many sub-launches as the score-block budget asks for (PFANN_SCORE_BLOCK_MB, default
        1024: one-segment queries against a 100 k-song database would otherwise want 7.8 GB of HBM and as much pinned
        host memory per launch group).  -> an iterable of (first query, one past the last, launch), LAZY beyond its first
        element: sub-launch 0 is in flight when this returns (the CLIs launch group g+1 before they read group g back),
        sub-launch i+1 is launched when the consumer asks for sub-launch i, i.e. just before it reads i back.  At most
        three score blocks of max_score_pairs pairs therefore exist at any time -- the one being read back, its
        successor, and the first one of the next launch group -- whatever the number of sub-launches (all of them at
        once until round 5: the budget then bounded only the pinned landing buffer)."""
        return self._launch_chunks(lambda e, qs, ql: self.query_launch(e, qs, ql, want_song_scores, mode),
                                   getattr(self, "_widest_shard", self.song_range[1] - self.song_range[0]), emb, qstart, qlen,
                                   want_song_scores)

    def _launch_chunks(self, launch, width, emb, qstart, qlen, want_song_scores):
        """The one cutter of a launch group: launch(rows, qstart, qlen) over runs of queries whose per-song blocks, `width`
        songs wide, stay within max_score_pairs (one run without blocks) -> LazyLaunches, see query_launch_chunks"""
        nq = len(qlen)
        step = max(1, nq) if not want_song_scores else max(1, min(nq, self.max_score_pairs // max(width, 1)))
        qstart = np.asarray(qstart, dtype=np.int64)

        def cut(j0, j1):
            r0 = int(qstart[j0])
            r1 = int(qstart[j1 - 1]) + int(qlen[j1 - 1])
            sub = emb if (j0 == 0 and j1 == nq) else emb[r0:r1]
            return launch(sub, qstart[j0:j1] - r0, qlen[j0:j1])
        return LazyLaunches([(j0, min(j0 + step, nq)) for j0 in range(0, nq, step)], cut)

    def _pinned(self, shape, dtype):
        """one reusable pinned landing buffer per result kind (a pinned allocation costs milliseconds)"""
        n = int(np.prod(shape))
        key = str(dtype)
        buf = self._pin.get(key)
        if buf is None or buf.numel() < n:
            buf = torch.empty(max(n, 1), dtype=dtype, pin_memory=True)
            self._pin[key] = buf
        return buf[:n].view(shape)

    def _launch(self, emb, match, mode=None, k=None, exclude=None, search=True):
        """The single-GPU launch skeleton: timed event, search, timed event, match(labels, mode) -> dict of what it left on
        the device, timed event; nothing is read back.  -> that dict + the keys every finish half reads.
        search=False (the dense forms, which pass mode 0): no search -- an empty search stage -- and match() takes no argument."""
        mode = default_mode(mode)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        I = self.index.search(emb, self.top_k if k is None else int(k), exclude=exclude)[1] if search else None
        ev[1].record()
        out = match(I, mode) if search else match()
        ev[2].record()
        return dict(out, ev=ev, keep=(emb, I), mode=mode)

    def _read_back(self, p):
        """The one read-back of a launch p: on the copy stream, behind its last event (a side stream copies that group's
        results; later groups keep running), p["res"] -> RESULT_DTYPE array and the per-song block p["ss"] -> a view of
        the reused pinned buffer (or None).  A launch that carries the three timed events (every one but
        query_topn_again's) gives the timer its stage split, as database.py:165 logs it."""
        ev, ss = p["ev"], p.get("ss")
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(self.index.device)
        land = None
        with torch.cuda.stream(self._copy_stream):
            self._copy_stream.wait_event(ev[-1])
            if ss is not None:
                land = self._pinned(ss.shape, torch.float32)
                land.copy_(ss, non_blocking=True)
            out = self.index.decode_results(p["res"])     # synchronises the copy stream: `land` is complete too
            if ss is not None:
                self._copy_stream.synchronize()
        if self.timer is not None and len(ev) >= 3:
            self.timer.mark_gpu("search", ev[0], ev[1])
            self.timer.mark_gpu("rerank", ev[1], ev[2])
            self.timer.resolve()
        return out, land

    def _answers(self, res, mode, tuples=result_tuples):
        # (the WHOLE database: under ranks a shard may be empty while the answers are those of all shards)
        return tuples(res, mode, self.frame_shift_mul, self.hop_size, empty_db=int(self.song_pos[-1]) == 0)

    def query_finish(self, p, reuse_buffers=False):
        """Second half: wait for that group only and return the list of (score, (song, time), song_score|None).
        reuse_buffers: the song_score blocks are views of a pinned buffer that the NEXT query_finish overwrites (the CLIs
        write them out at once)."""
        res, land = self._read_back(p)
        return [r + (b,) for r, b in zip(self._answers(res, p["mode"]), self._blocks(land, len(res), reuse_buffers))]

    @staticmethod
    def _blocks(land, nq, reuse_buffers):
        """the per-song block of each of nq queries: None without a landing buffer, else its rows -- views of the pinned
        buffer with reuse_buffers, a copy otherwise"""
        if land is None:
            return [None] * nq
        return land.numpy() if reuse_buffers else land.numpy().copy()

    def query_batch(self, emb, qstart, qlen, want_song_scores=False, mode=None):
        """emb: torch cuda [sum(qlen), d] unit-norm rows; -> list of (score, (song, time), song_score|None)."""
        return self.query_finish(self.query_launch(emb, qstart, qlen, want_song_scores, mode))

    # ---- ranked answers: the n best songs per query, no per-song block --------------------------------
    def query_topn_launch(self, emb, qstart, qlen, n, mode=None):
        """First half of query_topn_batch: search + top-N sequence match (pfann_match_topn) launched asynchronously."""
        if self.ranks is not None:
            raise _l.PfannError("top-N over a sharded database is not supported")
        return self._launch(emb, lambda I, mode: self._match_topn(emb, I, qstart, qlen, n, mode), mode)

    def _match_topn(self, emb, I, qstart, qlen, n, mode):
        top, n_found = self.index.match_topn(emb, I, qstart, qlen, n, self.frame_shift_mul, self.score_alpha, mode, False,
                                             to_host=False)
        return {"res": top, "n_found": n_found}

    def query_topn_again(self, p, qstart, qlen, n):
        """the ranked lists of a launch query_launch made (p), from the labels its search left on the device: for a caller
        that wants the per-song block AND the top-N (the matcher CLI with --top).  -> what query_topn_finish takes"""
        if self.ranks is not None:
            raise _l.PfannError("top-N over a sharded database is not supported")
        out = self._match_topn(*p["keep"], qstart, qlen, n, p["mode"])
        ev = torch.cuda.Event()
        ev.record()
        return dict(out, ev=[ev], keep=p["keep"], mode=p["mode"])

    def query_topn_finish(self, p):
        """Second half: -> per query a list of up to n (score, (song, time_s)), best first, by the formulas query_finish
        applies to the winner in the same mode; entry 0 IS query_finish's answer (also when there is no candidate).  Native
        path (mode 1): later entries whose float32 score is not > 0 are dropped (topn_tuples)."""
        return self._answers(self._read_back(p)[0], p["mode"], topn_tuples)

    def query_topn_batch(self, emb, qstart, qlen, n, mode=None):
        """emb: torch cuda [sum(qlen), d] unit-norm rows; -> per query the ranked list of (score, (song, time_s))."""
        return self.query_topn_finish(self.query_topn_launch(emb, qstart, qlen, n, mode))

    # ---- monitor mode: every window of long recordings ----------------------------------------------
    def monitor_launch(self, emb, rstart, rlen, window, hop, edge_window=0):
        """First half of monitor mode: ONE search of all rows (each row once, however many windows contain it), then the
        windowed matcher, launched asynchronously like query_launch.  emb: torch cuda [rows, d]; recording r owns rows
        [rstart[r], rstart[r] + rlen[r]); window, hop in segments.  edge_window > 0: the same labels are matched a second
        time in short windows of that many segments at hop 1 (monitor_finish leaves them in p["edge_rows"]): they place
        the edges of a detection far better than the long windows' scores do (monitor.merge_windows)."""
        self._whole_only("monitor mode is", "a recording is matched on one GPU against the whole database")
        return self._launch(emb, lambda I, mode: self._windows_launched(
            lambda w, h: self.index.match_windows(emb, I, rstart, rlen, w, h, self.frame_shift_mul, self.score_alpha, mode,
                                                  to_host=False), window, hop, edge_window))

    def _whole_only(self, what, why):
        """the refusal of a form that wants the whole database on one handle, under ranks"""
        if self.sharded is not None:
            raise _l.PfannError("%s not song-sharded: %s (run without PFANN_GPUS / ranks)" % (what, why))

    @staticmethod
    def _windows_launched(windows, window, hop, edge_window=0, long=None):
        """What a windowed launch leaves for its finish half, from windows(w, h) -> (res or (top, n_found), wfirst) on the device:
        the long windows -- `long` where the caller has made that call itself --, then, with edge_window > 0, the short windows
        of the edge pass at hop 1 as "fine" (else None)."""
        res, wfirst = windows(window, hop) if long is None else long
        out = {"res": res} if not isinstance(res, tuple) else {"res": res[0], "n_found": res[1]}
        return dict(out, wfirst=wfirst, fine=windows(edge_window, 1) if edge_window > 0 else None, hop=int(hop))

    def _dense_check(self, what):
        """the dense matcher is defined for the default family only: mode 0, frame_shift_mul 1, score_alpha 0.  Under ranks its
        windowed forms are collective (dist.ShardedIndex.dense_windows_global / dense_windows_topn_global)."""
        if self.frame_shift_mul != 1:
            raise _l.PfannError("%s: the dense matcher needs frame_shift_mul 1 (the database has %r)" % (what, self.frame_shift_mul))
        if self.score_alpha != 0:
            raise _l.PfannError("%s: the dense matcher needs score_alpha 0 (the database has %r)" % (what, self.score_alpha))
        if default_mode() != 0:
            raise _l.PfannError("%s: the dense matcher is the python path's form; the native mode (cpp_accelerate) is in effect" % what)

    def _dense_windows(self, emb, rstart, rlen, window, hop, stats=False):
        """-> ((results, statistics or None), wfirst) on the device: one handle, or under ranks part + all-gather + merge"""
        if self.sharded is not None:
            return self.sharded.dense_windows_global(emb, rstart, rlen, window, hop, stats=stats)
        if stats:
            return self.index.match_windows_dense_stats(emb, rstart, rlen, window, hop, to_host=False)
        res, wfirst = self.index.match_windows_dense(emb, rstart, rlen, window, hop, to_host=False)
        return (res, None), wfirst

    def _dense_windows_topn(self, emb, rstart, rlen, window, hop, n, want_song_scores=False):
        """-> ((top, n_found, block or None), wfirst) on the device, as _dense_windows; no per-song block under ranks"""
        if self.sharded is not None:
            (top, n_found), wfirst = self.sharded.dense_windows_topn_global(emb, rstart, rlen, window, hop, n)
            return (top, n_found, None), wfirst
        return self.index.match_windows_dense_topn(emb, rstart, rlen, window, hop, n, want_song_scores=want_song_scores, to_host=False)

    def monitor_dense_launch(self, emb, rstart, rlen, window, hop, edge_window=0, stats=False):
        """monitor_launch on the dense matcher (pfann_match_windows_dense): no search, every alignment of every song is a
        candidate of every window (and of every short window of the edge pass).  -> what monitor_finish reads.
        stats=True: the long windows go through pfann_match_windows_dense_stats and the launch carries their background
        statistics for monitor_dense_stats_finish; the edge pass stays as it is (its rows only place edges)."""
        self._dense_check("monitor_dense_launch")

        def windows(w, h):
            (res, _), wfirst = self._dense_windows(emb, rstart, rlen, w, h)
            return res, wfirst

        def match():
            if not stats:
                return self._windows_launched(windows, window, hop, edge_window)
            (res, st), wfirst = self._dense_windows(emb, rstart, rlen, window, hop, stats=True)
            return dict(self._windows_launched(windows, window, hop, edge_window, long=(res, wfirst)), stats=st,
                        rows_of=(int(window), np.asarray(rlen, dtype=np.int64)))
        return self._launch(emb, match, mode=0, search=False)

    def monitor_dense_stats_finish(self, p):
        """Second half of monitor_dense_launch(stats=True): -> (what monitor_finish returns, per recording a float64 array
        log10_fa aligned with its rows): log10 of the chance that the best of the window's candidates reaches its score when
        the window holds nothing of the database, from the window's own background (pfann_amd/significance.py); 0 where that
        cannot be said."""
        from . import significance as sg
        raw = self._read_back(p)[0]                      # (the statistics are complete behind the same event)
        stats = self.index.stats_to_host(p["stats"])
        window, rlen = p["rows_of"]
        wfirst, fsm = p["wfirst"], self.frame_shift_mul
        rows = monitor_rows(raw, wfirst, p["hop"], p["mode"], fsm, self.hop_size)
        self._edge_finish(p, fsm)
        hists, song_len = self._hists()
        fa = [sg.log10_false_alarms(raw[a:b], stats[a:b], min(window, int(L)), -1, hists, song_len)
              for a, b, L in zip(wfirst[:-1], wfirst[1:], rlen)]
        return rows, fa

    def _hists(self):
        """-> (the significance.OverlapHistograms of the songs' lengths, kept until they change; the lengths)"""
        from . import significance as sg
        song_len = np.diff(self.song_pos)
        if getattr(self, "_overlap_hists", None) is None or not np.array_equal(self._overlap_hists.song_len, song_len):
            self._overlap_hists = sg.OverlapHistograms(song_len)
        return self._overlap_hists, song_len

    def monitor_dense_topn_launch(self, emb, rstart, rlen, window, hop, n, edge_window=0):
        """monitor_topn_launch on the ranked dense matcher (pfann_match_windows_dense_topn): no search, the n best songs of every
        window -- and of every short window of the edge pass -- over every alignment.  -> what monitor_dense_topn_finish reads."""
        self._dense_check("monitor_dense_topn_launch")

        def windows(w, h):
            (top, n_found, _), wfirst = self._dense_windows_topn(emb, rstart, rlen, w, h, n)
            return (top, n_found), wfirst
        return self._launch(emb, lambda: self._windows_launched(windows, window, hop, edge_window), mode=0, search=False)

    def monitor_dense_topn_finish(self, p):
        """Second half of monitor_dense_topn_launch: what monitor_topn_finish returns, votes = len_s + window rows - 1 (every
        alignment of the song is a candidate)."""
        return self._windows_topn_finish(p, self.frame_shift_mul)

    # ---- plain queries through the dense form: every query is one recording and one window ----------------------------
    def query_dense_launch(self, emb, qstart, qlen, n=1, want_song_scores=False, stats=False):
        """First half of query_dense_batch: the ranked dense matcher (pfann_match_windows_dense_topn) with window = the longest
        query of the call (at most 64 segments; every query has at least one), so that by the short-recording rule every query is
        exactly one window over all its rows, and by the byte contract its answer does not depend on what it was batched with.
        No search.  The per-song block is converted to seconds where it lives, as query_launch does.
        stats=True: the same outputs and every query's background statistics from the one pass
        (pfann_match_windows_dense_topn_stats), for query_dense_stats_finish; not song-sharded."""
        self._dense_check("query_dense_launch")
        if stats and self.ranks is not None:
            raise _l.PfannError("query_dense_launch: the ranked statistics are not song-sharded (stats=True needs the whole database "
                                "on one handle: run without PFANN_GPUS / ranks)")
        if want_song_scores and self.sharded is not None:
            raise _l.PfannError("query_dense_launch: the per-song block is not song-sharded (want_song_scores=True needs the whole "
                                "database on one handle: run without PFANN_GPUS / ranks)")
        ql = np.ascontiguousarray(qlen, dtype=np.int32)
        if ql.shape[0] and (int(ql.min()) < 1 or int(ql.max()) > 64):
            raise _l.PfannError("query_dense_launch: a query has 1..64 segments (got %d..%d)" % (int(ql.min()), int(ql.max())))
        window = int(ql.max()) if ql.shape[0] else 1

        def match():
            out = {}
            if stats:
                (top, n_found, ss, out["stats"]), wfirst = self.index.match_windows_dense_topn_stats(
                    emb, qstart, ql, window, 1, n, want_song_scores=want_song_scores, to_host=False)
                out["rows_of"] = ql.astype(np.int64)
            else:
                (top, n_found, ss), wfirst = self._dense_windows_topn(emb, qstart, ql, window, 1, n, want_song_scores)
            assert int(wfirst[-1]) == ql.shape[0]
            self.index.song_scores_to_seconds(ss, 1, self.hop_size)
            return dict(out, res=top, n_found=n_found, ss=ss)
        return self._launch(emb, match, mode=0, search=False)

    def query_dense_launch_chunks(self, emb, qstart, qlen, n=1, want_song_scores=False, stats=False):
        """query_dense_launch cut by the score-block budget, lazily, exactly as query_launch_chunks cuts query_launch"""
        return self._launch_chunks(lambda e, qs, ql: self.query_dense_launch(e, qs, ql, n, want_song_scores, stats),
                                   len(self.songList), emb, qstart, qlen, want_song_scores)

    def query_dense_finish(self, p, reuse_buffers=False):
        """Second half: -> (answers, ranked): answers as query_finish gives them, [(score, (song, time_s), song_score|None)]
        from entry 0, and ranked as query_topn_finish gives them, per query up to n (score, (song, time_s)) best first; both
        through the one read-back and the one formatter.  reuse_buffers: as in query_finish."""
        return self._dense_answers(p, reuse_buffers)[1:]

    def _dense_answers(self, p, reuse_buffers):
        """the read-back of a query_dense_launch -> (raw ranked lists RESULT_DTYPE [nQ, n], answers, ranked)"""
        res, land = self._read_back(p)
        answers = [r + (b,) for r, b in zip(self._answers(res[:, 0], 0), self._blocks(land, len(res), reuse_buffers))]
        return res, answers, self._answers(res, 0, topn_tuples)

    def query_dense_batch(self, emb, qstart, qlen, n=1, want_song_scores=False):
        """emb: torch cuda [sum(qlen), d] unit-norm rows, queries of 1..64 segments -> (answers, ranked), see query_dense_finish"""
        return self.query_dense_finish(self.query_dense_launch(emb, qstart, qlen, n, want_song_scores))

    def query_dense_stats_finish(self, p, reuse_buffers=False):
        """Second half of query_dense_launch(stats=True): -> (answers, ranked, log10_fa).  answers and ranked are exactly
        query_dense_finish's, through the one read-back; log10_fa[j] is a float64 array aligned with ranked[j]: for every listed
        song the log10 of the chance that the best of the query's candidates reaches that song's score when the query holds
        nothing of the database, judged against the query's own background with the better-ranked entries and the entry itself
        left out (significance.log10_false_alarms_ranked); 0 where that cannot be said.  Every query is one window of its own
        rows, so the overlap histogram is that of its own length."""
        from . import significance as sg
        res, answers, ranked = self._dense_answers(p, reuse_buffers)
        stats = self.index.stats_to_host(p["stats"])     # (complete behind the event the read-back waited for)
        hists, song_len = self._hists()
        fa = []
        for top, st, L, rows in zip(res, stats, p["rows_of"], ranked):
            L = int(L)
            v = sg.log10_false_alarms_ranked(top, L, (st["n_full"], st["sum_q"], st["sumsq_q"]), hists(L), song_len)
            fa.append(v[:len(rows)])
        return answers, ranked, fa

    def query_dense_stats_batch(self, emb, qstart, qlen, n=1, want_song_scores=False):
        """query_dense_batch with a significance for every ranked entry -> (answers, ranked, log10_fa), see query_dense_stats_finish"""
        return self.query_dense_stats_finish(self.query_dense_launch(emb, qstart, qlen, n, want_song_scores, stats=True))

    # ---- rescored answers: the nominated matcher names n songs, the dense arithmetic scores every alignment of those ------
    def query_rescore_launch(self, emb, qstart, qlen, n):
        """First half of query_rescore_batch: search, then the n best nominated songs of every query (pfann_match_topn), then
        every alignment of those songs (pfann_match_songs_dense), on the one stream; nothing is read back.  A song's rescored
        entry is byte for byte the ranked dense matcher's entry for it, so the answer is query_dense_batch's wherever the dense
        answer's song is among the n nominated ones.  A query of more than 64 segments keeps its nominated list."""
        self._whole_only("query_rescore_launch: rescoring is", "the nominated songs are scored on one GPU against the whole database")
        self._dense_check("query_rescore_launch")
        n = DeviceIndex._check_n("query_rescore_launch", n)

        def match(I, mode):
            out = self._match_topn(emb, I, qstart, qlen, n, mode)
            top, n_found = self.index.match_songs_dense(emb, qstart, qlen, out["res"], to_host=False)
            return {"res": top, "n_found": n_found}
        return self._launch(emb, match, mode=0)

    def query_rescore_finish(self, p):
        """Second half: -> (answers, ranked) in query_dense_finish's form, without per-song blocks: answers
        [(score, (song, time_s), None)] from entry 0, ranked per query up to n (score, (song, time_s)) best first."""
        res = self._read_back(p)[0]
        answers = [r + (None,) for r in self._answers(res[:, 0], 0)]
        return answers, self._answers(res, 0, topn_tuples)

    def query_rescore_batch(self, emb, qstart, qlen, n):
        """emb: torch cuda [sum(qlen), d] unit-norm rows -> (answers, ranked), see query_rescore_finish"""
        return self.query_rescore_finish(self.query_rescore_launch(emb, qstart, qlen, n))

    # ---- nominated by the approximate dense pass, rescored exactly: dense-grade answers with a per-query certificate ------
    def query_nominate_rescore_launch(self, emb, qstart, qlen, n):
        """First half of query_nominate_rescore_batch: the n songs of every query with the best approximate dense score on the
        fp16 MFMA (pfann_nominate_songs_dense), then every alignment of those songs (pfann_match_songs_dense), on the one
        stream; no search, nothing is read back.  Refuses where query_rescore_launch refuses."""
        self._whole_only("query_nominate_rescore_launch: rescoring is", "the nominated songs are scored on one GPU against the whole database")
        self._dense_check("query_nominate_rescore_launch")
        n = DeviceIndex._check_n("query_nominate_rescore_launch", n)

        def match():
            cand, _, n_close = self.index.nominate_songs_dense(emb, qstart, qlen, n, to_host=False)
            top, n_found = self.index.match_songs_dense(emb, qstart, qlen, cand, to_host=False)
            return {"res": top, "n_found": n_found, "n_close": n_close, "n": n}
        return self._launch(emb, match, mode=0, search=False)

    def query_nominate_rescore_finish(self, p):
        """Second half: -> (answers, ranked, certified); answers and ranked in query_rescore_finish's form; certified[j]:
        0 <= n_close[j] <= n, the proof that entry 0 is the dense matcher's entry 0 (n_close: p["n_close_host"])."""
        answers, ranked = self.query_rescore_finish(p)
        p["n_close_host"] = p["n_close"].cpu().numpy()
        return answers, ranked, (p["n_close_host"] >= 0) & (p["n_close_host"] <= p["n"])

    def query_nominate_rescore_batch(self, emb, qstart, qlen, n):
        """emb: torch cuda [sum(qlen), d] rows -> (answers, ranked, certified), see query_nominate_rescore_finish"""
        return self.query_nominate_rescore_finish(self.query_nominate_rescore_launch(emb, qstart, qlen, n))

    # ---- monitor mode through the nomination: dense-grade windows without the fp32 dense pass, a certificate per window ------
    def monitor_nominate_launch(self, emb, rstart, rlen, window, hop, n, edge_window=0):
        """monitor_dense_launch without the fp32 dense pass: the n songs of every window with the best approximate dense score on
        the fp16 MFMA (pfann_nominate_windows_dense: the windows of a recording share their row dots), then every alignment of
        those songs for the windows as queries (pfann_match_songs_dense on window_queries), then entry 0 of every window, on the
        one stream; no search, nothing is read back.  edge_window > 0: the short windows at hop 1 take the same route.
        PFANN_NOMINATE_WINDOWS_GENERAL=1 (read per launch) routes the nomination through pfann_nominate_songs_dense on the
        expanded windows instead: the same bytes, for A/B timing.  Refuses where query_nominate_rescore_launch refuses.
        -> what monitor_nominate_finish reads."""
        self._whole_only("monitor_nominate_launch: rescoring is", "the nominated songs are scored on one GPU against the whole database")
        self._dense_check("monitor_nominate_launch")
        n = DeviceIndex._check_n("monitor_nominate_launch", n)
        general = os.environ.get("PFANN_NOMINATE_WINDOWS_GENERAL", "") == "1"

        def windows(w, h):
            qstart, qlen, wfirst = window_queries(rstart, rlen, w, h)
            if general:
                cand, _, n_close = self.index.nominate_songs_dense(emb, qstart, qlen, n, to_host=False, max_qlen=min(int(w), 64))
            else:
                (cand, _, n_close), _ = self.index.nominate_windows_dense(emb, rstart, rlen, w, h, n, to_host=False)
            top, _ = self.index.match_songs_dense(emb, qstart, qlen, cand, to_host=False)
            return top[:, 0].contiguous(), wfirst, n_close

        def match():
            DeviceIndex._window_hop("monitor_nominate_launch", window, hop)
            res, wfirst, n_close = windows(int(window), int(hop))
            out = {"res": res, "wfirst": wfirst, "hop": int(hop), "n_close": n_close, "n": n, "fine": None}
            if edge_window > 0:
                edge, efirst, out["edge_n_close"] = windows(int(edge_window), 1)
                out["fine"] = (edge, efirst)
            return out
        return self._launch(emb, match, mode=0, search=False)

    def monitor_nominate_finish(self, p):
        """Second half: -> (rows as monitor_finish gives them, per recording n_close int32 [windows], per recording certified bool
        [windows]): certified = 0 <= n_close <= n, the proof that the window's row IS monitor_dense_launch's row.  The edge
        pass is left in p["edge_rows"], p["edge_n_close"] and p["edge_certified"] in the same form."""
        rows = self.monitor_finish(p)

        def per_recording(n_close, wfirst):
            n_close = n_close.cpu().numpy()
            close = [n_close[a:b] for a, b in zip(wfirst[:-1], wfirst[1:])]
            return close, [(c >= 0) & (c <= p["n"]) for c in close]
        if p.get("fine") is not None:
            p["edge_n_close"], p["edge_certified"] = per_recording(p["edge_n_close"], p["fine"][1])
        return (rows,) + tuple(per_recording(p["n_close"], p["wfirst"]))

    def monitor_finish(self, p):
        """Second half: -> per recording a structured array (w0, score, song, time_s), one entry per window: its first
        row, and score / song / time exactly as query_finish reports them for that slice (no candidate: -inf, -1, 0)."""
        return self._windows_finish(p, self.frame_shift_mul)

    def _windows_finish(self, p, fsm, rows=monitor_rows):
        out = rows(self._read_back(p)[0], p["wfirst"], p["hop"], p["mode"], fsm, self.hop_size)
        self._edge_finish(p, fsm, rows)
        return out

    def _edge_finish(self, p, fsm, rows=monitor_rows):
        """the edge pass of a windowed launch, read back and formatted by `rows` (monitor_rows, or monitor_topn_rows for a
        ranked launch) into p["edge_rows"]"""
        if p.get("fine") is not None:                    # (complete behind the same event; the timer has its split already)
            edge, efirst = p["fine"]
            edge = self._read_back({"res": edge[0] if isinstance(edge, tuple) else edge, "ev": p["ev"][-1:]})[0]
            p["edge_rows"] = rows(edge, efirst, 1, p["mode"], fsm, self.hop_size)

    def monitor_topn_launch(self, emb, rstart, rlen, window, hop, n, edge_window=0):
        """monitor_launch with ranked answers (pfann_match_windows_topn): the n best songs of every window, and of every
        short window of the edge pass, from the same single search."""
        self._whole_only("monitor mode is", "a recording is matched on one GPU against the whole database")
        return self._launch(emb, lambda I, mode: self._windows_launched(
            lambda w, h: self.index.match_windows_topn(emb, I, rstart, rlen, w, h, n, self.frame_shift_mul, self.score_alpha, mode,
                                                       to_host=False), window, hop, edge_window))

    def monitor_topn_finish(self, p):
        """Second half: -> (per recording a structured array [windows, n] of (w0, score, song, time_s, votes), best song
        first, each entry formatted as monitor_finish formats a window's answer -- entry 0 IS that answer --, padding
        entries (-inf, -1, 0, votes 0); per recording n_found int32 [windows], the window's candidate songs, not capped at n).
        The ranked short windows of the edge pass are left in p["edge_rows"]."""
        return self._windows_topn_finish(p, self.frame_shift_mul)

    def _windows_topn_finish(self, p, fsm):
        out = self._windows_finish(p, fsm, monitor_topn_rows)
        n_found, wfirst = p["n_found"].cpu().numpy(), p["wfirst"]
        return out, [n_found[a:b] for a, b in zip(wfirst[:-1], wfirst[1:])]

    # ---- updates: songs added and removed without a rebuild (include/pfann_amd.h: "Database updates") ---------------
    def _update_check(self, what):
        if self.sharded is not None or self.ranks is not None:
            raise _l.PfannError("%s: the handle holds a shard of the database (monitor mode is not song-sharded)" % what)

    def _updated(self):
        self.song_pos = np.array(self.index.song_pos, dtype=np.int64)
        self.song_range = (0, len(self.songList))
        self._emb_map = None                         # (self-match reads it: the file behind it has other rows now)

    def add_songs(self, names, emb, rows_per_song, persist=True):
        """New songs behind the last one -> the id of the first.  names: their songList.txt lines; emb float32
        [sum(rows_per_song), d] (numpy or torch); rows_per_song may hold zeros (the builder's unreadable file).  The handle is
        updated first -- it is the one that can refuse the rows -- then, with persist, the files through dbfiles.add_songs.
        A blocking maintenance call: no query of this Database may be in flight."""
        self._update_check("add_songs")
        names = list(names)
        rps = np.ascontiguousarray(rows_per_song, dtype=np.int32).reshape(-1)
        if len(names) != rps.shape[0]:
            raise ValueError("add_songs: %d names for %d songs" % (len(names), rps.shape[0]))
        first = self.index.append(emb, rps)
        self.songList = list(self.songList) + names
        self._updated()
        if persist:
            from . import dbfiles
            host = emb.detach().cpu().numpy() if isinstance(emb, torch.Tensor) else emb
            dbfiles.add_songs(self.dir_for_db, names, host, rps)
        return first

    def song_ids(self, ids_or_names):
        """ids (int) and songList.txt lines (str; every song of that name) -> sorted ids; unknown ones raise ValueError"""
        out = set()
        for x in ids_or_names:
            if isinstance(x, str):
                hit = [i for i, n in enumerate(self.songList) if n == x]
                if not hit:
                    raise ValueError("no song %r in the database" % x)
                out.update(hit)
            elif 0 <= int(x) < len(self.songList):
                out.add(int(x))
            else:
                raise ValueError("no song #%d in the database (0..%d)" % (int(x), len(self.songList) - 1))
        return sorted(out)

    def remove_songs(self, ids_or_names, persist=True):
        """The songs lose their rows and keep their ids (0-row songs, as landmarkKey spells them) -> the ids.  Handle
        first, then with persist the files through dbfiles.remove_songs.  A blocking maintenance call."""
        self._update_check("remove_songs")
        ids = self.song_ids(ids_or_names)
        self.index.remove_songs(ids)
        self._updated()
        if persist:
            from . import dbfiles
            dbfiles.remove_songs(self.dir_for_db, ids)
        return ids

    # ---- self-match: the database asked about itself ------------------------------------------------
    def _embeddings_map(self):
        """the `embeddings` file of the database directory, memory-mapped [rows, d] (builder.py writes it)"""
        if getattr(self, "_emb_map", None) is None:
            path = os.path.join(self.dir_for_db, "embeddings")
            n_rows = int(self.song_pos[-1])
            if not os.path.exists(path) or os.path.getsize(path) != n_rows * self.d * 4:
                raise _l.PfannError("self-match reads the query rows from %s: missing, or not %d x %d float32" % (path, n_rows, self.d))
            self._emb_map = np.memmap(path, dtype=np.float32, mode="r", shape=(n_rows, self.d)) if n_rows else np.zeros((0, self.d), np.float32)
        return self._emb_map

    def self_match_launch(self, song_lo, song_hi, window, hop, k=None, emb=None, dense=False, top=1):
        """One launch group of self-match, asynchronous like monitor_launch: the rows of the songs [song_lo, song_hi) are the
        recordings (song s: rows [song_pos[s], song_pos[s + 1]) of `emb`, by default the memory-mapped `embeddings` file),
        every row is searched with its own song's rows left out (pfann_search_topk_excl: exact, the own rows are never
        nominated), and the windowed matcher answers every window of `window` rows, `hop` apart.  The rows are database
        rows, one per hop_size, so the matcher runs with frame_shift_mul 1.  Songs without rows give no windows.
        dense=True: no search; the dense matcher (pfann_match_windows_dense) scores every alignment of every OTHER song --
        the song's own id is its recording's excluded song -- so the recall does not depend on k.
        top=N > 1: the N best OTHER songs of every window, by pfann_match_windows_dense_topn (dense) or pfann_match_windows_topn
        on the masked search's labels; self_match_finish then answers as monitor_topn_finish does."""
        top = int(top)
        if not 1 <= top <= 64:
            raise _l.PfannError("self_match: top=%d outside 1..64" % top)
        if dense:
            self._dense_check("self_match")
        self._whole_only("self_match: the dense self-match is" if dense else "self-match is", "the whole database sits on one handle")
        song_lo, song_hi = int(song_lo), int(song_hi)
        if not 0 <= song_lo <= song_hi <= len(self.songList):
            raise ValueError("self_match: songs [%d, %d) outside 0..%d" % (song_lo, song_hi, len(self.songList)))
        emb = self._embeddings_map() if emb is None else emb
        rstart, rlen, lo, hi = self_match_ranges(self.song_pos, song_lo, song_hi)
        r0, r1 = int(self.song_pos[song_lo]), int(self.song_pos[song_hi])
        q = _l.upload_async(np.array(emb[r0:r1], dtype=np.float32).reshape(-1, self.d), self.index.device, np.float32)
        if dense:
            def match_dense():
                own = np.arange(song_lo, song_hi, dtype=np.int32)
                if top > 1:
                    (res, n_found, _), wfirst = self.index.match_windows_dense_topn(q, rstart, rlen, window, hop, top,
                                                                                    exclude_song=own, to_host=False)
                    long = (res, n_found), wfirst
                else:
                    long = self.index.match_windows_dense(q, rstart, rlen, window, hop, exclude_song=own, to_host=False)
                return dict(self._windows_launched(None, window, hop, long=long), songs=(song_lo, song_hi))
            return self._launch(q, match_dense, mode=0, search=False)

        def match(I, mode):
            if top > 1:
                long = self.index.match_windows_topn(q, I, rstart, rlen, window, hop, top, 1, self.score_alpha, mode, to_host=False)
            else:
                long = self.index.match_windows(q, I, rstart, rlen, window, hop, 1, self.score_alpha, mode, to_host=False)
            return dict(self._windows_launched(None, window, hop, long=long), songs=(song_lo, song_hi))
        return self._launch(q, match, k=k, exclude=(lo, hi))

    def self_match_finish(self, p):
        """-> per song of the group a structured array (w0, score, song, time_s), one entry per window, as monitor_finish; a
        launch with top > 1: per song the [windows, top] array of monitor_topn_finish (its n_found is left in p["n_found_rows"])"""
        if "n_found" in p:
            out, p["n_found_rows"] = self._windows_topn_finish(p, 1)
            return out
        return self._windows_finish(p, 1)

    def self_match(self, song_lo, song_hi, window, hop, k=None, emb=None, max_rows=None, dense=False, top=1):
        """Self-match of the songs [song_lo, song_hi): yields (song, rows) in song order, rows as monitor_finish gives them.
        The songs are cut into launch groups of at most max_rows rows (default PFANN_MAX_BATCH, 9728; a longer song is a
        group of its own) and group g + 1 is launched before group g is read back, as the monitor does.  dense, top: see
        self_match_launch (top > 1: rows is the ranked [windows, top] array of monitor_topn_finish)."""
        max_rows = int(os.environ.get("PFANN_MAX_BATCH", "9728")) if max_rows is None else int(max_rows)
        groups = self_match_groups(self.song_pos, int(song_lo), int(song_hi), max_rows)
        for p in launch_ahead(groups, lambda g: self.self_match_launch(g[0], g[1], window, hop, k, emb, dense, top)):
            yield from zip(range(*p["songs"]), self.self_match_finish(p))

    # ---- the reference's per-query contract ---------------------------------------------
    def query_embeddings(self, query):
        q = torch.as_tensor(np.ascontiguousarray(query, dtype=np.float32)) if not isinstance(query, torch.Tensor) else query
        q = q.to(self.index.device)
        if self.sharded is not None:
            # the reference's tuple on every rank: the shards' score columns all-gathered into the [n_songs, 2] block
            from .dist import all_gather_ragged, shard_songs
            p = self.query_launch(q, [0], [q.shape[0]], want_song_scores=True)
            counts = [hi - lo for lo, hi in shard_songs(self.song_pos, self.ranks.world)]
            with self.sharded.on_exchange_stream():         # (the block was produced there when the exchange stream is on)
                full = all_gather_ragged(p["ss"][0], counts, self.ranks.group).cpu().numpy()
            p["ss"] = None
            (score, best_song_t, _), = self.query_finish(p)
            return score, best_song_t, full
        (score, best_song_t, song_score), = self.query_batch(q, [0], [q.shape[0]], want_song_scores=True)
        return score, best_song_t, song_score

    query_embeddings_base = query_embeddings
