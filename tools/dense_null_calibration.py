"""Does the normal tail hold on real fingerprints?  The false-alarm level of the dense matcher's significance
(pfann_match_windows_dense_stats + pfann_amd/significance.py) measured at bench scale, on queries that ARE and that are NOT in
the database.

    python tools/dense_null_calibration.py [--db-songs 16950] [--queries 512] [--snr 0] [--ranked] [--out FILE]

Database and queries are bench.py's, as in tools/dense_vs_nominated.py: --db-songs synthetic 30 s songs (59 segments each) embedded
by the builder loop with the seeded, calibrated weights, and 10 s crops (19 segments) of songs spread over the database at the
given SNR.  Every query is answered twice, as one window over all its rows: with exclude_song = its true song, so that the query is
absent from the database (whatever the window then names is a false alarm), and with exclude_song = -1 (present).  For the nominal
levels 1e-1, 1e-2 and 1e-3: the fraction of absent queries flagged (log10_fa <= log10 level; nominal: the level itself) and the
fraction of present queries kept (flagged AND naming the true song); and the same two numbers for monitor.py's fixed
--min-score 0.2.  The rows of one song are correlated along a diagonal and the model is not iid: this is the measurement of how
far off nominal the union bound under a normal model is.  A tool, not a test: bench.py is not involved.

--ranked: the same measurement through the product path, Database.query_dense_stats_batch(n = 3)
(pfann_match_windows_dense_topn_stats + significance.log10_false_alarms_ranked) on a Database built from the same rows.  The
Database has no excluded song, so the absent class is made by removing the queries' true songs from the handle
(Database.remove_songs, all of them at once) and asking again.  Rank 1 must equal the unranked call's log10_fa on the same handle
to the last bit -- the statistics are the same integers -- and that is asserted for both classes.  Reported per level: the absent
queries with rank 1, rank 2, rank 3 and ANY of the three entries flagged; the present queries whose true song is flagged at any
rank; and the entries beside a true match (ranks 2 and 3 of a present query that name another song) that are flagged."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SEG_PER_SONG, QUERY_SEGS, HOP_S = 59, 19, 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--db-songs", type=int, default=16950)
    ap.add_argument("--queries", type=int, default=512)
    ap.add_argument("--snr", type=float, default=0.0)
    ap.add_argument("--max-batch", type=int, default=9728)
    ap.add_argument("--ranked", action="store_true", help="measure through Database.query_dense_stats_batch(n = 3)")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    import torch
    from pfann_amd import lib as plib
    from pfann_amd import synth
    from pfann_amd.builder import embed_files
    from pfann_amd.database import DeviceIndex
    from pfann_amd.engine import Engine
    from pfann_amd.utils import read_config
    plib.require_gpu()
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    params = read_config(os.path.join(repo, "configs", "default.json"))
    d = params["model"]["d"]
    dev = torch.device("cuda", 0)
    eng = Engine(params, 0, max_batch=a.max_batch)
    eng.load_state_dict(synth.make_state_dict_calibrated(params, seed=123))

    class PcmList:                       # what builder.embed_files needs of a MusicDataset: files + load_pcm(i)
        def __init__(self, ids, pcm_host):
            self.files = ["synthetic song %d" % i for i in ids]
            self.pcm = pcm_host

        def load_pcm(self, i):
            return self.pcm[i]

        def __len__(self):
            return len(self.files)

    n_songs = a.db_songs
    song_pos = np.arange(n_songs + 1, dtype=np.int64) * SEG_PER_SONG
    n_rows = int(song_pos[-1])
    rows = torch.empty((n_rows, d), device=dev, dtype=torch.float32)
    CH = 4 * max(1, a.max_batch // SEG_PER_SONG)
    host_buf = torch.empty((CH, SEG_PER_SONG * 4000 + 4000), dtype=torch.int16).pin_memory()
    for c0 in range(0, n_songs, CH):
        ids = list(range(c0, min(c0 + CH, n_songs)))
        host_buf[:len(ids)].copy_(synth.make_songs_torch(ids, 30.0, device=dev))
        torch.cuda.synchronize()
        for i, n_seg, e in embed_files(eng, PcmList(ids, host_buf), 4000, batch_windows=a.max_batch):
            assert n_seg == SEG_PER_SONG
            rows[int(song_pos[ids[i]]):int(song_pos[ids[i] + 1])] = e
        print("embedded %d of %d songs" % (ids[-1] + 1, n_songs), file=sys.stderr, flush=True)
    index = DeviceIndex(d, 0)
    index.load(rows, song_pos)

    Q = a.queries
    q_song = [int((j * 7919 + 13) % n_songs) for j in range(Q)]
    pcm, off = [], []
    for c0 in range(0, Q, CH):
        c1 = min(c0 + CH, Q)
        qp, qo = synth.make_queries_torch(synth.make_songs_torch(q_song[c0:c1], 30.0, device=dev), list(range(c0, c1)), 10.0, a.snr)
        pcm.append(qp)
        off.append(qo)
    pcm, q_off = torch.cat(pcm), torch.cat(off).cpu().numpy()
    q_len = pcm.shape[1]
    starts = (np.arange(Q, dtype=np.int64)[:, None] * q_len + np.arange(QUERY_SEGS, dtype=np.int64)[None, :] * 4000).reshape(-1)
    emb = eng.embed_windows(eng.pcm16_to_mono(pcm.reshape(-1).contiguous()), torch.as_tensor(starts).to(dev))
    qstart = np.arange(Q, dtype=np.int64) * QUERY_SEGS
    qlen = np.full(Q, QUERY_SEGS, dtype=np.int32)

    from pfann_amd import significance as sg
    from pfann_amd.monitor import DEFAULT_MIN_SCORE
    song_len = np.diff(song_pos)
    hists = sg.OverlapHistograms(song_len)

    def run(excl, index=index, hists=hists, song_len=song_len):
        (res, stats), wfirst = index.match_windows_dense_stats(emb, qstart, qlen, QUERY_SEGS, 1, exclude_song=excl)
        assert np.array_equal(wfirst, np.arange(Q + 1))
        fa = np.asarray([sg.log10_false_alarm(r["score"], QUERY_SEGS, r["song"], r["offset"], (s["n_full"], s["sum_q"], s["sumsq_q"]),
                                              hists(QUERY_SEGS, int(e)), song_len) for r, s, e in zip(res, stats, excl)])
        return res, fa
    truth = np.asarray(q_song, dtype=np.int32)
    if a.ranked:
        out = ranked_report(a, params, rows, song_pos, emb, qstart, qlen, truth, run)
        print("\n".join(out))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(out) + "\n")
        return 0
    absent, fa_absent = run(truth)
    present, fa_present = run(np.full(Q, -1, dtype=np.int32))
    assert (absent["song"] != truth).all()
    hit = present["song"] == truth
    out = ["dense null calibration: %d db rows (%d songs), %d queries of %d segments at SNR %g dB, one window per query"
           % (n_rows, n_songs, Q, QUERY_SEGS, a.snr),
           "present queries naming their song (top-1 hit rate): %.4f (%d)" % (hit.mean(), int(hit.sum())),
           "log10_fa of absent queries:  min %.2f  median %.2f  max %.2f" % (fa_absent.min(), np.median(fa_absent), fa_absent.max()),
           "log10_fa of present queries: min %.2f  median %.2f  max %.2f" % (fa_present.min(), np.median(fa_present), fa_present.max()),
           "%-24s %22s %26s" % ("threshold", "absent queries flagged", "present queries kept (hit)")]
    for level in (1e-1, 1e-2, 1e-3):
        fl = fa_absent <= np.log10(level)
        kp = (fa_present <= np.log10(level)) & hit
        out.append("%-24s %15.4f (%4d) %19.4f (%4d)" % ("--max-fa %g" % level, fl.mean(), int(fl.sum()), kp.mean(), int(kp.sum())))
    fl = absent["score"] >= DEFAULT_MIN_SCORE
    kp = (present["score"] >= DEFAULT_MIN_SCORE) & hit
    out.append("%-24s %15.4f (%4d) %19.4f (%4d)" % ("--min-score %g" % DEFAULT_MIN_SCORE, fl.mean(), int(fl.sum()), kp.mean(), int(kp.sum())))
    out.append("scores: absent %.4f .. %.4f, present hits %.4f .. %.4f" % (absent["score"].min(), absent["score"].max(),
                                                                          present["score"][hit].min() if hit.any() else float("nan"),
                                                                          present["score"][hit].max() if hit.any() else float("nan")))
    print("\n".join(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(out) + "\n")
    return 0


def ranked_report(a, params, rows, song_pos, emb, qstart, qlen, truth, run):
    """--ranked (module docstring) -> the lines of the report"""
    import tempfile
    from pfann_amd import significance as sg
    from pfann_amd.database import Database
    Q, n_songs = len(truth), len(song_pos) - 1
    none = np.full(Q, -1, dtype=np.int32)
    N_TOP = 3
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "songList.txt"), "w") as f:
            f.write("".join("synthetic song %d\n" % i for i in range(n_songs)))
        np.diff(song_pos).astype(np.int32).tofile(os.path.join(tmp, "landmarkKey"))
        rows.cpu().numpy().tofile(os.path.join(tmp, "embeddings"))
        db = Database(tmp, params["indexer"], params["hop_size"], d=rows.shape[1])

    def ask(what):
        """-> (song [Q, 3], log10_fa [Q, 3]; -1 / 0 past the list), rank 1 asserted bit-equal to the unranked call on this handle"""
        _, ranked, fa = db.query_dense_stats_batch(emb, qstart, qlen, n=N_TOP)
        song = np.full((Q, N_TOP), -1, dtype=np.int64)
        val = np.zeros((Q, N_TOP))
        for j, (lst, v) in enumerate(zip(ranked, fa)):
            song[j, :len(lst)] = [s for _, (s, _) in lst]
            val[j, :len(v)] = v
        lens = np.diff(db.song_pos)
        res, fa1 = run(none, index=db.index, hists=sg.OverlapHistograms(lens), song_len=lens)
        assert np.array_equal(song[:, 0], res["song"].astype(np.int64)), "%s: rank 1 names other songs than the unranked call" % what
        assert np.array_equal(val[:, 0], fa1), "%s: rank 1 is not the unranked call's log10_fa to the last bit" % what
        return song, val, fa1
    p_song, p_fa, p_fa1 = ask("present")
    _, fa_present_old = run(none)
    assert np.array_equal(p_fa1, fa_present_old), "present: the Database's handle answers differently from the tool's own handle"
    _, fa_absent_old = run(truth)
    gone = db.remove_songs(sorted({int(t) for t in truth}), persist=False)
    a_song, a_fa, _ = ask("absent")
    assert not np.isin(a_song, gone).any()
    hit = p_song[:, 0] == truth
    is_true = p_song == truth[:, None]
    beside = (p_song >= 0) & ~is_true & hit[:, None]
    beside[:, 0] = False                                   # ranks 2 and 3 of a query whose rank 1 is its true song
    out = ["dense null calibration through Database.query_dense_stats_batch(n = %d): %d db rows (%d songs), %d queries of %d segments at "
           "SNR %g dB, one window per query" % (N_TOP, int(song_pos[-1]), n_songs, Q, QUERY_SEGS, a.snr),
           "absent class: the %d true songs of the queries removed from the handle (the unranked tool excludes one song per query)" % len(gone),
           "rank 1 equals pfann_match_windows_dense_stats + log10_false_alarm on the same handle to the last bit: both classes, all %d "
           "queries; present rank 1 equals the unranked tool's present column likewise" % Q,
           "present queries naming their song at rank 1: %.4f (%d); at any rank: %.4f (%d)"
           % (hit.mean(), int(hit.sum()), is_true.any(1).mean(), int(is_true.any(1).sum()))]
    for r in range(N_TOP):
        out.append("log10_fa, rank %d: absent min %.2f median %.2f max %.2f; present min %.2f median %.2f max %.2f"
                   % (r + 1, a_fa[:, r].min(), np.median(a_fa[:, r]), a_fa[:, r].max(), p_fa[:, r].min(), np.median(p_fa[:, r]), p_fa[:, r].max()))
    out.append("%-14s | %-44s | %-24s | %-22s | %s" % ("threshold", "absent flagged: rank 1 / rank 2 / rank 3 / ANY", "absent rank 1, one song",
                                                    "present: true song", "present: other songs at ranks 2, 3"))
    out.append("%-14s | %-44s | %-24s | %-22s | %s" % ("", "(true songs removed)", "excluded (unranked tool)", "flagged at any rank",
                                                    "flagged, of %d entries" % int(beside.sum())))
    for level in (1e-1, 1e-2, 1e-3):
        t = np.log10(level)
        fl = a_fa <= t
        anyf = fl.any(1)
        old = fa_absent_old <= t
        kept = ((p_fa <= t) & is_true).any(1)
        bs = (p_fa <= t) & beside
        out.append("%-14s | %.4f / %.4f / %.4f / %.4f (%3d %3d %3d %3d) | %15.4f (%4d)   | %13.4f (%4d)   | %.4f (%d)"
                   % ("--max-fa %g" % level, fl[:, 0].mean(), fl[:, 1].mean(), fl[:, 2].mean(), anyf.mean(), int(fl[:, 0].sum()),
                      int(fl[:, 1].sum()), int(fl[:, 2].sum()), int(anyf.sum()), old.mean(), int(old.sum()), kept.mean(), int(kept.sum()),
                      bs.sum() / max(int(beside.sum()), 1), int(bs.sum())))
    return out


if __name__ == "__main__":
    sys.exit(main())
