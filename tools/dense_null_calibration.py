"""Does the normal tail hold on real fingerprints?  The false-alarm level of the dense matcher's significance
(pfann_match_windows_dense_stats + pfann_amd/significance.py) measured at bench scale, on queries that ARE and that are NOT in
the database.

    python tools/dense_null_calibration.py [--db-songs 16950] [--queries 512] [--snr 0] [--out FILE]

Database and queries are bench.py's, as in tools/dense_vs_nominated.py: --db-songs synthetic 30 s songs (59 segments each) embedded
by the builder loop with the seeded, calibrated weights, and 10 s crops (19 segments) of songs spread over the database at the
given SNR.  Every query is answered twice, as one window over all its rows: with exclude_song = its true song, so that the query is
absent from the database (whatever the window then names is a false alarm), and with exclude_song = -1 (present).  For the nominal
levels 1e-1, 1e-2 and 1e-3: the fraction of absent queries flagged (log10_fa <= log10 level; nominal: the level itself) and the
fraction of present queries kept (flagged AND naming the true song); and the same two numbers for monitor.py's fixed
--min-score 0.2.  The rows of one song are correlated along a diagonal and the model is not iid: this is the measurement of how
far off nominal the union bound under a normal model is.  A tool, not a test: bench.py is not involved."""
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

    def run(excl):
        (res, stats), wfirst = index.match_windows_dense_stats(emb, qstart, qlen, QUERY_SEGS, 1, exclude_song=excl)
        assert np.array_equal(wfirst, np.arange(Q + 1))
        fa = np.asarray([sg.log10_false_alarm(r["score"], QUERY_SEGS, r["song"], r["offset"], (s["n_full"], s["sum_q"], s["sumsq_q"]),
                                              hists(QUERY_SEGS, int(e)), song_len) for r, s, e in zip(res, stats, excl)])
        return res, fa
    truth = np.asarray(q_song, dtype=np.int32)
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


if __name__ == "__main__":
    sys.exit(main())
