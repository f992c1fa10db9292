"""What nomination costs in accuracy, at bench scale: the top-1 hit rate of the nominated pipeline (search k + sequence match)
and of the dense matcher (pfann_match_windows_dense: every alignment of every song) on the SAME queries, and, for the queries
where the two answers differ, whether the nominated path had the true alignment among its candidates at all.

    python tools/dense_vs_nominated.py [--db-songs 16950] [--queries 512] [--snr 0] [--k 100] [--out FILE]

Database and queries are bench.py's: --db-songs synthetic 30 s songs (59 segments each; 16950 songs = 1,000,050 rows) embedded
by the builder loop with the seeded, calibrated weights, and 10 s crops (19 segments) of songs spread over the database at the
given SNR.  A hit = the answer names the query's song (bench.py's top1_hit_rate); the true alignment = that song at the crop's
offset, to within half a hop (bench.py's top1_exact_0.25s).  A tool, not a test: bench.py is not involved."""
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
    ap.add_argument("--k", type=int, default=None, help="neighbours per row (default: the indexer's top_k)")
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
    k = a.k if a.k is not None else params["indexer"]["top_k"]
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

    _, I = index.search(emb, k)
    nom, _ = index.match(emb, I, qstart, qlen)
    dense, wfirst = index.match_windows_dense(emb, qstart, qlen, QUERY_SEGS, 1)
    assert np.array_equal(wfirst, np.arange(Q + 1))
    labels = I.cpu().numpy().reshape(Q, QUERY_SEGS, k)

    def nominated_truth(j):
        """did a label of one of the query's rows nominate the query's song at the crop's offset (to within half a hop)?"""
        lab = labels[j]
        t = np.broadcast_to(np.arange(QUERY_SEGS)[:, None], lab.shape)[lab >= 0]
        lab = lab[lab >= 0]
        song = lab // SEG_PER_SONG
        o = lab - song * SEG_PER_SONG - t
        return bool(((song == q_song[j]) & (np.abs(o * HOP_S - float(q_off[j])) <= 0.25)).any())

    hit = lambda r, j: int(r[j]["song"]) == q_song[j]
    exact = lambda r, j: hit(r, j) and abs(int(r[j]["offset"]) * HOP_S - float(q_off[j])) <= 0.25
    hn, hd = sum(hit(nom, j) for j in range(Q)), sum(hit(dense, j) for j in range(Q))
    en, ed = sum(exact(nom, j) for j in range(Q)), sum(exact(dense, j) for j in range(Q))
    differ = [j for j in range(Q) if (int(nom[j]["song"]), int(nom[j]["offset"])) != (int(dense[j]["song"]), int(dense[j]["offset"]))]
    split = {}
    for j in differ:
        key = ("true alignment nominated" if nominated_truth(j) else "true alignment NOT nominated",
               "dense hit" if hit(dense, j) else "dense miss", "nominated hit" if hit(nom, j) else "nominated miss")
        split[key] = split.get(key, 0) + 1
    never = sum(not nominated_truth(j) for j in range(Q))
    lower = sum(float(dense[j]["score"]) < float(nom[j]["score"]) - 1e-6 for j in range(Q))
    out = ["dense vs nominated: %d db rows (%d songs), %d queries of %d segments at SNR %g dB, k %d" % (n_rows, n_songs, Q, QUERY_SEGS, a.snr, k),
           "top-1 hit rate         nominated %.4f (%d)   dense %.4f (%d)" % (hn / Q, hn, hd / Q, hd),
           "top-1 exact to 0.25 s  nominated %.4f (%d)   dense %.4f (%d)" % (en / Q, en, ed / Q, ed),
           "queries whose true alignment no row nominated: %d of %d" % (never, Q),
           "queries where the two answers differ in (song, offset): %d" % len(differ)]
    out += ["    %-30s %-11s %-15s %d" % (key + (n,)) for key, n in sorted(split.items())]
    out += ["dense score below the nominated score by more than 1e-6: %d queries (the nominated set is a subset: expect 0)" % lower]
    print("\n".join(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(out) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
