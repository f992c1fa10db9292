"""What rescoring the nominated songs recovers, at bench scale: top-1 hit rate and exact-to-0.25 s rate of the nominated matcher,
of matcher.py --rescore at N = 1, 4, 16, 64 (pfann_match_topn's N best songs, every alignment of those scored by
pfann_match_songs_dense) and of the dense matcher, on the SAME queries; and per N in how many queries the true song is among
the N nominated ones, in how many the rescored answer is the dense answer, and that no rescored entry differs in bytes from the
ranked dense matcher's entry for the same song (a count; it must be 0).

    python tools/rescore_vs_nominated.py [--db-songs 16950] [--queries 512] [--snr 0] [--k 100] [--out FILE]

Database, queries, hit and exact are those of tools/dense_vs_nominated.py (bench.py's).  There is no target: the nominated and
the dense columns are the references the rescored rows are read against.  A tool, not a test: bench.py is not involved."""
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
    (dense_top, _, _), wfirst = index.match_windows_dense_topn(emb, qstart, qlen, QUERY_SEGS, 1, 64)
    assert np.array_equal(wfirst, np.arange(Q + 1))
    dense = dense_top[:, 0]
    hit = lambda r, j: int(r[j]["song"]) == q_song[j]
    exact = lambda r, j: hit(r, j) and abs(int(r[j]["offset"]) * HOP_S - float(q_off[j])) <= 0.25
    rate = lambda f, r: sum(f(r, j) for j in range(Q))
    row = "%-14s top-1 hit %.4f (%3d)   exact to 0.25 s %.4f (%3d)"
    out = ["rescore vs nominated vs dense: %d db rows (%d songs), %d queries of %d segments at SNR %g dB, k %d" % (n_rows, n_songs, Q, QUERY_SEGS, a.snr, k),
           row % ("nominated", rate(hit, nom) / Q, rate(hit, nom), rate(exact, nom) / Q, rate(exact, nom))]
    notes = []
    for n in (1, 4, 16, 64):
        named, _ = index.match_topn(emb, I, qstart, qlen, n, to_host=False)
        top, n_found = index.match_songs_dense(emb, qstart, qlen, named)
        named = index.decode_results(named)
        res = top[:, 0]
        among = sum(q_song[j] in named["song"][j] for j in range(Q))
        same = sum((int(res[j]["song"]), int(res[j]["offset"])) == (int(dense[j]["song"]), int(dense[j]["offset"])) for j in range(Q))
        compared = differing = 0
        for j in range(Q):                               # the songs both lists hold: the same 24 bytes?
            where = {int(s): i for i, s in enumerate(dense_top["song"][j]) if s >= 0}
            for e in top[j]:
                i = where.get(int(e["song"])) if e["song"] >= 0 else None
                if i is not None:
                    compared += 1
                    differing += e.tobytes() != dense_top[j, i].tobytes()
        out.append(row % ("--rescore %d" % n, rate(hit, res) / Q, rate(hit, res), rate(exact, res) / Q, rate(exact, res)))
        notes.append("N %2d: true song among the nominated songs in %d of %d queries; rescored answer = dense answer (song, offset) in %d; "
                     "entries that differ in bytes from the ranked dense matcher's entry for the same song: %d of %d compared"
                     % (n, among, Q, same, differing, compared))
    out.append(row % ("dense", rate(hit, dense) / Q, rate(hit, dense), rate(exact, dense) / Q, rate(exact, dense)))
    out += notes
    print("\n".join(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(out) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
