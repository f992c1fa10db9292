"""Generate tests/golden/monitor_windows.npz: the reference's own `Database.query_embeddings` on every window slice of two
synthetic recordings (monitor mode's definition: window [w0, w0 + W) of a recording answers as that slice does as a query).

Run once from the repo root where the reference checkout is present (never on the GPU box):
    python tests/golden/make_golden_monitor.py
The reference's database.py is imported and executed as it stands, with the stand-ins of make_golden.py for faiss (an
exact flat inner-product index) -- nothing of it is copied here.  The fixture holds arrays only.

Recordings: excerpts of three songs joined by noise rows, every row perturbed and renormalised; window 9, hop 2, so song
boundaries fall inside windows; the second recording (6 rows) is shorter than the window and answers as one slice.
The seed is chosen so that in every window the best candidate leads the second best by more than 4e-6 (float64 oracle,
asserted here and in tests/test_monitor_host.py): two fp32 scorers within 1e-6 of float64 each then agree on every decision.
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as mg  # noqa: E402  (REF, _FlatIP, _install_faiss)
from pfann_amd import synth  # noqa: E402

OUT = os.path.join(HERE, "monitor_windows.npz")
SEED, D, K, WINDOW, HOP, HOP_SIZE = 21, 32, 10, 9, 2, 0.5


def window_starts(L, window, hop):
    if L <= 0:
        return []
    if L < window:
        return [(0, L)]
    return [(w0, window) for w0 in range(0, L - window + 1, hop)]


def inputs(seed=SEED):
    """-> (db, key, rec rows, rstart, rlen)"""
    key = [int(x) for x in (14 + 20 * synth.uniform01(seed, "mon/key", 12))]
    key[4] = 0
    pos = np.pad(np.cumsum(key), (1, 0))
    db = synth.unit_rows(seed, "mon/db", sum(key), D).astype(np.float32)

    def noise(tag, n):
        return synth.unit_rows(seed + 1, "mon/" + tag, n, D).astype(np.float64)
    parts = [noise("n0", 5), db[pos[2] + 3: pos[2] + 16], noise("n1", 4), db[pos[7]: pos[7] + 12], noise("n2", 3),
             db[pos[9] + 5: pos[9] + 5 + 11], noise("n3", 4)]
    rec0 = np.concatenate(parts).astype(np.float64)
    rec1 = db[pos[5] + 2: pos[5] + 8].astype(np.float64)
    rec = np.concatenate([rec0, rec1])
    rec = rec + 0.5 * synth.unit_rows(seed + 2, "mon/perturb", rec.shape[0], D)
    rec = (rec / np.linalg.norm(rec, axis=1, keepdims=True)).astype(np.float32)
    return db, np.asarray(key, np.int32), rec, np.array([0, rec0.shape[0]], np.int64), np.array([rec0.shape[0], 6], np.int32)


def generate():
    store = {}
    mg._install_faiss(store)
    if mg.REF not in sys.path:
        sys.path.insert(0, mg.REF)
    import database as refdb
    db, key, rec, rstart, rlen = inputs()
    with tempfile.TemporaryDirectory() as td:
        key.tofile(os.path.join(td, "landmarkKey"))
        open(os.path.join(td, "songList.txt"), "w").write("".join("song%d.wav\n" % i for i in range(len(key))))
        idx = mg._FlatIP(db)
        store[os.path.join(td, "landmarkValue")] = idx
        dbo = refdb.Database(td, {"top_k": K, "frame_shift_mul": 1}, HOP_SIZE)
        _, labels = idx.search(rec, K)
        score, song, sec = [], [], []
        for s, L in zip(rstart, rlen):
            for w0, n in window_starts(int(L), WINDOW, HOP):
                sc, (sg, t), _ = dbo.query_embeddings(rec[s + w0: s + w0 + n])
                score.append(sc)
                song.append(sg)
                sec.append(t)
    return dict(db=db, landmarkKey=key, rec=rec, labels=labels.astype(np.int64), rstart=rstart, rlen=rlen,
                window=np.array(WINDOW), hop=np.array(HOP), hop_size=np.array(HOP_SIZE),
                score=np.asarray(score, np.float64), song=np.asarray(song, np.int64), time=np.asarray(sec, np.float64))


if __name__ == "__main__":
    out = generate()
    np.savez_compressed(OUT, **out)
    print("monitor_windows.npz: %d windows, songs %s" % (out["song"].shape[0], out["song"].tolist()))
