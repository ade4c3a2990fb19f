#!/usr/bin/env python3
"""Benchmark of the decode sessions (include/icer_hip_dec_session.h) -- NOT bench.py's metric.

    python tools/decode_session_bench.py [--reps 5] [--warmup 1] [--batch 64] [--only c4|lone]

Two workloads, each from ONE lossless master made by the HIP encoder (synth.gray_frame, filter A), its copies resident in HBM:
    c4      `--batch` frames of 2048 x 2048, 4 stages, 16 segments (BASELINE configs[3])
    lone    one frame of 4096 x 4096, 5 stages, 10 segments (BASELINE configs[1])
The master is re-cut (Recutter.recut) to the quotas q, 2 q and 4 q with q = an eighth of its bytes; the rungs are those three cuts
and the master, the increments between them come from Recutter.combine (DIFFERENCE).  Per round, in one process and taking
turns: the session is reset, then per rung the increment is fed (Session.feed_torch: icerx_session_feed_device) and the rung's
whole stream is decoded by the plain call (Decoder.decode_device: icerx_decode_device, which this feature leaves alone) -- each
timed around call + synchronise.  Median, minimum and maximum over `--reps` rounds after `--warmup` untimed ones.  Checked in the
same run: every feed's planes equal the plain call's.  After the timed rounds two untimed ones count, per rung, the chains by route
(`routes`): one pinned to the thread route (ICER_DEC_WAVE=0), where icerx_session_stats counts every chain of a feed, and one in
the mode of the run.  One JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"c4": dict(w=2048, h=2048, stages=4, segments=16), "lone": dict(w=4096, h=4096, stages=5, segments=10)}
FILT = 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--only", default=None, help="c4 or lone")
    a = ap.parse_args()
    import torch
    from icer_compression_amd import api, decoder, synth
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)                                   # torch's HIP runtime first (see tests/conftest.py)

    def run(name, n):
        cfg = WORKLOADS[name]
        w, h, stages, segments = cfg["w"], cfg["h"], cfg["stages"], cfg["segments"]
        rc, master, _ = api.compress([synth.gray_frame(w, h, 12345, 1)], stages, FILT, segments, 4 * w * h)
        assert rc == 0 and master, rc
        q = len(master) // 8
        rec = decoder.Recutter(w, h, 1, stages, segments)
        rungs = [row[0][1] for row in rec.recut([master], [q, 2 * q, 4 * q])] + [master]
        incs = [rungs[0]] + [rec.combine([rungs[i]], [rungs[i + 1]], decoder.COMBINE_DIFFERENCE)[0][1] for i in range(3)]
        rec.close()
        dec = decoder.Decoder(1, stages, FILT, segments)
        ses = decoder.Session(dec, n, w * h)
        d_incs = [torch.from_numpy(np.frombuffer(x * n, dtype=np.uint8).copy()).to(dev) for x in incs]
        d_rungs = [torch.from_numpy(np.frombuffer(x * n, dtype=np.uint8).copy()).to(dev) for x in rungs]
        fed = torch.zeros((n, 1, w * h), dtype=torch.int16, device=dev)
        plain = torch.zeros((n, 1, w * h), dtype=torch.int16, device=dev)
        times = {(kind, i): [] for kind in ("feed", "plain") for i in range(4)}
        same = True
        for rnd in range(a.warmup + a.reps):
            ses.reset()
            for i in range(4):
                torch.cuda.synchronize()
                t = time.perf_counter()
                rcs, _, _ = ses.feed_torch(d_incs[i], [len(incs[i])] * n, fed, offsets=[k * len(incs[i]) for k in range(n)])
                torch.cuda.synchronize()
                t_feed = (time.perf_counter() - t) * 1e3
                assert rcs == [0] * n, rcs
                t = time.perf_counter()
                rc, rcs, _, _ = dec.decode_device(n, d_rungs[i].data_ptr(), [k * len(rungs[i]) for k in range(n)], [len(rungs[i])] * n,
                                                  plain.data_ptr(), w * h)
                torch.cuda.synchronize()
                t_plain = (time.perf_counter() - t) * 1e3
                assert rc == 0 and rcs == [0] * n, (rc, rcs)
                if rnd >= a.warmup:
                    times[("feed", i)].append(t_feed)
                    times[("plain", i)].append(t_plain)
                same = same and bool(torch.equal(fed, plain))
        stats = ses.stats()

        def chain_counts(mode):
            """per rung (chains resumed in the wave-per-plane kernel, chains on the thread route) of one untimed round under ICER_DEC_WAVE=mode"""
            keep = os.environ.get("ICER_DEC_WAVE")
            if mode is None:
                os.environ.pop("ICER_DEC_WAVE", None)
            else:
                os.environ["ICER_DEC_WAVE"] = mode
            try:
                ses.reset()
                out = []
                for i in range(4):
                    before = ses.stats()
                    ses.feed_torch(d_incs[i], [len(incs[i])] * n, fed, offsets=[k * len(incs[i]) for k in range(n)])
                    torch.cuda.synchronize()
                    out.append((ses.stats()[0] - before[0], ses.stats()[1] - before[1]))
                return out
            finally:
                os.environ.pop("ICER_DEC_WAVE", None)
                if keep is not None:
                    os.environ["ICER_DEC_WAVE"] = keep

        # the share of chains by route: pinned to the thread route every chain of a feed is counted, in the mode of this run the
        # chains resumed behind a loader wave and those on the thread route are; what is left took the lane-per-plane kernel, or
        # the wave-per-plane kernel with nothing held (only the rung fed into an empty slot has such chains)
        total, own = chain_counts("0"), chain_counts(os.environ.get("ICER_DEC_WAVE") or None)
        routes = []
        for i in range(4):
            chains, (resumed, threads) = total[i][1], own[i]
            left = chains - resumed - threads
            routes.append({"chains": chains, "wave_per_plane_resumed": resumed, "thread_per_chain": threads,
                           "lane_per_plane_or_nothing_held": left,
                           "shares": [round(x / max(chains, 1), 4) for x in (resumed, threads, left)]})
        ses.close()
        dec.close()
        row = lambda v: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
        return {"frames": n, "size": [w, h], "stages": stages, "segments": segments, "parity": same,
                "rungs": [{"rung": ("q", "2q", "4q", "lossless")[i], "stream_bytes": len(rungs[i]), "increment_bytes": len(incs[i]),
                           "feed": row(times[("feed", i)]), "plain_decode_of_the_rung": row(times[("plain", i)]), "routes": routes[i]} for i in range(4)],
                "session_stats": dict(zip(("chains_resumed_wave_per_plane", "chains_thread_per_chain", "planes_decoded", "packets_dropped"), stats))}

    line = {"metric": "decode session: time of a feed beside the plain decode of the same rung", "unit": "ms", "reps": a.reps, "warmup": a.warmup,
            "ICER_DEC_WAVE": os.environ.get("ICER_DEC_WAVE", "")}
    ok = True
    for name, n in (("c4", a.batch), ("lone", 1)):
        if a.only in (None, name):
            line[name] = run(name, n)
            ok = ok and line[name]["parity"]
    print(json.dumps(line))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
