"""Re-cutting stored masters against the rate ladder and a plain copy (icerx_recut_device_async, include/icer_hip_dec.h).

For each case, with device events on one stream and after a warm-up: the frames are encoded once at the lossless quota and
their streams packed into one blob (the stored masters); then, measured in the same run,
  re-cut     one icerx_recut_device_async call that cuts every master to the case's quotas (tools/ladder_bench.py's ladders)
  ladder     icerx_encode_device_ladder on the source frames at the same quotas
  copy       a device-to-device copy of as many bytes as the re-cut writes
Every re-cut stream is checked against the ladder's (bytes, sizes, return codes).  Prints a markdown table (profiles/recut.md).

    python tools/recut_bench.py [--reps N] [--warmup W] [--case NAME ...]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CASES = {
    # name: (w, h, channels, stages, segments, frames, quotas)
    "lone 4096^2 gray": (4096, 4096, 1, 5, 10, 1, [2 * 4096 * 4096 + 100_000, 5_000_000, 1_000_000, 70_000]),
    "32 x 2048^2 gray": (2048, 2048, 1, 4, 16, 32, [2 * 2048 * 2048 + 100_000, 1_000_000, 300_000, 70_000]),
}


def run_case(torch, name, reps, warmup):
    from icer_compression_amd import api, decoder
    from ladder_bench import frames_for, timed
    w, h, C, stages, segs, n, quotas = CASES[name]
    dev = torch.device("cuda", 0)
    enc = api.Encoder(w, h, C, stages, 0, segs, max_frames=n)
    rec = decoder.Recutter(w, h, C, stages, segs)
    t = frames_for(torch, dev, w, h, C, n)
    Q, top = len(quotas), max(quotas)
    lad, lsz, lrc = enc.encode_ladder_torch(t, quotas)
    torch.cuda.synchronize()
    # the stored masters: the lossless streams one after another in one blob
    k = quotas.index(top)
    assert all(int(x) == 0 for x in lrc[k].tolist()), "the largest quota does not hold the lossless streams"
    lens = lsz[k].clone()
    blob = torch.cat([lad[k, f, : int(lens[f])] for f in range(n)]).contiguous()
    offsets = torch.cumsum(lens, 0) - lens
    out = torch.empty((Q, n, top), dtype=torch.uint8, device=dev)
    rsz, rrc = torch.empty((Q, n), dtype=torch.int64, device=dev), torch.empty((Q, n), dtype=torch.int32, device=dev)

    def recut():
        rec.recut_torch(blob, lens, quotas, out, rsz, rrc, offsets=offsets)

    def ladder():
        enc.encode_ladder_torch(t, quotas, lad, lsz, lrc)

    t_recut = timed(torch, recut, reps, warmup)
    t_ladder = timed(torch, ladder, reps, warmup)
    torch.cuda.synchronize()
    assert torch.equal(rsz, lsz) and torch.equal(rrc, lrc), (name, rsz.tolist(), lsz.tolist(), rrc.tolist(), lrc.tolist())
    mismatches = 0
    for q in range(Q):
        for f in range(n):
            s = int(lsz[q, f])
            mismatches += not torch.equal(out[q, f, :s], lad[q, f, :s])
    assert mismatches == 0, (name, mismatches)
    written = int(rsz.sum())
    src, dst = torch.empty(written, dtype=torch.uint8, device=dev), torch.empty(written, dtype=torch.uint8, device=dev)
    t_copy = timed(torch, lambda: dst.copy_(src), reps, warmup)
    print(f"| {name} | {blob.numel()} | {written} | {t_recut:.3f} | {t_ladder:.3f} | {t_copy:.3f} | {t_recut / t_ladder:.3f} | "
          f"{t_recut / t_copy:.1f} | {Q * n} streams exact; frame 0: "
          f"{', '.join(f'{int(s)} ({int(r)})' for s, r in zip(rsz[:, 0].tolist(), rrc[:, 0].tolist()))} |", flush=True)
    enc.close()
    rec.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--case", action="append", choices=list(CASES))
    args = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")                       # (torch's HIP runtime first, as bench.py does)
    print("| case | master bytes | bytes written | re-cut ms | ladder encode ms | copy of the written bytes ms | re-cut / ladder | "
          "re-cut / copy | check; stream bytes (rc) per quota |")
    print("|---|---|---|---|---|---|---|---|---|")
    for name in args.case or list(CASES):
        run_case(torch, name, args.reps, args.warmup)


if __name__ == "__main__":
    main()
