"""Rate ladder against separate calls (icerx_encode_device_ladder, include/icer_hip.h).

For each case, with device events on one stream and after a warm-up: one ladder call over the case's quotas, the same quotas
as separate icerx_encode_device calls back to back, and the single call at the largest quota.  Every stream of the ladder is
checked against the separate calls' (bytes, sizes, return codes).  Prints a markdown table (profiles/ladder.md).

    python tools/ladder_bench.py [--reps N] [--warmup W] [--case NAME ...]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {
    # name: (w, h, channels, stages, segments, frames, quotas)
    "lone 4096^2 gray": (4096, 4096, 1, 5, 10, 1, [2 * 4096 * 4096 + 100_000, 5_000_000, 1_000_000, 70_000]),
    "8 x 2048^2 gray (C4 shape)": (2048, 2048, 1, 4, 16, 8, [2 * 2048 * 2048 + 100_000, 1_000_000, 300_000, 70_000]),
    "4096^2 YUV, progressive": (4096, 4096, 3, 5, 10, 1, [140_000, 100_000, 70_000]),
}


def frames_for(torch, dev, w, h, channels, n):
    from icer_compression_amd import synth
    if channels == 1:
        return synth.gray_frames_torch(n, w, h, synth.DEFAULT_SEED, dev)
    planes = np.stack(synth.color_frame_yuv(w, h, synth.DEFAULT_SEED))[None].repeat(n, 0)
    return torch.from_numpy(np.ascontiguousarray(planes).view(np.int16)).to(dev)


def timed(torch, fn, reps, warmup):
    """median milliseconds of fn() between two events on the current stream"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def run_case(torch, name, reps, warmup):
    from icer_compression_amd import api
    w, h, C, stages, segs, n, quotas = CASES[name]
    dev = torch.device("cuda", 0)
    enc = api.Encoder(w, h, C, stages, 0, segs, max_frames=n)
    t = frames_for(torch, dev, w, h, C, n)
    Q, top = len(quotas), max(quotas)
    stride = top
    lad = torch.empty((Q, n, stride), dtype=torch.uint8, device=dev)
    lsz, lrc = torch.empty((Q, n), dtype=torch.int64, device=dev), torch.empty((Q, n), dtype=torch.int32, device=dev)
    sep = torch.empty((Q, n, stride), dtype=torch.uint8, device=dev)
    ssz, src = torch.empty((Q, n), dtype=torch.int64, device=dev), torch.empty((Q, n), dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def ladder():
        enc.encode_ladder_torch(t, quotas, lad, lsz, lrc)

    def separate():
        for q, quota in enumerate(quotas):
            enc.encode_device_ptrs(t.data_ptr(), n, quota, sep[q].data_ptr(), stride, ssz[q].data_ptr(), src[q].data_ptr(), st)

    def single():
        enc.encode_device_ptrs(t.data_ptr(), n, top, sep[0].data_ptr(), stride, ssz[0].data_ptr(), src[0].data_ptr(), st)

    t_ladder = timed(torch, ladder, reps, warmup)
    launch = enc.launch_info()
    parts = enc.parts()
    t_sep = timed(torch, separate, reps, warmup)
    # the check: the last runs of both
    ladder()
    separate()
    torch.cuda.synchronize()
    assert torch.equal(lsz, ssz) and torch.equal(lrc, src), (name, lsz.tolist(), ssz.tolist(), lrc.tolist(), src.tolist())
    mismatches = 0
    for q in range(Q):
        for f in range(n):
            s = int(lsz[q, f])
            mismatches += not torch.equal(lad[q, f, :s], sep[q, f, :s])
    assert mismatches == 0, (name, mismatches)
    t_single = timed(torch, single, reps, warmup)
    sizes = [int(x) for x in lsz[:, 0].tolist()]
    rcs = [int(x) for x in lrc[:, 0].tolist()]
    print(f"| {name} | {Q} | {t_ladder:.3f} | {t_sep:.3f} | {t_single:.3f} | {t_ladder / t_single:.3f} | {t_sep / t_ladder:.2f} | "
          f"{'split' if launch['split'] else 'window' if launch['pipeline_waves'] == 0 else 'pipeline'}, {parts} part(s) | "
          f"{Q * n} streams exact; frame 0: {', '.join(f'{s} ({r})' for s, r in zip(sizes, rcs))} |", flush=True)
    enc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--case", action="append", choices=list(CASES))
    args = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")                       # (torch's HIP runtime first, as bench.py does)
    print("| case | quotas | ladder ms | separate calls ms | single call at the largest quota ms | ladder / single | "
          "separate / ladder | launch | check; stream bytes (rc) per quota |")
    print("|---|---|---|---|---|---|---|---|---|")
    for name in args.case or list(CASES):
        run_case(torch, name, args.reps, args.warmup)


if __name__ == "__main__":
    main()
