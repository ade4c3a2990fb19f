"""Quality-targeted encode against the rate ladder (icerx_encode_device_target / icerx_encode_device_ladder, include/icer_hip.h).

For each case, with device events on one stream and after a warm-up: one target call over the case's four MSE targets under a
byte cap, one ladder call over four quotas whose largest is that cap, and the single call at the cap.  Prints a markdown table
(profiles/quality_target.md).  With ICER_HIP_LIB naming another build of the library (the parent commit's) only the ladder and
the single call are timed.

    python tools/target_bench.py [--reps N] [--warmup W] [--case NAME ...]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.ladder_bench import frames_for, timed  # noqa: E402

CASES = {
    # name: (w, h, channels, stages, segments, frames, byte cap, smaller quotas of the ladder, MSE targets)
    "lone 4096^2 gray": (4096, 4096, 1, 5, 10, 1, 2 * 4096 * 4096 + 100_000, [5_000_000, 1_000_000, 70_000], [0.0, 2.0, 20.0, 200.0]),
    "256 x 2048^2 gray (C4)": (2048, 2048, 1, 4, 16, 256, 2 * 2048 * 2048 + 100_000, [1_000_000, 300_000, 70_000], [0.0, 2.0, 20.0, 200.0]),
}


def run_case(torch, name, reps, warmup):
    from icer_compression_amd import api
    w, h, C, stages, segs, n, cap, lower, targets = CASES[name]
    dev = torch.device("cuda", 0)
    enc = api.Encoder(w, h, C, stages, 0, segs, max_frames=n)
    t = frames_for(torch, dev, w, h, C, n)
    quotas = [cap] + lower
    Q = len(quotas)
    stride = cap
    out = torch.empty((Q * n, stride), dtype=torch.uint8, device=dev)
    sizes, dist, equiv = (torch.empty(Q * n, dtype=torch.int64, device=dev) for _ in range(3))
    rcs, reached = (torch.empty(Q * n, dtype=torch.int32, device=dev) for _ in range(2))
    st = torch.cuda.current_stream(dev).cuda_stream

    def ladder():
        enc.encode_ladder_ptrs(t.data_ptr(), n, quotas, out.data_ptr(), stride, sizes.data_ptr(), rcs.data_ptr(), st)

    def single():
        enc.encode_device_ptrs(t.data_ptr(), n, cap, out.data_ptr(), stride, sizes.data_ptr(), rcs.data_ptr(), st)

    def target():
        enc.encode_target_ptrs(t.data_ptr(), n, targets, cap, out.data_ptr(), stride, sizes.data_ptr(), rcs.data_ptr(), reached.data_ptr(),
                               dist.data_ptr(), equiv.data_ptr(), st)

    t_single = timed(torch, single, reps, warmup)
    t_ladder = timed(torch, ladder, reps, warmup)
    if not hasattr(enc.lib, "icerx_encode_device_target"):
        print(f"| {name} | - | {t_ladder:.3f} | {t_single:.3f} | - | (this build has no target call) |", flush=True)
        enc.close()
        return
    t_target = timed(torch, target, reps, warmup)
    torch.cuda.synchronize()
    sz = sizes.cpu().numpy().reshape(Q, n)[:, 0]
    psnr = [10 * np.log10(65535.0 ** 2 / max(d / 16.0 / (w * h * C), 1e-12)) for d in dist.cpu().numpy().view(np.uint64).reshape(Q, n)[:, 0]]
    print(f"| {name} | {t_target:.3f} | {t_ladder:.3f} | {t_single:.3f} | {t_target / t_ladder:.3f} | frame 0: "
          f"{', '.join(f'MSE {m:g}: {int(s)} B, {p:.1f} dB' for m, s, p in zip(targets, sz, psnr))} |", flush=True)
    enc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--case", action="append", choices=list(CASES))
    args = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")                       # (torch's HIP runtime first, as bench.py does)
    print("| case | target call, 4 targets ms | ladder, 4 quotas ms | single call at the cap ms | target / ladder | "
          "stream bytes and estimated PSNR per target |")
    print("|---|---|---|---|---|---|")
    for name in args.case or list(CASES):
        run_case(torch, name, args.reps, args.warmup)


if __name__ == "__main__":
    main()
