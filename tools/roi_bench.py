"""Region-of-interest encode beside the rate ladder (icerx_encode_device_roi / icerx_encode_device_ladder, include/icer_hip.h).

For each case and quota set, with device events on one stream and after a warm-up: the ladder call and the ROI call (a
rectangle of an eighth of the frame's sides at (w / 8, h / 8) in every frame, shift 3) on the same frames at the same quotas,
timed in turns so that both see the same drift.  Three quota sets per case: one whose largest quota is at or above the
progressive threshold (w * h * channels / 2 bytes: both calls run the same coder launches), one below it and one far below it
(the ladder call runs in progressive mode and stops coding once the quota is spent, the ROI call codes every unit).  Before
timing, the ROI call at shift 0 is checked against the ladder call (bytes, sizes, return codes).  Prints a markdown table
(profiles/roi.md).

    python tools/roi_bench.py [--reps N] [--warmup W] [--case NAME ...]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {
    # name: (w, h, channels, stages, segments, frames, {quota set: quotas})
    "lone 4096^2 gray": (4096, 4096, 1, 5, 10, 1, {"at or above the threshold": [2 * 4096 * 4096 + 100_000, 5_000_000, 1_000_000],
                                                    "below the threshold": [5_000_000, 1_000_000, 70_000],
                                                    "far below the threshold": [140_000, 100_000, 70_000]}),
    "8 x 2048^2 gray (C4 shape)": (2048, 2048, 1, 4, 16, 8, {"at or above the threshold": [2 * 2048 * 2048 + 100_000, 1_000_000, 300_000],
                                                              "below the threshold": [1_000_000, 300_000, 70_000],
                                                              "far below the threshold": [100_000, 70_000, 40_000]}),
}
SHIFT = 3


def one_ms(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def run_case(torch, name, reps, warmup):
    from icer_compression_amd import api, synth
    w, h, C, stages, segs, n, sets = CASES[name]
    dev = torch.device("cuda", 0)
    enc = api.Encoder(w, h, C, stages, 0, segs, max_frames=n)
    t = synth.gray_frames_torch(n, w, h, synth.DEFAULT_SEED, dev)
    rois = torch.tensor([[w // 8, h // 8, w // 8, h // 8]] * n, dtype=torch.int32, device=dev)
    for label, quotas in sets.items():
        Q, top = len(quotas), max(quotas)
        lad = torch.empty((Q, n, top), dtype=torch.uint8, device=dev)
        lsz, lrc = torch.empty((Q, n), dtype=torch.int64, device=dev), torch.empty((Q, n), dtype=torch.int32, device=dev)

        def ladder():
            enc.encode_ladder_torch(t, quotas, lad, lsz, lrc)

        def roi(shift=SHIFT):
            return enc.encode_roi_torch(t, rois, shift, quotas)

        # the check: shift 0 is the ladder
        ladder()
        out, sizes, rcs, _, _ = roi(0)
        torch.cuda.synchronize()
        assert torch.equal(lsz, sizes) and torch.equal(lrc, rcs), (name, label, lsz.tolist(), sizes.tolist())
        for q in range(Q):
            for f in range(n):
                s = int(lsz[q, f])
                assert torch.equal(lad[q, f, :s], out[q, f, :s]), (name, label, q, f)
        del out
        for _ in range(warmup):
            ladder()
            roi()
        torch.cuda.synchronize()
        ms = {"ladder": [], "roi": []}
        for _ in range(reps):
            ms["ladder"].append(one_ms(torch, ladder))
            launch_ladder = enc.launch_info()
            ms["roi"].append(one_ms(torch, roi))
            launch_roi = enc.launch_info()
        kind = lambda li: "split" if li["split"] else "window" if li["pipeline_waves"] == 0 else "pipeline"
        _, sizes, _, kept, fg = roi()
        torch.cuda.synchronize()
        ml, mr = float(np.median(ms["ladder"])), float(np.median(ms["roi"]))
        print(f"| {name} | {label}: {', '.join(str(q) for q in quotas)} | {ml:.3f} ({min(ms['ladder']):.3f} .. {max(ms['ladder']):.3f}) | "
              f"{mr:.3f} ({min(ms['roi']):.3f} .. {max(ms['roi']):.3f}) | {mr - ml:+.3f} | {mr / ml:.3f} | {kind(launch_ladder)} / {kind(launch_roi)} | "
              f"{Q * n} streams exact at shift 0; frame 0 at shift {SHIFT}: {int(fg[0])} foreground units of {enc.info()['units_per_frame']}, "
              f"K {', '.join(str(int(k)) for k in kept[:, 0].tolist())}, bytes {', '.join(str(int(s)) for s in sizes[:, 0].tolist())} |", flush=True)
    enc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--case", action="append", choices=list(CASES))
    args = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")                       # (torch's HIP runtime first, as bench.py does)
    print("| case | quotas | ladder ms: median (min .. max) | ROI ms: median (min .. max) | ROI - ladder ms | ROI / ladder | "
          "launch: ladder / ROI | check; the ROI streams |")
    print("|---|---|---|---|---|---|---|---|")
    for name in args.case or list(CASES):
        run_case(torch, name, args.reps, args.warmup)


if __name__ == "__main__":
    main()
