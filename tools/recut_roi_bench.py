"""Cutting stored masters by (resolution, byte quota, ROI shift) (icerx_recut_device_roi_async, include/icer_hip_dec.h) beside
the two calls it stands next to.

The master sets are those of profiles/recut_cuts.md and profiles/budget.md: one lossless 4096 x 4096 gray master (5 stages,
10 segments) and 64 lossless 2048 x 2048 gray masters (the C4 shape: 4 stages, 16 segments), resident in HBM as the encoder left
them.  Every frame's rectangle is an eighth of the frame's sides at (w / 8, h / 8), as in tools/roi_bench.py.  Per case a
four-cut call and a sixteen-cut call, reduces 0 .. 3, shifts 3 and 0 side by side.  Timed with device events on one stream
after a warm-up, the three calls in turns so that all see the same drift; median, minimum and maximum (spread = max - min):
  roi       icerx_recut_device_roi_async with the cuts (r, Q, shift)
  cuts      icerx_recut_device_cuts_async with the same (r, Q) on the same masters: existing code, the baseline
  encode    icerx_encode_device_roi on the original frames at the distinct quotas of the call, shift 3: the call the re-cut
            replaces for stored data (reduce 0 only: it has no other)
Before timing, every shift-0 cut is checked against the cuts call's row, and every (0, Q, 3) cut against the ROI encode's.
Prints a markdown table (profiles/recut_roi.md).  --calls K: no timing, K calls of the new call alone (for a kernel trace).

    python tools/recut_roi_bench.py [--reps N] [--warmup W] [--case NAME ...] [--calls K]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {
    # name: (w, h, stages, segments, frames, quotas Q0 > Q1 > Q2 > Q3)
    "lone 4096^2 gray": (4096, 4096, 5, 10, 1, [5_000_000, 1_000_000, 300_000, 70_000]),
    "64 x 2048^2 gray (C4)": (2048, 2048, 4, 16, 64, [1_000_000, 300_000, 100_000, 40_000]),
}
MAX_REDUCE, SHIFT = 3, 3


def cut_sets(q):
    four = [(0, q[1], SHIFT), (0, q[1], 0), (1, q[2], SHIFT), (2, q[3], SHIFT)]
    sixteen = [(r, q[min(3, r + k)], s) for r in range(MAX_REDUCE + 1) for k, s in ((0, SHIFT), (0, 0), (1, SHIFT), (2, 9))]
    return {"4 cuts": four, "16 cuts": sixteen}


def one_ms(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stat(ms):
    return f"{float(np.median(ms)):.3f} ({min(ms):.3f} .. {max(ms):.3f})"


def run_case(torch, name, reps, warmup, calls):
    from icer_compression_amd import api, decoder, synth
    w, h, stages, segs, n, quotas = CASES[name]
    dev = torch.device("cuda", 0)
    top = 2 * w * h + 100_000
    enc = api.Encoder(w, h, 1, stages, 0, segs, max_frames=n)
    t = synth.gray_frames_torch(n, w, h, synth.DEFAULT_SEED, dev)
    masters = torch.empty((n, top), dtype=torch.uint8, device=dev)
    lens, mrc = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    enc.encode_torch(t, top, masters, lens, mrc)
    torch.cuda.synchronize()
    assert mrc.tolist() == [0] * n, "a master is not complete"
    rois = torch.tensor([[w // 8, h // 8, w // 8, h // 8]] * n, dtype=torch.int32, device=dev)
    rec = decoder.Recutter(w, h, 1, stages, segs, max_reduce=MAX_REDUCE)
    for label, cuts in cut_sets(quotas).items():
        Q, stride = len(cuts), max(c[1] for c in cuts)
        out, base = (torch.zeros((Q, n, stride), dtype=torch.uint8, device=dev) for _ in range(2))
        sz, bsz = (torch.zeros((Q, n), dtype=torch.int64, device=dev) for _ in range(2))
        rc, brc, kept, fg = (torch.zeros((Q, n), dtype=torch.int32, device=dev) for _ in range(4))
        enc_quotas = sorted({c[1] for c in cuts if c[0] == 0}, reverse=True)

        def roi():
            rec.recut_roi_torch(masters, lens, rois, cuts, out, sz, rc, kept, fg)

        def plain():
            rec.recut_cuts_torch(masters, lens, [(c[0], c[1]) for c in cuts], base, bsz, brc)

        def encode():
            return enc.encode_roi_torch(t, rois, SHIFT, enc_quotas)

        if calls:
            for _ in range(calls):
                roi()
            torch.cuda.synchronize()
            continue
        # the checks: shift 0 is the cuts call; (0, Q, 3) is the ROI encode of the frame
        roi()
        plain()
        eout, esz, erc, ekept, efg = encode()
        torch.cuda.synchronize()
        exact = 0
        for c, (r, q, s) in enumerate(cuts):
            if s == 0:
                assert torch.equal(sz[c], bsz[c]) and torch.equal(rc[c], brc[c]) and torch.equal(out[c], base[c]), (name, label, cuts[c])
                exact += n
            elif r == 0 and s == SHIFT:
                e = enc_quotas.index(q)
                assert torch.equal(sz[c], esz[e]) and torch.equal(rc[c], erc[e]) and torch.equal(kept[c], ekept[e]) and \
                    torch.equal(fg[c], efg), (name, label, cuts[c])
                assert all(torch.equal(out[c, f, : int(sz[c, f])], eout[e, f, : int(sz[c, f])]) for f in range(n)), (name, label, cuts[c])
                exact += n
        del eout
        for _ in range(warmup):
            roi()
            plain()
            encode()
        torch.cuda.synchronize()
        ms = {"roi": [], "cuts": [], "encode": []}
        for _ in range(reps):
            ms["cuts"].append(one_ms(torch, plain))
            ms["roi"].append(one_ms(torch, roi))
            ms["encode"].append(one_ms(torch, encode))
        m = {k: float(np.median(v)) for k, v in ms.items()}
        print(f"| {name} | {label}: {', '.join(f'({r}, {q}, {s})' for r, q, s in cuts)} | {stat(ms['roi'])} | {stat(ms['cuts'])} | "
              f"{m['roi'] - m['cuts']:+.3f} | {m['roi'] / m['cuts']:.3f} | {stat(ms['encode'])} ({len(enc_quotas)} quotas) | "
              f"{m['roi'] / m['encode']:.4f} | {exact} streams exact; frame 0: {int(fg[0, 0])} foreground units, "
              f"K {', '.join(str(int(k)) for k in kept[:, 0].tolist())} |", flush=True)
    rec.close()
    enc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--case", action="append", choices=list(CASES))
    ap.add_argument("--calls", type=int, default=0)
    args = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")                       # (torch's HIP runtime first, as bench.py does)
    if not args.calls:
        print("| masters | cuts (reduce, quota, shift) | roi ms: median (min .. max) | cuts ms: median (min .. max) | roi - cuts ms | roi / cuts | "
              "ROI encode ms: median (min .. max) | roi / encode | checks; the ROI cuts |")
        print("|---|---|---|---|---|---|---|---|---|")
    for name in args.case or list(CASES):
        run_case(torch, name, args.reps, args.warmup, args.calls)


if __name__ == "__main__":
    main()
