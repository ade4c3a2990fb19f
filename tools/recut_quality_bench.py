"""Re-cutting stored masters to distortion targets and to shared byte budgets (icerx_recut_device_target_async /
icerx_recut_device_budget_async, include/icer_hip_dec_quality.h) against what they replace and against their floor.

64 C4 frames (2048^2 gray, 4 stages, 16 segments) are encoded once at the lossless quota (the stored masters, in rows as the
encoder leaves them) and a target call at target 0 gives their distortion sidecars.  Then, for four targets and for four
budgets, with device events on one stream, after a warm-up, in the same run:
  re-cut     the new call on masters and sidecars
  encode     icerx_encode_device_target / _budget on the source frames with the same targets / budgets and cap
  quota      icerx_recut_device_async on the masters at four of the equivalent quotas the new call reported -- about the same
             bytes written, by the call that needs no sidecar: the floor
Every re-cut output is checked against the encoder's (streams, sizes, return codes, reached / at_cap, distortions, equivalent
quotas, thresholds, totals).  Each figure is the median of --reps calls, given with the spread (max - min) over --runs repeats
of the whole measurement.  Prints a markdown table (profiles/recut_quality.md).

    python tools/recut_quality_bench.py [--reps N] [--warmup W] [--runs R] [--frames F] [--once target|budget]

--once: calls of that kind only, and nothing after the last one, for tools/kernel_timeline.sh:
    TL_SCRIPT=tools/recut_quality_bench.py TL_FIRST=mark_headers_kernel TL_LAST=recut_gather_kernel tools/kernel_timeline.sh out.txt --once target
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

W, H, C, STAGES, FILT, SEGS = 2048, 2048, 1, 4, 0, 16
CAP = 2 * W * H + 100_000
TARGETS = [5.0, 20.0, 80.0, 320.0]                  # mean squared errors
BUDGET_BYTES_PER_FRAME = [1_000_000, 300_000, 100_000, 30_000]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--once", choices=["target", "budget"])
    args = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")                       # (torch's HIP runtime first, as bench.py does)
    from icer_compression_amd import api, decoder
    from ladder_bench import frames_for, timed
    n, dev = args.frames, torch.device("cuda", 0)
    enc = api.Encoder(W, H, C, STAGES, FILT, SEGS, max_frames=n)
    rec = decoder.Recutter(W, H, C, STAGES, SEGS, filt=FILT)
    t = frames_for(torch, dev, W, H, C, n)
    budgets = [b * n for b in BUDGET_BYTES_PER_FRAME]
    Q = len(TARGETS)

    # the stored masters and their sidecars
    enc.encode_target_torch(t, [0.0], CAP)
    side = enc.distortion_sidecar_torch(n)
    masters = torch.empty((n, CAP), dtype=torch.uint8, device=dev)
    lens, mrc = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    enc.encode_torch(t, CAP, masters, lens, mrc)
    torch.cuda.synchronize()
    assert all(int(x) == 0 for x in mrc.tolist()), "the masters are not complete"

    out = torch.empty((Q, n, CAP), dtype=torch.uint8, device=dev)
    sizes, dist, equiv = (torch.empty((Q, n), dtype=torch.int64, device=dev) for _ in range(3))
    rcs, flag = (torch.empty((Q, n), dtype=torch.int32, device=dev) for _ in range(2))
    thr, tot = (torch.empty(Q, dtype=torch.int64, device=dev) for _ in range(2))

    def recut_target():
        rec.recut_target_torch(masters, lens, side, [(0, x) for x in TARGETS], CAP, out, sizes, rcs, flag, dist, equiv)

    def recut_budget():
        rec.recut_budget_torch(masters, lens, side, budgets, CAP, out, sizes, rcs, flag, dist, equiv, thr, tot)

    if args.once:
        fn = recut_target if args.once == "target" else recut_budget
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        return

    def check(got, want, what):
        for k, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a.reshape(b.shape), b), f"{what}: output {k} differs from the encoder's"

    def streams_equal(want_out, want_sizes):
        return all(torch.equal(out[q, f, :int(want_sizes[q, f])], want_out[q, f, :int(want_sizes[q, f])]) for q in range(Q) for f in range(n))

    rows = []
    for kind, fn, encode in (("4 targets", recut_target, lambda: enc.encode_target_torch(t, TARGETS, CAP)),
                             ("4 budgets", recut_budget, lambda: enc.encode_budget_torch(t, budgets, CAP))):
        fn()
        want = encode()
        torch.cuda.synchronize()
        check((sizes, rcs, flag, dist, equiv) + ((thr, tot) if kind == "4 budgets" else ()), want[1:], kind)
        assert streams_equal(want[0], want[1]), f"{kind}: a stream differs from the encoder's"
        written = int(sizes.sum())
        # the floor: the byte-quota re-cut at four of the equivalent quotas (the median frame's, one per cut)
        quotas = [int(equiv[q].sort().values[n // 2]) for q in range(Q)]
        qout = torch.empty((Q, n, max(quotas)), dtype=torch.uint8, device=dev)
        qsz, qrc = torch.empty((Q, n), dtype=torch.int64, device=dev), torch.empty((Q, n), dtype=torch.int32, device=dev)

        def quota():
            rec.recut_torch(masters, lens, quotas, qout, qsz, qrc)

        quota()
        torch.cuda.synchronize()
        qwritten = int(qsz.sum())
        ms = {"re-cut": [], "encode": [], "quota": []}
        for _ in range(args.runs):
            ms["re-cut"].append(timed(torch, fn, args.reps, args.warmup))
            ms["encode"].append(timed(torch, encode, args.reps, args.warmup))
            ms["quota"].append(timed(torch, quota, args.reps, args.warmup))
        rows.append((kind, written, qwritten, ms))
    print(f"| {n} C4 frames | bytes written | re-cut ms (spread) | encode from pixels ms (spread) | byte-quota re-cut ms (spread), bytes | "
          "re-cut / encode | re-cut / byte-quota |")
    print("|---|---|---|---|---|---|---|")
    for kind, written, qwritten, ms in rows:
        med = {k: float(np.median(v)) for k, v in ms.items()}
        sp = {k: max(v) - min(v) for k, v in ms.items()}
        print(f"| {kind} | {written} | {med['re-cut']:.3f} ({sp['re-cut']:.3f}) | {med['encode']:.3f} ({sp['encode']:.3f}) | "
              f"{med['quota']:.3f} ({sp['quota']:.3f}), {qwritten} | {med['re-cut'] / med['encode']:.4f} | {med['re-cut'] / med['quota']:.2f} |", flush=True)
    enc.close()
    rec.close()


if __name__ == "__main__":
    main()
