"""Refinement increments against the re-cut they top up (icerx_combine_device_async, include/icer_hip_dec.h).

64 lossless 4096^2 gray masters (5 stages, 10 segments) are encoded once and packed into one blob.  One icerx_recut_device_async
call cuts them to a held and a wanted quota side by side; then, with device events on one stream and after a warm-up, median of
the repetitions:
  difference   icerx_combine_device_async DIFFERENCE straight on that call's output block (what the server sends)
  union        icerx_combine_device_async UNION on the same block (the wanted cut again, from its parts)
  re-cut       icerx_recut_device_async of the masters to the wanted quota alone: the yardstick (profiles/recut.md)
  re-cut x 2   the call that made the block, both quotas
Every union is checked against the wanted cut and every increment's size against the difference of the two cuts' sizes.  Prints a
markdown table (profiles/combine.md).

    python tools/combine_bench.py [--frames N] [--reps N] [--warmup W]
"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

W = H = 4096
STAGES, SEGMENTS = 5, 10
LOSSLESS, HELD, WANTED = 2 * W * H + 100_000, 1_000_000, 5_000_000
CHUNK = 8                                            # frames encoded per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")                       # (torch's HIP runtime first, as bench.py does)
    from icer_compression_amd import api, decoder, synth
    from ladder_bench import timed
    dev = torch.device("cuda", 0)
    n = args.frames
    enc = api.Encoder(W, H, 1, STAGES, 0, SEGMENTS, max_frames=CHUNK)
    rec = decoder.Recutter(W, H, 1, STAGES, SEGMENTS)
    # the stored masters: the lossless streams one after another in one blob (different frames: a seed per chunk)
    parts, lens = [], []
    for at in range(0, n, CHUNK):
        k = min(CHUNK, n - at)
        t = synth.gray_frames_torch(k, W, H, synth.DEFAULT_SEED + at, dev)
        lad, lsz, lrc = enc.encode_ladder_torch(t, [LOSSLESS])
        torch.cuda.synchronize()
        assert all(int(x) == 0 for x in lrc[0].tolist()), "a master is not lossless"
        parts += [lad[0, f, : int(lsz[0, f])].clone() for f in range(k)]
        lens += [int(x) for x in lsz[0].tolist()]
        del t, lad
    enc.close()
    blob = torch.cat(parts).contiguous()
    del parts
    lens = torch.tensor(lens, dtype=torch.int64, device=dev)
    offsets = torch.cumsum(lens, 0) - lens
    stride = WANTED
    block = torch.zeros((2, n, stride), dtype=torch.uint8, device=dev)
    bsz, brc = torch.zeros((2, n), dtype=torch.int64, device=dev), torch.zeros((2, n), dtype=torch.int32, device=dev)
    one = torch.zeros((1, n, stride), dtype=torch.uint8, device=dev)
    osz, orc = torch.zeros((1, n), dtype=torch.int64, device=dev), torch.zeros((1, n), dtype=torch.int32, device=dev)
    out = torch.zeros((n, stride), dtype=torch.uint8, device=dev)
    sizes, rcs = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    counts = torch.zeros((n, 2), dtype=torch.int32, device=dev)

    def recut_two():
        rec.recut_torch(blob, lens, [HELD, WANTED], block, bsz, brc, offsets=offsets)

    def recut_one():
        rec.recut_torch(blob, lens, [WANTED], one, osz, orc, offsets=offsets)

    def combine(op):
        rec.combine_torch(block, op, bsz[0], bsz[1], out, sizes, rcs, counts, base_b=n * stride, stream_stride=stride)

    t_two = timed(torch, recut_two, args.reps, args.warmup)
    t_one = timed(torch, recut_one, args.reps, args.warmup)
    t_diff = timed(torch, lambda: combine(decoder.COMBINE_DIFFERENCE), args.reps, args.warmup)
    torch.cuda.synchronize()
    assert rcs.tolist() == [0] * n and torch.equal(sizes, bsz[1] - bsz[0]), "an increment is not the difference of the two cuts"
    inc_bytes, inc_packets = int(sizes.sum()), int(counts[:, 0].sum())
    t_union = timed(torch, lambda: combine(decoder.COMBINE_UNION), args.reps, args.warmup)
    torch.cuda.synchronize()
    assert rcs.tolist() == [0] * n and torch.equal(sizes, bsz[1]), "a union is not as long as the wanted cut"
    assert all(torch.equal(out[f, : int(sizes[f])], block[1, f, : int(sizes[f])]) for f in range(n)), "a union is not the wanted cut"
    print("| masters | master bytes | block bytes (the combine's blob) | held bytes | wanted bytes | increment bytes (packets) | "
          "difference ms | union ms | re-cut to the wanted quota ms | re-cut to both ms | difference / re-cut | union / re-cut |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    print(f"| {n} x {W}^2 gray | {blob.numel()} | {block.numel()} | {int(bsz[0].sum())} | {int(bsz[1].sum())} | {inc_bytes} ({inc_packets}) | "
          f"{t_diff:.3f} | {t_union:.3f} | {t_one:.3f} | {t_two:.3f} | {t_diff / t_one:.2f} | {t_union / t_one:.2f} |", flush=True)
    rec.close()


if __name__ == "__main__":
    main()
