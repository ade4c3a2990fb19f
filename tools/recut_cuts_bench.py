"""Cutting a stored master by resolution as well as by byte quota (icerx_recut_device_cuts_async, include/icer_hip_dec.h)
against the byte-quota re-cut and against what the same streams cost without it.

The master is profiles/recut.md's: the lone 4096 x 4096 gray frame of tools/ladder_bench.py (5 stages, filter A, 10 segments)
encoded once at the lossless quota, resident in HBM.  Per part: `--warmup` untimed calls, then `--reps` timed ones between two
device events on one stream; median, minimum and maximum are reported (spread = max - min).  The parts:
  recut          icerx_recut_device_async at the four quotas of profiles/recut.md
  cuts r=0       icerx_recut_device_cuts_async, four cuts (0, quota) at the same quotas: must give the same rows
  pyramid        one call with the cuts (0, Q), (1, Q / 4), (2, Q / 16), (3, Q / 64), Q the lossless quota
  r alone        one call with the single cut (r, Q), r = 0 .. 3
  decode+encode  what a stream at 1/2^r size costs without the cut: the reduced decode at r (Decoder(reduce=r).decode_torch)
                 and an encode of its planes at the reduced geometry with stages - r (Encoder.encode_torch), timed apart
Every cut at r >= 1 with the generous quota is checked against tests/reduced_model.derive of the master, byte for byte.  A
library without the cuts (an earlier build) runs `recut` alone.  One JSON line.

    python tools/recut_cuts_bench.py [--reps N] [--warmup W]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

W = H = 4096
STAGES, FILT, SEGMENTS = 5, 0, 10
QUOTAS = [2 * W * H + 100_000, 5_000_000, 1_000_000, 70_000]
MAX_REDUCE = 3


def timed(torch, fn, reps, warmup):
    """milliseconds of fn() between two events on the current stream: median, min, max over `reps` calls"""
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
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")                       # (torch's HIP runtime first, as bench.py does)
    from icer_compression_amd import api, decoder
    from ladder_bench import frames_for
    dev = torch.device("cuda", 0)
    top = QUOTAS[0]
    enc = api.Encoder(W, H, 1, STAGES, FILT, SEGMENTS, max_frames=1)
    t = frames_for(torch, dev, W, H, 1, 1)
    master = torch.empty((1, top), dtype=torch.uint8, device=dev)
    lens, mrc = torch.empty(1, dtype=torch.int64, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    enc.encode_torch(t, top, master, lens, mrc)
    torch.cuda.synchronize()
    assert int(mrc[0]) == 0, "the master is not complete"
    blob = master[0, : int(lens[0])].clone()
    offsets = torch.zeros(1, dtype=torch.int64, device=dev)
    enc.close()
    have_cuts = hasattr(decoder.load_library(), "icerx_recut_device_cuts_async")
    rec = decoder.Recutter(W, H, 1, STAGES, SEGMENTS, max_reduce=MAX_REDUCE) if have_cuts else decoder.Recutter(W, H, 1, STAGES, SEGMENTS)

    def rows(Q):
        return (torch.zeros((Q, 1, top), dtype=torch.uint8, device=dev), torch.zeros((Q, 1), dtype=torch.int64, device=dev),
                torch.full((Q, 1), 77, dtype=torch.int32, device=dev))

    res = {"master_bytes": int(blob.numel())}
    out, sz, rc = rows(len(QUOTAS))
    res["recut"] = timed(torch, lambda: rec.recut_torch(blob, lens, QUOTAS, out, sz, rc, offsets=offsets), args.reps, args.warmup)
    res["recut"]["sizes"] = sz[:, 0].tolist()
    ok = True
    if have_cuts:
        from tests import reduced_model as rm
        host = blob.cpu().numpy().tobytes()
        out0, sz0, rc0 = rows(len(QUOTAS))
        cuts0 = [(0, q) for q in QUOTAS]
        res["cuts_r0"] = timed(torch, lambda: rec.recut_cuts_torch(blob, lens, cuts0, out0, sz0, rc0, offsets=offsets), args.reps, args.warmup)
        ok = ok and torch.equal(sz0, sz) and torch.equal(rc0, rc) and all(torch.equal(out0[q, 0, : int(sz[q, 0])], out[q, 0, : int(sz[q, 0])])
                                                                         for q in range(len(QUOTAS)))
        pyramid = [(r, top >> (2 * r)) for r in range(MAX_REDUCE + 1)]
        outp, szp, rcp = rows(len(pyramid))
        res["pyramid"] = timed(torch, lambda: rec.recut_cuts_torch(blob, lens, pyramid, outp, szp, rcp, offsets=offsets), args.reps, args.warmup)
        res["pyramid"].update({"cuts": pyramid, "sizes": szp[:, 0].tolist(), "rcs": rcp[:, 0].tolist()})
        res["alone"], res["decode_encode"] = [], []
        for r in range(MAX_REDUCE + 1):
            out1, sz1, rc1 = rows(1)
            one = timed(torch, lambda: rec.recut_cuts_torch(blob, lens, [(r, top)], out1, sz1, rc1, offsets=offsets), args.reps, args.warmup)
            want = rm.derive(host, r)
            exact = int(rc1[0, 0]) == 0 and out1[0, 0, : int(sz1[0, 0])].cpu().numpy().tobytes() == want
            ok = ok and exact
            one.update({"reduce": r, "bytes": int(sz1[0, 0]), "equals_derived_stream": bool(exact)})
            res["alone"].append(one)
            # the same stream without the cut: reduced decode, then an encode at the reduced geometry
            rw, rh = decoder.reduced_size(W, H, r)
            dec = decoder.Decoder(1, STAGES, FILT, SEGMENTS, reduce=r)
            planes = torch.zeros((1, 1, rw * rh), dtype=torch.int16, device=dev)
            drc = torch.full((1,), 77, dtype=torch.int32, device=dev)
            ws, hs = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
            t_dec = timed(torch, lambda: dec.decode_torch(blob, lens, planes, drc, ws, hs, offsets=offsets), args.reps, args.warmup)
            enc_r = api.Encoder(rw, rh, 1, STAGES - r, FILT, SEGMENTS, max_frames=1)
            frames = planes.view(1, rh, rw)
            eout = torch.zeros((1, top), dtype=torch.uint8, device=dev)
            esz, erc = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
            t_enc = timed(torch, lambda: enc_r.encode_torch(frames, top, eout, esz, erc), args.reps, args.warmup)
            same = int(drc[0]) == 0 and int(erc[0]) == 0 and eout[0, : int(esz[0])].cpu().numpy().tobytes() == want
            res["decode_encode"].append({"reduce": r, "decode": t_dec, "encode": t_enc, "bytes": int(esz[0]), "equals_the_cut": bool(same)})
            dec.close()
            enc_r.close()
    rec.close()
    res["parity"] = bool(ok)
    print(json.dumps({"metric": "ms per call, cuts of one stored 4096x4096 gray master", "unit": "ms", "higher_is_better": False,
                      "config": {"warmup": args.warmup, "quotas": QUOTAS}, **res}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
