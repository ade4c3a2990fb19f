#!/usr/bin/env python3
"""Reduced-resolution decode benchmark of libicer_hip_dec.so (include/icer_hip_dec.h, "Decoding at 1/2^r resolution") -- NOT
bench.py's metric.

    python tools/decode_reduced_bench.py [--batch 64] [--reps 9] [--batch-reps 5] [--warmup 2] [--no-check]

Workload: tools/decode_bench.py's -- the stream the HIP encoder makes of the BASELINE configs[1] frame (4096 x 4096 gray, 5
stages, filter A, 10 segments, lossless: the reference golden, checked), resident in HBM, decoded to uint16 planes that stay
in HBM -- alone and `--batch` times per call, in ONE process, through
    plain    icerx_decoder_create                      (the yardstick: tools/decode_bench.py's call)
    r = 0    icerx_decoder_create_reduced, reduce 0    (the same kernels on the same chains: must agree with `plain`)
    r = 1..3 icerx_decoder_create_reduced              (no chain of level <= r is started)
each through the synchronous call (icerx_decode_device, planned on the host) and the asynchronous one
(icerx_decode_device_async via Decoder.decode_torch, planned on the device).  Per configuration: `--warmup` untimed calls, then
`--reps` timed ones (wall clock around call + synchronise); median, minimum and maximum are reported, the spread is max - min.
Unless --no-check, every configuration's lone-stream image is compared with the decoder oracle's decode of the derived stream
(tests/reduced_model.py) -- for r = 0 with the encoder's input.  One JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W = H = 4096
STAGES, FILT, SEGMENTS = 5, 0, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--batch-reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-reduce", type=int, default=3)
    ap.add_argument("--no-check", action="store_true")
    a = ap.parse_args()
    import torch
    from icer_compression_amd import api, decoder, synth
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)                                   # torch's HIP runtime first (see tests/conftest.py)
    img = synth.gray_frame(W, H, 12345, 1)
    rc, stream, _ = api.compress([img], STAGES, FILT, SEGMENTS, 2 * W * H)
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "golden.json")))["C2_4096_gray_5st_10seg"]
    assert rc == 0 and len(stream) == gold["size"] and "%08x" % zlib.crc32(stream) == gold["crc32"], "encoder stream is not the golden"

    want = {}
    if not a.no_check:
        from oracle.binding import Oracle
        from tests import reduced_model as rm
        orc = Oracle()
        want[0] = img.reshape(-1)
        for r in range(1, a.max_reduce + 1):
            rw, rh = rm.reduced_size(W, H, r)
            rc_, w_, h_, planes = orc.decompress(rm.derive(stream, r), 1, STAGES - r, FILT, SEGMENTS, bufsize=rw * rh)
            assert (rc_, w_, h_) == (0, rw, rh)
            want[r] = planes[0][: rw * rh]

    def timed(call, warmup, reps):
        for _ in range(warmup):
            call()
            torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            call()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t) * 1e3)
        return {"median_ms": round(statistics.median(times), 3), "min_ms": round(min(times), 3), "max_ms": round(max(times), 3), "reps": reps}

    def run(n, reps, r, plain):
        rw, rh = decoder.reduced_size(W, H, r)
        stride = rw * rh
        d_data = torch.from_numpy(np.frombuffer(stream * n, dtype=np.uint8).copy()).to(dev)
        d_out = torch.zeros((n, stride), dtype=torch.int16, device=dev)
        dec = decoder.Decoder(1, STAGES, FILT, SEGMENTS)
        if not plain:                                            # (the new constructor for every r, 0 included)
            import ctypes as C
            dec.close()
            rc_ = dec.lib.icerx_decoder_create_reduced(C.byref(dec.handle), -1, 1, STAGES, FILT, SEGMENTS, 16, r)
            assert rc_ == 0 and dec.lib.icerx_decoder_reduce(dec.handle) == r
            dec.reduce = r
        offs, lens = [k * len(stream) for k in range(n)], [len(stream)] * n
        state = {}

        def sync():
            state["sync"] = dec.decode_device(n, d_data.data_ptr(), offs, lens, d_out.data_ptr(), stride)
        res = {"sync": timed(sync, a.warmup, reps)}
        rc2, rcs, ws, hs = state["sync"]
        ok = rc2 == 0 and all(x == 0 for x in rcs) and set(ws) == {rw} and set(hs) == {rh}
        t_lens = torch.tensor(lens, dtype=torch.int64, device=dev)
        t_offs = torch.tensor(offs, dtype=torch.int64, device=dev)
        t_rcs = torch.full((n,), 77, dtype=torch.int32, device=dev)
        t_ws, t_hs = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
        first = d_out[0].clone()
        d_out.zero_()

        def asyn():
            dec.decode_torch(d_data, t_lens, d_out, t_rcs, t_ws, t_hs, offsets=t_offs)
        res["async"] = timed(asyn, a.warmup, reps)
        ok = ok and t_rcs.cpu().tolist() == [0] * n and t_ws.cpu().tolist() == [rw] * n and t_hs.cpu().tolist() == [rh] * n
        ok = ok and all(bool(torch.equal(d_out[k], first)) for k in range(n))
        if r in want:
            ok = ok and np.array_equal(first.cpu().numpy().view(np.uint16), want[r])
        dec.close()
        res.update({"reduce": r, "constructor": "icerx_decoder_create" if plain else "icerx_decoder_create_reduced", "w": rw, "h": rh,
                    "parity": bool(ok), "checked_against_oracle": r in want})
        return res

    rows = {"lone": [], "batch": []}
    for name, n, reps in (("lone", 1, a.reps), ("batch", a.batch, a.batch_reps)):
        if n < 1:
            continue
        rows[name].append(run(n, reps, 0, True))
        for r in range(0, a.max_reduce + 1):
            rows[name].append(run(n, reps, r, False))
    ok = all(x["parity"] for v in rows.values() for x in v)
    line = {"metric": "ms per call, reduced-resolution decode, 4096x4096 gray", "unit": "ms", "higher_is_better": False,
            "config": {"workload": "stream of BASELINE configs[1] (4096x4096 gray, 5 stages, filter A, 10 segments, lossless, 9 948 227 bytes) "
                                   "resident in HBM -> uint16 planes of ceil(4096 / 2^r)^2 samples in HBM",
                       "streams_per_batch_call": a.batch, "warmup": a.warmup, "ICER_DEC_WAVE": os.environ.get("ICER_DEC_WAVE", ""),
                       "parity": bool(ok)},
            "lone": rows["lone"], "batch": rows["batch"]}
    print(json.dumps(line))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
