#!/usr/bin/env python3
"""Times icerx_decode_device_async (Decoder.decode_torch) against icerx_decode_device -- NOT bench.py's metric.

    python tools/decode_async_bench.py [--batches 1,8,64] [--reps 3]

Workload: the C2 stream (4096 x 4096 gray, 5 stages, filter A, 10 segments, lossless: the reference golden), n copies
resident in HBM, decoded to uint16 planes in HBM.  Per n: the whole synchronous call, and the asynchronous call from enqueue
to the stream's completion (workspace already cached), both as Mpixels/s; every frame is compared with the input.  Then the
encode -> decode round trip of one C2 frame on one stream (encode_torch, decode_torch of its d_out / d_sizes, one
synchronise).  One JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W = H = 4096
STAGES, FILT, SEGMENTS = 5, 0, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import torch
    from icer_compression_amd import api, decoder, synth
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    img = synth.gray_frame(W, H, 12345, 1)
    rc, stream, _ = api.compress([img], STAGES, FILT, SEGMENTS, 2 * W * H)
    assert rc == 0
    want = torch.from_numpy(img.view(np.int16)).to(dev)
    line = {"metric": "Mpixels/s decode, async vs sync, C2 stream", "unit": "Mpixels/s", "streams": {}}
    for n in [int(x) for x in a.batches.split(",")]:
        d_data = torch.from_numpy(np.frombuffer(stream * n, dtype=np.uint8).copy()).to(dev)
        d_out = torch.zeros((n, H * W), dtype=torch.int16, device=dev)
        dec = decoder.Decoder(1, STAGES, FILT, SEGMENTS)
        offs, lens = [k * len(stream) for k in range(n)], [len(stream)] * n
        t_sync = []
        for _ in range(a.reps + 1):
            torch.cuda.synchronize()
            t = time.perf_counter()
            rc2, rcs, _, _ = dec.decode_device(n, d_data.data_ptr(), offs, lens, d_out.data_ptr(), W * H)
            torch.cuda.synchronize()
            t_sync.append(time.perf_counter() - t)
        ok_sync = rc2 == 0 and rcs == [0] * n and all(bool(torch.equal(d_out[k].view(H, W), want)) for k in range(n))
        d_out.zero_()
        d_lens = torch.full((n,), len(stream), dtype=torch.int64, device=dev)
        rcs_t = torch.zeros(n, dtype=torch.int32, device=dev)
        ws_t = torch.zeros(n, dtype=torch.int64, device=dev)
        hs_t = torch.zeros(n, dtype=torch.int64, device=dev)
        st = torch.cuda.Stream()
        t_async, t_enq = [], []
        with torch.cuda.stream(st):
            for _ in range(a.reps + 1):
                st.synchronize()
                t = time.perf_counter()
                dec.decode_torch(d_data, d_lens, d_out, rcs_t, ws_t, hs_t, stream_stride=len(stream))
                t_enq.append(time.perf_counter() - t)
                st.synchronize()
                t_async.append(time.perf_counter() - t)
        ok_async = rcs_t.cpu().tolist() == [0] * n and all(bool(torch.equal(d_out[k].view(H, W), want)) for k in range(n))
        ts, ta = min(t_sync[1:]), min(t_async[1:])
        line["streams"][str(n)] = {"sync": round(n * W * H / ts / 1e6, 1), "async": round(n * W * H / ta / 1e6, 1),
                                   "sync_ms": round(ts * 1e3, 2), "async_ms": round(ta * 1e3, 2),
                                   "async_enqueue_ms": round(min(t_enq[1:]) * 1e3, 3), "parity": bool(ok_sync and ok_async)}
        dec.close()
        del d_data, d_out
        torch.cuda.empty_cache()
    # encode -> decode on one stream, nothing through the host
    quota = 2 * W * H
    enc = api.Encoder(W, H, channels=1, stages=STAGES, filt=FILT, segments=SEGMENTS, max_frames=1)
    dec = decoder.Decoder(1, STAGES, FILT, SEGMENTS)
    frames = want.view(1, 1, H, W)
    out = torch.zeros((1, quota + 64), dtype=torch.uint8, device=dev)
    sizes = torch.zeros(1, dtype=torch.int64, device=dev)
    e_rcs = torch.zeros(1, dtype=torch.int32, device=dev)
    planes = torch.zeros((1, H * W), dtype=torch.int16, device=dev)
    rcs_t = torch.zeros(1, dtype=torch.int32, device=dev)
    ws_t = torch.zeros(1, dtype=torch.int64, device=dev)
    hs_t = torch.zeros(1, dtype=torch.int64, device=dev)
    st = torch.cuda.Stream()
    times = []
    with torch.cuda.stream(st):
        for _ in range(a.reps + 1):
            st.synchronize()
            t = time.perf_counter()
            enc.encode_torch(frames, quota, out, sizes, e_rcs)
            dec.decode_torch(out, sizes, planes, rcs_t, ws_t, hs_t)
            st.synchronize()
            times.append(time.perf_counter() - t)
    ok = e_rcs.item() == 0 and rcs_t.item() == 0 and bool(torch.equal(planes.view(H, W), want))
    line["round_trip"] = {"ms": round(min(times[1:]) * 1e3, 2), "parity": ok}
    enc.close()
    dec.close()
    print(json.dumps(line))


if __name__ == "__main__":
    main()
