"""Device-resident timing of the standalone wavelet transform: icerx_wavelet_forward_device /
icerx_wavelet_inverse_device on one 4096 x 4096 uint16 plane, 5 stages, every filter, with HIP events on torch's
stream around the C call alone (median over repeats).  Prints one JSON line per (direction, filter).

    python tools/wavelet_bench.py [--size 4096] [--stages 5] [--reps 20] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--stages", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bits", type=int, default=16, choices=(8, 16))
    a = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")
    from icer_compression_amd import api, decoder
    g = torch.Generator(device="cuda").manual_seed(1)
    dt = torch.int16 if a.bits == 16 else torch.int8
    src = torch.randint(0, 1 << (a.bits - 4), (1, a.size, a.size), device="cuda", generator=g, dtype=torch.int32).to(dt)
    enc, dec = api.load_library(), decoder.load_library()
    # the workspace, the result codes and the argument conversion are set up once, outside the timed window
    ws = torch.empty(int(enc.icerx_wavelet_workspace_bytes(a.size, a.size, 1, a.bits)), dtype=torch.uint8, device="cuda")
    rcs = torch.zeros(1, dtype=torch.int32, device="cuda")
    for name, fn in (("forward", enc.icerx_wavelet_forward_device), ("inverse", dec.icerx_wavelet_inverse_device)):
        for filt in range(7):
            plane = src.clone()
            st = torch.cuda.current_stream().cuda_stream
            args = (plane.data_ptr(), 1, a.size, a.size, a.size * a.size, a.stages, filt, a.bits, ws.data_ptr(), rcs.data_ptr(), st)
            times = []
            for r in range(a.warmup + a.reps):
                plane.copy_(src)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = fn(*args)
                e1.record()
                e1.synchronize()
                assert rc == 0, rc
                if r >= a.warmup:
                    times.append(e0.elapsed_time(e1))
            print(json.dumps({"direction": name, "filter": "ABCDEFQ"[filt], "size": a.size, "stages": a.stages, "bits": a.bits,
                              "median_ms": round(statistics.median(times), 4), "min_ms": round(min(times), 4), "reps": a.reps}), flush=True)


if __name__ == "__main__":
    main()
