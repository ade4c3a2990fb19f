#!/usr/bin/env python3
"""Benchmark of the window decode (include/icer_hip_dec_window.h) -- NOT bench.py's metric.

    python tools/decode_window_bench.py [--batch 64] [--reps 5] [--warmup 1] [--segments 32,10] [--q-case 1]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/decode_window_bench.py --calls-only 3 --case centre --warmup 0

Workload: one lossless 4096 x 4096 gray master (synth.gray_frame, 5 stages, filter A) per segment count of `--segments`, made by
the HIP encoder, `--batch` copies of it resident in HBM.  Per master, in ONE process and taking turns round by round:
    plain    Decoder.decode_torch (icerx_decode_device_async) of the whole frames, then the crop of the 1024 x 1024 centre
             window with a torch copy -- the baseline; its run-to-run spread (max - min) is the yardstick for the last row
    centre / corner / full    Decoder.decode_window_torch with a 1024 x 1024 window at the centre, at the top-left corner, and
             with the full frame
each timed around call + synchronise; median, minimum and maximum over `--reps` rounds after `--warmup` untimed ones, with the
chains run / chains of the plain call from the call's info.  Then the same for a lone stream.  `--q-case`: a filter-Q master
at 32 segments with a top-left and a bottom-right window (the dependence of the other filters runs to the end of a line).
Checked in the same run: every window equals the crop of the plain call's frame.  `--calls-only N`: one plain call (for the
check), then nothing but N calls of `--case` (plain, centre, corner, full) on the first master of `--segments`, for a kernel trace
(the new kernels are win_*_kernel and window_frames_kernel).  `--masters DIR` keeps the masters between runs.  One JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W = H = 4096
STAGES = 5
SIDE = 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--segments", default="32,10")
    ap.add_argument("--q-case", type=int, default=1)
    ap.add_argument("--calls-only", type=int, default=0)
    ap.add_argument("--case", default="centre", help="--calls-only: plain, centre, corner or full")
    ap.add_argument("--masters", default=None, help="a directory of masters kept between runs (master_f<filt>_s<segments>.bin)")
    a = ap.parse_args()
    import torch
    from icer_compression_amd import api, decoder, synth
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)                                   # torch's HIP runtime first (see tests/conftest.py)
    img = synth.gray_frame(W, H, 12345, 1)
    stride = W * H

    def master(filt, segments):
        path = os.path.join(a.masters, f"master_f{filt}_s{segments}.bin") if a.masters else None
        if path and os.path.exists(path):
            return open(path, "rb").read()
        rc, stream, _ = api.compress([img], STAGES, filt, segments, 4 * W * H)
        assert rc == 0 and stream, rc
        if path:
            os.makedirs(a.masters, exist_ok=True)
            open(path, "wb").write(stream)
        return stream

    def run(stream, filt, segments, n, windows, reps, only=None):
        """windows: {name: (x, y, w, h)} -> rows; only: the one case to call (the plain call once, for the parity check)"""
        d_data = torch.from_numpy(np.frombuffer(stream * n, dtype=np.uint8).copy()).to(dev)
        dec = decoder.Decoder(1, STAGES, filt, segments)
        lens = torch.tensor([len(stream)] * n, dtype=torch.int64, device=dev)
        offs = torch.tensor([i * len(stream) for i in range(n)], dtype=torch.int64, device=dev)
        rcs = torch.full((n,), 77, dtype=torch.int32, device=dev)
        ws, hs = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
        full = torch.zeros((n, stride), dtype=torch.int16, device=dev)
        info = torch.zeros((n, 6), dtype=torch.int32, device=dev)
        outs = {name: torch.zeros((n, min(w * h, stride)), dtype=torch.int16, device=dev) for name, (x, y, w, h) in windows.items()}
        wins = {name: torch.tensor([list(win)] * n, dtype=torch.int32, device=dev) for name, win in windows.items()}
        first = next(iter(windows.values()))
        crop = torch.zeros((n, first[3], first[2]), dtype=torch.int16, device=dev)

        def plain():
            dec.decode_torch(d_data, lens, full, rcs, ws, hs, offsets=offs)
            crop.copy_(full.view(n, H, W)[:, first[1]: first[1] + first[3], first[0]: first[0] + first[2]])

        def window(name):
            dec.decode_window_torch(d_data, lens, outs[name], rcs, ws, hs, wins[name], info, stride, offsets=offs)

        calls = {"plain": plain, **{name: (lambda name=name: window(name)) for name in windows}}
        times, counts = {name: [] for name in calls}, {}
        if only is not None:
            plain()
            calls = {only: calls[only]}
            times = {only: []}
        for rnd in range(a.warmup + reps):
            for name, call in calls.items():                      # (the cases take turns)
                torch.cuda.synchronize()
                t = time.perf_counter()
                call()
                torch.cuda.synchronize()
                if rnd >= a.warmup:
                    times[name].append((time.perf_counter() - t) * 1e3)
                assert rcs.cpu().tolist() == [0] * n, name
                if name != "plain":
                    counts[name] = info[0].cpu().tolist()
        ok = True
        for name, (x, y, w, h) in windows.items():
            if only is not None and name != only:
                continue
            want = full.view(n, H, W)[:, y: y + h, x: x + w].reshape(n, -1)
            ok = ok and bool(torch.equal(outs[name][:, : want.shape[1]], want))
        dec.close()
        rows = []
        for name, ts in times.items():
            row = {"case": name, "streams": n, "filter": filt, "segments": segments, "median_ms": round(statistics.median(ts), 2),
                   "min_ms": round(min(ts), 2), "max_ms": round(max(ts), 2), "reps": reps}
            if name in counts:
                row["chains_run"], row["chains_full"] = counts[name][4], counts[name][5]
            rows.append(row)
        return rows, ok

    c0 = (W - SIDE) // 2
    filter_a = {"centre": (c0, c0, SIDE, SIDE), "corner": (0, 0, SIDE, SIDE), "full": (0, 0, W, H)}
    if a.calls_only:
        segments = int(a.segments.split(",")[0])
        windows = filter_a if a.case == "plain" else {a.case: filter_a[a.case]}
        rows, ok = run(master(0, segments), 0, segments, a.batch, windows, a.calls_only, only=a.case)
        print(json.dumps({"calls_only": a.calls_only, "case": a.case, "warmup": a.warmup, "rows": rows, "parity": ok}))
        return 0 if ok else 1
    rows, parity = [], True
    for segments in [int(s) for s in a.segments.split(",") if s]:
        stream = master(0, segments)
        for n in (a.batch, 1):
            r, ok = run(stream, 0, segments, n, filter_a, a.reps)
            rows += r
            parity = parity and ok
    if a.q_case:
        r, ok = run(master(6, 32), 6, 32, a.batch, {"top-left": (0, 0, SIDE, SIDE), "bottom-right": (W - SIDE, H - SIDE, SIDE, SIDE)}, a.reps)
        rows += r
        parity = parity and ok
    print(json.dumps({"metric": "ms per call, window decode of lossless 4096x4096 gray masters", "unit": "ms", "higher_is_better": False,
                      "config": {"workload": "lossless masters, 5 stages, resident in HBM -> uint16 windows in HBM; plain = whole frames + crop",
                                 "warmup": a.warmup, "ICER_DEC_WAVE": os.environ.get("ICER_DEC_WAVE", ""), "parity": bool(parity)},
                      "rows": rows}))
    return 0 if parity else 1


if __name__ == "__main__":
    sys.exit(main())
