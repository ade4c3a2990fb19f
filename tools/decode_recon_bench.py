#!/usr/bin/env python3
"""Benchmark of the decoder's reconstruction option (include/icer_hip_dec.h, "Reconstructing truncated coefficients inside
their interval") -- NOT bench.py's metric.

    python tools/decode_recon_bench.py [--quota 2000000] [--batch 64] [--reps 9] [--batch-reps 5] [--warmup 2]
                                       [--parent-lib PATH] [--psnr-quotas 500000,1000000,2000000,4000000]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/decode_recon_bench.py --calls-only 5

Workload: the BASELINE configs[1] frame (4096 x 4096 gray, synth.gray_frame, 5 stages, filter A, 10 segments) encoded by the HIP
encoder at the byte quota `--quota` (lossy), the stream resident in HBM, decoded to uint16 planes that stay in HBM -- alone and
`--batch` times per call, in ONE process, with
    k = 0    the decoder as it was (reconstruct_kernel is not launched)
    k = 3    the recommended reconstruction point (one extra pass, csrc/decoder_recon.hpp)
    parent   `--parent-lib`: a build of the parent commit's libicer_hip_dec.so, k = 0 by construction
each through the synchronous call (icerx_decode_device) and the asynchronous one (Decoder.decode_torch).  The configurations
take turns: every round times one call of each, so that drift of the machine meets all of them alike.  `--warmup` untimed
rounds, then `--reps` timed ones (wall clock around call + synchronise); median, minimum and maximum are reported, a row's spread
is max - min.  Checked in the same run: k = 0 delivers the parent's image bit for bit, and k = 3 changes it.

PSNR: the same frame at each quota of `--psnr-quotas`, decoded with k = 0 .. 4, against the encoder's input.

`--calls-only N`: nothing but N lone synchronous decodes with k = 3, for a kernel trace (the new kernel is reconstruct_kernel).
One JSON line.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W = H = 4096
STAGES, FILT, SEGMENTS = 5, 0, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quota", type=int, default=2_000_000)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--batch-reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--psnr-quotas", default="500000,1000000,2000000,4000000")
    ap.add_argument("--calls-only", type=int, default=0)
    a = ap.parse_args()
    import torch
    from icer_compression_amd import api, decoder, synth
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)                                   # torch's HIP runtime first (see tests/conftest.py)
    img = synth.gray_frame(W, H, 12345, 1)

    def encode(quota):
        rc, stream, _ = api.compress([img], STAGES, FILT, SEGMENTS, quota)
        assert stream and rc in (0, -5), rc
        return stream
    stream = encode(a.quota)
    stride = W * H

    def setup(n, lib, k):
        dec = decoder.Decoder(1, STAGES, FILT, SEGMENTS, lib=lib, reconstruct=k)
        c = {"dec": dec, "n": n, "out": torch.zeros((n, stride), dtype=torch.int16, device=dev),
             "offs": [i * len(stream) for i in range(n)], "lens": [len(stream)] * n}
        c["t_lens"] = torch.tensor(c["lens"], dtype=torch.int64, device=dev)
        c["t_offs"] = torch.tensor(c["offs"], dtype=torch.int64, device=dev)
        c["t_rcs"] = torch.full((n,), 77, dtype=torch.int32, device=dev)
        c["t_ws"], c["t_hs"] = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
        return c

    def sync_call(c, d_data):
        rc, rcs, ws, hs = c["dec"].decode_device(c["n"], d_data.data_ptr(), c["offs"], c["lens"], c["out"].data_ptr(), stride)
        assert rc == 0 and set(rcs) == {0} and set(ws) == {W} and set(hs) == {H}, (rc, rcs)

    def async_call(c, d_data):
        c["dec"].decode_torch(d_data, c["t_lens"], c["out"], c["t_rcs"], c["t_ws"], c["t_hs"], offsets=c["t_offs"])

    if a.calls_only:
        c = setup(1, None, 3)
        d_data = torch.from_numpy(np.frombuffer(stream, dtype=np.uint8).copy()).to(dev)
        for _ in range(a.calls_only):
            sync_call(c, d_data)
            torch.cuda.synchronize()
        print(json.dumps({"calls_only": a.calls_only, "k": 3, "stream_bytes": len(stream)}))
        return 0

    parent = decoder.bind(os.path.abspath(a.parent_lib)) if a.parent_lib else None
    assert parent is None or not hasattr(parent, "icerx_decoder_set_reconstruction"), "--parent-lib has the option: not the parent"

    def run(n, reps):
        d_data = torch.from_numpy(np.frombuffer(stream * n, dtype=np.uint8).copy()).to(dev)
        confs = {"k0": setup(n, None, 0), "k3": setup(n, None, 3)}
        if parent is not None:
            confs["parent"] = setup(n, parent, 0)
        res = {}
        for kind, call in (("sync", sync_call), ("async", async_call)):
            times = {name: [] for name in confs}
            for rnd in range(a.warmup + reps):
                for name, c in confs.items():                     # (the configurations take turns)
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    call(c, d_data)
                    torch.cuda.synchronize()
                    if rnd >= a.warmup:
                        times[name].append((time.perf_counter() - t) * 1e3)
            if kind == "async":
                for c in confs.values():
                    assert c["t_rcs"].cpu().tolist() == [0] * n
            for name, ts in times.items():
                res[f"{name}_{kind}"] = {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3),
                                         "max_ms": round(max(ts), 3), "reps": reps}
        ok = all(bool(torch.equal(c["out"][i], c["out"][0])) for c in confs.values() for i in range(n))
        changed = not bool(torch.equal(confs["k3"]["out"][0], confs["k0"]["out"][0]))
        same_as_parent = bool(torch.equal(confs["parent"]["out"][0], confs["k0"]["out"][0])) if parent is not None else None
        for c in confs.values():
            c["dec"].close()
        res.update({"streams": n, "frames_equal_within_call": ok, "k3_changes_the_image": changed, "k0_equals_parent": same_as_parent})
        return res

    rows = [run(1, a.reps)] + ([run(a.batch, a.batch_reps)] if a.batch > 1 else [])

    # PSNR per k
    psnr = []
    ref = torch.from_numpy(img.astype(np.int32)).to(dev).reshape(-1).double()
    for q in [int(x) for x in a.psnr_quotas.split(",") if x]:
        s = encode(q)
        d_data = torch.from_numpy(np.frombuffer(s, dtype=np.uint8).copy()).to(dev)
        out = torch.zeros((1, stride), dtype=torch.int16, device=dev)
        row = {"quota": q, "stream_bytes": len(s), "psnr_db": {}, "mse": {}}
        for k in range(5):
            dec = decoder.Decoder(1, STAGES, FILT, SEGMENTS, reconstruct=k)
            rc, rcs, ws, hs = dec.decode_device(1, d_data.data_ptr(), [0], [len(s)], out.data_ptr(), stride)
            torch.cuda.synchronize()
            dec.close()
            assert rc == 0 and rcs == [0], (rc, rcs)
            mse = float(((out[0].double() - ref) ** 2).mean())
            row["mse"][str(k)] = round(mse, 4)
            row["psnr_db"][str(k)] = round(10 * math.log10(255.0 ** 2 / mse), 3) if mse > 0 else None
        psnr.append(row)

    ok = all(r["frames_equal_within_call"] and r["k3_changes_the_image"] and r["k0_equals_parent"] in (None, True) for r in rows)
    line = {"metric": "ms per call, decode with reconstruction point k, 4096x4096 gray", "unit": "ms", "higher_is_better": False,
            "config": {"workload": f"4096x4096 gray, 5 stages, filter A, 10 segments, quota {a.quota} B ({len(stream)} B used), stream "
                                   "resident in HBM -> uint16 planes in HBM", "warmup": a.warmup,
                       "ICER_DEC_WAVE": os.environ.get("ICER_DEC_WAVE", ""), "parent_lib": bool(a.parent_lib), "parity": bool(ok)},
            "rows": rows, "psnr_8bit_peak": psnr}
    print(json.dumps(line))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
