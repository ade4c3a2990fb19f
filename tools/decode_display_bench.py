#!/usr/bin/env python3
"""Times the decoder's display path (Decoder.decode_display_torch, planes_to_display_torch) -- NOT bench.py's metric.

    python tools/decode_display_bench.py [--streams 16] [--side 1024] [--reps 9] [--conv-side 4096]

Workload: one `side` x `side` RGB frame encoded as Y Cb Cr (4 stages, filter A, 10 segments, one byte per pixel of quota),
`streams` copies of its stream resident in HBM.  Timed with device events on one non-default stream, workspaces cached, after
two warm-up rounds, the three decode cases ALTERNATING inside every round so that they see the same machine:
    a  decode_torch                      -> uint16 planes                          (icerx_decode_device_async)
    b  decode_display_torch              -> RGB888                                 (icerx_decode_device_display_async)
    c  decode_torch + a conversion written in torch ops (int64, the same formulas)
    d  planes_to_display_torch alone on 3 planes of conv-side^2 uint16 samples (windows of 20 calls), and a device copy of
       the same plane buffer (Tensor.copy_) timed the same way: d's bytes/s (6 read + 3 written per pixel) as a fraction of
       the copy's bytes/s (2 x the buffer)
Per case: the median and the min / max over the rounds (the run-to-run spread inside one process).  b's image must equal c's.
One JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES, FILT, SEGMENTS = 4, 0, 10


def torch_display(torch, planes):
    """(n, 3, pixels) int16 storage of uint16 samples -> (n, pixels, 3) uint8, in torch ops"""
    v = planes.to(torch.int64) & 0xFFFF
    y, cb, cr = v[:, 0], v[:, 1], v[:, 2]
    r = y + ((91881 * cr) >> 16) - 179
    g = y - ((22544 * cb + 46793 * cr) >> 16) + 135
    b = y + ((116129 * cb) >> 16) - 226
    return torch.stack([r, g, b], dim=-1).clamp_(0, 255).to(torch.uint8)


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=16)
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--conv-side", type=int, default=4096)
    a = ap.parse_args()
    import torch
    from icer_compression_amd import api, decoder, synth
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda", 0)
    n, side = a.streams, a.side
    pixels = side * side
    rgb = np.stack([synth.gray_frame(side, side, 100 + c, 1).astype(np.uint8) for c in range(3)], axis=-1)
    quota = pixels
    enc = api.Encoder(side, side, 3, STAGES, FILT, SEGMENTS, max_frames=1)
    coded = torch.zeros((1, quota + 64), dtype=torch.uint8, device=dev)
    sizes = torch.zeros(1, dtype=torch.int64, device=dev)
    e_rcs = torch.zeros(1, dtype=torch.int32, device=dev)
    enc.encode_torch_frontend(torch.from_numpy(rgb[None]).to(dev), quota, coded, sizes, e_rcs)
    torch.cuda.synchronize()
    assert e_rcs.item() in (0, -5), e_rcs.item()
    length = int(sizes.item())
    enc.close()
    data = coded[:, :length].repeat(n, 1).contiguous()
    lens = torch.full((n,), length, dtype=torch.int64, device=dev)
    planes = torch.zeros((n, 3, pixels), dtype=torch.int16, device=dev)
    image = torch.zeros((n, pixels, 3), dtype=torch.uint8, device=dev)
    rcs = torch.zeros(n, dtype=torch.int32, device=dev)
    ws, hs = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
    dec = decoder.Decoder(3, STAGES, FILT, SEGMENTS)
    st = torch.cuda.Stream()
    cases = {
        "a_plain": lambda: dec.decode_torch(data, lens, planes, rcs, ws, hs),
        "b_display": lambda: dec.decode_display_torch(data, lens, image, rcs, ws, hs),
        "c_plain_then_torch": lambda: (dec.decode_torch(data, lens, planes, rcs, ws, hs), torch_display(torch, planes)),
    }
    times = {k: [] for k in cases}
    with torch.cuda.stream(st):
        for rnd in range(a.reps + 2):
            for name, fn in cases.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                fn()
                e1.record(st)
                st.synchronize()
                if rnd >= 2:
                    times[name].append(e0.elapsed_time(e1))
        assert rcs.cpu().tolist() == [0] * n
        dec.decode_torch(data, lens, planes, rcs, ws, hs)
        same = bool(torch.equal(torch_display(torch, planes), image))
        st.synchronize()
    dec.close()
    line = {"metric": "decode to display images, ms per call", "streams": n, "side": side, "stream_bytes": length,
            "mpixels_per_call": round(n * pixels / 1e6, 2), "parity_b_equals_c": same}
    for name, ms in times.items():
        line[name] = spread(ms)
    del data, planes, image
    torch.cuda.empty_cache()

    # d: the conversion alone against a copy of the same buffer
    cs = a.conv_side
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    src = torch.randint(-32768, 32767, (1, 3, cs, cs), dtype=torch.int16, device=dev, generator=g)
    dup = torch.empty_like(src)
    calls = 20
    t_conv, t_copy = [], []
    with torch.cuda.stream(st):
        for rnd in range(a.reps + 2):
            for kind in ("conv", "copy"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(calls):
                    if kind == "conv":
                        out = decoder.planes_to_display_torch(src)
                    else:
                        dup.copy_(src)
                e1.record(st)
                st.synchronize()
                if rnd >= 2:
                    (t_conv if kind == "conv" else t_copy).append(e0.elapsed_time(e1) / calls)
    conv_bytes, copy_bytes = 9 * cs * cs, 2 * src.numel() * 2
    conv_rate = conv_bytes / (statistics.median(t_conv) * 1e-3) / 1e9
    copy_rate = copy_bytes / (statistics.median(t_copy) * 1e-3) / 1e9
    line["d_conversion"] = dict(spread(t_conv), side=cs, gbytes_per_s=round(conv_rate, 1), gpixels_per_s=round(cs * cs / (statistics.median(t_conv) * 1e-3) / 1e9, 2))
    line["d_copy"] = dict(spread(t_copy), gbytes_per_s=round(copy_rate, 1))
    line["d_fraction_of_copy_bandwidth"] = round(conv_rate / copy_rate, 3)
    del out
    print(json.dumps(line))


if __name__ == "__main__":
    main()
