"""Regenerates tests/golden/fullsize_batch_golden.json: the UNTOUCHED reference encoder (oracle/_ref/libicer_ref.so, built by
oracle/Makefile) on every frame of a few full-size batches through filters other than A, for tests/test_gpu_fullsize.py
(batch_golden.json, which bench.py reads, holds filter A alone and is not touched here):

  gray8_2048_filt{B,D,F,Q}   8 x 2048x2048 gray, 4 stages, 16 segments, lossless quota 2*W*H; frame k has seed DEFAULT_SEED + k and
                             is synth.gray_frame(mode 1), but frame 2 is noise (mode 0) and frame 5 12-bit (gray_frame_12bit)
  yuv3_2048_filt{C,E}        3 x 2048x2048 YUV (synth.color_frame_yuv, seed DEFAULT_SEED + k), lossless quota 2*W*H*3

Per frame: [rc, stream length, zlib CRC-32] of icer_compress_image_[yuv_]uint16 and [rc, sha256[:16] of the planes, planes == input]
of the reference DECODER on that stream.  Every frame must be coded (rc 0, a stream) and decode (rc 0), the smooth
gray and the YUV frames to their input, or the generator stops.  Three kinds need not come back exactly from the reference itself, and
what it does with them is recorded: filter C (its inverse is not exact), and the 12-bit and -- through the filters of larger gain --
the noise frame, whose coefficients go beyond the 9 coded bit planes.

    python tests/golden/make_fullsize_batch_golden.py [processes]      (about a minute on 8 cores)

The reference library is not re-entrant, hence worker PROCESSES."""
import hashlib
import json
import multiprocessing as mp
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

GRAY_CONTENT = ["gray", "gray", "noise", "gray", "gray", "gray12", "gray", "gray"]
CONFIGS = {}
for _f in (1, 3, 5, 6):
    CONFIGS["gray8_2048_filt" + "ABCDEFQ"[_f]] = dict(w=2048, h=2048, channels=1, stages=4, filter=_f, segments=16, quota=2 * 2048 * 2048,
                                                     base_seed=12345, content=GRAY_CONTENT)
for _f in (2, 4):
    CONFIGS["yuv3_2048_filt" + "ABCDEFQ"[_f]] = dict(w=2048, h=2048, channels=3, stages=4, filter=_f, segments=16, quota=2 * 2048 * 2048 * 3,
                                                    base_seed=12345, content=["yuv"] * 3)


def frame_planes(c, k):
    """the planes of frame k of configuration c (tests/test_gpu_fullsize.py builds its inputs by the same rule, from the JSON)"""
    from icer_compression_amd import synth
    kind, seed = c["content"][k], c["base_seed"] + k
    if kind == "yuv":
        return list(synth.color_frame_yuv(c["w"], c["h"], seed))
    if kind == "gray12":
        return [synth.gray_frame_12bit(c["w"], c["h"], seed, 1)]
    return [synth.gray_frame(c["w"], c["h"], seed, 0 if kind == "noise" else 1)]


def one(job):
    name, k = job
    from oracle.binding import Reference
    c = CONFIGS[name]
    planes = frame_planes(c, k)
    ref = Reference()
    rc, stream, _ = ref.compress(planes, c["stages"], c["filter"], c["segments"], c["quota"])
    drc, dw, dh, back = ref.decompress_raw(stream, len(planes), c["stages"], c["filter"], c["segments"]) if stream else (-99, 0, 0, [])
    hsh = hashlib.sha256()
    for p in back:
        hsh.update(p.tobytes())
    same = bool(back) and (dw, dh) == (c["w"], c["h"]) and all((d.reshape(c["h"], c["w"]) == p).all() for d, p in zip(back, planes))
    return name, k, [rc, len(stream), "%08x" % zlib.crc32(stream)], [drc, hsh.hexdigest()[:16], bool(same)]


def main():
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else (os.cpu_count() or 1)
    jobs = [(n, k) for n, c in CONFIGS.items() for k in range(len(c["content"]))]
    out = {n: {"config": c, "frames": [None] * len(c["content"]), "decoded": [None] * len(c["content"])} for n, c in CONFIGS.items()}
    t0 = time.time()
    with mp.Pool(procs) as pool:
        for name, k, enc, dec in pool.imap_unordered(one, jobs):
            # a golden must not be vacuous: a coded frame, within the quota, that the reference decodes to its input
            assert enc[0] == 0 and 0 < enc[1] <= CONFIGS[name]["quota"], (name, k, enc)
            assert dec[0] == 0 and (dec[2] or CONFIGS[name]["filter"] == 2 or CONFIGS[name]["content"][k] in ("gray12", "noise")), (name, k, dec)
            out[name]["frames"][k], out[name]["decoded"][k] = enc, dec
            print(name, k, enc, dec, f"{time.time() - t0:.0f} s", flush=True)
    with open(os.path.join(ROOT, "tests", "golden", "fullsize_batch_golden.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
    print("done", time.time() - t0)


if __name__ == "__main__":
    main()
