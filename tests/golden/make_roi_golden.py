"""Writes tests/golden/roi_golden.json: size, return code, K and sha256 (16 hex digits) of the streams tests/roi_model.py cuts from
the REFERENCE encoder's lossless streams, for every case of tests/roi_cases.py -- what tests/test_gpu_roi.py expects of
icerx_encode_device_roi where the reference is not at hand.  Run from the repository root: python tests/golden/make_roi_golden.py"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle.binding import Reference                      # noqa: E402
from tests import encoder_batch_cases as ebc             # noqa: E402
from tests import roi_cases as rc                         # noqa: E402
from tests import roi_model as rm                         # noqa: E402


def main():
    ref = Reference()
    out = {}
    for name, g in rc.GEOMETRIES.items():
        m = rc.model(name)
        compress = ref.compress_u8 if g.bits == 8 else ref.compress
        qs = rc.quotas(name)
        for b, specs in enumerate(rc.BATCHES[name]):
            rects = rc.rectangles(name, b)
            lossless = []
            for spec in specs:
                code, stream, _ = compress(ebc.oracle_planes(g, spec), g.stages, g.filt, g.segments, qs[0])
                assert (code == 0 and stream) if rc.has_stream(spec) else (code == -1 and not stream), (name, spec, code, len(stream))
                lossless.append(stream)
            for shift in rc.SHIFTS:
                rows = {"size": [[0] * len(specs) for _ in qs], "rc": [[-1] * len(specs) for _ in qs], "kept": [[0] * len(specs) for _ in qs],
                        "sha256_16": [[hashlib.sha256(b"").hexdigest()[:16]] * len(specs) for _ in qs], "foreground": []}
                for f, (stream, roi) in enumerate(zip(lossless, rects)):
                    if not stream:
                        rows["foreground"].append(rm.roi_order(m, roi, shift)[2])
                        continue
                    res, n_fg = rm.roi_streams(m, stream, roi, shift, qs)
                    rows["foreground"].append(n_fg)
                    for q, (s, code, K) in enumerate(res):
                        rows["size"][q][f], rows["rc"][q][f], rows["kept"][q][f] = len(s), code, K
                        rows["sha256_16"][q][f] = hashlib.sha256(s).hexdigest()[:16]
                out[rc.golden_key(name, b, shift)] = rows
    path = os.path.join(ROOT, "tests", "golden", "roi_golden.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=0, sort_keys=True, separators=(",", ":"))
        fh.write("\n")
    print(path, os.path.getsize(path), "bytes,", len(out), "calls")


if __name__ == "__main__":
    main()
