"""A seeded sample of frame geometries for the rate ladder, the re-cut and the quality target (icerx_encode_device_ladder,
icerx_recut_device_async, icerx_encode_device_target), shared by tests/test_geometry_sweep.py (CPU) and
tests/test_gpu_geometry_sweep.py.  The same sample, with a rectangle per frame and a list of (reduce, quota, shift) cuts
(tests/sweep_cut_cases.py), runs through the ROI encode, the re-cuts by resolution and by region, the reduced decoders and the
display decode (icerx_encode_device_roi, icerx_recut_device_cuts_async, icerx_recut_device_roi_async,
icerx_decoder_create_reduced): tests/test_geometry_sweep_cuts.py (CPU) and tests/test_gpu_geometry_sweep_cuts.py; and
tests/test_emu_roi.py and tests/test_gpu_budget_sweep.py take their geometries from it.

Draws: sides 9 .. 200 with at most 40 000 samples a frame, 1 .. 6 stages, filters 0 .. 6, 1 .. 32 segments, 1 or 3 channels,
16 or 8 bits, and a batch of three frame specs.  A draw is kept only if the oracle codes every frame of its batch at the
lossless quota with rc 0 (it refuses a geometry whose first packet has more segments than samples; 8-bit content may leave
int8 under the longer filters).  A geometry whose kept grid (quirk P1) leaves the plane is never given to it -- 9 x 9, 1 stage,
17 segments: HH keeps the 4 x 5 grid of HL at its own origin (5, 5) -- since there the reference, the oracle and the planner
(csrc/plan.hpp accepts it) all read outside the frame: an open defect, and nothing to compare.  Until the coverage conditions below
hold, only draws that count towards an unmet one are kept; then any, up to about TARGET.  The conditions were chosen so that
the oracle alone can meet them: a seed that misses one is replaced, the conditions stay."""
from __future__ import annotations

import functools

import numpy as np

from tests import encoder_batch_cases as ebc
from tests import target_model as tm

SEED = 20261018
TARGET = 24
MAX_SAMPLES = 40_000
MAX_DRAWS = 100_000


def n_units(g: ebc.Geometry) -> int:
    """(a kept grid has as many rectangles as a fresh one: P1 does not change the count)"""
    return (3 * g.stages + 1) * tm.coded_planes(g.bits) * g.channels * g.segments


def subbands(g: ebc.Geometry):
    """(width, height) of every subband that is coded"""
    out = [tm.subband_rect(g.w, g.h, lv, sb)[:2] for lv in range(1, g.stages + 1) for sb in (tm.HL, tm.LH, tm.HH)]
    return out + [tm.subband_rect(g.w, g.h, g.stages, tm.LL)[:2]]


def is_p1(g: ebc.Geometry) -> bool:
    """some subband's grid fails (whether the frame is coded all the same is the oracle's word)"""
    return any(tm.grid_fails(sw, sh, g.segments) for sw, sh in subbands(g))


def leaves_plane(g: ebc.Geometry) -> bool:
    """a kept grid (P1) laid at the failing subband's origin reaches past the plane's right or bottom edge"""
    if not is_p1(g):
        return False
    try:
        m = tm.Model(g.w, g.h, g.channels, g.stages, g.filt, g.segments, g.bits)
    except tm.Refused:
        return False
    return any(x + rw > g.w or y + rh > g.h for (_, x, y, rw, rh, _) in m.families)


def two_row_classes(g: ebc.Geometry) -> bool:
    """some subband's grid has top rows and, below them, rows of one column more"""
    for sw, sh in subbands(g):
        if not tm.grid_fails(sw, sh, g.segments):
            r, _, r_t = tm.grid_rows(sw, sh, g.segments)
            if r_t < r:
                return True
    return False


# (name, geometries needed, what counts)
CONDITIONS = [(f"{k} stages", 2, lambda g, k=k: g.stages == k) for k in range(1, 7)] + \
             [(f"filter {f} at 16 bits", 2, lambda g, f=f: g.bits == 16 and g.filt == f) for f in range(7)] + [
    ("1 segment", 1, lambda g: g.segments == 1),
    ("32 segments", 1, lambda g: g.segments == 32),
    ("7 .. 31 segments", 3, lambda g: 7 <= g.segments <= 31),
    ("YUV", 6, lambda g: g.channels == 3),
    ("8 bits", 5, lambda g: g.bits == 8),
    ("8 bits YUV", 2, lambda g: g.bits == 8 and g.channels == 3),
    ("8 bits under filter A (the only dense 8-bit kind, noise6)", 1, lambda g: g.bits == 8 and g.filt == 0),
    ("P1: a subband's grid fails", 3, is_p1),
    ("two classes of segment rows", 3, two_row_classes),
    ("an odd side", 4, lambda g: g.w % 2 == 1 or g.h % 2 == 1),
    ("rows shorter than a wavefront", 2, lambda g: g.w < 64),
    ("more than 2048 units", 2, lambda g: n_units(g) > 2048),
    ("at most 64 units", 2, lambda g: n_units(g) <= 64),
]


def coverage(geometries):
    """{condition: (geometries that count, geometries needed)}"""
    return {name: (sum(1 for g in geometries if fn(g)), need) for name, need, fn in CONDITIONS}


def unmet(geometries):
    return [name for name, (have, need) in coverage(geometries).items() if have < need]


def draw_geometry(rng) -> ebc.Geometry:
    while True:
        w, h = int(rng.integers(9, 201)), int(rng.integers(9, 201))
        if w * h <= MAX_SAMPLES:
            break
    return ebc.Geometry(w, h, (1, 3)[int(rng.integers(0, 2))], int(rng.integers(1, 7)), int(rng.integers(0, 7)), int(rng.integers(1, 33)),
                        bits=(16, 8)[int(rng.integers(0, 2))])


def draw_specs(rng, g: ebc.Geometry):
    """three frames, the first one dense where the filter allows a dense kind (16 bits: noise8 or wide; 8 bits: noise6 under
    filter A only, the other filters take 6-bit noise out of int8 -- encoder_batch_cases.plane8)"""
    if g.bits == 16:
        kinds = [("noise8", "wide")[int(rng.integers(0, 2))]] + [ebc.CODED16[int(i)] for i in rng.integers(0, len(ebc.CODED16), 2)]
        if g.channels == 3 and rng.integers(0, 2):                    # (a kind per channel)
            kinds[2] = tuple(ebc.CODED16[int(i)] for i in rng.integers(0, len(ebc.CODED16), 3))
    else:
        pool = [k for k in ebc.KINDS8 if k != "full8" and (k != "noise6" or g.filt == 0)]
        kinds = ["noise6" if g.filt == 0 else "smooth6"] + [pool[int(i)] for i in rng.integers(0, len(pool), 2)]
    return [(k, int(rng.integers(0, 4))) for k in kinds]


def coded_by(orc, g: ebc.Geometry, specs) -> bool:
    """the oracle codes every frame of the batch completely at the lossless quota"""
    compress = orc.compress_u8 if g.bits == 8 else orc.compress
    q = ebc.quota(g, "lossless")
    return all(compress(ebc.oracle_planes(g, s), g.stages, g.filt, g.segments, q)[0] == 0 for s in specs)


def sample(orc, seed=SEED, target=TARGET):
    """[(geometry, specs)]: see the module's text"""
    rng = np.random.default_rng(seed)
    kept = []
    for _ in range(MAX_DRAWS):
        missing = unmet([g for g, _ in kept])
        if not missing and len(kept) >= target:
            break
        g = draw_geometry(rng)
        specs = draw_specs(rng, g)                                     # (drawn for every geometry: one stream of numbers per seed)
        if g in [k for k, _ in kept]:
            continue
        if missing and not any(fn(g) for name, _, fn in CONDITIONS if name in missing):
            continue
        if not leaves_plane(g) and coded_by(orc, g, specs):
            kept.append((g, specs))
    return kept


@functools.lru_cache(maxsize=None)
def cases():
    """the committed seed's sample (made once per process; the oracle is the only judge)"""
    from oracle.binding import Oracle
    return tuple(sample(Oracle()))


def case_id(g: ebc.Geometry) -> str:
    return f"{g.w}x{g.h}-{g.channels}ch-{g.stages}st-f{g.filt}-{g.segments}seg-{g.bits}b"
