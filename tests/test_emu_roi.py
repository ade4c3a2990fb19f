"""Region-of-interest ranks and cuts (csrc/roi_core.hpp): roi_rank_kernel's phases and scan_roi_wave, built for the CPU from the
kernel source (tests/emu/roi_emu.cpp) over the planner's own units, give what tests/roi_model.py defines -- ranks, the inverse
order, foreground counts, K, final offsets, sizes, return codes and the slot-bound flag -- on the geometries of
tests/geometry_sweep_cases.py: every shift 0 .. 16, rectangles that are empty, full, inside a segment, across the border, the
last pixel, outside; random bit counts with 0, kUnitTooBig and kUnitFailed among them; quotas around one packet header (0, 27,
28, 29), quotas on which a prefix of the ROI order ends exactly, repeats."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import geometry_sweep_cases as gsc
from tests import roi_model as rm
from tests import target_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOO_BIG, FAILED, NONE, HEADER = rm.TOO_BIG, rm.FAILED, rm.NONE, rm.HEADER

u8p = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")
u32p = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")
u64p = np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS")
i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")


@pytest.fixture(scope="module")
def lib():
    src = os.path.join(ROOT, "tests", "emu", "roi_emu.cpp")
    so = os.path.join(ROOT, "tests", "emu", "libroi_emu.so")
    csrc = os.path.join(ROOT, "icer_compression_amd", "csrc")
    newest = max([os.path.getmtime(os.path.join(csrc, f)) for f in os.listdir(csrc)] + [os.path.getmtime(src)])
    if not os.path.exists(so) or os.path.getmtime(so) < newest:
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", so, src])
    L = C.CDLL(so)
    L.emu_roi_plan.restype = C.c_int
    L.emu_roi_plan.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int]
    L.emu_roi_tables.restype = None
    L.emu_roi_tables.argtypes = [u32p, u64p, u32p]
    L.emu_roi_rank.restype = None
    L.emu_roi_rank.argtypes = [u32p, C.c_uint32, C.c_uint32, u32p, u32p, C.POINTER(C.c_uint32)]
    L.emu_scan_roi.restype = C.c_uint32
    L.emu_scan_roi.argtypes = [u32p, u64p, C.c_uint32, C.c_int, u8p, u32p, u32p, u64p, u64p, i32p, u32p]
    return L


def rectangles(rng, m: tm.Model):
    """empty, the full frame, one inside a single segment of the finest HH subband, one across the right and bottom border, the
    last pixel, one with x >= w, one whose corner wraps 32 bits, random ones"""
    w, h = m.w, m.h
    k = next(i for i, u in enumerate(m.units) if u[1] == 1 and u[2] == tm.HH and u[4] == (m.units[-1][4] + 1) // 2)
    sx, sy, sw, sh = rm.local_rect(m, k)
    inside = (2 * sx + sw, 2 * sy + sh, 1, 1)
    out = [(5, 5, 0, 9), (0, 0, w, h), inside, (w - 3, h - 2, 50, 50), (w - 1, h - 1, 1, 1), (w, 0, 4, 4), (2, 3, 0xFFFFFFFF, 0xFFFFFFFE),
           (-1, -1, 4, 4)]
    for _ in range(3):
        x, y = int(rng.integers(0, w)), int(rng.integers(0, h))
        out.append((x, y, int(rng.integers(1, w)), int(rng.integers(1, h))))
    return out


def random_bits(rng, n):
    bits = rng.integers(1, 6000, n).astype(np.uint32)
    bits[rng.random(n) < 0.15] = 0
    if rng.random() < 0.5:                                             # (the other frames can be kept whole)
        bits[rng.random(n) < 0.03] = TOO_BIG
    return bits


def quota_set(rng, bits, order, n_q):
    """0, 27, 28, 29, quotas on which a kept prefix of the ROI order ends exactly (and one byte either side), the quota at which
    a unit just fails, random ones, one that keeps everything, a repeat"""
    pb = [int(bits[u]) for u in order]
    prefix = np.cumsum([0] + [tm.unit_len(b) for b in pb if b != TOO_BIG])
    cands = [0, 27, 28, 29]
    for k in rng.choice(len(prefix), size=min(4, len(prefix)), replace=False):
        cands += [int(prefix[k]) - 1, int(prefix[k]), int(prefix[k]) + 1]
    for k in rng.choice(len(pb), size=min(3, len(pb)), replace=False):
        if pb[k] not in (TOO_BIG, FAILED):
            used = sum(tm.unit_len(b) for b in pb[:k] if b not in (TOO_BIG, FAILED))
            cands += [used + HEADER + pb[k] // 8, used + HEADER + pb[k] // 8 + 1]
    cands += [int(x) for x in rng.integers(0, int(prefix[-1]) + 100, 4)] + [int(prefix[-1]) + 10 ** 6]
    qs = [max(0, int(c)) for c in rng.choice(cands, size=n_q - 1, replace=True)]
    qs.append(qs[int(rng.integers(0, len(qs)))] if qs else 28)
    rng.shuffle(qs)
    return np.array(qs, np.uint64)


def test_roi_rank_and_scan_equal_the_model(lib):
    rng = np.random.default_rng(20261019)
    seen = {"bound_flag": 0, "failed": 0, "skip": 0, "cut": 0, "all_kept": 0, "nothing": 0, "mixed_order": 0, "ties": 0}
    shifts_seen = set()
    for gi, (g, _) in enumerate(gsc.cases()):
        m = tm.Model(g.w, g.h, g.channels, g.stages, g.filt, g.segments, g.bits)
        n = lib.emu_roi_plan(g.w, g.h, g.channels, g.stages, g.segments, g.bits)
        assert n == m.n_units, (gsc.case_id(g), n)
        forder, prio, desc = np.empty(n, np.uint32), np.empty(n, np.uint64), np.empty((n, 6), np.uint32)
        lib.emu_roi_tables(forder, prio, desc)
        want_forder = rm.final_order(m)
        assert forder.tolist() == want_forder, gsc.case_id(g)
        assert prio.tolist() == [u[6] for u in m.units], gsc.case_id(g)
        assert desc.tolist() == [[u[1], u[2]] + list(m.families[u[5]][1:5]) for u in m.units], gsc.case_id(g)
        assert max(u[6] for u in m.units) <= 1 << 24
        rects = rectangles(rng, m)
        for ri, roi in enumerate(rects):
            # every shift on one rectangle of the geometry (a different kind from geometry to geometry), two on the others
            shifts = range(rm.MAX_SHIFT + 1) if ri == gi % len(rects) else sorted({int(rng.integers(0, 4)), int(rng.integers(4, 17))})
            roi_arr = np.array([v & 0xFFFFFFFF for v in roi], np.uint32)
            for shift in shifts:
                shifts_seen.add(shift)
                rank, order, fgc = np.full(n, 7, np.uint32), np.full(n, 7, np.uint32), C.c_uint32(7)
                lib.emu_roi_rank(roi_arr, shift, int(rng.integers(0, 1 << 30)) * (shift % 2), rank, order, C.byref(fgc))
                w_rank, w_order, w_fg = rm.roi_order(m, roi, shift)
                what = (gsc.case_id(g), roi, shift)
                assert fgc.value == w_fg, what
                assert order.tolist() == w_order and rank.tolist() == w_rank, what
                seen["mixed_order"] += w_order != list(range(n))
                if shift and 0 < w_fg < n:
                    fg = rm.foreground(m, roi)
                    eff = {}
                    for k, u in enumerate(m.units):
                        eff.setdefault(u[6] << shift if fg[k] else u[6], set()).add(fg[k])
                    seen["ties"] += any(len(v) == 2 for v in eff.values())
                # the ranked scan
                bits = random_bits(rng, n)
                skip = int(rng.random() < 0.05)
                if rng.random() < 0.06:
                    bits[int(rng.integers(0, n))] = FAILED
                bound = (rng.random(n) < 0.5).astype(np.uint8)
                n_q = int(rng.integers(1, 17 if n <= 600 else 4))          # (the model walks every quota in Python)
                quotas = quota_set(rng, bits, w_order, n_q)
                foff = np.full(n_q * n, 7, np.uint64)
                sizes, rcs, kept = np.full(n_q, 7, np.uint64), np.full(n_q, 7, np.int32), np.full(n_q, 7, np.uint32)
                flags = lib.emu_scan_roi(bits, quotas, n_q, skip, bound, rank, order, foff, sizes, rcs, kept)
                w_flags = 0
                for q, quota in enumerate(quotas):
                    wf, ws, wr, wk, fl = rm.scan(bits, want_forder, w_rank, w_order, int(quota), skip, bound)
                    w_flags |= fl
                    assert foff[q * n: (q + 1) * n].tolist() == wf, (what, q)
                    assert (int(sizes[q]), int(rcs[q]), int(kept[q])) == (ws, wr, wk), (what, q, int(quota))
                    seen["cut"] += wr == rm.QUOTA_EXCEEDED
                    seen["all_kept"] += wr == rm.OK
                    seen["nothing"] += ws == 0 and wr == rm.QUOTA_EXCEEDED
                assert flags == w_flags, (what, flags, w_flags)
                seen["bound_flag"] += w_flags == 1
                seen["failed"] += bool(w_flags & 2)
                seen["skip"] += skip
    assert shifts_seen == set(range(rm.MAX_SHIFT + 1))
    assert all(v >= 5 for v in seen.values()), seen


def test_identities_of_the_order(lib):
    """shift 0, an empty rectangle, one outside the frame, a foreground of every unit (the full frame, unless a kept grid of
    quirk P1 reaches past its subband) and an encoder of one segment all give the priority order itself"""
    for g, _ in gsc.cases():
        m = tm.Model(g.w, g.h, g.channels, g.stages, g.filt, g.segments, g.bits)
        n = lib.emu_roi_plan(g.w, g.h, g.channels, g.stages, g.segments, g.bits)
        cases = [((3, 3, 9, 9), 0), ((3, 3, 0, 9), 5), ((g.w, g.h, 9, 9), 7), ((0, 0, g.w, g.h), 16)]
        if g.segments == 1:
            cases.append(((g.w // 2, g.h // 2, 1, 1), 9))
        for roi, shift in cases:
            rank, order, fgc = np.empty(n, np.uint32), np.empty(n, np.uint32), C.c_uint32()
            lib.emu_roi_rank(np.array(roi, np.uint32), shift, 3, rank, order, C.byref(fgc))
            if roi == (0, 0, g.w, g.h) and fgc.value != n:
                assert gsc.is_p1(g), gsc.case_id(g)
                continue
            assert order.tolist() == list(range(n)) and rank.tolist() == list(range(n)), (gsc.case_id(g), roi, shift)
