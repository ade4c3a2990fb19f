"""The region-of-interest encode (icerx_encode_device_roi, csrc/roi_core.hpp) in plain Python integers.  This file is the
definition; include/icer_hip.h and DESIGN.md 3 "Region of interest" restate it.

A stream is made of the packets of the frame's lossless stream -- one per coding unit, the planner's units in priority order
(tests/target_model.py restates csrc/plan.hpp) -- and the rule only chooses which of them are kept:

  foreground   unit u of level l has the rectangle [sx, sx + sw) x [sy, sy + sh) in its subband's own coordinates.  With the
               frame's rectangle clipped to the frame, [x0, x1) x [y0, y1), and a guard G = 2 coefficients, u is foreground when
               it belongs to LL, or when the clipped rectangle is not empty and
                   sx < ceil(x1 / 2^l) + G,  sx + sw + G > floor(x0 / 2^l),  and the same two in y.
  order        eff(u) = prio(u) << shift for foreground units, prio(u) for the others; the units sorted by eff descending,
               ties by unit index ascending.  rank[u] = u's position, order[i] = the unit at position i.  A frame whose clipped
               rectangle is empty has no region of interest: its shift is 0, so its order is the priority order (its LL units
               still count as foreground).
  cut          the quota walk P3 over the units in that order gives K; the units with rank < K are kept, in the final order.
"""
from __future__ import annotations

from tests import target_model as tm

GUARD = 2
MAX_SHIFT = 16
HEADER, TOO_BIG, FAILED, NONE = tm.HEADER, tm.TOO_BIG, tm.FAILED, tm.NONE
OK, QUOTA_EXCEEDED, INTEGER_OVERFLOW, FATAL = 0, -5, -1, -10
MAX_STAGES = 6


def final_order(m: tm.Model):
    """the units' indices in final stream order (D7, csrc/plan.hpp): segment up, subband down, level down, plane down, channel
    up; the 8-bit YUV variant walks subband, level and plane up"""
    where = {}
    for k, (ch, lv, sb, lsb, sg, _, _) in enumerate(m.units):
        where[(ch, lv, sb, lsb, sg)] = k
    up = m.bits == 8 and m.channels == 3
    out = []
    for sg in range(tm.MAX_SEGMENTS + 1):
        for isb in range(4):
            for ilv in range(MAX_STAGES + 1):
                for il in range(m.P):
                    for ch in range(m.channels):
                        sb, lv, lsb = (isb, ilv, il) if up else (3 - isb, MAX_STAGES - ilv, m.P - 1 - il)
                        k = where.get((ch, lv, sb, lsb, sg))
                        if k is not None:
                            out.append(k)
    assert len(out) == m.n_units
    return out


def clip(roi, w, h):
    """(x0, y0, x1, y1) of a rectangle (x, y, w, h) whose entries are read as uint32"""
    rx, ry, rw, rh = (int(v) & 0xFFFFFFFF for v in roi)
    return min(rx, w), min(ry, h), min(rx + rw, w), min(ry + rh, h)


def local_rect(m: tm.Model, k: int):
    """(sx, sy, sw, sh) of unit k: its rectangle less its subband's origin"""
    _, lv, sb, _, _, fam, _ = m.units[k]
    _, x, y, rw, rh, _ = m.families[fam]
    _, _, ox, oy = tm.subband_rect(m.w, m.h, lv, sb)
    return x - ox, y - oy, rw, rh


def local_rects(m: tm.Model):
    """local_rect of every unit (kept on the model: they depend on the geometry alone)"""
    if not hasattr(m, "roi_local_rects"):
        m.roi_local_rects = [local_rect(m, k) for k in range(m.n_units)]
    return m.roi_local_rects


def foreground(m: tm.Model, roi):
    """[bool] per unit"""
    x0, y0, x1, y1 = clip(roi, m.w, m.h)
    empty = x1 <= x0 or y1 <= y0
    out = []
    for (_, lv, sb, _, _, _, _), (sx, sy, sw, sh) in zip(m.units, local_rects(m)):
        if sb == tm.LL:
            out.append(True)
            continue
        s = 1 << lv
        out.append(not empty and
                   sx < -(-x1 // s) + GUARD and sx + sw + GUARD > x0 // s and
                   sy < -(-y1 // s) + GUARD and sy + sh + GUARD > y0 // s)
    return out


def roi_order(m: tm.Model, roi, shift: int):
    """(rank, order, foreground units)"""
    assert 0 <= shift <= MAX_SHIFT
    fg = foreground(m, roi)
    x0, y0, x1, y1 = clip(roi, m.w, m.h)
    if x1 <= x0 or y1 <= y0:
        shift = 0
    eff = [(u[6] << shift) if f else u[6] for u, f in zip(m.units, fg)]
    assert all(0 < e < 1 << 64 for e in eff)
    order = sorted(range(m.n_units), key=lambda k: (-eff[k], k))
    rank = [0] * m.n_units
    for i, k in enumerate(order):
        rank[k] = i
    return rank, order, sum(fg)


def scan(bits, forder, rank, order, quota, skip=0, bound=None):
    """scan_roi_wave for one frame at one quota.  bits[u]: payload bits per unit (TOO_BIG, FAILED as the coder reports them).
    Returns (final offsets per unit, size, rc, K, flag bits)"""
    n = len(bits)
    if skip:
        return [NONE] * n, 0, INTEGER_OVERFLOW, 0, 0
    if any(int(b) == FAILED for b in bits):
        return [NONE] * n, 0, FATAL, 0, 2
    K, used = tm.quota_cut([bits[u] for u in order], quota)
    foff, off = [NONE] * n, 0
    for u in forder:
        if rank[u] < K:
            foff[u] = off
            off += tm.unit_len(bits[u])
    assert off == used
    flags = int(K < n and int(bits[order[K]]) == TOO_BIG and bool(bound is not None and bound[order[K]]))
    return foff, off, (QUOTA_EXCEEDED if K < n else OK), K, flags


def split_stream(m: tm.Model, stream: bytes):
    """{unit index: the packet's bytes} of a stream"""
    index, out, at = m.unit_index(), {}, 0
    for (ch, lv, sb, lsb, sg, bits) in tm.parse_stream(stream):
        n = tm.unit_len(bits)
        out[index[(ch, lv, sb, lsb, sg)]] = stream[at: at + n]
        at += n
    return out


def roi_streams(m: tm.Model, lossless: bytes, roi, shift: int, quotas):
    """the ROI streams of a frame whose lossless stream is `lossless` (every unit has a packet there), one per quota.
    Returns ([(stream, rc, K)], foreground units)"""
    packets = split_stream(m, lossless)
    assert len(packets) == m.n_units, "the lossless stream holds every unit's packet"
    bits = [int.from_bytes(packets[k][16:20], "little") for k in range(m.n_units)]        # (the header's payload bit count)
    forder = final_order(m)
    rank, order, n_fg = roi_order(m, roi, shift)
    out = []
    for quota in quotas:
        _, size, rc, K, _ = scan(bits, forder, rank, order, int(quota))
        stream = b"".join(packets[u] for u in forder if rank[u] < K)
        assert len(stream) == size
        out.append((stream, rc, K))
    return out, n_fg


def roi_stream(m: tm.Model, lossless: bytes, roi, shift: int, quota: int):
    """one quota of roi_streams: (stream, rc, K, foreground units)"""
    (res,), n_fg = roi_streams(m, lossless, roi, shift, [quota])
    return res + (n_fg,)


def kept_planes_are_top_runs(m: tm.Model, stream: bytes) -> bool:
    """in every family that has a packet in `stream` the kept planes are P - 1, P - 2, ... without a hole"""
    planes = {}
    for (ch, lv, sb, lsb, sg, _) in tm.parse_stream(stream):
        planes.setdefault((ch, lv, sb, sg), set()).add(lsb)
    return all(p == set(range(m.P - len(p), m.P)) for p in planes.values())
