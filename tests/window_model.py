"""The definition of the window decode (include/icer_hip_dec_window.h) in plain Python, written independently of the C++:
  - the window image is the crop of what the plain call of the same decoder delivers (clip / expected);
  - the needed-rectangle rule and the chain counts (axis / levels / chain_table / kept);
  - strip(): a stream without the packets of the chains the rule drops -- what test_window_model.py decodes with the oracle
    to show that the rule is sufficient.
Shared by tests/test_window_model.py, test_window_plan_device.py, test_window_mock.py and test_gpu_window.py."""
from tests import reduced_model as rm
from tests.display_model import display_of
from tests.recon_model import MAX_PLANES, MAX_SEGMENTS, MAX_STAGES, dim_high, dim_low, rects_of

QUOTA = -5
PAIRWISE = (True, False, False, False, False, False, False)          # filter A: beta = 0 and alpha_-1 = 0


def clip(win, w, h):
    """(x0, y0, ww, wh) of the window clipped to a w x h image; an empty one has ww = wh = 0"""
    x, y, ww, wh = (int(v) for v in win)
    x0, y0 = min(x, w), min(y, h)
    ww, wh = min(ww, w - x0), min(wh, h - y0)
    return (x0, y0, 0, 0) if ww == 0 or wh == 0 else (x0, y0, ww, wh)


def axis(n, a, b, pairwise, bits):
    """a line of n stored samples, restored samples [a, b) wanted -> (lows [lo0, lo1), highs [hi0, hi1)) needed"""
    nl, nh = (n + 1) // 2, n // 2
    if a >= b:
        return (0, 0), (0, 0)
    if n < 8 or (bits == 8 and n % 2):
        return (0, nl), (0, nh)
    ka, kb = a >> 1, (b - 1) >> 1
    if pairwise:
        hi = (ka, min(kb, nh - 1) + 1)
        lo = (max(ka - 1, 0), min(kb + 1, nl - 1) + 1)
    else:
        hi = (ka, nh)
        lo = (max(ka - 2, 0), nl)
    return lo, ((hi[0], hi[1]) if hi[0] < hi[1] else (0, 0))


def levels(w, h, stages, win, filt, bits):
    """per level 1 .. stages: ((lows x, highs x), (lows y, highs y)) needed for the clipped window `win` of a w x h image"""
    x0, y0, ww, wh = win
    X, Y, out = (x0, x0 + ww), (y0, y0 + wh), []
    for lv in range(1, stages + 1):
        ax = axis(dim_low(w, lv - 1), X[0], X[1], PAIRWISE[filt], bits)
        ay = axis(dim_low(h, lv - 1), Y[0], Y[1], PAIRWISE[filt], bits)
        out.append((ax, ay))
        X, Y = ax[0], ay[0]
    return out


def chain_table(orc, stream, channels, stages, segments, bits, w, h):
    """[(channel, level, subband, segment, (x, y, w, h) inside the subband)] of every chain the plain call runs on a frame that
    reaches the transform, in the planner's order; the packet table as the decoder fills it"""
    planes = 9 if bits == 16 else 7
    stream = bytes(stream)
    table = set()
    for o, _ in rm.walk(stream):
        hd = stream[o: o + rm.HEADER]
        lv, sb, sg, lsb, ch = hd[4], hd[5], hd[6], hd[7] & 15, (hd[7] >> 4 if channels == 3 else 0)
        if lv <= MAX_STAGES and sb < 4 and sg <= MAX_SEGMENTS and lsb < MAX_PLANES and ch < 3:
            table.add((ch, lv, sb, sg, lsb))
    out = []
    for lv in range(1, stages + 1):
        for ch in range(channels):
            for sb in range(0 if lv == stages else 1, 4):
                lw, lh, hw, hh = dim_low(w, lv), dim_low(h, lv), dim_high(w, lv), dim_high(h, lv)
                rects = rects_of(orc, *((lw, lh), (hw, lh), (lw, hh), (hw, hh))[sb], segments)
                assert rects is not None
                out += [(ch, lv, sb, sg, r) for sg, r in enumerate(rects[: MAX_SEGMENTS + 1]) if (ch, lv, sb, sg, planes - 1) in table]
    return out


def meets(rect, xr, yr):
    x, y, rw, rh = rect
    return x < xr[1] and x + rw > xr[0] and y < yr[1] and y + rh > yr[0]


def kept(chain_list, w, h, stages, win, filt, bits):
    """the chains of chain_list that the clipped window `win` depends on"""
    need = levels(w, h, stages, win, filt, bits)
    out = []
    for c in chain_list:
        ch, lv, sb, sg, rect = c
        (lox, hix), (loy, hiy) = need[lv - 1]
        if meets(rect, hix if sb & 1 else lox, hiy if sb & 2 else loy):
            out.append(c)
    return out


def transformed(rc, w, h, stages):
    """the frame reaches the transform and the transform has levels: the window restricts its chains"""
    return rc == 0 and w * h > 0 and dim_low(w, stages) >= 3 and dim_low(h, stages) >= 3


def strip(stream, keep, channels):
    """the accepted packets of `stream` whose chain (channel, level, subband, segment) is in `keep`, in stream order"""
    stream = bytes(stream)
    ids = {c[:4] for c in keep}
    out = []
    for o, n in rm.walk(stream):
        hd = stream[o: o + rm.HEADER]
        if ((hd[7] >> 4) if channels == 3 else 0, hd[4], hd[5], hd[6]) in ids:
            out.append(stream[o: o + n])
    return b"".join(out)


def delivered(rc, w, h, full_stride):
    """the plain call delivers samples for this frame"""
    return not (rc in (-11, -4, QUOTA) or w * h == 0 or w * h > full_stride)


def expected(orc, want, win, frame_stride, full_stride, channels, stages, filt, segments, bits, stream, display=False):
    """want = (rc, w, h, flat planes) of the plain call (the decoder oracle's, or a model's of it) for `stream` ->
    (rc, (x0, y0, ww, wh), window, chains run, chains of the plain call): window = None when nothing is written, else a list
    of (wh, ww) planes, or for display the (wh, ww) / (wh, ww, 3) uint8 image; the counts are None for a frame that keeps all
    its chains (how many those are is the plain planner's business)"""
    rc, w, h, planes = want
    if not delivered(rc, w, h, full_stride):
        return rc, (0, 0, 0, 0), None, 0, 0
    c = clip(win, w, h)
    x0, y0, ww, wh = c
    if transformed(rc, w, h, stages):
        table = chain_table(orc, stream, channels, stages, segments, bits, w, h)
        full, run = len(table), len(kept(table, w, h, stages, c, filt, bits))
    else:
        full = run = None
    if ww * wh > frame_stride:
        return QUOTA, c, None, 0, full
    if ww * wh == 0:
        return rc, c, None, run, full
    crop = [p[: w * h].reshape(h, w)[y0: y0 + wh, x0: x0 + ww] for p in planes]
    if display:
        return rc, c, display_of([p.reshape(-1) for p in crop], channels).reshape((wh, ww) if channels == 1 else (wh, ww, 3)), run, full
    return rc, c, crop, run, full


def windows_for(w, h):
    """the windows a w x h image is tried with: interior, each edge and corner, a single pixel, the whole image, straddling the
    border, wholly outside"""
    a, b = max(w // 4, 1), max(h // 4, 1)
    return [(w // 3, h // 3, a, b), (0, h // 3, a, b), (w - a, h // 3, a, b), (w // 3, 0, a, b), (w // 3, h - b, a, b),
            (0, 0, a, b), (w - a, 0, a, b), (0, h - b, a, b), (w - a, h - b, a, b), (w // 2 + 1, h // 2 - 1, 1, 1), (w - 1, h - 1, 1, 1),
            (0, 0, w, h), (w - a // 2 - 1, h - b // 2 - 1, a, b), (w + 3, 2, 5, 5), (1, h, 4, 4)]
