"""The definition of the decoder's reconstruction option (include/icer_hip_dec.h, "Reconstructing truncated coefficients inside
their interval") in plain numpy, with no product code: expected(orc, stream, k, ...) is what a decoder set to k eighths must
deliver.  Shared by tests/test_recon_model.py, test_recon_mock.py and test_gpu_recon.py.

    decode the stream with the decoder oracle; undo the finishing and the inverse transform to recover the sign-magnitude words;
    find each chain's p from the packets the decoder's walk accepts (tests/reduced_model.walk) and the segment grid
    (orc.partition); add off(p, k) to every non-zero magnitude; transform back and finish.

The inverse transform is restated here (inverse_lines: the reference's inverse lifting, icer_wavelet.c:467-550 and its int8 twin
:298-383, vectorised across lines) together with its undo (undo_lines: the same steps in reverse order).  The forward transform
is NOT used to recover coefficients: the reference's forward and inverse are not mutual inverses for filter C.

FILTER C.  Its inverse step for the second high of a line reads that value ITSELF before updating it (the reference's offset
slip, icer_wavelet.c:489-492): new = old + floor((K - 2 * old) / 8).  That map is onto but not one-to-one -- of four consecutive
`old` one pair shares its `new` -- so no exact undo of filter C's inverse exists.  undo_lines returns the smaller pre-image there
(inverse after undo is still the identity; undo after inverse is not).  The entropy stage does not know the filter, so
expected() recovers the words of a filter-C stream from the oracle's decode of the SAME stream with filter A, whose undo is
exact, and transforms them with filter C.  Every use asserts first that the k = 0 result equals the oracle's own image with the
stream's filter; that assertion fails if a pixel was clamped at zero or a word could not be recovered, so test inputs are chosen
with nothing clamped and nothing overflowing."""
import functools

import numpy as np

from tests import reduced_model as rm
from tests.decoder_batch_cases import oracle_decode

# alpha_-1, alpha_0, alpha_1, beta in sixteenths for filters A, B, C, D, E, F, Q (icer_config.c:18-24)
FILT = ((0, 4, 4, 0), (0, 4, 6, 4), (-1, 4, 8, 6), (0, 4, 5, 2), (0, 3, 8, 6), (0, 3, 9, 8), (0, 4, 4, 4))
MAX_STAGES, MAX_SEGMENTS, MAX_PLANES = 6, 32, 9
EXACT_UNDO = tuple(f[0] == 0 for f in FILT)


def off(p, k):
    """what a non-zero magnitude with p missing planes gains at k eighths"""
    return (k * ((1 << p) - 1)) >> 3


def dim_low(n, lv):
    return (n + (1 << lv) - 1) >> lv


def dim_high(n, lv):
    return dim_low(n, lv - 1) // 2


def trunc(v, bits):
    """wrap to the signed sample width, as the reference's stores do"""
    half = 1 << (bits - 1)
    return ((v + half) & ((1 << bits) - 1)) - half


# ------------------------------------------------------------------------------------------ the interleave, as a permutation
def _find_k(length):
    """icer_find_k (icer_wavelet.c:823-847), in its uint8 arithmetic"""
    lo, hi, res = 0, 11, 0
    while lo < hi:
        mid = (hi + lo) // 2
        s = 3 ** mid + 1
        if length > s:
            lo, res = mid + 1, mid
        elif length < s:
            hi = (mid - 1) & 0xFF
        else:
            break
    return res


@functools.lru_cache(maxsize=None)
def interleave_order(n, bits):
    """icer_interleave_uint16 / _uint8 (icer_wavelet.c:705-763 / :570-628) followed on an index list: entry i = the position in
    the [lows | highs] layout of the value that ends up at i.  (The uint8 routine rotates with another bound on odd lengths.)"""
    a = list(range(n))
    odd = n & 1
    m = n - odd
    if odd:
        t = a[m // 2]
        a[m // 2: m] = a[m // 2 + 1: m + 1]
        a[n - 1] = t

    def rev(i, j):
        while i < j:
            a[i], a[j] = a[j], a[i]
            i, j = i + 1, j - 1
    done = 0
    while done < m:
        seg = 3 ** _find_k(m - done) + 1
        half, left = seg // 2, m - done
        halfleft = left // 2 - (0 if (bits == 8 and odd) else 1)
        rev(done + half, done + halfleft + half)
        rev(done + half, done + seg - 1)
        rev(done + seg, done + halfleft + half)
        i = 1
        while i < seg:
            j, carry = i, a[done + i]
            while True:
                j = 2 * j if j < half else (j - half) * 2 + 1
                a[done + j], carry = carry, a[done + j]
                if j == i:
                    break
            i *= 3
        done += seg
    assert sorted(a) == list(range(n))
    return np.asarray(a, np.int64)


# ------------------------------------------------------------------------------------------ one level along axis 0
def _adds(lo, hi, k, filt, nl, nh, odd):
    """what the inverse step adds to high k of every line: from the lows, and the highs as they stand"""
    am1, a0, a1, be = FILT[filt]

    def R(i):
        return trunc(lo[i - 1] - lo[i], 16)
    if k == 0:
        return R(1) // 4
    if k == 1 and am1 != 0:
        x = 0 if (odd and nl == 3) else hi[1]
        return (2 * R(1) + 3 * R(2) - 2 * x + 4) // 8
    if not odd and k == nh - 1:
        return R(nh - 1) // 4
    rm_ = R(k - 1) if k >= 2 else 1
    dn = 0 if (odd and k + 1 == nl - 1) else hi[k + 1]
    return (am1 * rm_ + a0 * R(k) + a1 * R(k + 1) - be * dn + 8) // 16


def inverse_lines(a, filt, bits):
    """icer_inverse_wavelet_transform_1d_* on every column of a (n, lines) integer array: [lows | highs] -> samples"""
    a = np.asarray(a, np.int64)
    n = a.shape[0]
    assert n >= 5, "the decoder never transforms a shorter line"
    nl, nh, odd = (n + 1) // 2, n // 2, n & 1
    lo, hi = a[:nl].copy(), a[nl:].copy()
    for k in range(nh - 1, -1, -1):
        hi[k] = trunc(hi[k] + _adds(lo, hi, k, filt, nl, nh, odd), bits)
    v = np.empty_like(a)
    s = lo[:nh] + (hi + 1) // 2
    v[:nh] = trunc(s, bits)
    v[nl:] = trunc(s - hi, bits)
    if odd:
        v[nl - 1] = lo[nl - 1]
    return v[interleave_order(n, bits)]


def undo_lines(out, filt, bits):
    """the steps of inverse_lines in reverse order: samples -> [lows | highs].  Exact for every filter but C (see the module's
    docstring): there the second high of a line is the smaller of its pre-images."""
    out = np.asarray(out, np.int64)
    n = out.shape[0]
    assert n >= 5
    nl, nh, odd = (n + 1) // 2, n // 2, n & 1
    v = np.empty_like(out)
    v[interleave_order(n, bits)] = out
    hi = trunc(v[:nh] - v[nl:], bits)
    lo = np.empty((nl,) + out.shape[1:], np.int64)
    lo[:nh] = trunc(v[:nh] - (hi + 1) // 2, bits)
    if odd:
        lo[nl - 1] = v[nl - 1]
    for k in range(nh):
        if k == 1 and FILT[filt][0] != 0 and not (odd and nl == 3):
            # new = trunc(old + floor((K - 2 old) / 8)): rises by 1, 1, 1, 0 with old -- search the few candidates around
            def R(i):
                return trunc(lo[i - 1] - lo[i], 16)
            K = 2 * R(1) + 3 * R(2) + 4
            new, top = hi[1].copy(), 1 << (bits - 1)
            found = np.zeros(new.shape, bool)
            old = np.zeros_like(new)
            for wrap in (0, -1, 1):                              # (the store may have wrapped: new + wrap * 2^bits before it)
                target = new + wrap * 2 * top
                guess = (8 * target - K) // 6                    # (old + (K - 2 old) / 8 = target, without the floor)
                for d in range(-4, 5):
                    c = guess + d
                    hit = ~found & (c >= -top) & (c < top) & (c + (K - 2 * c) // 8 == target)
                    old[hit] = c[hit]
                    found |= hit
            assert found.all()
            hi[1] = old
            continue
        hi[k] = trunc(hi[k] - _adds(lo, hi, k, filt, nl, nh, odd), bits)
    return np.concatenate([lo, hi])


# ------------------------------------------------------------------------------------------ all stages
def inverse_stages(s, stages, filt, bits):
    """icer_inverse_wavelet_transform_stages_* on an (h, w) array of signed samples: deepest level first, the columns of the
    level's region, then its rows; nothing when the deepest LL is thinner than 3 (ICER_TOO_MANY_STAGES, ignored by the decoder)"""
    s = np.array(s, np.int64)
    h, w = s.shape
    if dim_low(w, stages) < 3 or dim_low(h, stages) < 3:
        return s
    for it in range(1, stages + 1):
        cw, ch = dim_low(w, stages - it), dim_low(h, stages - it)
        s[:ch, :cw] = inverse_lines(s[:ch, :cw], filt, bits)
        s[:ch, :cw] = inverse_lines(s[:ch, :cw].T, filt, bits).T
    return s


def undo_stages(s, stages, filt, bits):
    s = np.array(s, np.int64)
    h, w = s.shape
    if dim_low(w, stages) < 3 or dim_low(h, stages) < 3:
        return s
    for it in range(stages, 0, -1):
        cw, ch = dim_low(w, stages - it), dim_low(h, stages - it)
        s[:ch, :cw] = undo_lines(s[:ch, :cw].T, filt, bits).T
        s[:ch, :cw] = undo_lines(s[:ch, :cw], filt, bits)
    return s


# ------------------------------------------------------------------------------------------ the finishing and its undo
def finish(words, mean, stages, filt, bits):
    """sign-magnitude words (h, w) -> the decoded plane: sign-magnitude removal, the LL mean modulo the sample width, the
    inverse transform, negative samples to zero (icer_compress.c:519-535); unsigned samples of the width"""
    sign_bit = bits - 1
    words = np.asarray(words, np.int64)
    mag = words & ((1 << sign_bit) - 1)
    s = np.where((words >> sign_bit) & 1, -mag, mag)
    h, w = s.shape
    llh, llw = dim_low(h, stages), dim_low(w, stages)
    s[:llh, :llw] = trunc(s[:llh, :llw] + trunc(mean, bits), bits)
    s = inverse_stages(s, stages, filt, bits)
    return np.maximum(s, 0).astype(np.uint16 if bits == 16 else np.uint8)


def unfinish(plane, mean, stages, filt, bits):
    """a decoded plane (h, w) in which nothing was clamped -> its sign-magnitude words (zero magnitudes without a sign)"""
    sign_bit = bits - 1
    s = trunc(np.asarray(plane, np.int64), bits)
    s = undo_stages(s, stages, filt, bits)
    h, w = s.shape
    llh, llw = dim_low(h, stages), dim_low(w, stages)
    s[:llh, :llw] = trunc(s[:llh, :llw] - trunc(mean, bits), bits)
    return np.where(s < 0, (1 << sign_bit) | ((-s) & ((1 << sign_bit) - 1)), s)


# ------------------------------------------------------------------------------------------ the chains and their p
def rects_of(orc, sw, sh, segments):
    """the segment rectangles of a sw x sh subband in coding order (icer_partition.c:299-385): the top region row by row, then
    the bottom region; None when the grid cannot be made"""
    rc, q = orc.partition(sw, sh, segments)
    if rc != 0:
        return None
    _, _, r, c, r_t, _, x_t, c_t0, y_t, r_t0, x_b, c_b0, y_b, r_b0, _ = q
    out, y = [], 0
    for rows, cols, xs, c0, ys, r0 in ((r_t, c, x_t, c_t0, y_t, r_t0), (r - r_t, c + 1, x_b, c_b0, y_b, r_b0)):
        for row in range(rows):
            hh, x = ys + (1 if row >= r0 else 0), 0
            for col in range(cols):
                ww = xs + (1 if col >= c0 else 0)
                out.append((x, y, ww, hh))
                x += ww
            y += hh
    return out


def chains(orc, stream, channels, stages, segments, bits, w, h):
    """[(channel, x, y, w, h, p, level)] of every chain a decoder runs on the stream, in image coordinates, and the channels' LL means.
    The packet table as the decoder fills it: the accepted packets in stream order, the last of a kind wins."""
    planes = 9 if bits == 16 else 7
    stream = bytes(stream)
    table, mean = {}, [0, 0, 0]
    for o, _ in rm.walk(stream):
        hd = stream[o: o + rm.HEADER]
        lv, sb, sg, lsb, ch = hd[4], hd[5], hd[6], hd[7] & 15, (hd[7] >> 4 if channels == 3 else 0)
        if lv <= MAX_STAGES and sb < 4 and sg <= MAX_SEGMENTS and lsb < MAX_PLANES and ch < 3:
            table[(ch, lv, sb, sg, lsb)] = o
        if ch < 3:
            mean[ch] = hd[2] | hd[3] << 8
    out = []
    for lv in range(1, stages + 1):
        for ch in range(channels):
            for sb in range(0 if lv == stages else 1, 4):
                lw, lh, hw, hh = dim_low(w, lv), dim_low(h, lv), dim_high(w, lv), dim_high(h, lv)
                sw, sh, ox, oy = ((lw, lh, 0, 0), (hw, lh, lw, 0), (lw, hh, 0, lh), (hw, hh, lw, lh))[sb]
                rects = rects_of(orc, sw, sh, segments)
                assert rects is not None, "a frame that reaches the transform has every grid"
                for sg, (x, y, rw, rh) in enumerate(rects[: MAX_SEGMENTS + 1]):
                    t = 0
                    while t < planes and (ch, lv, sb, sg, planes - 1 - t) in table:
                        t += 1
                    if t:
                        out.append((ch, ox + x, oy + y, rw, rh, planes - t, lv))
    return out, mean


def reconstruct(words, chain_list, k, bits):
    """the rule, on the words of every channel (a list of (h, w) arrays): in place"""
    mask = (1 << (bits - 1)) - 1
    for ch, x, y, rw, rh, p, _ in chain_list:
        o = off(p, k)
        if o:
            view = words[ch][y: y + rh, x: x + rw]
            view[(view & mask) != 0] += o
    return words


# ------------------------------------------------------------------------------------------ the model
def expected(orc, stream, k, channels, stages, filt, segments, bufsize, bits=16, w0=0, h0=0):
    """(rc, w, h, planes) of a decoder set to k eighths: flat planes of bufsize samples, as decoder_batch_cases.oracle_decode
    gives them.  A frame that does not reach the transform (rc != 0), or holds no sample, is the oracle's result as it is."""
    res = oracle_decode(orc, stream, channels, stages, filt, segments, bufsize, bits, w0, h0)
    rc, w, h, planes = res
    if rc != 0 or w * h == 0:
        return res
    # the words: from the stream's own filter where its undo is exact, else from the decode with filter A (module docstring)
    wf = filt if EXACT_UNDO[filt] else 0
    src = planes if wf == filt else oracle_decode(orc, stream, channels, stages, wf, segments, bufsize, bits, w0, h0)[3]
    chain_list, mean = chains(orc, stream, channels, stages, segments, bits, w, h)
    words = [unfinish(src[c][: w * h].reshape(h, w), mean[c], stages, wf, bits) for c in range(channels)]
    for c in range(channels):
        same = finish(words[c], mean[c], stages, filt, bits)
        assert np.array_equal(same.reshape(-1), planes[c][: w * h]), f"the model at k = 0 is not the oracle's image (channel {c}, filter {filt})"
    if k == 0:
        return res
    reconstruct(words, chain_list, k, bits)
    out = []
    for c in range(channels):
        p = np.zeros(max(bufsize, 1), planes[c].dtype)
        p[: w * h] = finish(words[c], mean[c], stages, filt, bits).reshape(-1)
        out.append(p)
    return rc, w, h, out


def expected_reduced(orc, stream, k, r, channels, stages, filt, segments, bufsize, bits=16, w0=0, h0=0):
    """a reduced decoder (stages, reduce = r) set to k: the rule on the derived stream at stages - r"""
    return expected(orc, rm.derive(stream, r), k, channels, stages - r, filt, segments, bufsize, bits, w0, h0)


def missing_planes(orc, stream, channels, stages, segments, bits=16):
    """(level, p) of every chain of a stream (test helper: is a case lossy where it should be?)"""
    hd = next(iter(rm.walk(stream)), None)
    if hd is None:
        return []
    o = hd[0]
    w, h = int.from_bytes(stream[o + 8: o + 12], "little"), int.from_bytes(stream[o + 12: o + 16], "little")
    return [(c[6], c[5]) for c in chains(orc, stream, channels, stages, segments, bits, w, h)[0]]
