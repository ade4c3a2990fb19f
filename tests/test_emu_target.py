"""The distortion target on a CPU (csrc/distortion_core.hpp built from tests/emu/distortion_emu.cpp): the families' residual
energies against numpy under launch-order and random wave schedules, scan_target_wave against a plain Python walk
(tests/target_model.py) with its equivalent quota fed back to scan_frame_wave, the committed subband weights against a
regeneration, and the distortion estimate against what the oracle's decoder actually leaves."""
import ctypes as C
import importlib.util
import os
import subprocess

import numpy as np
import pytest

from tests import encoder_batch_cases as ebc
from tests import target_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOO_BIG, FAILED, NONE = tm.TOO_BIG, tm.FAILED, tm.NONE

# The accuracy include/icer_hip.h states for D / 16 as an estimate of the decoded image's squared error: the worst
# |10 log10(estimate / actual)| that test_estimate_against_oracle_decode measures (profiles/quality_target.md), rounded up to the
# next 0.5 dB.
STATED_ACCURACY_DB = 6.0

u8p = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")
u16p = np.ctypeslib.ndpointer(dtype=np.uint16, flags="C_CONTIGUOUS")
u32p = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")
u64p = np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    src = os.path.join(ROOT, "tests", "emu", "distortion_emu.cpp")
    so = str(tmp_path_factory.mktemp("dist") / "libdistortion_emu.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-o", so, src])
    L = C.CDLL(so)
    L.emu_family_energy.restype = C.c_uint32
    L.emu_family_energy.argtypes = [u16p, C.c_uint32, u32p, C.c_uint32, C.c_uint32, C.c_uint32, u64p]
    L.emu_scan_frame.restype = C.c_int
    L.emu_scan_frame.argtypes = [u32p, u32p, C.c_uint32, C.c_uint64, u64p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    L.emu_scan_target.restype = C.c_uint32
    L.emu_scan_target.argtypes = [u32p, u32p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int, u32p, u32p, u8p, u64p, u32p, C.c_uint32, C.c_uint32,
                                  u64p, u32p, u16p, u64p, u64p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.emu_subband_gain.restype = C.c_uint32
    return L


# ---- the energy pass ------------------------------------------------------------------------------------------------------------
def numpy_energy(plane, rect, P):
    x0, y0, w, h = rect
    m = plane[y0: y0 + h, x0: x0 + w].astype(np.uint64) & np.uint64(0x7FFF)
    sent = (1 << P) - 1
    out = []
    for b in range(P + 1):
        r = (m & np.uint64(0x7FFF & ~sent)) | (m & np.uint64(sent & ((1 << b) - 1)))
        out.append(int((r * r).sum(dtype=np.uint64)))
    return out


@pytest.mark.parametrize("P", [9, 7])
def test_energy_pass_equals_numpy(emu, P):
    """rectangles of 1 x 1, 63 x 1, 65 x 3 and 97 x 61 (two workgroups) at odd offsets, one of 150 x 121 (five workgroups), an
    all-zero one; magnitudes with bits at and above P; every wave schedule gives the same table"""
    rng = np.random.default_rng(90 + P)
    H, W = 260, 333
    mag = rng.integers(0, 1 << 15, (H, W))
    small = rng.random((H, W)) < 0.5
    mag[small] = rng.integers(0, 1 << P, int(small.sum()))                 # half of them inside the coded planes
    mag[rng.random((H, W)) < 0.05] = 0x7FFF                                # the largest magnitude
    plane = (mag | (rng.integers(0, 2, (H, W)) << 15)).astype(np.uint16)
    rects = [(7, 3, 1, 1), (11, 5, 63, 1), (101, 9, 65, 3), (3, 15, 97, 61), (131, 81, 150, 121), (5, 211, 40, 33), (301, 1, 1, 200)]
    plane[211: 244, 5: 45] = 0x8000                                        # (an all-zero family: signs only)
    flat = np.array(rects, np.uint32).ravel()
    want = np.array([numpy_energy(plane, r, P) for r in rects], np.uint64)
    assert (want[5] == 0).all() and want[0, P] == int(plane[3, 7] & 0x7FFF) ** 2
    for seed in (0, 1, 2, 77, 20261018):
        E = np.full((len(rects), P + 1), 12345, np.uint64)
        n_wg = emu.emu_family_energy(plane, W, flat, len(rects), P, seed, E)
        assert n_wg == sum((r[2] * r[3] + 4095) // 4096 for r in rects) and n_wg >= 12
        assert np.array_equal(E, want), (seed, np.argwhere(E != want)[:4].tolist())
    # r_b grows with b, and b = P leaves the whole magnitude
    assert (np.diff(want.astype(object), axis=1) >= 0).all()
    assert int(want[4, P]) == int((plane[81: 202, 131: 281].astype(np.int64) & 0x7FFF).__pow__(2).sum())


# ---- the target walk ------------------------------------------------------------------------------------------------------------
def random_frame(rng, P):
    """families of P planes each, their units merged at random into one priority order (a family's planes from the top down);
    bit counts with empty units and units that outgrew their slot; energies that grow with b; weights"""
    n_fam = int(rng.integers(1, 24))
    todo = [list(range(P - 1, -1, -1)) for _ in range(n_fam)]
    fam, lsb = [], []
    while any(todo):
        f = int(rng.choice([i for i, t in enumerate(todo) if t]))
        fam.append(f)
        lsb.append(todo[f].pop(0))
    n = len(fam)
    bits = rng.integers(1, 40000, n).astype(np.uint32)
    bits[rng.random(n) < 0.15] = 0
    bits[rng.random(n) < 0.04] = TOO_BIG
    steps = rng.integers(0, 1 << 36, (n_fam, P + 1)).astype(np.uint64)
    steps[rng.random((n_fam, P + 1)) < 0.3] = 0                             # (planes that change nothing: D_k == D_k+1)
    E = np.cumsum(steps, axis=1, dtype=np.uint64)
    weight = rng.integers(1, 120000, n_fam).astype(np.uint32)
    return np.array(fam, np.uint32), np.array(lsb, np.uint32), bits, E, weight


def test_target_walk_equals_plain_walk(emu):
    rng = np.random.default_rng(20261018)
    P = 9
    seen = {"met": 0, "cap": 0, "tie": 0, "all": 0, "none": 0, "exact": 0, "bound_flag": 0, "too_big_before": 0, "too_big_after": 0,
            "failed": 0, "skip": 0, "empty_at_cut": 0}
    for case in range(500):
        P = 9 if case % 3 else 7
        fam, lsb, bits, E, weight = random_frame(rng, P)
        n, n_fam = len(bits), len(weight)
        skip = int(case % 29 == 7)
        if case % 31 == 11:
            bits[int(rng.integers(0, n))] = FAILED
        order = rng.permutation(n).astype(np.uint32)
        bound = (rng.random(n) < 0.5).astype(np.uint8)
        # the LL means' loss: some families are LL families of one of three channels, some means are above one byte
        chan = rng.integers(0, 3, n_fam).astype(np.uint32)
        ll_term = np.where(rng.random(n_fam) < 0.2, rng.integers(1, 1 << 24, n_fam), 0).astype(np.uint64)
        means = rng.choice([0, 38, 255, 256, 460, 2047, 32767], 3).astype(np.uint16)
        D = [sum(int(weight[f]) * int(E[f, P]) + int(ll_term[f]) * (int(means[chan[f]]) & 0xFF00) ** 2 for f in range(n_fam))]
        for k in range(n):
            D.append(D[-1] - int(weight[fam[k]]) * (int(E[fam[k], lsb[k] + 1]) - int(E[fam[k], lsb[k]])))
        assert D[-1] >= 0 and D[0] < 2 ** 64
        coded = [int(b) for b in bits if b not in (TOO_BIG, FAILED)]
        total = sum(tm.unit_len(b) for b in coded)
        for trial in range(6):
            kx = int(rng.integers(0, n + 1))
            T = [0, D[0], D[0] + 5, D[kx], max(D[kx] - 1, 0), int(rng.integers(0, D[0] + 1, dtype=np.uint64))][trial]
            cap = int(rng.choice([0, 27, 28, total + 10 ** 6, int(rng.integers(0, total + 100)), int(rng.integers(0, total + 100))]))
            foff = np.full(n, 7, np.uint64)
            out = np.full(3, 7, np.uint64)
            rc, reached = C.c_int32(7), C.c_int32(7)
            flags = emu.emu_scan_target(bits, order, n, T, cap, skip, fam, lsb, bound, E, weight, n_fam, P, ll_term, chan, means, foff, out, C.byref(rc),
                                        C.byref(reached))
            size, dist, equiv = (int(x) for x in out)
            if skip or (bits == FAILED).any():
                assert (foff == NONE).all() and size == 0 and rc.value == (-1 if skip else -10), case
                assert (reached.value, dist, equiv) == (0, 0, cap) and flags == (0 if skip else 2), case
                seen["skip" if skip else "failed"] += 1
                continue
            K, used, wrc, wreached, wD, wequiv, by_cap = tm.target_walk(bits, D, T, cap)
            assert (foff != NONE).sum() == K and (foff[:K] != NONE).all(), (case, trial)
            assert (size, rc.value, reached.value, dist, equiv) == (used, wrc, wreached, wD, wequiv), (case, trial, K)
            assert flags == int(by_cap and K < n and bits[K] == TOO_BIG and bound[K]), (case, trial)
            if reached.value:
                assert D[K] <= T and (K == 0 or D[K - 1] > T)
            # the equivalent quota makes this very cut in the plain walk
            row = np.empty(n, np.uint64)
            kept, u2 = C.c_uint32(), C.c_uint64()
            rc2 = emu.emu_scan_frame(bits, order, n, equiv, row, C.byref(kept), C.byref(u2))
            assert (kept.value, u2.value, rc2) == (K, size, rc.value) and np.array_equal(row, foff), (case, trial, K, equiv)
            too_big = np.flatnonzero(bits == TOO_BIG)
            seen["met"] += reached.value and not by_cap
            seen["cap"] += not reached.value
            seen["tie"] += reached.value and by_cap
            seen["all"] += K == n
            seen["none"] += K == 0
            seen["exact"] += trial == 3 and reached.value
            seen["bound_flag"] += flags == 1
            seen["too_big_before"] += bool(len(too_big) and too_big[0] < K)      # (never: the cap stops at the first)
            seen["too_big_after"] += bool(len(too_big) and too_big[0] > K)
            seen["empty_at_cut"] += K < n and bits[K] == 0
    assert seen.pop("too_big_before") == 0
    assert all(v >= 5 for v in seen.values()), seen


# ---- the subband weights --------------------------------------------------------------------------------------------------------
def test_committed_weight_table_is_the_generated_one(emu):
    spec = importlib.util.spec_from_file_location("subband_gain", os.path.join(ROOT, "tools", "subband_gain.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    text = gen.render(gen.table())
    with open(gen.HEADER) as fh:
        assert fh.read() == text, "csrc/subband_gain.hpp is not what tools/subband_gain.py writes"
    w = tm.committed_weights()
    assert w.min() >= 1
    for f in range(7):
        for lv in range(1, 7):
            for sb in range(4):
                assert emu.emu_subband_gain(f, lv, sb) == w[f, lv - 1, sb]


# ---- the estimate against a real decode -----------------------------------------------------------------------------------------
def unit_bits_of(model, stream):
    """payload bits of every unit in priority order, from the packets of a stream that holds them all"""
    where = model.unit_index()
    bits = np.zeros(model.n_units, np.uint32)
    got = tm.parse_stream(stream)
    assert len(got) == model.n_units
    for (ch, lv, sb, lsb, sg, b) in got:
        bits[where[(ch, lv, sb, lsb, sg)]] = b
    return bits


def words16(g, planes):
    """the oracle's planes as the encoder's 16-bit sign-magnitude words"""
    if g.bits == 16:
        return planes
    return [(((p.astype(np.uint16) & 0x80) << 8) | (p & 0x7F)).astype(np.uint16) for p in planes]


def class_cuts(model):
    """the unit counts at which a priority class ends"""
    prio = [u[6] for u in model.units]
    return [k for k in range(1, model.n_units + 1) if k == model.n_units or prio[k] != prio[k - 1]]


def estimate_and_actual(orc, g, spec, model):
    """[(K, D_K / 16, actual squared error)] at one cut per priority class"""
    src = ebc.oracle_planes(g, spec)
    compress = orc.compress_u8 if g.bits == 8 else orc.compress
    big = ebc.quota(g, "lossless")
    rc, full, coef = compress(src, g.stages, g.filt, g.segments, big)
    assert rc == 0
    bits = unit_bits_of(model, full)
    D = model.distortions(model.energy_table(words16(g, coef)), tm.ll_means(orc, src, g.stages, g.filt) if g.bits == 16 else None)
    out = []
    for K in class_cuts(model):
        used = sum(tm.unit_len(b) for b in bits[:K])
        if K == model.n_units:
            equiv, wrc = big, 0
        else:
            equiv, wrc = (used + tm.HEADER + (int(bits[K]) >> 3) if bits[K] else used + tm.HEADER - 1), tm.QUOTA_EXCEEDED
        rc, stream, _ = compress(src, g.stages, g.filt, g.segments, equiv)
        assert rc == wrc and len(stream) == used, (spec, K, rc, wrc, len(stream), used)
        drc, w, h, planes = orc.decompress(stream, g.channels, g.stages, g.filt, g.segments, bits=g.bits)
        assert drc == 0 and (w, h) == (g.w, g.h)
        err = 0
        for s, d in zip(src, planes):
            a = s.astype(np.int8 if g.bits == 8 else np.int64).astype(np.int64).ravel()
            b = d[: g.w * g.h].astype(np.int8 if g.bits == 8 else np.int64).astype(np.int64)
            err += int(((a - b) ** 2).sum())
        out.append((K, D[K] / 16.0, err))
    return out


ESTIMATE_GEOMETRIES = [ebc.Geometry(256, 192, 1, 3, 0, 6), ebc.Geometry(256, 192, 1, 3, 6, 6),
                       ebc.Geometry(128, 96, 3, 3, 0, 5), ebc.Geometry(128, 96, 3, 3, 6, 5)]


@pytest.fixture(scope="module")
def estimate_cases(oracle):
    """[(geometry, kind, K, D_K / 16, actual squared error)] with an actual error of at least 1 per sample"""
    out = []
    for g in ESTIMATE_GEOMETRIES:
        model = tm.Model(g.w, g.h, g.channels, g.stages, g.filt, g.segments, g.bits)
        for kind in ebc.CODED16:
            if kind == "blank":
                continue
            for (K, est, act) in estimate_and_actual(oracle, g, (kind, 0), model):
                if act >= g.samples:
                    out.append((g, kind, K, est, act))
    return out


def test_estimate_against_oracle_decode(estimate_cases):
    """D / 16 against the squared error the oracle's decoder leaves -- filters A and Q, 256 x 192 gray and 128 x 96 YUV, every
    coded kind but blank, one cut per priority class, wherever the actual error is at least 1 per sample -- within the accuracy
    the header states, which is the measured worst case rounded up to 0.5 dB (profiles/quality_target.md has the figures)."""
    worst = (0.0, None)
    for c in estimate_cases:
        db = abs(10 * np.log10(c[3] / c[4])) if c[3] > 0 else float("inf")
        print(f"filter {c[0].filt} {c[0].channels}ch {c[1]}: K {c[2]} estimate {c[3]:.0f} actual {c[4]} -> {db:.3f} dB")
        if db > worst[0]:
            worst = (db, c)
    print("worst:", worst, "cases:", len(estimate_cases))
    assert len(estimate_cases) >= 100
    assert worst[0] <= STATED_ACCURACY_DB, worst
    assert np.ceil(worst[0] * 2) / 2 == STATED_ACCURACY_DB, f"the stated accuracy is not the measured {worst[0]:.3f} dB rounded up to 0.5 dB"


def test_everything_kept_on_8_bit_data_is_exact(oracle):
    """8-bit data has no magnitude bits above the coded planes: with every unit kept the estimate and the decoder's error are both 0"""
    g = ebc.Geometry(256, 192, 1, 3, 0, 6, bits=8)
    model = tm.Model(g.w, g.h, 1, g.stages, g.filt, g.segments, 8)
    for kind in ("noise6", "smooth6"):
        src = ebc.oracle_planes(g, (kind, 0))
        rc, stream, coef = oracle.compress_u8(src, g.stages, g.filt, g.segments, ebc.quota(g, "lossless"))
        assert rc == 0
        D = model.distortions(model.energy_table(words16(g, coef)))
        assert D[-1] == 0 and D[0] > 0
        drc, w, h, planes = oracle.decompress(stream, 1, g.stages, g.filt, g.segments, bits=8)
        assert drc == 0 and np.array_equal(planes[0][: g.w * g.h].reshape(g.h, g.w), src[0])
