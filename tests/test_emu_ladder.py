"""Rate ladder assembly (csrc/assemble_ladder.hpp): scan_ladder_wave and copy_unit_ladder, built for the CPU from the kernel
source (tests/emu/ladder_emu.cpp), give per quota what scan_kernel's scan_frame_wave and one plain copy per quota give --
final offsets, stream sizes, return codes, the slot-bound flag and every destination byte -- on seeded random frames: unit
bit counts of 0, kUnitTooBig and kUnitFailed among them, shuffled final orders, quotas around one packet header (0, 27, 28,
29), quotas on which a prefix of the stream ends exactly, repeated quotas, and destination rows at every byte alignment."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = 28
TOO_BIG, FAILED = 0xFFFFFFFF, 0xFFFFFFFE
NONE = 0xFFFFFFFFFFFFFFFF
SENT = 0xA5

u8p = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")
u32p = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")
u64p = np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS")
i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")


def _lib():
    src = os.path.join(ROOT, "tests", "emu", "ladder_emu.cpp")
    so = os.path.join(ROOT, "tests", "emu", "libladder_emu.so")
    csrc = os.path.join(ROOT, "icer_compression_amd", "csrc")
    newest = max([os.path.getmtime(os.path.join(csrc, f)) for f in os.listdir(csrc)] + [os.path.getmtime(src)])
    if not os.path.exists(so) or os.path.getmtime(so) < newest:
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", so, src])
    L = C.CDLL(so)
    L.emu_scan_frame.restype = C.c_int
    L.emu_scan_frame.argtypes = [u32p, u32p, C.c_uint32, C.c_uint64, u64p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    L.emu_scan_ladder.restype = C.c_uint32
    L.emu_scan_ladder.argtypes = [u32p, u32p, C.c_uint32, u64p, C.c_uint32, C.c_int, u8p, u64p, u64p, i32p]
    L.emu_copy_unit.restype = None
    L.emu_copy_unit.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_size_t, C.c_uint32]
    return L


def unit_len(b):
    return HEADER + (int(b) + 7) // 8


def random_frame(rng, n):
    """bit counts in priority order: mostly coded units of a few bytes to a few KiB, some empty, some that outgrew their slot"""
    bits = rng.integers(1, 40000, n).astype(np.uint32)
    bits[rng.random(n) < 0.15] = 0
    bits[rng.random(n) < 0.1] = TOO_BIG
    return bits


def quota_set(rng, bits, n_q):
    """0, 27, 28, 29, quotas on which a kept prefix ends exactly (and one byte either side), a unit's own boundary, random
    ones, a repeat"""
    prefix = np.cumsum([0] + [unit_len(b) for b in bits if b != TOO_BIG][: len(bits)])
    cands = [0, 27, 28, 29]
    for k in rng.choice(len(prefix), size=min(4, len(prefix)), replace=False):
        cands += [int(prefix[k]) - 1, int(prefix[k]), int(prefix[k]) + 1]
    for k in rng.choice(len(bits), size=min(3, len(bits)), replace=False):       # used + 28 + floor(bits / 8): the unit just fails
        if bits[k] not in (TOO_BIG, FAILED):
            used = int(sum(unit_len(b) for b in bits[:k] if b not in (TOO_BIG, FAILED)))
            cands += [used + HEADER + int(bits[k]) // 8, used + HEADER + int(bits[k]) // 8 + 1]
    cands += [int(x) for x in rng.integers(0, int(prefix[-1]) + 100, 4)] + [int(prefix[-1]) + 10 ** 6]
    qs = [max(0, c) for c in rng.choice(cands, size=n_q - 1, replace=True)]
    qs.append(qs[int(rng.integers(0, len(qs)))] if qs else 28)                    # a duplicate
    rng.shuffle(qs)
    return np.array(qs, np.uint64)


def expected_scan(L, bits, order, quotas, skip, bound):
    """scan_kernel's result per quota: scan_frame_wave unless the frame was skipped or has a failed unit"""
    n = len(bits)
    foff = np.full((len(quotas), n), NONE, np.uint64)
    sizes, rcs, flags = np.zeros(len(quotas), np.uint64), np.zeros(len(quotas), np.int32), 0
    for q, quota in enumerate(quotas):
        if skip:
            rcs[q] = -1
        elif (bits == FAILED).any():
            rcs[q], flags = -10, flags | 2
        else:
            kept, used = C.c_uint32(), C.c_uint64()
            row = np.empty(n, np.uint64)
            rcs[q] = L.emu_scan_frame(bits, order, n, int(quota), row, C.byref(kept), C.byref(used))
            foff[q], sizes[q] = row, used.value
            if kept.value < n and bits[kept.value] == TOO_BIG and bound[kept.value]:
                flags |= 1
    return foff, sizes, rcs, flags


def test_ladder_scan_equals_one_scan_per_quota():
    L = _lib()
    rng = np.random.default_rng(20261016)
    seen = {"bound_flag": 0, "failed": 0, "skip": 0, "cut": 0, "all_kept": 0, "nothing": 0}
    for case in range(400):
        n = int(rng.integers(1, 200))
        bits = random_frame(rng, n)
        skip = int(case % 23 == 5)
        if case % 17 == 3:
            bits[int(rng.integers(0, n))] = FAILED
        order = rng.permutation(n).astype(np.uint32)
        bound = (rng.random(n) < 0.5).astype(np.uint8)
        n_q = int(rng.integers(1, 17))
        quotas = quota_set(rng, bits, n_q)
        foff = np.full(n_q * n, 7, np.uint64)
        sizes, rcs = np.full(n_q, 7, np.uint64), np.full(n_q, 7, np.int32)
        flags = L.emu_scan_ladder(bits, order, n, quotas, n_q, skip, bound, foff, sizes, rcs)
        wf, ws, wr, wflags = expected_scan(L, bits, order, quotas, skip, bound)
        assert np.array_equal(foff.reshape(n_q, n), wf), case
        assert np.array_equal(sizes, ws) and np.array_equal(rcs, wr), (case, sizes, ws, rcs, wr)
        assert flags == wflags, (case, flags, wflags)
        seen["bound_flag"] += wflags == 1
        seen["failed"] += bool(wflags & 2)
        seen["skip"] += skip
        seen["cut"] += int((wr == -5).sum())
        seen["all_kept"] += int((wr == 0).sum())
        seen["nothing"] += int(((ws == 0) & (wr == -5)).sum())
    assert all(v >= 5 for v in seen.values()), seen


def test_ladder_copy_equals_one_copy_per_quota():
    """every kept unit at its offset in every quota's row (rows of odd stride: every byte alignment), nothing else written"""
    L = _lib()
    rng = np.random.default_rng(7)
    for case in range(60):
        n = int(rng.integers(1, 60))
        bits = random_frame(rng, n)
        small = rng.random(n) < 0.4                                          # units of a few bytes: many per stream, all lengths mod 4
        bits[small] = rng.integers(0, 200, int(small.sum()))
        order = rng.permutation(n).astype(np.uint32)
        n_q = int(rng.integers(1, 17))
        quotas = quota_set(rng, bits, n_q)
        foff = np.empty(n_q * n, np.uint64)
        sizes, rcs = np.empty(n_q, np.uint64), np.empty(n_q, np.int32)
        L.emu_scan_ladder(bits, order, n, quotas, n_q, 0, np.zeros(n, np.uint8), foff, sizes, rcs)
        # slots: each unit's words at a 4-byte aligned offset, random content
        lens = [unit_len(b) if b != TOO_BIG else 0 for b in bits]
        slot_off = np.cumsum([0] + [(x + 3) // 4 * 4 + 4 * int(rng.integers(0, 3)) for x in lens])
        slots = rng.integers(0, 256, int(slot_off[-1]) + 16).astype(np.uint8)
        stride = int(sizes.max()) + 1 + 2 * int(rng.integers(0, 3))        # odd or even, rows start at every alignment
        if stride % 2 == 0:
            stride += 1
        base = case % 4
        buf = np.full(base + n_q * stride + 8, SENT, np.uint8)
        want = buf.copy()
        for u in range(n):
            offs = foff.reshape(n_q, n)[:, u]
            for q in range(n_q):
                if offs[q] != NONE:
                    o = base + q * stride + int(offs[q])
                    want[o: o + lens[u]] = slots[slot_off[u]: slot_off[u] + lens[u]]
            if (offs != NONE).any():
                nth = (256, 64, 3, 1)[(case + u) % 4]
                L.emu_copy_unit(slots.ctypes.data + int(slot_off[u]), lens[u], foff.ctypes.data + 8 * u, n, n_q, buf.ctypes.data + base,
                                stride, nth)
        assert np.array_equal(buf, want), (case, np.argwhere(buf != want)[:4].ravel().tolist())
        for q in range(n_q):                                                   # each row is the stream scan_frame_wave laid out
            row = buf[base + q * stride: base + q * stride + int(sizes[q])]
            offs = foff.reshape(n_q, n)[q]
            kept = [int(order[j]) for j in range(n) if offs[order[j]] != NONE]
            assert row.tobytes() == b"".join(slots[slot_off[u]: slot_off[u] + lens[u]].tobytes() for u in kept), (case, q)
