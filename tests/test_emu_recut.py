"""Re-cutting stored streams (csrc/recut_core.hpp): the per-frame plan step of recut_plan_kernel (frame status, unit bit counts
out of the packet table, recut_scan_wave per quota) and copy_unit_recut, built for the CPU from the kernel source
(tests/emu/recut_emu.cpp), give per quota what one scan_frame_wave and one plain copy per quota give -- final offsets, stream
sizes, return codes and every destination byte -- on seeded random frames: units missing at random positions, unit lengths of
every value mod 4 (and copies of 0 bytes), sources and destinations at every byte alignment, 256 / 64 / 3 / 1 threads, quotas
around one packet header (0, 27, 28, 29), quotas on, one below and one above a kept prefix's exact end, repeats, 1-16 quotas."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = 28
TOO_BIG = 0xFFFFFFFF
NO_PACKET = 0xFFFFFFFF
NONE = 0xFFFFFFFFFFFFFFFF
SENT = 0xA5
QUOTA_EXCEEDED, OUT_OF_DATA, INVALID_INPUT = -5, -7, -11

u32p = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")
u64p = np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS")
i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")

_LIB = None


def _lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    src = os.path.join(ROOT, "tests", "emu", "recut_emu.cpp")
    so = os.path.join(ROOT, "tests", "emu", "librecut_emu.so")
    csrc = os.path.join(ROOT, "icer_compression_amd", "csrc")
    newest = max([os.path.getmtime(os.path.join(csrc, f)) for f in os.listdir(csrc)] + [os.path.getmtime(src)])
    if not os.path.exists(so) or os.path.getmtime(so) < newest:
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", so, src])
    L = C.CDLL(so)
    L.emu_scan_frame.restype = C.c_int
    L.emu_scan_frame.argtypes = [u32p, u32p, C.c_uint32, C.c_uint64, u64p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    L.emu_recut_plan.restype = C.c_int
    L.emu_recut_plan.argtypes = [C.c_int, C.c_uint32, C.c_int, u32p, u32p, u32p, C.c_uint32, u32p, u64p, C.c_uint32, C.c_uint32,
                                 u32p, u64p, u64p, i32p]
    L.emu_copy_recut.restype = None
    L.emu_copy_recut.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_size_t, C.c_uint32]
    _LIB = L
    return L


def unit_len(b):
    return HEADER + (int(b) + 7) // 8


def quota_set(rng, bits, n_q):
    """0, 27, 28, 29, quotas on which a kept prefix ends exactly (and one byte either side), a unit's own boundary, random
    ones, one beyond everything, a repeat; shuffled"""
    present = [b for b in bits if b != TOO_BIG]
    prefix = np.cumsum([0] + [unit_len(b) for b in present])
    cands = [0, 27, 28, 29]
    for k in rng.choice(len(prefix), size=min(4, len(prefix)), replace=False):
        cands += [int(prefix[k]) - 1, int(prefix[k]), int(prefix[k]) + 1]
    for k in rng.choice(len(bits), size=min(3, len(bits)), replace=False):       # used + 28 + floor(bits / 8): the unit just fails
        if bits[k] != TOO_BIG:
            used = int(sum(unit_len(b) for b in bits[:k] if b != TOO_BIG))
            cands += [used + HEADER + int(bits[k]) // 8, used + HEADER + int(bits[k]) // 8 + 1]
    cands += [int(x) for x in rng.integers(0, int(prefix[-1]) + 100, 4)] + [int(prefix[-1]) + 10 ** 6] * 3
    qs = [max(0, int(c)) for c in rng.choice(cands, size=n_q - 1, replace=True)]
    qs.append(qs[int(rng.integers(0, len(qs)))] if qs else 28)                    # a duplicate
    rng.shuffle(qs)
    return np.array(qs, np.uint64)


def random_table(rng, n, p_missing):
    """a packet table and the unit -> slot map into it: (tab_off, tab_bits, unit_slot, the bit counts wanted).  Slots that no
    unit names hold packets too (a packet of a kind the geometry has no unit for); bit counts of every length mod 8 and 0"""
    n_slots = n + int(rng.integers(0, 40))
    unit_slot = rng.permutation(n_slots)[:n].astype(np.uint32)
    tab_off = rng.integers(0, 1 << 20, n_slots).astype(np.uint32)
    tab_bits = rng.integers(1, 40000, n_slots).astype(np.uint32)
    small = rng.random(n_slots) < 0.4
    tab_bits[small] = rng.integers(0, 200, int(small.sum()))
    tab_bits[rng.random(n_slots) < 0.1] = 0
    missing = rng.random(n_slots) < p_missing
    tab_off[missing] = NO_PACKET
    tab_bits[missing] = rng.integers(0, 1 << 32, int(missing.sum()))            # (never written by the walk: anything)
    want = np.where(tab_off[unit_slot] == NO_PACKET, TOO_BIG, tab_bits[unit_slot]).astype(np.uint32)
    return tab_off, tab_bits, unit_slot, want


def plan(L, inside, cursor, other, tab_off, tab_bits, unit_slot, order, quotas, nth):
    n, n_q = len(unit_slot), len(quotas)
    bits = np.full(n, 0x77777777, np.uint32)
    foff = np.full(n_q * n, 7, np.uint64)
    sizes, rcs = np.full(n_q, 7, np.uint64), np.full(n_q, 7, np.int32)
    status = L.emu_recut_plan(inside, cursor, other, tab_off, tab_bits, unit_slot, n, order, quotas, n_q, nth, bits, foff, sizes, rcs)
    return status, bits, foff.reshape(n_q, n), sizes, rcs


def test_recut_plan_equals_one_scan_per_quota():
    L = _lib()
    rng = np.random.default_rng(20261017)
    seen = {"cut": 0, "all_kept": 0, "nothing": 0, "missing_decides": 0, "status": 0}
    for case in range(400):
        n = int(rng.integers(1, 200))
        tab_off, tab_bits, unit_slot, want_bits = random_table(rng, n, (0.0, 0.02, 0.3)[case % 3])
        order = rng.permutation(n).astype(np.uint32)
        quotas = quota_set(rng, want_bits, int(rng.integers(1, 17)))
        nth = (256, 64, 3, 1)[case % 4]
        status, bits, foff, sizes, rcs = plan(L, 1, 28 + case, 0, tab_off, tab_bits, unit_slot, order, quotas, nth)
        assert status == 0 and np.array_equal(bits, want_bits), case
        for q, quota in enumerate(quotas):
            kept, used = C.c_uint32(), C.c_uint64()
            row = np.empty(n, np.uint64)
            rc = L.emu_scan_frame(want_bits, order, n, int(quota), row, C.byref(kept), C.byref(used))
            assert np.array_equal(foff[q], row) and sizes[q] == used.value and rcs[q] == rc, (case, q, int(quota))
            # the stream is the kept prefix of the priority order and fits the quota
            assert used.value == sum(unit_len(b) for b in want_bits[:kept.value]) and used.value <= int(quota)
            assert (rc == 0) == (kept.value == n) and rc in (0, QUOTA_EXCEEDED)
            seen["cut"] += rc == QUOTA_EXCEEDED and used.value > 0
            seen["all_kept"] += rc == 0
            seen["nothing"] += rc == QUOTA_EXCEEDED and used.value == 0
            # the walk ends at a unit without a packet although the quota had room for more than a header
            seen["missing_decides"] += kept.value < n and want_bits[kept.value] == TOO_BIG and used.value + HEADER < int(quota)
    # frames with a status keep nothing at any quota
    for case, (inside, cursor, other, want) in enumerate([(0, 100, 0, INVALID_INPUT), (1, 0, 0, OUT_OF_DATA), (1, 100, 1, INVALID_INPUT),
                                                          (0, 0, 1, INVALID_INPUT), (1, 0, 1, INVALID_INPUT)] * 2):
        n = int(rng.integers(1, 150))
        tab_off, tab_bits, unit_slot, want_bits = random_table(rng, n, 0.1)
        quotas = quota_set(rng, want_bits, 1 + case)
        status, bits, foff, sizes, rcs = plan(L, inside, cursor, other, tab_off, tab_bits, unit_slot, rng.permutation(n).astype(np.uint32),
                                              quotas, 64)
        assert status == want and (foff == NONE).all() and (sizes == 0).all() and (rcs == want).all(), case
        seen["status"] += 1
    assert all(v >= 5 for v in seen.values()), seen


def test_recut_copy_every_alignment_and_length():
    """one packet of every length 0 .. 47 from every source alignment to three kept destinations of different alignments (and a
    dropped one), by 256 / 64 / 3 / 1 threads: the plain copy, and not a byte beside it"""
    L = _lib()
    rng = np.random.default_rng(11)
    store = rng.integers(0, 256, 256).astype(np.uint8)
    pitch = 101
    for length in range(48):
        for sa in range(4):
            for da in range(4):
                for nth in (256, 64, 3, 1):
                    offs = np.array([da, NONE, da + 1 + 4 * (length % 3), da + 2], np.uint64)    # rows of odd pitch on top
                    buf = np.full(8 + 4 * pitch, SENT, np.uint8)
                    want = buf.copy()
                    for q, o in enumerate(offs):
                        if o != NONE:
                            want[q * pitch + int(o): q * pitch + int(o) + length] = store[64 + sa: 64 + sa + length]
                    assert store.ctypes.data % 4 == 0 and buf.ctypes.data % 4 == 0
                    L.emu_copy_recut(store.ctypes.data + 64 + sa, length, offs.ctypes.data, 1, 4, buf.ctypes.data, pitch, nth)
                    assert np.array_equal(buf, want), (length, sa, da, nth, np.argwhere(buf != want)[:4].ravel().tolist())


def test_recut_copy_equals_one_copy_per_quota():
    """packets at arbitrary byte offsets of a master, every kept one at its offset in every quota's row (rows of odd stride and
    a base at every alignment), nothing else written; each row is the stream scan_frame_wave laid out"""
    L = _lib()
    rng = np.random.default_rng(7)
    for case in range(64):
        n = int(rng.integers(1, 60))
        tab_off, tab_bits, unit_slot, bits = random_table(rng, n, (0.0, 0.05)[case % 2])
        order = rng.permutation(n).astype(np.uint32)
        quotas = quota_set(rng, bits, int(rng.integers(1, 17)))
        n_q = len(quotas)
        _, _, foff, sizes, rcs = plan(L, 1, 28, 0, tab_off, tab_bits, unit_slot, order, quotas, 64)
        # the master: the packets one after another in a shuffled order with 0-5 junk bytes between them, from a base of every alignment
        lens = [unit_len(b) if b != TOO_BIG else 0 for b in bits]
        src_base = case % 4
        at, where = src_base + int(rng.integers(0, 3)) * 4, {}
        for u in rng.permutation(n):
            where[int(u)] = at
            at += lens[u] + int(rng.integers(0, 6))
        master = rng.integers(0, 256, at + 16).astype(np.uint8)
        before = master.copy()
        stride = int(sizes.max()) + 1 + 2 * int(rng.integers(0, 3))
        if stride % 2 == 0:
            stride += 1
        base = (case // 4) % 4
        buf = np.full(base + n_q * stride + 8, SENT, np.uint8)
        want = buf.copy()
        assert master.ctypes.data % 4 == 0 and buf.ctypes.data % 4 == 0
        for u in range(n):
            offs = np.ascontiguousarray(foff[:, u])
            for q in range(n_q):
                if offs[q] != NONE:
                    o = base + q * stride + int(offs[q])
                    want[o: o + lens[u]] = master[where[u]: where[u] + lens[u]]
            if (offs != NONE).any():
                nth = (256, 64, 3, 1)[(case + u) % 4]
                L.emu_copy_recut(master.ctypes.data + where[u], lens[u], offs.ctypes.data, 1, n_q, buf.ctypes.data + base, stride, nth)
        assert np.array_equal(buf, want), (case, np.argwhere(buf != want)[:4].ravel().tolist())
        assert np.array_equal(master, before)
        for q in range(n_q):
            row = buf[base + q * stride: base + q * stride + int(sizes[q])]
            kept = [int(order[j]) for j in range(n) if foff[q][order[j]] != NONE]
            assert row.tobytes() == b"".join(master[where[u]: where[u] + lens[u]].tobytes() for u in kept), (case, q)
