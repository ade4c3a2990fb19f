"""The two planners of a reduced-resolution decoder -- plan_decode with `reduce` (decoder_plan.hpp, synchronous calls) and the
device planner with DPlanGeom::reduce (decoder_dplan.hpp, asynchronous calls) -- compiled by g++ (tests/emu/dplan_reduced_emu.cpp):
they must agree on every frame's kept packets, rc, size, means, transform flag, levels and chains, as
tests/test_decoder_plan_device.py asks of the plain planners, and both must equal the plain plan_decode at stages - r of the
frame's derived stream (tests/reduced_model.py).  CPU only."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

from oracle.binding import Oracle
from tests import decoder_batch_cases as dbc
from tests import reduced_model as rm
from tests.test_oracle_decoder import packets, random_case

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emu", "dplan_reduced_emu.cpp")
u64 = np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS")
u8p = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    lib_path = str(tmp_path_factory.mktemp("rplan") / "libdplan_reduced_emu.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-DICER_WAVE_EMU", "-o", lib_path, SRC])
    lib = C.CDLL(lib_path)
    lib.emu_rplan.argtypes = [u8p, C.c_uint32, u8p, C.c_int, u64, u64, u64, u64, C.c_int, C.c_int, C.c_uint, C.c_int, C.c_int, C.c_uint64,
                              u64, u64, u64]
    lib.emu_rplan_message.restype = C.c_char_p
    return lib


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def plan(emu, blob, offsets, lens, channels, stages, segments, bits, r, bufsize, ws=None, hs=None):
    """-> (frames with a kept packet, frames whose valid packets were all dropped, chains)"""
    n = len(offsets)
    blob = bytes(blob)
    derived = [rm.derive(blob[o: o + ln], r) for o, ln in zip(offsets, lens)]
    dlens = [len(s) for s in derived]
    doffs = [sum(dlens[:k]) for k in range(n)]
    arr = lambda b: np.frombuffer(b, np.uint8).copy() if len(b) else np.zeros(1, np.uint8)        # noqa: E731
    ws = np.asarray(ws if ws is not None else [0] * n, np.uint64)
    hs = np.asarray(hs if hs is not None else [0] * n, np.uint64)
    out = np.zeros(3, np.uint64)
    rc = emu.emu_rplan(arr(blob), len(blob), arr(b"".join(derived)), n, np.asarray(offsets, np.uint64), np.asarray(lens, np.uint64),
                       np.asarray(doffs, np.uint64), np.asarray(dlens, np.uint64), channels, stages, segments, bits, r, bufsize, ws, hs, out)
    assert rc == 0, (r, emu.emu_rplan_message().decode())
    return int(out[0]), int(out[1]), int(out[2])


def pack(streams):
    lens = [len(s) for s in streams]
    return b"".join(streams), [sum(lens[:k]) for k in range(len(lens))], lens


@pytest.mark.parametrize("filt", [0, 3, 6])
def test_reduced_planners_on_the_mixed_batches(emu, orc, filt):
    """gray and YUV, 16 and 8 bits, whole, quota-cut, damaged, truncated, empty, too-small and too-large frames"""
    for ch in (1, 3):
        for bits in (16, 8):
            b = dbc.mixed_batch(orc, ch, bits, filt, "mock")
            blob, offs, lens = pack(b.streams)
            for r in range(1, b.stages):
                rw, rh = rm.reduced_size(*dbc.SIZES["mock"][1], r)
                for bufsize in (b.stride, rw * rh, rw * rh - 1):
                    kept, _, chains = plan(emu, blob, offs, lens, ch, b.stages, b.segments, bits, r, bufsize)
                    assert kept >= len(b.streams) - 2 and chains > 0


def test_reduced_planners_reduce_zero_is_the_plain_plan(emu, orc):
    b = dbc.mixed_batch(orc, 3, 16, 4, "mock")
    blob, offs, lens = pack(b.streams)
    kept, dropped, _ = plan(emu, blob, offs, lens, 3, b.stages, b.segments, 16, 0, b.stride)
    assert kept >= len(b.streams) - 2 and dropped == 0


def test_reduced_planners_on_valid_damaged_and_foreign_packets(emu, orc):
    """frames that mix valid packets with damaged ones (header and payload), packets of another image (other size fields, other
    levels: higher than the decoder's stages, 0), junk and preamble runs; a frame laid over two others; a frame whose valid
    packets are all of level <= r: it keeps its size in-values, as an empty stream does"""
    from icer_compression_amd import synth
    img = synth.gray_frame(160, 120, 3, 1)
    st, sg = 4, 5
    rc, x, _ = orc.compress([img], st, 1, sg, 2 * 160 * 120)
    other = orc.compress([synth.gray_frame(90, 70, 5, 1)], 6, 1, sg, 2 * 90 * 70)[1]        # (levels up to 6, another size)
    pk, opk = packets(x), packets(other)
    rng = np.random.default_rng(7)
    lv0 = bytearray(pk[3]); lv0[4] = 0                                                     # a level-0 packet with good CRCs
    lv0[24:28] = zlib.crc32(bytes(lv0[:24])).to_bytes(4, "little")
    variants = [x, b"", b"\x5b\x60" * 40, x[: len(x) // 2], x[: len(x) - 1], x[5:], b"".join(reversed(pk)), b"".join(pk + pk[:7]),
                b"\x00" * 9 + x + b"\x5b\x60\x00",
                b"".join(p for pair in zip(pk, opk) for p in pair),                         # foreign packets in between
                b"".join(opk[:9]) + x, x + b"".join(opk[-9:]), bytes(lv0) + x, x + bytes(lv0),
                rm.flip_in_packet(x, 1, False, 2), rm.flip_in_packet(x, st, True, 0), rm.flip_in_packet(rm.flip_in_packet(x, 2, True, 1), 3, False, 1)]
    only = {r: b"".join(p for p in pk if p[4] <= r) for r in (1, 2, 3)}
    for _ in range(10):
        s = bytearray(x)
        for _ in range(int(rng.integers(1, 6))):
            s[int(rng.integers(0, len(s)))] ^= 1 << int(rng.integers(0, 8))
        variants.append(bytes(s))
    for r in (1, 2, 3):
        frames = variants + [only[r], only[1]]
        blob, offs, lens = pack(frames)
        offs, lens = offs + [offs[3], 7], lens + [lens[3] + lens[4] + 11, len(blob) - 7]      # over two frames; nearly all of the blob
        n = len(offs)
        rw, rh = rm.reduced_size(160, 120, r)
        for bufsize in (rw * rh, rw * rh - 1, 160 * 120):
            kept, dropped, chains = plan(emu, blob, offs, lens, 1, st, sg, 16, r, bufsize, list(range(5, 5 + n)), list(range(40, 40 + n)))
            assert kept >= n - 6 and dropped >= 2


def test_reduced_planners_on_random_streams(emu, orc):
    """the random streams of test_oracle_decoder.py at every r, with their own and with wrong segment counts, several to a blob"""
    rng = np.random.default_rng(11)
    done = 0
    while done < 40:
        planes, st, filt, sg, ch, bits, quota = random_case(rng)
        if st < 2:
            continue
        rc, stream, _ = (orc.compress if bits == 16 else orc.compress_u8)(planes, st, filt, sg, quota)
        if not stream:
            continue
        dsg = sg if rng.random() < 0.8 else int(rng.integers(1, 33))
        h, w = planes[0].shape
        junk = rng.integers(0, 256, int(rng.integers(0, 40))).astype(np.uint8).tobytes()
        blob = junk + stream + b"\x5b\x60" * 20 + stream[: len(stream) // 2]
        offs = [len(junk), len(junk) + len(stream) + 40, 0, len(junk) + 3]
        lens = [len(stream), len(stream) // 2, len(blob), len(stream) - 3]
        for r in range(1, st):
            rw, rh = rm.reduced_size(w, h, r)
            for bufsize in (rw * rh, rw * rh - 1):
                plan(emu, blob, offs, lens, ch, st, dsg, bits, r, bufsize, [5, 6, 7, 8], [9, 10, 11, 12])
        done += 1
