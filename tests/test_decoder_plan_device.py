"""The device planner of the asynchronous decode (icer_compression_amd/csrc/decoder_dplan.hpp), compiled by g++
(tests/emu/dplan_emu.cpp), against the host planner of the synchronous decode (plan_decode): candidates over the whole blob with
per-frame validity must give every frame plan_decode's accepted packets, rc, size, means, transform flag, levels and chains.
CPU only.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle.binding import Oracle
from tests import decoder_batch_cases as dbc
from tests.test_oracle_decoder import packets, random_case

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emu", "dplan_emu.cpp")
CSRC = os.path.join(HERE, "..", "icer_compression_amd", "csrc")
u64 = np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS")
u8p = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    lib_path = str(tmp_path_factory.mktemp("dplan") / "libdplan_emu.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-DICER_WAVE_EMU", "-o", lib_path, SRC])
    lib = C.CDLL(lib_path)
    lib.emu_dplan.argtypes = [u8p, C.c_uint32, C.c_int, u64, u64, C.c_int, C.c_int, C.c_uint, C.c_int, C.c_uint64, u64, u64, u64]
    lib.emu_dplan_message.restype = C.c_char_p
    lib.emu_dgrid.argtypes = [C.c_uint64, C.c_uint64, C.c_uint]
    lib.emu_dpos.argtypes = [C.c_uint32, C.c_int]
    return lib


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def plan(emu, blob, offsets, lens, channels, stages, segments, bits, bufsize, ws=None, hs=None):
    """runs both planners over the frames of `blob`; -> (blob candidates, frames with an accepted packet)"""
    n = len(offsets)
    blob = np.frombuffer(bytes(blob), np.uint8).copy() if len(blob) else np.zeros(1, np.uint8)
    ws = np.asarray(ws if ws is not None else [0] * n, np.uint64)
    hs = np.asarray(hs if hs is not None else [0] * n, np.uint64)
    out = np.zeros(3, np.uint64)
    rc = emu.emu_dplan(blob, len(blob) if n else 0, n, np.asarray(offsets, np.uint64), np.asarray(lens, np.uint64), channels, stages,
                       segments, bits, bufsize, ws, hs, out)
    assert rc == 0, emu.emu_dplan_message().decode()
    assert out[0] <= (len(blob) + 1) // 2
    return int(out[0]), int(out[1])


def plan_batch(emu, b):
    streams = b.streams
    lens = [len(s) for s in streams]
    offs = list(np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)) if streams else []
    return plan(emu, b"".join(streams), offs, lens, b.channels, b.stages, b.segments, b.bits, b.stride)


@pytest.mark.parametrize("filt", [0, 3, 6])
def test_planner_on_the_mixed_batches(emu, orc, filt):
    """cases 1 + 2 at CPU scale: gray and YUV, 16 and 8 bits, streams that stop early in between (damaged, truncated,
    empty, rc -5 and -3)"""
    for ch in (1, 3):
        for bits in (16, 8):
            b = dbc.mixed_batch(orc, ch, bits, filt, "mock")
            cands, walked = plan_batch(emu, b)
            assert cands > 0 and walked >= len(b.streams) - 2


def test_planner_past_the_first_capacity(emu, orc):
    """case 5: more packets than the synchronous header kernel's first capacity"""
    b = dbc.header_pass_batch(orc)
    cands, _ = plan_batch(emu, b)
    assert cands > sum(len(s) for s in b.streams) // 64 + 1024


@pytest.mark.parametrize("ch,bits", [(1, 16), (3, 8)])
def test_planner_on_the_blob_layout(emu, orc, ch, bits):
    """case 7: junk around and between the streams, offsets out of order, the same bytes twice, a zero-length entry inside
    another stream, ws / hs in-values"""
    lay = dbc.Layout(orc, dbc.mixed_batch(orc, ch, bits, 4, "mock"))
    b = lay.batch
    plan(emu, lay.blob.tobytes(), lay.offsets, lay.lens, b.channels, b.stages, b.segments, b.bits, b.stride, lay.w_in, lay.h_in)


def test_planner_on_random_and_damaged_streams(emu, orc):
    """the random streams of test_oracle_decoder.py, decoded with their own and with wrong parameters, several to a blob
    with junk between them; and the damaged variants of one stream"""
    from icer_compression_amd import synth
    rng = np.random.default_rng(99)
    done = 0
    for _ in range(60):
        planes, st, filt, sg, ch, bits, quota = random_case(rng)
        rc, stream, _ = (orc.compress if bits == 16 else orc.compress_u8)(planes, st, filt, sg, quota)
        if not stream:
            continue
        dsg = sg if rng.random() < 0.8 else int(rng.integers(1, 33))
        h, w = planes[0].shape
        junk = rng.integers(0, 256, int(rng.integers(0, 40))).astype(np.uint8).tobytes()
        blob = junk + stream + b"\x5b\x60" * 20 + stream[: len(stream) // 2]
        offs = [len(junk), len(junk) + len(stream) + 40, 0, len(junk) + 3]
        lens = [len(stream), len(stream) // 2, len(blob), len(stream) - 3]
        for bufsize in (w * h, w * h - 1):
            plan(emu, blob, offs, lens, ch, st, dsg, bits, bufsize, [5, 6, 7, 8], [9, 10, 11, 12])
        done += 1
    assert done > 40
    img = synth.gray_frame(160, 120, 3, 1)
    rc, stream, _ = orc.compress([img], 3, 1, 5, 2 * 160 * 120)
    pk = packets(stream)
    variants = [b"", b"\x5b\x60" * 40, stream[: len(stream) // 2], stream[: len(stream) - 1], stream[5:],
                b"".join(reversed(pk)), b"".join(pk + pk[:7]), b"\x00" * 9 + stream + b"\x5b\x60\x00"]
    for _ in range(10):
        s = bytearray(stream)
        for _ in range(int(rng.integers(1, 6))):
            s[int(rng.integers(0, len(s)))] ^= 1 << int(rng.integers(0, 8))
        variants.append(bytes(s))
    blob, offs, lens = b"", [], []
    for s in variants:
        offs.append(len(blob)); lens.append(len(s))
        blob += s
    plan(emu, blob, offs, lens, 1, 3, 5, 16, 160 * 120)
    plan(emu, blob, offs, lens, 1, 3, 5, 16, 160 * 120 - 1)


def test_candidate_bound_on_preamble_runs(emu):
    """a blob of nothing but preambles (and one with a valid header at every other byte is impossible: two preambles
    cannot overlap) stays within ceil(data_bytes / 2) candidates"""
    for blob in (b"\x5b\x60" * 500, b"\x5b" + b"\x5b\x60" * 300, b"\x60\x5b" * 77):
        plan(emu, blob, [0], [len(blob)], 1, 2, 4, 16, 1000)


def test_device_grid_equals_make_grid(emu):
    for w in list(range(1, 40)) + [63, 64, 65, 127, 511, 1024, 2047, 4096]:
        for h in (1, 2, 3, 5, 8, 17, 33, 100, 1000, 2049):
            for sg in (1, 2, 3, 4, 5, 6, 7, 10, 13, 16, 20, 31, 32, 33):
                assert emu.emu_dgrid(w, h, sg) == 0, (w, h, sg)


def test_device_interleave_positions(emu):
    for n in range(2, 300):
        for bits in (16, 8):
            assert emu.emu_dpos(n, bits) == 0, (n, bits)
