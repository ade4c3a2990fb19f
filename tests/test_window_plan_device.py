"""The two planners of a window decode -- plan_decode_window (decoder_plan.hpp, the synchronous calls) and the device planner
with dplan_window_keeps (decoder_dplan.hpp, the asynchronous calls) -- compiled by g++ (tests/emu/dplan_window_emu.cpp): they must
agree on every frame's rc, size, clipped window, geometry and kept chains, and their counts must be the model's
(tests/window_model.py).  CPU only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle.binding import Oracle
from tests import window_model as wm
from tests.test_decoder_async_emu import _batch
from tests.test_window_mock import pick_windows

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emu", "dplan_window_emu.cpp")
u64 = np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS")
u32 = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")
i64 = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")
u8p = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    lib_path = str(tmp_path_factory.mktemp("wplan") / "libdplan_window_emu.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-DICER_WAVE_EMU", "-o", lib_path, SRC])
    lib = C.CDLL(lib_path)
    lib.emu_wplan.argtypes = [u8p, C.c_uint32, C.c_int, u64, u64, u32, C.c_int, C.c_int, C.c_uint, C.c_int, C.c_int, C.c_uint64, C.c_uint64, i64]
    lib.emu_wplan_message.restype = C.c_char_p
    return lib


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def plan(emu, b, wins, out_stride):
    lens = [len(s) for s in b.streams]
    offs = [sum(lens[:k]) for k in range(len(lens))]
    blob = np.frombuffer(b"".join(b.streams), np.uint8).copy()
    out = np.zeros((len(lens), 6), np.int64)
    rc = emu.emu_wplan(blob, len(blob), len(lens), np.asarray(offs, np.uint64), np.asarray(lens, np.uint64),
                       np.asarray(wins, np.uint32).reshape(-1).copy(), b.channels, b.stages, b.segments, b.bits, b.filt, b.stride, out_stride, out)
    assert rc == 0, emu.emu_wplan_message().decode()
    return out


@pytest.mark.parametrize("filt", [0, 2, 6])
@pytest.mark.parametrize("ch,bits", [(1, 16), (3, 16), (1, 8), (3, 8)])
def test_window_planners_agree_with_each_other_and_the_model(emu, orc, ch, bits, filt):
    b = _batch(orc, ch, bits, filt)
    restricted = 0
    for shift in range(0, 15, 2):
        wins = pick_windows(b, shift)
        for out_stride in (b.stride, 300):
            got = plan(emu, b, wins, out_stride)
            for k, s in enumerate(b.streams):
                rc, clip, _, run, full = wm.expected(orc, b.want[k], wins[k], out_stride, b.stride, ch, b.stages, filt, b.segments, bits, s)
                assert got[k][0] == rc and got[k][1] == clip[2] * clip[3], (k, list(got[k]), rc, clip)
                assert bool(got[k][5]) == (rc == wm.QUOTA and b.want[k][0] != wm.QUOTA), (k, list(got[k]))
                if not wm.delivered(*b.want[k][:3], b.stride):
                    assert list(got[k][1:]) == [0] * 5, (k, list(got[k]))
                elif full is not None:
                    assert (got[k][2], got[k][3]) == (run, full) and got[k][4] == 1, (k, list(got[k]), run, full)
                    restricted += run < full
                elif not got[k][5]:
                    assert got[k][2] == got[k][3] and got[k][4] == 0, (k, list(got[k]))
    assert restricted >= 10
