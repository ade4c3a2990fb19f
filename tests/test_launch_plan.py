"""The encoder's launch policy (csrc/launch_plan.hpp): which kernels an encode call launches, in which instances and shapes, in how
many parts.  The header is host-only C++, built here with g++ behind a small C driver (tests/emu/launch_plan_driver.cpp); the
table below pins every default decision."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "icer_compression_amd", "csrc", "launch_plan.hpp")
DRIVER = os.path.join(ROOT, "tests", "emu", "launch_plan_driver.cpp")
SO = os.path.join(ROOT, "tests", "emu", "liblaunch_plan_driver.so")
MAX_PARTS = 4
LIST = {0: "WgOne", 1: "WgSmall", 2: "WgFour"}
PIPE = {0: "large", 1: "lone", 2: "batch"}
WINDOW = {0: "WgFour", 1: "WgFull"}
W = H = 4096
SUBS = 100                       # sub-range workgroups per frame, when the encoder plans them


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(HEADER), os.path.getmtime(DRIVER)):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", SO, DRIVER])
    L = C.CDLL(SO)
    L.lp_tuning.argtypes = [C.c_char_p, C.POINTER(C.c_int)]
    L.lp_plan.argtypes = [C.c_char_p, C.c_int, C.c_long, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                          C.c_ulonglong, C.c_int, C.POINTER(C.c_int)]
    return L


def tuning(L, env=""):
    out = (C.c_int * 11)()
    L.lp_tuning(env.encode(), out)
    keys = ("coder", "pipe_waves", "hybrid_percent", "hybrid_frames", "split_chunks", "list_waves", "slot_bpp", "overlap_parts",
            "fail_frame", "fail_unit", "fail_calls")
    return dict(zip(keys, out))


def plan(L, n, max_frames=None, channels=1, env="", quota=None, wg_available=True, wg_once=False, synchronous=True, n_cus=256):
    """what one call of `n` frames launches; `synchronous`: icerx_encode_device (may be enqueued in parts), else the async call"""
    max_frames = n if max_frames is None else max_frames
    quota = 2 * W * H * channels if quota is None else quota
    out = (C.c_int * (4 + 11 * MAX_PARTS))()
    L.lp_plan(env.encode(), channels, W, H, max_frames, n_cus, SUBS, int(wg_available), int(wg_once), n, quota, int(synchronous), out)
    v = list(out)
    call = {"progressive": bool(v[0]), "use_wg": bool(v[1]), "subs_planned": bool(v[3]), "parts": []}
    for k in range(v[2]):
        f0, nf, hybrid, split, subs, grid, inst, pct, pipe, pm, window = v[4 + 11 * k: 15 + 11 * k]
        call["parts"].append({"frames": (f0, nf), "split": bool(split), "subs": subs,
                              "list": (grid, LIST[inst], pct) if hybrid else None,
                              "pipe": None if call["use_wg"] else PIPE[pipe],
                              "position_major": None if call["use_wg"] else bool(pm),
                              "window": WINDOW[window] if call["use_wg"] else None})
    return call


def pipe_call(c, split=False, lst=None, pipe="large", pm=False):
    """every part of a pipeline call alike; returns the parts' (frames) for the caller to check"""
    assert not c["progressive"] and not c["use_wg"]
    for p in c["parts"]:
        assert (p["split"], p["list"], p["pipe"], p["position_major"]) == (split, lst, pipe, pm), p
        assert p["subs"] == (SUBS if split else 0)
    return [p["frames"] for p in c["parts"]]


BATCH_LIST = (512, "WgOne", 95)


def test_lone_gray_frame_is_split(lib):
    c = plan(lib, 1)
    assert c["subs_planned"]
    assert pipe_call(c, split=True, lst=(256, "WgFour", 90), pipe="lone") == [(0, 1)]


def test_split_off(lib):
    c = plan(lib, 1, env="ICER_HIP_SPLIT=0")
    assert not c["subs_planned"]
    assert pipe_call(c) == [(0, 1)]


def test_lone_frame_of_a_larger_encoder_is_not_split(lib):
    c = plan(lib, 1, max_frames=8)                   # 8 planes > 4: no sub-ranges planned
    assert not c["subs_planned"]
    assert pipe_call(c) == [(0, 1)]


def test_small_batch_without_the_half_stream(lib):
    assert pipe_call(plan(lib, 3), lst=BATCH_LIST, pipe="batch", pm=True) == [(0, 3)]


def test_synchronous_batch_in_two_parts(lib):
    assert pipe_call(plan(lib, 8), lst=BATCH_LIST, pipe="batch", pm=True) == [(0, 4), (4, 4)]
    assert pipe_call(plan(lib, 5, max_frames=8), lst=BATCH_LIST, pipe="batch", pm=True) == [(0, 3), (3, 2)]


def test_asynchronous_batch_in_one_part(lib):
    assert pipe_call(plan(lib, 8, synchronous=False), lst=BATCH_LIST, pipe="batch", pm=True) == [(0, 8)]


def test_more_parts(lib):
    c = plan(lib, 10, env="ICER_HIP_OVERLAP_PARTS=4")
    assert pipe_call(c, lst=BATCH_LIST, pipe="batch", pm=True) == [(0, 3), (3, 3), (6, 2), (8, 2)]
    assert pipe_call(plan(lib, 7, max_frames=8, env="ICER_HIP_OVERLAP_PARTS=4"), lst=BATCH_LIST, pipe="batch", pm=True) == [(0, 7)]
    assert pipe_call(plan(lib, 8, env="ICER_HIP_OVERLAP_PARTS=1"), lst=BATCH_LIST, pipe="batch", pm=True) == [(0, 8)]


@pytest.mark.parametrize("n, wg_once, quota, window", [
    (1, False, W * H // 2 - 1, "WgFour"),           # progressive
    (1, True, None, "WgFull"),                      # lossless re-run after a unit time-out
    (4, True, None, "WgFour"),
])
def test_window_coder(lib, n, wg_once, quota, window):
    c = plan(lib, n, quota=quota, wg_once=wg_once)
    assert c["use_wg"] and c["progressive"] == (quota is not None)
    assert [(p["frames"], p["split"], p["list"], p["window"]) for p in c["parts"]] == [((0, n), False, None, window)]


def test_progressive_on_the_pipeline(lib):
    c = plan(lib, 1, quota=W * H // 2 - 1, env="ICER_HIP_CODER=pipe")
    assert c["progressive"] and not c["use_wg"]
    assert [(p["split"], p["list"], p["pipe"], p["position_major"]) for p in c["parts"]] == [(False, None, "large", False)]
    c = plan(lib, 8, quota=W * H // 2 - 1, env="ICER_HIP_CODER=pipe")      # (the quota is per frame)
    assert c["progressive"] and [(p["frames"], p["list"], p["pipe"], p["position_major"]) for p in c["parts"]] == [((0, 8), None, "batch", False)]


def test_window_coder_not_granted(lib):
    c = plan(lib, 1, wg_available=False)
    assert not c["subs_planned"]
    assert pipe_call(c) == [(0, 1)]
    assert plan(lib, 1, quota=1000, wg_available=False)["use_wg"] is False
    assert pipe_call(plan(lib, 8, wg_available=False), pipe="batch", pm=True) == [(0, 8)]      # (no half stream either)


def test_yuv_frame(lib):
    c = plan(lib, 1, channels=3)
    assert not c["subs_planned"]
    assert pipe_call(c, lst=BATCH_LIST) == [(0, 1)]


def test_routing_off(lib):
    assert pipe_call(plan(lib, 8, env="ICER_HIP_HYBRID=0"), pipe="batch", pm=True) == [(0, 4), (4, 4)]


def test_routing_from_one_plane(lib):
    assert pipe_call(plan(lib, 1, max_frames=8, env="ICER_HIP_HYBRID_FRAMES=1"), lst=BATCH_LIST) == [(0, 1)]


def test_routing_per_part(lib):
    """parts of one call are decided one by one: with HYBRID_FRAMES=3 five frames split (3, 2) and only the first part routes"""
    c = plan(lib, 5, max_frames=8, env="ICER_HIP_HYBRID_FRAMES=3")
    assert [(p["frames"], p["list"]) for p in c["parts"]] == [((0, 3), BATCH_LIST), ((3, 2), None)]


def test_pinned_instances(lib):
    assert pipe_call(plan(lib, 1, env="ICER_HIP_PIPE_WAVES=8"), split=True, lst=(256, "WgFour", 90), pipe="lone") == [(0, 1)]
    assert pipe_call(plan(lib, 1, env="ICER_HIP_PIPE_WAVES=11"), split=True, lst=(256, "WgFour", 90), pipe="large") == [(0, 1)]
    assert pipe_call(plan(lib, 3, env="ICER_HIP_PIPE_WAVES=11"), lst=BATCH_LIST, pipe="large", pm=True) == [(0, 3)]
    assert pipe_call(plan(lib, 3, env="ICER_HIP_LIST_WAVES=2"), lst=(512, "WgSmall", 95), pipe="batch", pm=True) == [(0, 3)]
    assert pipe_call(plan(lib, 1, env="ICER_HIP_LIST_WAVES=1"), split=True, lst=(256, "WgOne", 90), pipe="lone") == [(0, 1)]
    assert pipe_call(plan(lib, 1, n_cus=304), split=True, lst=(304, "WgFour", 90), pipe="lone") == [(0, 1)]


def test_window_coder_pinned(lib):
    c = plan(lib, 8, env="ICER_HIP_CODER=wg")
    assert c["use_wg"] and [(p["frames"], p["window"]) for p in c["parts"]] == [((0, 8), "WgFour")]
    assert not plan(lib, 1, env="ICER_HIP_CODER=wg")["subs_planned"]


def test_tuning_defaults_and_ranges(lib):
    d = tuning(lib)
    assert d == {"coder": 0, "pipe_waves": 0, "hybrid_percent": 95, "hybrid_frames": 2, "split_chunks": 1, "list_waves": 0,
                 "slot_bpp": 3, "overlap_parts": 2, "fail_frame": -1, "fail_unit": -1, "fail_calls": 0}
    ignored = ("ICER_HIP_SPLIT=64", "ICER_HIP_SPLIT=127", "ICER_HIP_SLOT_BPP=0", "ICER_HIP_SLOT_BPP=25", "ICER_HIP_HYBRID=101",
               "ICER_HIP_HYBRID=-1", "ICER_HIP_HYBRID_FRAMES=0", "ICER_HIP_PIPE_WAVES=9", "ICER_HIP_LIST_WAVES=3",
               "ICER_HIP_OVERLAP_PARTS=0", "ICER_HIP_OVERLAP_PARTS=5", "ICER_HIP_TEST_FAIL_UNIT=3", "ICER_HIP_TEST_FAIL_UNIT=2048:1",
               "ICER_HIP_TEST_FAIL_UNIT=1:2:0")
    for env in ignored:
        assert tuning(lib, env) == d, env
    assert tuning(lib, "ICER_HIP_SPLIT=0")["split_chunks"] == 0
    assert tuning(lib, "ICER_HIP_SPLIT=128")["split_chunks"] == 128
    assert tuning(lib, "ICER_HIP_SLOT_BPP=24")["slot_bpp"] == 24
    assert tuning(lib, "ICER_HIP_HYBRID=0")["hybrid_percent"] == 0
    assert tuning(lib, "ICER_HIP_CODER=pipe")["coder"] == 1 and tuning(lib, "ICER_HIP_CODER=wg")["coder"] == 2
    assert tuning(lib, "ICER_HIP_CODER=other")["coder"] == 0
    t = tuning(lib, "ICER_HIP_TEST_FAIL_UNIT=1:7")
    assert (t["fail_frame"], t["fail_unit"], t["fail_calls"]) == (1, 7, 1)
    t = tuning(lib, "ICER_HIP_TEST_FAIL_UNIT=0:3:2,ICER_HIP_OVERLAP_PARTS=4,ICER_HIP_LIST_WAVES=2")
    assert (t["fail_frame"], t["fail_unit"], t["fail_calls"], t["overlap_parts"], t["list_waves"]) == (0, 3, 2, 4, 2)
