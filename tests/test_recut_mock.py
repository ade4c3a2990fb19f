"""icerx_recut_device_async end to end on the CPU: decoder.hip with csrc/recut.hpp compiled by g++ against
tests/emu/hip_mock_async.h (device memory = host memory, a launch = a loop over the grid), as tests/test_decoder_async_emu.py
builds it.  Masters come from the oracle at the `lossless` and `cut` quota classes, for YUV and gray geometries of 16 and 8 bit
(the uint8 YUV final order runs the other way); every quota class not above the master's is re-cut and compared with the
oracle's stream at that quota, byte for byte; the classes above a cut master give the master itself with
ICER_BYTE_QUOTA_EXCEEDED.  The masters lie in the blob at odd offsets with junk between them, or in rows of a stride with
d_offsets = NULL.  CPU only."""
import os
import subprocess

import numpy as np
import pytest

from tests import encoder_batch_cases as ebc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SENT, SENT_SIZE, SENT_RC = 0xA5, 0x7777777777777777, 0x66666666
QUOTA_EXCEEDED, OUT_OF_DATA, INVALID_INPUT, FATAL = -5, -7, -11, -10
GUARD = 4096                                       # sentinel bytes behind the workspace a call is handed

GEOMETRIES = {
    "yuv16": (ebc.Geometry(256, 192, 3, 3, 1, 5), [("smooth", 0), ("noise8", 1), ("blank", 0), (("sparse", "dot", "wide"), 2)]),
    "gray16": (ebc.Geometry(512, 384, 1, 2, 3, 2), [("noise8", 0), ("flat", 1), ("sparse", 2), ("smooth", 3), ("wide", 4)]),
    "yuv8": (ebc.Geometry(128, 96, 3, 3, 0, 5, bits=8), [("noise6", 0), ("smooth6", 1), ("blank8", 2)]),
    "gray8": (ebc.Geometry(256, 192, 1, 3, 0, 6, bits=8), [("smooth6", 0), ("noise6", 1), ("blank8", 2)]),
}


@pytest.fixture(scope="module")
def expected(oracle):
    return ebc.Expected(oracle)


@pytest.fixture(scope="module")
def mock_lib(tmp_path_factory):
    from icer_compression_amd import decoder
    lib_path = str(tmp_path_factory.mktemp("mock_recut") / "libdecoder_mock_recut.so")
    subprocess.check_call(["g++", "-x", "c++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas",
                           "-DICER_HOST_MOCK", "-DICER_WAVE_EMU", "-include", os.path.join(HERE, "emu", "hip_mock_async.h"),
                           "-o", lib_path, os.path.join(ROOT, "icer_compression_amd", "csrc", "decoder.hip")])
    return decoder.bind(lib_path)


def recutter(lib, g):
    from icer_compression_amd import decoder
    return decoder.Recutter(g.w, g.h, g.channels, g.stages, g.segments, bits=g.bits, lib=lib)


def recut_call(r, blob, offsets, lens, quotas, stream_stride=0, stride=None, ws_bytes=None, **override):
    """icerx_recut_device_async on host arrays (the mock's device memory) into Q * n + 1 sentinel rows of an odd stride.
    -> (rc of the call, res[q][f] = (rc, stream)) after checking the buffer promises"""
    n, Q = len(lens), len(quotas)
    stride = stride or (max(quotas) + 5) | 1
    out = np.full((Q * n + 1, stride), SENT, np.uint8)
    sizes = np.full(Q * n + 1, SENT_SIZE, np.uint64)
    rcs = np.full(Q * n + 1, SENT_RC, np.int32)
    offs = np.asarray(offsets, np.uint64) if offsets is not None else None
    ln = np.asarray(lens, np.uint64)
    keep = blob.copy()
    need = r.workspace_bytes(n, len(blob), Q)
    work = np.full(need + GUARD, 0xCD, np.uint8)                        # (the call is handed `need` bytes; a guard tail behind them)
    args = dict(n=n, d_data=blob.ctypes.data, data_bytes=len(blob), d_offsets=offs.ctypes.data if offs is not None else None,
                stream_stride=stream_stride, d_lens=ln.ctypes.data, quotas=quotas, d_out=out.ctypes.data, out_stride=stride,
                d_sizes=sizes.ctypes.data, d_rcs=rcs.ctypes.data, d_workspace=work.ctypes.data,
                workspace_bytes=need if ws_bytes is None else ws_bytes, stream=None)
    if "quotas_arg" in override:                                        # (the quotas as passed, whatever the rows are sized for)
        override["quotas"] = override.pop("quotas_arg")
    args.update(override)
    rc = r.recut_device_async_ptrs(**args)
    assert (work[need:] == 0xCD).all(), "written behind the workspace"
    assert np.array_equal(blob, keep), "the masters were modified"
    if rc != 0:
        assert (out == SENT).all() and (sizes == SENT_SIZE).all() and (rcs == SENT_RC).all(), "a refused call wrote"
        return rc, None
    assert (out[Q * n] == SENT).all() and sizes[Q * n] == SENT_SIZE and rcs[Q * n] == SENT_RC, "written past the Q * n rows"
    res = []
    for q, quota in enumerate(quotas):
        row = []
        for f in range(n):
            k = q * n + f
            s = int(sizes[k])
            assert 0 <= s <= quota, (q, f, s, quota)
            assert (out[k, s:] == SENT).all(), f"quota {q} frame {f}: bytes written behind its stream of {s} bytes"
            row.append((int(rcs[k]), out[k, :s].tobytes()))
        res.append(row)
    return rc, res


def pack_odd(rng, streams):
    """the streams in one blob, each at an odd offset, random junk before, between and behind them"""
    parts, offsets, at = [], [], 0
    for s in streams:
        gap = int(rng.integers(1, 40))
        if (at + gap) % 2 == 0:
            gap += 1
        parts.append(rng.integers(0, 256, gap).astype(np.uint8).tobytes())
        at += gap
        offsets.append(at)
        parts.append(s)
        at += len(s)
    parts.append(rng.integers(0, 256, 7).astype(np.uint8).tobytes())
    return np.frombuffer(b"".join(parts), np.uint8).copy(), offsets


def pack_rows(streams):
    """row k of an odd stride holds stream k (the encoder's layout; d_offsets = NULL)"""
    stride = (max(len(s) for s in streams) + 6) | 1
    blob = np.full(len(streams) * stride, 0x5B, np.uint8)             # (filled with half a preamble)
    for k, s in enumerate(streams):
        blob[k * stride: k * stride + len(s)] = np.frombuffer(s, np.uint8)
    return blob, stride


def wanted(expected, g, spec, master, master_quota, quota):
    """what a re-cut of `master` (made at master_quota) to `quota` gives"""
    if quota > master_quota and master[0] == QUOTA_EXCEEDED:
        return QUOTA_EXCEEDED, master[1]                               # (documented: the master itself)
    want = expected(g, spec, quota)
    return want[0], want[1]


@pytest.mark.parametrize("master_cls", ["lossless", "cut"])
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_recut_mock_equals_oracle(mock_lib, expected, name, master_cls):
    g, specs = GEOMETRIES[name]
    rng = np.random.default_rng(sum(map(ord, name + master_cls)))
    mq = ebc.quota(g, master_cls)
    masters = [expected(g, s, mq) for s in specs]
    assert all(m[0] in (0, QUOTA_EXCEEDED) for m in masters)
    assert master_cls == "lossless" or any(m[0] == QUOTA_EXCEEDED for m in masters), "no master of this batch is cut"
    quotas = [ebc.quota(g, c) for c in ebc.QUOTA_CLASSES]              # (every class not above the master's, and those above)
    quotas.append(quotas[int(rng.integers(0, len(quotas)))])
    rng.shuffle(quotas)
    quotas = [int(q) for q in quotas]
    r = recutter(mock_lib, g)
    streams = [m[1] for m in masters]
    blob, offsets = pack_odd(rng, streams)
    rows, stride = pack_rows(streams)
    for what, (rc, got) in (("odd offsets", recut_call(r, blob, offsets, [len(s) for s in streams], quotas)),
                            ("stride", recut_call(r, rows, None, [len(s) for s in streams], quotas, stream_stride=stride))):
        assert rc == 0, what
        for q, quota in enumerate(quotas):
            for f, spec in enumerate(specs):
                if master_cls == "lossless":
                    assert masters[f][0] == 0
                ebc.check_frame(*got[q][f], wanted(expected, g, spec, masters[f], mq, quota),
                                f"{name} {master_cls} master, {what}: quota {quota} frame {f} {spec}")
    r.close()


def test_recut_mock_frame_errors_and_refused_calls(mock_lib, expected):
    g, specs = GEOMETRIES["gray16"]
    other = ebc.Geometry(256, 192, 1, 2, 3, 2)
    mq = ebc.quota(g, "lossless")
    good = [expected(g, s, mq)[1] for s in specs[:2]]
    alien = expected(other, ("smooth", 0), ebc.quota(other, "lossless"))[1]
    rng = np.random.default_rng(5)
    junk = rng.integers(0, 256, 3000).astype(np.uint8).tobytes()
    streams = [good[0], junk, alien, good[1], b""]
    blob, offsets = pack_odd(rng, streams)
    lens = [len(s) for s in streams]
    offsets += [len(blob) - 10, len(blob) + 1]                          # two frames that leave the blob
    lens += [11, 0]
    quotas = [ebc.quota(g, "cut"), 60, mq]
    r = recutter(mock_lib, g)
    rc, got = recut_call(r, blob, offsets, lens, quotas)
    assert rc == 0
    for q, quota in enumerate(quotas):
        for f, s in ((0, specs[0]), (3, specs[1])):
            ebc.check_frame(*got[q][f], expected(g, s, quota), f"a neighbour of bad frames: quota {quota} frame {f}")
        assert [got[q][f] for f in (1, 2, 4, 5, 6)] == [(OUT_OF_DATA, b""), (INVALID_INPUT, b""), (OUT_OF_DATA, b""),
                                                         (INVALID_INPUT, b""), (INVALID_INPUT, b"")], quota
    # refused calls write nothing (recut_call checks that)
    n = len(lens)
    need = r.workspace_bytes(n, len(blob), len(quotas))
    cases = {
        "no quotas": dict(n_quotas=0), "17 quotas": dict(quotas_arg=[60] * 17), "negative quota count": dict(n_quotas=-1),
        "no frames": dict(n=0), "negative frames": dict(n=-1), "too many frames": dict(n=65536),
        "null quotas": dict(quotas_arg=None, n_quotas=2), "null data": dict(d_data=None), "null lens": dict(d_lens=None),
        "null out": dict(d_out=None), "null sizes": dict(d_sizes=None), "null rcs": dict(d_rcs=None), "null workspace": dict(d_workspace=None),
        "stride below the largest quota": dict(out_stride=mq - 1), "workspace too small": dict(workspace_bytes=need - 1),
    }
    for what, kw in cases.items():
        assert recut_call(r, blob, offsets, lens, quotas, **kw)[0] == INVALID_INPUT, what
    assert recut_call(r, blob, offsets, lens, quotas, data_bytes=0xFFFFFFFF - 64)[0] == FATAL
    assert r.lib.icerx_recut_device_async(None, n, blob.ctypes.data, len(blob), None, 0, None, None, 1, None, 0, None, None, None, 0,
                                          None) == INVALID_INPUT
    r.close()


def test_recutter_create_refuses_what_the_planner_refuses(mock_lib):
    from icer_compression_amd import decoder
    for args, code in (((64, 64, 2, 3, 4), -11), ((0, 64, 1, 3, 4), -11), ((64, 64, 1, 0, 4), -4), ((64, 64, 1, 7, 4), -4),
                       ((16, 16, 1, 4, 1), -4), ((64, 64, 1, 3, 33), -3), ((64, 64, 1, 3, 0), -11)):
        with pytest.raises(RuntimeError, match=f"icerx_recutter_create: {code} "):
            decoder.Recutter(*args, lib=mock_lib)
    with pytest.raises(RuntimeError, match="icerx_recutter_create: -11 "):
        decoder.Recutter(64, 64, 1, 3, 4, bits=12, lib=mock_lib)
