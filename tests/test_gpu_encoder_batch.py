"""The encoder's batch entry points on batches of mixed content, and encoders kept for many calls, against the oracle
(oracle/icer_oracle.c) frame by frame: frames of every kind side by side in one launch (blank, dense, 12-bit, aborted ones --
tests/encoder_batch_cases.py), the odd frame at either end and on both sides of the boundary of a call in two parts, route
lists that are full or empty, and seeded sequences of calls on long-lived encoders whose size, quota, entry point and content
change from call to call.  Every call also checks the promises of include/icer_hip.h about the caller's buffers: d_frames is
not modified, nothing is written beyond the n_frames rows of d_out / entries of d_sizes and d_rcs, nor behind a frame's stream
within its row."""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

from icer_compression_amd import api
from tests import encoder_batch_cases as ebc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT, SENT_SIZE, SENT_RC = 0xA5, 0x5A5A5A5A5A5A5A5A, -777
FRONT_ENDS = {"u8": "icerx_encode_device_u8", "rgb8": "icerx_encode_device_rgb8", "s8": "icerx_encode_device_s8"}


@pytest.fixture(scope="module")
def expected(oracle):
    return ebc.Expected(oracle)


def encode(enc, g, entry, frames, q):
    """one call of `entry` ("host", "sync", "async" (+ wait), "u8", "rgb8", "s8", or "batch": icerx_compress_batch_uint16_devices
    on device 0) on the batch `frames`, into n + 1 rows / entries filled with a sentinel.  Returns [(rc, stream)] per frame."""
    n = frames.shape[0]
    stride = q + 5                                      # (>= the quota; odd: rows start at every byte alignment)
    if entry in ("host", "batch"):
        keep = frames.copy()
        out = np.full((n + 1, stride), SENT, np.uint8)
        sizes, rcs = np.full(n + 1, SENT_SIZE, np.uint64), np.full(n + 1, SENT_RC, np.int32)
        if entry == "host":
            enc.encode_host_into(frames, q, out, sizes, rcs)
        else:
            rc = api.compress_batch(frames, g.stages, g.filt, g.segments, q, out, sizes, rcs, devices=[0])
            assert rc == 0, api.load_library().icerx_last_error()
        assert np.array_equal(frames, keep), "the input frames were modified"
    else:
        import torch
        dev = torch.device("cuda", 0)
        t = torch.from_numpy(frames.view(np.int16) if frames.dtype == np.uint16 else frames).to(dev)
        keep = t.clone()
        out = torch.full((n + 1, stride), SENT, dtype=torch.uint8, device=dev)
        sizes = torch.full((n + 1,), SENT_SIZE, dtype=torch.int64, device=dev)
        rcs = torch.full((n + 1,), SENT_RC, dtype=torch.int32, device=dev)
        args = (t.data_ptr(), n, q, out.data_ptr(), stride, sizes.data_ptr(), rcs.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        if entry == "sync":
            enc.encode_device_ptrs(*args)
        elif entry == "async":
            enc.encode_device_async_ptrs(*args)
            enc.wait()
        else:
            rc = getattr(enc.lib, FRONT_ENDS[entry])(enc.handle, *args)
            assert rc == 0, enc.lib.icerx_last_error()
        torch.cuda.synchronize()
        assert torch.equal(t, keep), "the input frames were modified on the device"
        out, sizes, rcs = out.cpu().numpy(), sizes.cpu().numpy(), rcs.cpu().numpy()
    assert (out[n] == SENT).all(), "bytes written past the n frames' rows of the output"
    assert int(sizes[n]) == SENT_SIZE and int(rcs[n]) == SENT_RC, "sizes / rcs written past n_frames entries"
    res = []
    for k in range(n):
        s = int(sizes[k])
        assert 0 <= s <= q, (k, s, q)
        assert (out[k, s:] == SENT).all(), f"frame {k}: bytes written behind its stream of {s} bytes"
        res.append((int(rcs[k]), out[k, :s].tobytes()))
    return res


def check(expected, g, specs, q, got, what, enc=None, coef_frames=None):
    """every frame against the oracle; the coefficient planes of `coef_frames` (default all) where they are comparable"""
    for k, spec in enumerate(specs):
        ebc.check_frame(*got[k], expected(g, spec, q), f"{what}: frame {k} {spec}")
    if enc is not None:
        for k in range(len(specs)) if coef_frames is None else coef_frames:
            want = expected(g, specs[k], q)
            if ebc.coefficients_comparable(want):
                ebc.check_coefficients(g, [enc.coefficients(k, c) for c in range(g.channels)], want, f"{what}: frame {k} {specs[k]}")


def launch_kind(enc):
    """what the encoder's last call launched: "window" (the window coder alone), "two-part", "split", "hybrid" (the list kernel beside
    the pipeline) or "pipeline" (the pipeline alone)"""
    li = enc.launch_info()
    if li["pipeline_waves"] == 0:
        return "window"
    if enc.parts() > 1:
        return "two-part"
    if li["split"]:
        return "split"
    return "hybrid" if li["window_coder_beside"] else "pipeline"


# ---- mixed batches through every batch entry point -------------------------------------------------------------------------
GRAY = ebc.Geometry(256, 192, 1, 3, 0, 6)
BACKGROUND = [("smooth", 0), ("noise8", 0), ("sparse", 0), ("smooth", 1), ("flat", 0), ("noise8", 1)]


def odd_one_out(background, odd_kinds):
    """6-frame batches with the odd frame first, last, and on both sides of the boundary of a synchronous call in two parts
    (3 + 3: launch_plan.hpp plan_launch), and one batch of every kind"""
    out = []
    for kind in odd_kinds:
        for pos in (0, len(background) - 1, len(background) // 2 - 1, len(background) // 2):
            specs = list(background)
            specs[pos] = (kind, 7)
            out.append(specs)
    return out


GRAY_BATCHES = odd_one_out(BACKGROUND, ("overflow", "blank", "wide", "mean")) + [[(k, 0) for k in ebc.KINDS16]]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("entry", ["host", "sync", "async", "batch-sub1", "batch-sub2"])
def test_mixed_gray_batches(expected, monkeypatch, entry):
    if entry.startswith("batch"):
        monkeypatch.setenv("ICER_HIP_BATCH_SUB", entry[-1])
    enc = None if entry.startswith("batch") else api.Encoder(GRAY.w, GRAY.h, 1, GRAY.stages, GRAY.filt, GRAY.segments, max_frames=9)
    for cls in ebc.QUOTA_CLASSES:
        q = ebc.quota(GRAY, cls)
        for specs in GRAY_BATCHES:
            got = encode(enc, GRAY, entry.split("-")[0], ebc.batch(GRAY, specs), q)
            check(expected, GRAY, specs, q, got, f"{entry} {cls}", enc)
            if enc is not None and cls in ("lossless", "cut") and len(specs) == 6:
                assert enc.parts() == (1 if entry == "async" else 2), (entry, enc.parts())
    if enc is not None:
        assert enc.stats()["unit_timeouts"] == 0
        enc.close()
    else:
        api.load_library().icerx_batch_release()


YUV = ebc.Geometry(128, 96, 3, 3, 2, 5)
YUV_BACKGROUND = [("smooth", 0), ("noise8", 0), (("smooth", "sparse", "flat"), 0), ("wide", 0), ("dot", 0), ("smooth", 1)]
YUV_BATCHES = odd_one_out(YUV_BACKGROUND, (("smooth", "overflow", "smooth"), ("blank", "blank", "mean"), "blank")) + \
    [[(k, 0) for k in ebc.KINDS16]]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("entry", ["host", "sync", "async"])
def test_mixed_yuv_batches(expected, entry):
    """colour frames of mixed kinds, per channel too: a frame of which one channel alone overflows or fails the LL mean check"""
    enc = api.Encoder(YUV.w, YUV.h, 3, YUV.stages, YUV.filt, YUV.segments, max_frames=9)
    for cls in ebc.QUOTA_CLASSES:
        q = ebc.quota(YUV, cls)
        for specs in YUV_BATCHES:
            check(expected, YUV, specs, q, encode(enc, YUV, entry, ebc.batch(YUV, specs), q), f"{entry} {cls}", enc)
    assert enc.stats()["unit_timeouts"] == 0
    enc.close()


FRONT_END_CASES = {
    "u8": (ebc.Geometry(256, 192, 1, 3, 0, 6, raw="gray8"), ebc.RAW_GRAY, ("blank", "white")),
    "rgb8": (ebc.Geometry(160, 128, 3, 3, 1, 4, raw="rgb8"), ebc.RAW_RGB, ("black", "white")),
    "s8": (ebc.Geometry(256, 192, 1, 3, 0, 6, bits=8), ebc.KINDS8, ("full8", "blank8")),
}


@pytest.mark.timeout(300)
@pytest.mark.parametrize("entry", list(FRONT_END_CASES))
def test_mixed_front_end_batches(expected, entry):
    """8-bit gray, packed RGB888 and the uint8 twins (int8 storage, the int8 overflow among them) in mixed batches"""
    g, kinds, odd = FRONT_END_CASES[entry]
    background = [(kinds[(i + 2) % len(kinds)], i) for i in range(6)]
    batches = odd_one_out(background, odd) + [[(k, 0) for k in kinds]]
    enc = api.Encoder(g.w, g.h, g.channels, g.stages, g.filt, g.segments, max_frames=6, sample_bits=g.bits)
    for cls in ebc.QUOTA_CLASSES:
        q = ebc.quota(g, cls)
        for specs in batches:
            got = encode(enc, g, entry, ebc.batch(g, specs), q)
            # (the front ends convert into the encoder's own buffer: the coefficient planes are those of the converted frames)
            check(expected, g, specs, q, got, f"{entry} {cls}", enc)
    assert enc.stats()["unit_timeouts"] == 0
    enc.close()


# ---- route-list edges -----------------------------------------------------------------------------------------------------
def routed_when_blank(emu, g, percent):
    """units route_units_kernel lists for an all-blank frame: every unit of at least 16 chunks whose share of full (64-sample)
    chunks reaches `percent` (a last chunk with fewer samples is never blank)"""
    n, units = emu.plan_units(g.w, g.h, g.channels, g.stages, g.segments)
    npix = units[:, 2].astype(np.int64) * units[:, 3]
    nch, full = (npix + 63) // 64, npix // 64
    return n, int(np.count_nonzero((nch >= 16) & (full * 100 >= percent * nch)))


@pytest.mark.timeout(300)
def test_route_lists_full_and_empty(expected, emu, monkeypatch):
    """a batch of blank frames puts every unit big enough on the list kernel's list, a batch of 12-bit noise none; the same for
    a lone frame cut into sub-ranges (its own threshold, 90 %)"""
    g = ebc.Geometry(512, 384, 1, 2, 0, 2)
    q = ebc.quota(g, "lossless")
    n_units, listed95 = routed_when_blank(emu, g, 95)
    assert listed95 == n_units                          # (this geometry has no unit below 16 chunks or with a partial chunk)
    enc = api.Encoder(g.w, g.h, 1, g.stages, g.filt, g.segments, max_frames=3)
    assert enc.info()["units_per_frame"] == n_units
    for kind, per_frame in (("blank", listed95), ("wide", 0), ("blank", listed95)):
        specs = [(kind, s) for s in range(3)]
        r0 = enc.routing()
        check(expected, g, specs, q, encode(enc, g, "sync", ebc.batch(g, specs), q), kind, enc)
        r1 = enc.routing()
        assert launch_kind(enc) == "hybrid", enc.launch_info()
        assert (r1["routed_units"] - r0["routed_units"], r1["routed_calls"] - r0["routed_calls"]) == (3 * per_frame, 1), (kind, r0, r1)
    enc.close()
    monkeypatch.setenv("ICER_HIP_SPLIT", "128")
    _, listed90 = routed_when_blank(emu, g, 90)
    enc = api.Encoder(g.w, g.h, 1, g.stages, g.filt, g.segments, max_frames=1)
    for kind, per_frame in (("blank", listed90), ("wide", 0), ("blank", listed90)):
        r0 = enc.routing()
        check(expected, g, [(kind, 0)], q, encode(enc, g, "sync", ebc.batch(g, [(kind, 0)]), q), f"lone {kind}", enc)
        r1 = enc.routing()
        assert launch_kind(enc) == "split", enc.launch_info()
        assert (r1["routed_units"] - r0["routed_units"], r1["routed_calls"] - r0["routed_calls"]) == (per_frame, 1), (kind, r0, r1)
    assert enc.stats()["unit_timeouts"] == 0
    enc.close()


# ---- seeded sequences of calls on long-lived encoders ------------------------------------------------------------------------
QUOTA_WEIGHTS = {"lossless": 0.3, "cut": 0.25, "progressive": 0.15, "tiny27": 0.1, "tiny28": 0.1, "tiny60": 0.1}
SEQUENCES = {
    # name: geometry, max_frames, ICER_HIP_SPLIT, entry points, frame kinds, the launch kinds the encoder can reach
    "gray4": (ebc.Geometry(512, 384, 1, 2, 3, 2), 4, "128", ("sync", "async", "host"), ebc.KINDS16,
              {"split", "hybrid", "two-part", "window"}),
    "odd8": (ebc.Geometry(517, 389, 1, 3, 5, 6), 8, None, ("sync", "async", "host"), ebc.KINDS16,
             {"pipeline", "hybrid", "two-part", "window"}),
    "yuv3": (ebc.Geometry(256, 192, 3, 3, 1, 5), 3, None, ("sync", "async", "host"),
             ebc.KINDS16 + (("smooth", "overflow", "smooth"), ("wide", "blank", "noise8")), {"hybrid", "window"}),
    "s8x4": (ebc.Geometry(512, 384, 1, 2, 0, 2, bits=8), 4, "128", ("s8",), ebc.KINDS8, {"split", "hybrid", "two-part", "window"}),
}
CALLS = 48


@pytest.mark.timeout(420)
@pytest.mark.parametrize("name", list(SEQUENCES))
def test_long_lived_encoder_sequence(expected, monkeypatch, name):
    """one encoder, CALLS calls: per call n in [1, max_frames], a quota class, an entry point and the kinds of the frames are
    drawn (seeded).  Slot tables rebuilt for every new quota, route-list cursors per part, sub-range state shared by split and
    unsplit launches, the window coder of progressive mode, the pending record of the asynchronous call: all of it carried from
    call to call.  Every stream equals the oracle's, the caller's buffers keep their promises, and the sequence reaches every
    launch kind its encoder can make."""
    g, mf, split, entries, kinds, reachable = SEQUENCES[name]
    if split:
        monkeypatch.setenv("ICER_HIP_SPLIT", split)
    rng = np.random.default_rng(sum(map(ord, name)))
    enc = api.Encoder(g.w, g.h, g.channels, g.stages, g.filt, g.segments, max_frames=mf, sample_bits=g.bits)
    classes, weights = list(QUOTA_WEIGHTS), list(QUOTA_WEIGHTS.values())
    seen = {}
    for call in range(CALLS):
        n = 1 if rng.random() < 0.25 else int(rng.integers(2, mf + 1))
        cls = classes[int(rng.choice(len(classes), p=weights))]
        entry = entries[int(rng.integers(0, len(entries)))]
        specs = [(kinds[int(rng.integers(0, len(kinds)))], int(rng.integers(0, 2))) for _ in range(n)]
        q = ebc.quota(g, cls)
        got = encode(enc, g, entry, ebc.batch(g, specs), q)
        kind = launch_kind(enc)
        seen[kind] = seen.get(kind, 0) + 1
        check(expected, g, specs, q, got, f"{name} call {call} ({entry}, n={n}, {cls}, {kind})", enc, coef_frames=[int(rng.integers(0, n))])
    print(f"{name}: launch kinds {dict(sorted(seen.items()))}, routing {enc.routing()}, stats {enc.stats()}")
    assert set(seen) == reachable, (name, seen)
    assert enc.stats()["unit_timeouts"] == 0
    enc.close()


# ---- slot retries in the middle of a sequence ---------------------------------------------------------------------------------
RETRY = ebc.Geometry(256, 256, 1, 1, 0, 1)
RETRY_SPECS = [("blank", 0), ("flat", 0), ("noise8", 0), ("dot", 0)]


def slot_area_at_1bpp(emu, g):
    """the slot area of a frame provisioned at 1 bit per sample when no unit is capped by the quota (plan.hpp assign_slots: per unit a
    28-byte header and (samples + 31) / 32 + 16 words): the most ICER_HIP_SLOT_BPP=1 can provision before the first retry"""
    _, units = emu.plan_units(g.w, g.h, g.channels, g.stages, g.segments)
    npix = units[:, 2].astype(np.int64) * units[:, 3]
    return int(np.sum(28 + 4 * ((npix + 31) // 32 + 16)))


def retry_quota(emu, g):
    """a quota above the slot area at 1 bit per sample: the rows an entry point stages for itself are min(quota, slot area) + 4 bytes
    long, so they depend on the slot table and must grow when a retry enlarges it"""
    q = ebc.quota(g, "lossless")
    if q <= slot_area_at_1bpp(emu, g):
        q = 2 * g.w * g.h
    assert q > slot_area_at_1bpp(emu, g)
    return q


@pytest.mark.timeout(300)
@pytest.mark.parametrize("entry", ["sync", "async", "host"])
def test_slot_retry_mid_sequence(expected, emu, monkeypatch, entry):
    """slots provisioned at 1 bit per sample (ICER_HIP_SLOT_BPP, read at create): in a mixed batch only the noise frame outgrows
    its slots and the batch is run again with larger ones (asynchronous: inside the wait; host: with longer staging rows, the quota
    being above the first slot area); the calls after it, at other quotas, rebuild the slot table at the doubled bound.  Every
    stream stays exact."""
    monkeypatch.setenv("ICER_HIP_SLOT_BPP", "1")
    g, specs = RETRY, RETRY_SPECS
    enc = api.Encoder(g.w, g.h, 1, g.stages, g.filt, g.segments, max_frames=4)
    assert enc.info()["slot_bits_per_pixel"] == 1
    q = retry_quota(emu, g)
    assert q > enc.info()["slot_bytes_per_frame"], (q, enc.info())     # (and above what the first call will plan: retry_quota)
    check(expected, g, specs, q, encode(enc, g, entry, ebc.batch(g, specs), q), f"{entry} retry", enc)
    retries = enc.stats()["slot_retries"]
    assert retries >= 1 and enc.info()["slot_bits_per_pixel"] > 1, (enc.stats(), enc.info())
    assert enc.info()["slot_bytes_per_frame"] > slot_area_at_1bpp(emu, g)      # (the staged rows of the first run were too short for the second)
    for cls in ("cut", "progressive", "tiny60", "lossless"):
        q = ebc.quota(g, cls)
        for order in (specs, specs[::-1], specs[:2]):
            check(expected, g, order, q, encode(enc, g, entry, ebc.batch(g, order), q), f"{entry} after the retry, {cls}", enc)
    assert enc.info()["slot_bits_per_pixel"] > 1
    assert enc.stats()["slot_retries"] == retries and enc.stats()["unit_timeouts"] == 0, enc.stats()
    enc.close()


def run_child(code, tmp_path, **env):
    """`code` in a process of its own (the pooled encoders of the host batch and of the lib_icer entry points read the environment when
    they are created, and live as long as the process); returns the JSON object of its last line of output"""
    prologue = f"import json, sys, zlib\nimport numpy as np\nsys.path.insert(0, {ROOT!r})\nfrom icer_compression_amd import api\ntmp = {str(tmp_path)!r}\n"
    r = subprocess.run([sys.executable, "-c", prologue + code], capture_output=True, text=True, timeout=240, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.timeout(300)
def test_slot_retry_inside_the_host_batch_pipeline(expected, emu, tmp_path):
    """icerx_compress_batch_uint16_devices in sub-batches of two: the noise frame of sub-batch 0 outgrows its slots while sub-batch 1 is
    in flight with rows of the old stride; the pipeline re-allocates its rows, codes sub-batch 0 again and issues sub-batch 1 again.
    A second call of the same process, at another quota, runs on the grown slots without a retry."""
    g = RETRY
    specs = [RETRY_SPECS[0], RETRY_SPECS[2], RETRY_SPECS[1], RETRY_SPECS[3]]        # (blank, noise8 | flat, dot)
    quotas = [retry_quota(emu, g), ebc.quota(g, "cut")]
    np.save(tmp_path / "frames.npy", ebc.batch(g, specs))
    got = run_child(f"""
frames = np.load(tmp + "/frames.npy")
n, calls = frames.shape[0], []
for q in {quotas!r}:
    out = np.zeros((n, q + 5), np.uint8); sizes = np.zeros(n, np.uint64); rcs = np.zeros(n, np.int32)
    rc = api.compress_batch(frames, {g.stages}, {g.filt}, {g.segments}, q, out, sizes, rcs, devices=[0])
    calls.append({{"rc": rc, "rcs": rcs.tolist(), "sizes": sizes.tolist(), "crc": [zlib.crc32(out[k, :int(sizes[k])].tobytes()) for k in range(n)],
                  "stats": api.process_stats()}})
print(json.dumps(calls))
""", tmp_path, ICER_HIP_SLOT_BPP="1", ICER_HIP_BATCH_SUB="2")
    for q, call in zip(quotas, got):
        assert call["rc"] == 0, call
        for k, spec in enumerate(specs):
            rc, stream = expected(g, spec, q)[:2]
            assert (call["rcs"][k], call["sizes"][k], call["crc"][k]) == (rc, len(stream), zlib.crc32(stream)), (q, k, spec)
        assert call["stats"]["unit_timeouts"] == 0, call["stats"]
    assert got[0]["stats"]["slot_retries"] >= 1 and got[1]["stats"]["slot_retries"] == got[0]["stats"]["slot_retries"], [c["stats"] for c in got]


@pytest.mark.timeout(300)
def test_slot_retry_inside_the_drop_in_call(expected, emu, tmp_path):
    """icer_compress_image_uint16 on a noise image with slots at 1 bit per sample: the cached encoder runs the image again with larger
    slots and a longer staging row; the stream and the coefficient plane left in the caller's image are the oracle's.  A second image
    in the same process is coded on the grown slots without a retry."""
    g = RETRY
    specs = [("noise8", 0), ("noise8", 1)]
    q = retry_quota(emu, g)
    np.save(tmp_path / "frames.npy", ebc.batch(g, specs))
    got = run_child(f"""
frames = np.load(tmp + "/frames.npy")
calls = []
for k in range(frames.shape[0]):
    rc, stream, planes = api.compress(list(frames[k]), {g.stages}, {g.filt}, {g.segments}, {q})
    np.save(tmp + f"/planes{{k}}.npy", np.stack(planes))
    with open(tmp + f"/stream{{k}}.bin", "wb") as fh:
        fh.write(stream)
    calls.append({{"rc": rc, "stats": api.process_stats()}})
print(json.dumps(calls))
""", tmp_path, ICER_HIP_SLOT_BPP="1")
    for k, spec in enumerate(specs):
        want = expected(g, spec, q)
        ebc.check_frame(got[k]["rc"], (tmp_path / f"stream{k}.bin").read_bytes(), want, f"drop-in call {k} {spec}")
        ebc.check_coefficients(g, list(np.load(tmp_path / f"planes{k}.npy")), want, f"drop-in call {k} {spec}")
        assert got[k]["stats"]["unit_timeouts"] == 0, got[k]["stats"]
    assert got[0]["stats"]["slot_retries"] >= 1 and got[1]["stats"]["slot_retries"] == got[0]["stats"]["slot_retries"], [c["stats"] for c in got]
