"""Quality-targeted encode on the GPU (icerx_encode_device_target, include/icer_hip.h) against the plain model of
tests/target_model.py: the families' energy table equals numpy's from the encoder's own coefficient planes; every stream is
the one a separate icerx_encode_device (or _s8) call makes at the reported equivalent quota; the cut is the first at which
the distortion recomputed in Python meets the threshold, or the byte cap's; nothing is written behind a stream or beyond the
rows; a refused call writes nothing."""
import ctypes as C

import numpy as np
import pytest

from icer_compression_amd import api, decoder
from tests import encoder_batch_cases as ebc
from tests import target_model as tm
from tests import test_gpu_encoder_batch as tb
from tests.test_gpu_ladder import device_frames, separate

pytestmark = pytest.mark.gpu

SENT, SENT_SIZE, SENT_RC = tb.SENT, tb.SENT_SIZE, tb.SENT_RC
HUGE = 1e30                                   # an MSE no frame has: met by the empty stream


def target(enc, t, targets, cap):
    """icerx_encode_device_target on the cuda tensor `t` into T * n + 1 rows / entries filled with sentinels (rows of odd
    stride).  Returns per [target][frame] a dict of rc, stream, reached, dist, equiv, after checking the buffer promises."""
    import torch
    n, T = t.shape[0], len(targets)
    stride = cap + 5
    keep = t.clone()
    dev = t.device
    out = torch.full((T * n + 1, stride), SENT, dtype=torch.uint8, device=dev)
    sizes, dist, equiv = (torch.full((T * n + 1,), SENT_SIZE, dtype=torch.int64, device=dev) for _ in range(3))
    rcs, reached = (torch.full((T * n + 1,), SENT_RC, dtype=torch.int32, device=dev) for _ in range(2))
    enc.encode_target_ptrs(t.data_ptr(), n, targets, cap, out.data_ptr(), stride, sizes.data_ptr(), rcs.data_ptr(), reached.data_ptr(),
                           dist.data_ptr(), equiv.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(t, keep), "the input frames were modified on the device"
    out, sizes, rcs, reached = out.cpu().numpy(), sizes.cpu().numpy(), rcs.cpu().numpy(), reached.cpu().numpy()
    dist, equiv = dist.cpu().numpy().view(np.uint64), equiv.cpu().numpy().view(np.uint64)
    assert (out[T * n] == SENT).all(), "bytes written past the T * n rows of the output"
    for a, s in ((sizes, SENT_SIZE), (rcs, SENT_RC), (reached, SENT_RC), (dist, SENT_SIZE), (equiv, SENT_SIZE)):
        assert int(a[T * n]) == s, "an output array was written past T * n entries"
    res = []
    for q in range(T):
        row = []
        for f in range(n):
            k = q * n + f
            s = int(sizes[k])
            assert 0 <= s <= cap, (q, f, s, cap)
            assert (out[k, s:] == SENT).all(), f"target {q} frame {f}: bytes written behind its stream of {s} bytes"
            row.append(dict(rc=int(rcs[k]), stream=out[k, :s].tobytes(), reached=int(reached[k]), dist=int(dist[k]), equiv=int(equiv[k])))
        res.append(row)
    return res


def check_call(orc, enc, g, model, specs, t, targets, cap, got, what):
    """checks 1-3 of a finished call; returns the (target, frame) pairs whose target was met below the cap"""
    n = t.shape[0]
    at_cap = separate(enc, t, cap)
    tables = [enc.distortion_table(f, model.n_families) for f in range(n)]   # (before any other target call; separate calls leave it alone)
    memo = {cap: at_cap}
    met = []
    for f in range(n):
        if at_cap[f][0] == api.ICER_INTEGER_OVERFLOW:            # a skipped frame: no stream at any target
            for q in range(len(targets)):
                r = got[q][f]
                assert (r["rc"], r["stream"], r["reached"], r["dist"], r["equiv"]) == (-1, b"", 0, 0, cap), (what, q, f, r)
            continue
        words = [enc.coefficients(f, c) for c in range(g.channels)]
        assert np.array_equal(tables[f], model.energy_table(words)), f"{what}: frame {f}: the energy table is not numpy's"
        D = model.distortions(tables[f], frame_means(orc, g, specs[f]))
        for q, mse in enumerate(targets):
            r = got[q][f]
            T = enc.target_threshold(mse)
            assert T == model.threshold(mse)
            K = len(tm.parse_stream(r["stream"]))
            assert r["rc"] == (tm.QUOTA_EXCEEDED if K < model.n_units else 0), (what, q, f, K, r["rc"])
            assert r["dist"] == D[K], (what, q, f, K)
            if r["reached"]:
                assert D[K] <= T and (K == 0 or D[K - 1] > T), (what, q, f, K, D[K], T)
                met.append((q, f))
            else:
                assert D[K] > T and (r["rc"], r["stream"]) == at_cap[f], f"{what}: target {q} frame {f}: not the stream at the cap"
            if K >= 1:
                if r["equiv"] not in memo:
                    memo[r["equiv"]] = separate(enc, t, r["equiv"])
                w = memo[r["equiv"]][f]
                assert (r["rc"], r["stream"]) == w, f"{what}: target {q} frame {f}: K {K}, {len(r['stream'])} bytes, the separate call at " \
                    f"{r['equiv']} gives rc {w[0]} / {len(w[1])} bytes, first difference at {ebc.first_difference(r['stream'], w[1])}"
    return met, at_cap, tables


def frame_means(orc, g, spec):
    """the LL means of a frame's channels (16-bit encoders: the part above one byte is lost in the packet header and counts in D)"""
    return tm.ll_means(orc, ebc.oracle_planes(g, spec), g.stages, g.filt) if g.bits == 16 else None


def shuffled_targets(rng, mid):
    ts = [0.0, mid, mid, HUGE]
    order = rng.permutation(4)
    return [ts[i] for i in order], {name: [int(np.flatnonzero(order == i)[0]) for i in idx] for name, idx in
                                     (("zero", [0]), ("mid", [1, 2]), ("huge", [3]))}


GEOMETRIES = {
    # name: (geometry, max_frames, mid MSE, batches of specs)
    "ragged": (ebc.Geometry(97, 61, 1, 3, 0, 5), 3, 20.0, [[("smooth", 0), ("noise8", 1), ("sparse", 0)]]),
    "lone": (ebc.Geometry(512, 384, 1, 2, 3, 1), 1, 30.0, [[("noise8", 0)], [("smooth", 2)]]),
    "s8": (ebc.Geometry(256, 192, 1, 3, 0, 6, bits=8), 4, 6.0, [[("noise6", 0), ("smooth6", 1), ("blank8", 2), ("full8", 3)]]),
    "yuv": (ebc.Geometry(128, 96, 3, 3, 1, 5), 3, 25.0, [[("smooth", 0), ("noise8", 0), (("smooth", "overflow", "smooth"), 1)]]),
    "mixed": (ebc.Geometry(256, 192, 1, 3, 0, 6), 9, 12.0, [[("noise8", 0), ("blank", 0), ("smooth", 1), ("wide", 0), ("dot", 3)]]),
}


@pytest.mark.timeout(300)
@pytest.mark.parametrize("cap_class", ["lossless", "progressive"])
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_target_streams_tables_and_cuts(oracle, monkeypatch, name, cap_class):
    g, mf, mid, batches = GEOMETRIES[name]
    if name == "lone":
        monkeypatch.setenv("ICER_HIP_SPLIT", "128")            # (sub-ranges of 128 chunks: the lone frame's split launch shape)
    model = tm.Model(g.w, g.h, g.channels, g.stages, g.filt, g.segments, g.bits)
    if g.bits == 16:                                             # (the model's packet order is the oracle's)
        assert [p[:4] for p in tm.packets(g.stages, g.channels, 9)] == [p[:4] for p in oracle.packets(g.stages, g.channels)]
    rng = np.random.default_rng(sum(map(ord, name + cap_class)))
    cap = ebc.quota(g, cap_class)
    enc = api.Encoder(g.w, g.h, g.channels, g.stages, g.filt, g.segments, max_frames=mf, sample_bits=g.bits)
    assert model.n_units == enc.info()["units_per_frame"]
    seen_zero = seen_met = 0
    for b, specs in enumerate(batches):
        targets, where = shuffled_targets(rng, mid)
        t = device_frames(ebc.batch(g, specs))
        got = target(enc, t, targets, cap)
        if name == "mixed" and cap_class == "lossless":
            assert enc.parts() == 2, enc.parts()
        if name == "lone" and cap_class == "lossless":
            assert enc.launch_info()["split"], enc.launch_info()
        met, at_cap, tables = check_call(oracle, enc, g, model, specs, t, targets, cap, got, f"{name} {cap_class} batch {b}")
        seen_met += len(met)
        for f in range(len(specs)):
            if at_cap[f][0] == api.ICER_INTEGER_OVERFLOW:
                continue
            z, (m1, m2), hg = got[where["zero"][0]][f], (got[q][f] for q in where["mid"]), got[where["huge"][0]][f]
            assert m1 == m2, "a repeated target gave two different rows"
            assert hg["stream"] == b"" and hg["reached"] == 1 and hg["rc"] == tm.QUOTA_EXCEEDED
            # target 0 is the stream at the cap wherever the last unit the cap keeps still takes distortion out (or none reaches 0)
            D = model.distortions(tables[f], frame_means(oracle, g, specs[f]))
            Kcap = len(tm.parse_stream(at_cap[f][1]))
            if Kcap == 0 or D[Kcap - 1] > 0:
                assert (z["rc"], z["stream"]) == at_cap[f], f"{name} frame {f}: target 0 is not the stream at the cap"
                seen_zero += 1
    assert seen_zero >= 1 and seen_met >= 2, (seen_zero, seen_met)
    # one stream through the decoder beside the separate call's
    f = 0
    r = got[where["mid"][0]][f]
    if r["stream"]:
        dec = decoder.Decoder(g.channels, g.stages, g.filt, g.segments, bits=g.bits)
        w = separate(enc, t, r["equiv"])[f][1]
        rc, frames = dec.decode_host([r["stream"], w], g.w * g.h)
        assert rc == 0 and frames[0][:3] == frames[1][:3] == (0, g.w, g.h)
        assert all(np.array_equal(a, b) for a, b in zip(frames[0][3], frames[1][3]))
        dec.close()
    assert enc.stats()["unit_timeouts"] == 0
    enc.close()


@pytest.mark.timeout(300)
def test_kept_grid_geometry_has_more_families_than_segments(oracle):
    """71 x 172 YUV, 5 stages, 16 segments (found by tests/test_gpu_geometry_sweep.py): the level-5 subbands have fewer samples
    than segments, their planes keep the rectangles of the packet before them (quirk P1, csrc/plan.hpp) and every distinct
    rectangle is a family: the energy table has more rows than units / 9"""
    g = ebc.Geometry(71, 172, 3, 5, 6, 16)
    specs = [("wide", 0), ("noise8", 1), ("smooth", 0)]
    model = tm.Model(g.w, g.h, g.channels, g.stages, g.filt, g.segments)
    assert model.stale and model.n_families > model.n_units // 9
    enc = api.Encoder(g.w, g.h, g.channels, g.stages, g.filt, g.segments, max_frames=3)
    assert enc.info()["units_per_frame"] == model.n_units
    t = device_frames(ebc.batch(g, specs))
    targets, cap = [0.0, 40.0, HUGE], ebc.quota(g, "lossless")
    got = target(enc, t, targets, cap)
    with pytest.raises(api.IcerHipError):
        enc.distortion_table(1)                                  # (units / 9 rows: not this geometry's table)
    assert enc.distortion_table(1, model.n_families).shape == (model.n_families, 10)
    met, _, _ = check_call(oracle, enc, g, model, specs, t, targets, cap, got, "kept grid")
    assert len(met) >= 3
    assert enc.stats()["unit_timeouts"] == 0
    enc.close()


@pytest.mark.timeout(300)
def test_target_slot_retry(oracle, monkeypatch):
    """slots of 1 bit per sample: the noise frame outgrows them where the cap makes the cut, the batch is redone with larger slots"""
    monkeypatch.setenv("ICER_HIP_SLOT_BPP", "1")
    g = ebc.Geometry(256, 256, 1, 1, 0, 1)
    model = tm.Model(g.w, g.h, 1, g.stages, g.filt, g.segments)
    enc = api.Encoder(g.w, g.h, 1, g.stages, g.filt, g.segments, max_frames=4)
    assert enc.info()["slot_bits_per_pixel"] == 1
    specs = [("blank", 0), ("flat", 0), ("noise8", 0), ("dot", 0)]
    t = device_frames(ebc.batch(g, specs))
    targets, cap = [0.0, 3.0, HUGE], ebc.quota(g, "lossless")
    got = target(enc, t, targets, cap)
    assert enc.stats()["slot_retries"] >= 1 and enc.info()["slot_bits_per_pixel"] > 1, (enc.stats(), enc.info())
    check_call(oracle, enc, g, model, specs, t, targets, cap, got, "after the retry")
    assert enc.stats()["unit_timeouts"] == 0
    enc.close()


@pytest.mark.timeout(300)
def test_psnr_targets_and_torch_outputs():
    import torch
    g = ebc.Geometry(256, 192, 1, 3, 0, 6, bits=8)
    enc = api.Encoder(g.w, g.h, 1, g.stages, g.filt, g.segments, max_frames=2, sample_bits=8)
    t = device_frames(ebc.batch(g, [("noise6", 0), ("smooth6", 0)]))
    cap = ebc.quota(g, "lossless")
    out, sizes, rcs, reached, dist, equiv = enc.encode_target_torch(t, [30.0, 40.0], cap, psnr=True)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (2, 2, cap) and all(tuple(x.shape) == (2, 2) for x in (sizes, rcs, reached, dist, equiv))
    for q, db in enumerate((30.0, 40.0)):
        T = enc.target_threshold(255.0 ** 2 / 10 ** (db / 10))
        assert T == int(255.0 ** 2 / 10 ** (db / 10) * float(g.samples * 16))
        for f in range(2):
            assert int(reached[q, f]) == 1 and int(dist[q, f]) <= T
    assert (sizes[1] >= sizes[0]).all().item()                  # (a higher PSNR never takes fewer bytes)
    enc.close()


@pytest.mark.timeout(300)
def test_invalid_target_calls_write_nothing():
    import torch
    g = tb.GRAY
    enc = api.Encoder(g.w, g.h, 1, g.stages, g.filt, g.segments, max_frames=3)
    dev = torch.device("cuda", 0)
    t = device_frames(ebc.batch(g, [("smooth", 0), ("noise8", 0), ("sparse", 0)]))
    keep = t.clone()
    targets, cap = [4.0, 0.0], ebc.quota(g, "cut")
    T, n, stride = len(targets), 3, cap + 5
    out = torch.full((T * n, stride), SENT, dtype=torch.uint8, device=dev)
    sizes, dist, equiv = (torch.full((T * n,), SENT_SIZE, dtype=torch.int64, device=dev) for _ in range(3))
    rcs, reached = (torch.full((T * n,), SENT_RC, dtype=torch.int32, device=dev) for _ in range(2))
    st = torch.cuda.current_stream(dev).cuda_stream
    L = enc.lib

    def call(handle=enc.handle, frames=t.data_ptr(), nf=n, ts=targets, nt=None, c=cap, o=out.data_ptr(), s=stride, sz=sizes.data_ptr(),
             rc=rcs.data_ptr(), re=reached.data_ptr(), di=dist.data_ptr(), eq=equiv.data_ptr()):
        arr = None if ts is None else (C.c_double * max(len(ts), 1))(*ts)
        return L.icerx_encode_device_target(handle, frames, nf, arr, len(ts) if nt is None else nt, c, o, s, sz, rc, re, di, eq, st)

    cases = {
        "no targets": dict(nt=0), "17 targets": dict(ts=[1.0] * 17), "a NaN target": dict(ts=[1.0, float("nan")]),
        "a negative target": dict(ts=[-1.0, 1.0]), "null encoder": dict(handle=None), "null frames": dict(frames=None),
        "null targets": dict(ts=None, nt=2), "null out": dict(o=None), "null sizes": dict(sz=None), "null rcs": dict(rc=None),
        "null reached": dict(re=None), "null dist": dict(di=None), "null equiv": dict(eq=None), "no frames": dict(nf=0),
        "too many frames": dict(nf=4), "stride below the cap": dict(s=cap - 1),
    }
    for what, kw in cases.items():
        assert call(**kw) == api.ICER_INVALID_INPUT, what
    side = torch.full((n, stride), SENT, dtype=torch.uint8, device=dev)
    s_sizes, s_rcs = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    enc.encode_device_async_ptrs(t.data_ptr(), n, cap, side.data_ptr(), stride, s_sizes.data_ptr(), s_rcs.data_ptr(), st)
    assert call() == api.ICER_INVALID_INPUT, "pending asynchronous encode"
    enc.wait()
    torch.cuda.synchronize()
    untouched = (out == SENT).all().item() and all((x == SENT_SIZE).all().item() for x in (sizes, dist, equiv)) and \
        all((x == SENT_RC).all().item() for x in (rcs, reached))
    assert untouched, "a refused call wrote"
    assert torch.equal(t, keep)
    with pytest.raises(api.IcerHipError):
        enc.distortion_table(0)                                  # (no target call has been made)
    assert call() == 0                                           # (the same arguments are accepted once nothing is pending)
    torch.cuda.synchronize()
    assert not (sizes == SENT_SIZE).any().item() and not (reached == SENT_RC).any().item()
    assert enc.distortion_table(2).shape == (enc.info()["units_per_frame"] // 9, 10)
    enc.close()
