"""Re-cutting stored masters to a distortion target or a shared byte budget on the GPU (include/icer_hip_dec_quality.h,
include/icer_hip_sidecar.h): the encoder's sidecar export against its host table and the model's LL means; the target and the
budget call on masters encoded on the device against Encoder.encode_target / encode_budget on the original frames, every output;
cuts at 1/2 size against the model; the chain into the decoder; frames with a status, bad sidecars and refused calls."""
import numpy as np
import pytest

from icer_compression_amd import api, decoder
from tests import budget_model as bm
from tests import encoder_batch_cases as ebc
from tests import reduced_model as red
from tests import target_model as tm
from tests import test_gpu_ladder as tl
from tests import test_gpu_recut as tr
from tests.recut_quality_cases import check_target, header_means, model_of, reduced_view, unit_bits
from tests.test_gpu_budget import budget as encode_budget
from tests.test_gpu_target import frame_means, target as encode_target

pytestmark = pytest.mark.gpu

SENT, SENT_SIZE, SENT_RC = tr.SENT, tr.SENT_SIZE, tr.SENT_RC
SENT64 = 0x5555555555555555
OUT_OF_DATA, INVALID_INPUT, FATAL = -7, -11, -10
FILTERS = {"A": 0, "C": 2, "Q": 6}
YUV = ebc.Geometry(96, 80, 3, 3, 1, 3)
MIXED = {
    "yuv": (YUV, [("smooth", 0), ("noise8", 1), ("blank", 0), ("flat", 1), (("sparse", "dot", "wide"), 2)]),      # (flat: LL means above one byte)
    "gray": (ebc.Geometry(131, 77, 1, 2, 3, 2), [("noise8", 0), ("flat", 1), ("blank", 2), ("wide", 3), ("smooth", 4)]),
    "gray8": (ebc.Geometry(96, 80, 1, 3, 0, 6, bits=8), [("blank8", 0), ("noise6", 1), ("smooth6", 2), ("noise6", 4), ("smooth6", 3)]),
}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    decoder.load_library()
    return torch


def quality_recutter(g, max_reduce=0):
    return decoder.Recutter(g.w, g.h, g.channels, g.stages, g.segments, bits=g.bits, max_reduce=max_reduce, filt=g.filt)


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def quality(torch, r, kind, data, lens, side, cuts, cap, offsets=None, stream_stride=None, reduce=0):
    """recut_target_torch (cuts = [(reduce, mse)]) or recut_budget_torch (cuts = budgets) into Q * n + 1 sentinel rows of an odd
    stride -> (res[c][f] dict as test_gpu_target.target / test_gpu_budget.budget give them, thresholds, totals) after checking the
    buffer promises"""
    n, Q = int(lens.shape[0]), len(cuts)
    stride = (cap + 5) | 1
    dev = data.device
    keep, keep_side = data.clone(), side.clone()
    out = torch.full((Q * n + 1, stride), SENT, dtype=torch.uint8, device=dev)
    sizes, dist, equiv = (torch.full((Q * n + 1,), SENT_SIZE, dtype=torch.int64, device=dev) for _ in range(3))
    rcs, flag = (torch.full((Q * n + 1,), SENT_RC, dtype=torch.int32, device=dev) for _ in range(2))
    thr, tot = (torch.full((Q + 1,), SENT_SIZE, dtype=torch.int64, device=dev) for _ in range(2))
    m = Q * n
    if kind == "target":
        r.recut_target_torch(data, lens, side, cuts, cap, out[:m], sizes[:m], rcs[:m], flag[:m], dist[:m], equiv[:m], offsets=offsets,
                             stream_stride=stream_stride)
    else:
        r.recut_budget_torch(data, lens, side, cuts, cap, out[:m], sizes[:m], rcs[:m], flag[:m], dist[:m], equiv[:m], thr[:Q], tot[:Q],
                             reduce=reduce, offsets=offsets, stream_stride=stream_stride)
    torch.cuda.synchronize()
    assert torch.equal(data, keep) and torch.equal(side, keep_side), "the masters or the sidecars were modified on the device"
    out, sizes, rcs, flag = out.cpu().numpy(), sizes.cpu().numpy(), rcs.cpu().numpy(), flag.cpu().numpy()
    dist, equiv, thr, tot = u64(dist), u64(equiv), u64(thr), u64(tot)
    assert (out[m] == SENT).all(), "bytes written past the Q * n rows of the output"
    for a, s in ((sizes, SENT_SIZE), (rcs, SENT_RC), (flag, SENT_RC), (dist, SENT_SIZE), (equiv, SENT_SIZE)):
        assert int(a[m]) == s, "an output array was written past Q * n entries"
    assert int(thr[Q]) == SENT_SIZE and int(tot[Q]) == SENT_SIZE
    name = "reached" if kind == "target" else "at_cap"
    res = []
    for c in range(Q):
        row = []
        for f in range(n):
            k = c * n + f
            s = int(sizes[k])
            assert 0 <= s <= cap and (out[k, s:] == SENT).all(), f"cut {c} frame {f}: bytes written behind its stream of {s} bytes"
            row.append({"rc": int(rcs[k]), "stream": out[k, :s].tobytes(), name: int(flag[k]), "dist": int(dist[k]), "equiv": int(equiv[k])})
        res.append(row)
    return res, [int(x) for x in thr[:Q]], [int(x) for x in tot[:Q]]


def padded_sidecars(torch, enc, n, pad=3):
    """the sidecars of the last target or budget call in rows of a padded stride; the padding must stay as it was"""
    side = torch.full((n, enc.sidecar_entries + pad), SENT64, dtype=torch.int64, device="cuda")
    enc.distortion_sidecar_torch(n, out=side)
    torch.cuda.synchronize()
    assert (u64(side)[:, enc.sidecar_entries:] == SENT64).all(), "the export wrote behind a row's entries"
    return side


# ---- 1. the sidecar export ----------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("filt", list(FILTERS))
@pytest.mark.parametrize("kind", ["gray16", "yuv16", "gray8", "yuv8"])
def test_sidecar_export_is_the_table_and_the_means(torch, oracle, kind, filt):
    bits, channels = (16 if kind.endswith("16") else 8), (3 if kind.startswith("yuv") else 1)
    g = ebc.Geometry(96, 80, channels, 3, FILTERS[filt], 3, bits=bits)
    specs = [("smooth", 0), ("noise8", 1)] if bits == 16 else [("smooth6", 0), ("blank8", 1)]
    model = model_of(g)
    enc = tr.encoder(g, 3)
    assert enc.sidecar_entries == model.n_families * (model.P + 1) + 1
    lib, h = enc.lib, enc.handle
    dst = torch.full((3, enc.sidecar_entries), SENT64, dtype=torch.int64, device="cuda")
    assert lib.icerx_get_distortion_sidecar_device(h, 1, dst.data_ptr(), enc.sidecar_entries, None) == INVALID_INPUT      # (no table yet)
    t = tl.device_frames(ebc.batch(g, specs))
    cap = ebc.quota(g, "lossless")
    got = encode_target(enc, t, [0.0], cap)
    side = u64(padded_sidecars(torch, enc, 2))
    whole = tl.separate(enc, t, cap)                 # (a target-0 stream ends where the distortion reaches 0: the means are read from complete streams)
    for f, spec in enumerate(specs):
        assert got[0][f]["rc"] in (0, tm.QUOTA_EXCEEDED) and whole[f][0] == 0
        assert np.array_equal(side[f, :-4].reshape(model.n_families, model.P + 1), enc.distortion_table(f, model.n_families)), (kind, filt, f)
        word = int(side[f, enc.sidecar_entries - 1])
        means = [(word >> (16 * c)) & 0xFFFF for c in range(4)]
        assert means[channels:] == [0] * (4 - channels)
        in_header = header_means(whole[f][1], channels)
        if bits == 16:
            assert means[:channels] == frame_means(oracle, g, spec) and [m & 0xFF for m in means[:channels]] == in_header
        else:
            assert means[:channels] == in_header
    for kw in (dict(n=0), dict(n=3), dict(stride=enc.sidecar_entries - 1), dict(dst=None)):       # (the call had two frames)
        a = dict(dict(n=2, stride=enc.sidecar_entries, dst=dst.data_ptr()), **kw)
        assert lib.icerx_get_distortion_sidecar_device(h, a["n"], a["dst"], a["stride"], None) == INVALID_INPUT, kw
    torch.cuda.synchronize()
    assert (u64(dst) == SENT64).all(), "a refused export wrote"
    assert lib.icerx_distortion_sidecar_entries(None) == 0
    enc.close()


# ---- 2. against the encoder on the original frames ------------------------------------------------------------------------------
def masters_and_sidecars(torch, enc, t, g):
    """a target call at target 0 for the sidecars, then the masters at the lossless quota in rows of an odd stride"""
    encode_target(enc, t, [0.0], ebc.quota(g, "lossless"))
    side = padded_sidecars(torch, enc, t.shape[0])
    masters, sizes, rcs = tr.encode_masters(torch, enc, t, ebc.quota(g, "lossless"))
    assert masters.shape[1] % 2 == 1 and [int(x) for x in rcs.cpu()] == [0] * t.shape[0]
    return masters, sizes, side


def as_blob(torch, rng, masters, sizes):
    host, sz = masters.cpu().numpy(), sizes.cpu().numpy()
    return tr.blob_of(torch, rng, [host[f, :int(sz[f])].tobytes() for f in range(len(sz))])


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", list(MIXED))
def test_target_equals_the_encoder(torch, name):
    g, specs = MIXED[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    enc, r = tr.encoder(g, len(specs)), quality_recutter(g)
    assert r.sidecar_entries == enc.sidecar_entries
    t = tl.device_frames(ebc.batch(g, specs))
    masters, sizes, side = masters_and_sidecars(torch, enc, t, g)
    mid = 20.0 if g.bits == 16 else 4.0
    mses = [mid, 0.0, 1e30, mid / 8, mid]
    assert all(r.target_threshold(x) == enc.target_threshold(x) for x in mses + [-1.0, float("nan"), 1e300])
    blob, offsets, lens = as_blob(torch, rng, masters, sizes)
    seen = set()
    for cap in (ebc.quota(g, "lossless"), ebc.quota(g, "progressive")):
        want = encode_target(enc, t, mses, cap)
        seen |= {row["reached"] for cut in want for row in cut}
        got, _, _ = quality(torch, r, "target", masters, sizes, side, [(0, x) for x in mses], cap)
        assert got == want, f"{name}, cap {cap}: rows of an odd stride"
        got, _, _ = quality(torch, r, "target", blob, lens, side, [(0, x) for x in mses], cap, offsets=offsets)
        assert got == want, f"{name}, cap {cap}: d_offsets"
    assert seen == {0, 1}, "over the two caps, both a target that is met and a cut the cap made (8-bit data meets target 0 at the lossless cap)"
    enc.close()
    r.close()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", list(MIXED))
def test_budget_equals_the_encoder(torch, name):
    g, specs = MIXED[name]
    rng = np.random.default_rng(sum(map(ord, name)) + 1)
    enc, r = tr.encoder(g, len(specs)), quality_recutter(g)
    t = tl.device_frames(ebc.batch(g, specs))
    masters, sizes, side = masters_and_sidecars(torch, enc, t, g)
    total = int(sizes.sum())
    budgets = [total // 3, 27, total + 9, total // 11, 0, total]
    blob, offsets, lens = as_blob(torch, rng, masters, sizes)
    for cap in (ebc.quota(g, "lossless"), ebc.quota(g, "cut")):
        want = encode_budget(enc, t, budgets, cap)
        assert quality(torch, r, "budget", masters, sizes, side, budgets, cap) == want, f"{name}, cap {cap}: rows of an odd stride"
        assert quality(torch, r, "budget", blob, lens, side, budgets, cap, offsets=offsets) == want, f"{name}, cap {cap}: d_offsets"
    enc.close()
    r.close()


@pytest.mark.timeout(300)
def test_budget_of_70_small_frames(torch):
    g = ebc.Geometry(32, 24, 1, 2, 0, 1)
    kinds = ("smooth", "noise8", "sparse", "wide", "flat", "dot", "blank")
    specs = [(kinds[k % len(kinds)], k) for k in range(70)]
    enc, r = tr.encoder(g, 70), quality_recutter(g)
    t = tl.device_frames(ebc.batch(g, specs))
    masters, sizes, side = masters_and_sidecars(torch, enc, t, g)
    total, cap = int(sizes.sum()), ebc.quota(g, "lossless")
    budgets = [total // 2, total // 9, 2 * total]
    assert quality(torch, r, "budget", masters, sizes, side, budgets, cap) == encode_budget(enc, t, budgets, cap)
    enc.close()
    r.close()


# ---- 3. cuts at half size ------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", ["gray", "yuv"])
def test_reduce_1_equals_the_model(torch, oracle, name):
    g = {"gray": ebc.Geometry(61, 45, 1, 3, 2, 2), "yuv": ebc.Geometry(61, 45, 3, 3, 0, 2)}[name]
    specs = [("noise8", 0), ("smooth", 1), ("wide", 2)]
    model = model_of(g)
    view, fam_map = reduced_view(model, g, 1)
    enc, r = tr.encoder(g, len(specs)), quality_recutter(g, max_reduce=1)
    t = tl.device_frames(ebc.batch(g, specs))
    masters, sizes, side = masters_and_sidecars(torch, enc, t, g)
    host, sz = masters.cpu().numpy(), sizes.cpu().numpy()
    derived = [red.derive(host[f, :int(sz[f])].tobytes(), 1) for f in range(len(specs))]
    bits = [unit_bits(view, s) for s in derived]
    D = [view.distortions(enc.distortion_table(f, model.n_families)[fam_map], frame_means(oracle, g, specs[f])) for f in range(len(specs))]
    cap = ebc.quota(g, "lossless")
    mses = [sorted(d[len(d) // 2] for d in D)[1] / float(view.samples * 16), 0.0]
    assert all(r.target_threshold(x, 1) == view.threshold(x) for x in mses)
    got, _, _ = quality(torch, r, "target", masters, sizes, side, [(1, x) for x in mses], cap)
    for c, x in enumerate(mses):
        for f in range(len(specs)):
            check_target(got[c][f], tm.target_walk(bits[f], D[f], view.threshold(x), cap), f"{name}: target {c} frame {f}", flag="reached")
    # the equivalent quota through the cuts call, and the budget call at this reduce against the allocation
    cuts = sorted({(1, row["equiv"]) for cut in got for row in cut})
    out = torch.zeros((len(cuts) * len(specs), cap + 3), dtype=torch.uint8, device="cuda")
    cs, cr = torch.zeros(out.shape[0], dtype=torch.int64, device="cuda"), torch.zeros(out.shape[0], dtype=torch.int32, device="cuda")
    r.recut_cuts_torch(masters, sizes, cuts, out, cs, cr)
    torch.cuda.synchronize()
    out, cs, cr = out.cpu().numpy(), cs.cpu().numpy(), cr.cpu().numpy()
    for c in range(len(mses)):
        for f in range(len(specs)):
            k = cuts.index((1, got[c][f]["equiv"])) * len(specs) + f
            assert (int(cr[k]), out[k, :int(cs[k])].tobytes()) == (got[c][f]["rc"], got[c][f]["stream"]), (name, c, f)
    total = sum(len(s) for s in derived)
    budgets = [total // 2, total + 1, 30]
    got, thr, tot = quality(torch, r, "budget", masters, sizes, side, budgets, cap, reduce=1)
    for b, B in enumerate(budgets):
        want, T, total_b = bm.allocate([(bits[f], D[f], False) for f in range(len(specs))], B, cap)
        assert (thr[b], tot[b]) == (T, total_b), (name, B)
        for f, w in enumerate(want):
            x = got[b][f]
            assert (x["rc"], len(x["stream"]), x["at_cap"], x["dist"], x["equiv"]) == (w["rc"], w["size"], w["at_cap"], w["dist"], w["equiv"]), (name, B, f)
    enc.close()
    r.close()


# ---- 4. encoder -> target re-cut -> decoder on one stream ---------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_chain_target_recut_decode_without_the_host(torch):
    g, specs = MIXED["yuv"]
    n, mses = len(specs), [30.0, 0.0]
    cap = ebc.quota(g, "lossless")
    enc, r = tr.encoder(g, n), quality_recutter(g)
    d = decoder.Decoder(g.channels, g.stages, g.filt, g.segments, bits=g.bits)
    st = torch.cuda.Stream()
    try:
        with torch.cuda.stream(st):
            t = tl.device_frames(ebc.batch(g, specs))
            enc.encode_target_torch(t, [0.0], cap)           # (for the energy tables; the masters are complete streams)
            side = enc.distortion_sidecar_torch(n)
            masters, sizes, _ = tr.encode_masters(torch, enc, t, cap)
            Q = len(mses)
            out = torch.zeros((Q, n, cap + 3), dtype=torch.uint8, device="cuda")
            cut_sizes, dist, equiv = (torch.zeros((Q, n), dtype=torch.int64, device="cuda") for _ in range(3))
            cut_rcs, reached = (torch.zeros((Q, n), dtype=torch.int32, device="cuda") for _ in range(2))
            r.recut_target_torch(masters, sizes, side, [(0, x) for x in mses], cap, out, cut_sizes, cut_rcs, reached, dist, equiv)
            planes = torch.full((Q, n, g.channels, g.w * g.h), 0x5A, dtype=torch.int16, device="cuda")
            rcs = torch.full((Q, n), 77, dtype=torch.int32, device="cuda")
            ws, hs = torch.zeros((Q, n), dtype=torch.int64, device="cuda"), torch.zeros((Q, n), dtype=torch.int64, device="cuda")
            for q in range(Q):                               # (a cut's block goes into the decoder as it is)
                d.decode_torch(out[q], cut_sizes[q], planes[q], rcs[q], ws[q], hs[q])
        st.synchronize()
        want = encode_target(enc, t, mses, cap)
        for q in range(Q):
            res = d.decode_host([row["stream"] for row in want[q]], g.w * g.h)[1]
            for f in range(n):
                assert int(cut_sizes[q, f]) == len(want[q][f]["stream"])
                for c in range(g.channels):
                    assert int(rcs[q, f]) == res[f][0] and np.array_equal(planes[q, f, c].cpu().numpy().view(np.uint16), res[f][3][c]), (q, f, c)
    finally:
        d.close()
        enc.close()
        r.close()


# ---- 5. frames with a status, bad sidecars, refused calls -----------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_statuses_bad_sidecars_and_refusals(torch, oracle):
    g = YUV
    specs = [("noise8", 0), ("smooth", 1), (("smooth", "overflow", "smooth"), 2)]          # (the last one: the encoder drops it)
    model = model_of(g)
    enc, r = tr.encoder(g, len(specs)), quality_recutter(g)
    t = tl.device_frames(ebc.batch(g, specs))
    cap = ebc.quota(g, "lossless")
    mses = [10.0, 0.0]
    want = encode_target(enc, t, mses, cap)
    side = padded_sidecars(torch, enc, len(specs))
    masters, sizes, rcs = tr.encode_masters(torch, enc, t, cap)
    assert [int(x) for x in rcs.cpu()] == [0, 0, -1]
    host, sz = masters.cpu().numpy(), sizes.cpu().numpy()
    good = [host[f, :int(sz[f])].tobytes() for f in range(2)]
    other = ebc.Geometry(64, 48, 3, 3, 1, 3)
    alien = oracle.compress(ebc.oracle_planes(other, ("smooth", 0)), other.stages, other.filt, other.segments, ebc.quota(other, "lossless"))[1]
    rows = u64(side).copy()
    P1 = model.P + 1
    bad_mono, bad_bound = rows[0].copy(), rows[0].copy()
    bad_mono[5 * P1 + 3] = bad_mono[5 * P1 + 4] + np.uint64(1)
    fam = model.families[7]
    bad_bound[7 * P1 + model.P] = np.uint64(fam[3] * fam[4] * 32767 * 32767 + 1)
    streams = [good[0], good[1], b"", alien, good[0], good[0], good[1]]          # (frame 2: the dropped frame's empty master)
    side_rows = [rows[0], rows[1], rows[2], rows[0], bad_mono, bad_bound, rows[1]]
    status = {2: OUT_OF_DATA, 3: INVALID_INPUT, 4: INVALID_INPUT, 5: INVALID_INPUT}
    same_as = {0: 0, 1: 1, 6: 1}
    blob, offsets, lens = tr.blob_of(torch, np.random.default_rng(21), streams)
    side2 = torch.from_numpy(np.stack(side_rows).view(np.int64)).cuda()
    got, _, _ = quality(torch, r, "target", blob, lens, side2, [(0, x) for x in mses], cap, offsets=offsets)
    for c in range(len(mses)):
        for f in range(len(streams)):
            if f in status:
                assert got[c][f] == dict(rc=status[f], stream=b"", reached=0, dist=0, equiv=cap), (c, f, got[c][f]["rc"])
            else:
                assert got[c][f] == want[c][same_as[f]], (c, f)
        assert dict(want[c][2], rc=OUT_OF_DATA) == got[c][2]              # (the encoder's own row of the dropped frame, but for the code)
    bits = {f: unit_bits(model, streams[f]) for f in same_as}
    D = {f: model.distortions(rows[k][:-4].reshape(model.n_families, P1), frame_means(oracle, g, specs[k])) for f, k in same_as.items()}
    frames = [(bits[f], D[f], False) if f in same_as else ([], [0], status[f]) for f in range(len(streams))]
    total = sum(len(streams[f]) for f in same_as)
    budgets = [total // 2, total]
    gotb, thr, tot = quality(torch, r, "budget", blob, lens, side2, budgets, cap, offsets=offsets)
    for b, B in enumerate(budgets):
        wb, T, total_b = bm.allocate(frames, B, cap)
        assert (thr[b], tot[b]) == (T, total_b)
        for f, w in enumerate(wb):
            x = gotb[b][f]
            assert (x["rc"], len(x["stream"]), x["at_cap"], x["dist"], x["equiv"]) == (w["rc"], w["size"], w["at_cap"], w["dist"], w["equiv"]), (B, f)
    # refused calls write nothing
    n, Q = len(streams), 2
    stride = cap + 5
    out = torch.full((Q * n, stride), SENT, dtype=torch.uint8, device="cuda")
    sizes_o, dist, equiv = (torch.full((Q * n,), SENT_SIZE, dtype=torch.int64, device="cuda") for _ in range(3))
    rcs_o, flag = (torch.full((Q * n,), SENT_RC, dtype=torch.int32, device="cuda") for _ in range(2))
    thr_o, tot_o = (torch.full((Q,), SENT_SIZE, dtype=torch.int64, device="cuda") for _ in range(2))
    plain = tr.recutter(g)
    for kind in ("target", "budget"):
        need = (r.target_workspace_bytes if kind == "target" else r.budget_workspace_bytes)(n, blob.numel(), Q)
        work = torch.full((need,), 0xCD, dtype=torch.uint8, device="cuda")
        base = dict(n=n, d_data=blob.data_ptr(), data_bytes=blob.numel(), d_offsets=offsets.data_ptr(), stream_stride=0, d_lens=lens.data_ptr(),
                    d_sidecar=side2.data_ptr(), sidecar_stride=side2.shape[1], byte_cap=cap, d_out=out.data_ptr(), out_stride=stride,
                    d_sizes=sizes_o.data_ptr(), d_rcs=rcs_o.data_ptr(), d_dist=dist.data_ptr(), d_equiv_quota=equiv.data_ptr(),
                    d_workspace=work.data_ptr(), workspace_bytes=need, stream=0)
        if kind == "target":
            base.update(reduces=[0, 0], targets_mse=mses, d_reached=flag.data_ptr())
            cases = {"17 cuts": dict(reduces=[0] * 17, targets_mse=[1.0] * 17), "a reduce above max_reduce": dict(reduces=[0, 1]),
                     "a negative target": dict(targets_mse=[1.0, -1.0]), "a NaN target": dict(targets_mse=[float("nan"), 1.0]),
                     "null reached": dict(d_reached=None), "null targets": dict(targets_mse=None, n_cuts=2)}
        else:
            base.update(reduce=0, budgets=budgets, d_at_cap=flag.data_ptr(), d_threshold=thr_o.data_ptr(), d_total=tot_o.data_ptr())
            cases = {"17 budgets": dict(budgets=[9] * 17), "a reduce above max_reduce": dict(reduce=1), "null budgets": dict(budgets=None, n_budgets=2),
                     "null threshold": dict(d_threshold=None), "null total": dict(d_total=None), "null at_cap": dict(d_at_cap=None)}
        cases.update({"no frames": dict(n=0), "too many frames": dict(n=65536), "null data": dict(d_data=None), "null lens": dict(d_lens=None),
                      "null sidecar": dict(d_sidecar=None), "null out": dict(d_out=None), "null sizes": dict(d_sizes=None), "null rcs": dict(d_rcs=None),
                      "null dist": dict(d_dist=None), "null equiv": dict(d_equiv_quota=None), "null workspace": dict(d_workspace=None),
                      "stride below the cap": dict(out_stride=cap - 1), "sidecar stride below the entries": dict(sidecar_stride=r.sidecar_entries - 1),
                      "a workspace one byte short": dict(workspace_bytes=need - 1)})
        for what, kw in cases.items():
            fn = r.recut_target_device_async_ptrs if kind == "target" else r.recut_budget_device_async_ptrs
            assert fn(**dict(base, **kw)) == INVALID_INPUT, f"{kind}: {what}"
        assert (r.recut_target_device_async_ptrs if kind == "target" else r.recut_budget_device_async_ptrs)(**dict(base, data_bytes=0xFFFFFFFF - 64)) == FATAL
        assert (plain.recut_target_device_async_ptrs if kind == "target" else plain.recut_budget_device_async_ptrs)(**base) == INVALID_INPUT, "a plain recutter"
        torch.cuda.synchronize()
        for a, s in ((out, SENT), (sizes_o, SENT_SIZE), (dist, SENT_SIZE), (equiv, SENT_SIZE), (rcs_o, SENT_RC), (flag, SENT_RC), (thr_o, SENT_SIZE),
                     (tot_o, SENT_SIZE), (work, 0xCD)):
            assert bool((a == s).all()), f"{kind}: a refused call wrote"
    assert plain.sidecar_entries == 0 and plain.target_workspace_bytes(n, blob.numel(), Q) == 0
    plain.close()
    enc.close()
    r.close()


# ---- 6. the host conveniences ---------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_bytes_in_bytes_out(torch):
    g, specs = MIXED["gray"]
    enc, r = tr.encoder(g, len(specs)), quality_recutter(g)
    t = tl.device_frames(ebc.batch(g, specs))
    cap = ebc.quota(g, "lossless")
    encode_target(enc, t, [0.0], cap)
    rows = u64(enc.distortion_sidecar_torch(len(specs)))
    masters = [s for _, s in tl.separate(enc, t, cap)]
    mses = [15.0, 0.0]
    assert r.recut_target(masters, rows, [(0, x) for x in mses], cap) == encode_target(enc, t, mses, cap)
    budgets = [sum(map(len, masters)) // 4, 10 ** 9]
    want = encode_budget(enc, t, budgets, cap)
    assert r.recut_budget(masters, rows, budgets, cap) == want
    enc.close()
    r.close()
