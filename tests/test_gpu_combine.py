"""icerx_combine_device_async / decoder.Recutter.combine_torch on the GPU (icer_compression_amd/csrc/combine.hpp): the difference
and the union of two stored cuts of a frame.  Masters are encoded on the device at the lossless quota; one recut_roi_torch call
delivers the held and the wanted cut side by side; DIFFERENCE runs straight on that call's output block, UNION on a blob of the
held cut and the increment; everything equals tests/combine_model.py on the same bytes.  The increment appended to the held cut
decodes as the union does; lens written by a torch kernel on the same stream need no synchronisation; two calls are in flight on
two streams; a refused call and a frame whose row is too small write nothing where they must not.  (The same source runs on the
CPU in tests/test_combine_mock.py.)"""
import numpy as np
import pytest

from icer_compression_amd import decoder
from tests import combine_model as cm
from tests import encoder_batch_cases as ebc
from tests import roi_cases as rc
from tests import test_gpu_ladder as tl
from tests import test_gpu_recut as tg
from tests import test_gpu_roi as tgr
from tests.decoder_batch_cases import oracle_decode
from tests.sweep_cut_cases import reads_on
from tests.test_gpu_recut import torch                      # noqa: F401  (fixture)
from tests.test_gpu_recut_roi import rois_on_the_stream

pytestmark = pytest.mark.gpu

SENT, SENT_SIZE, SENT_RC, SENT_U32 = tg.SENT, tg.SENT_SIZE, tg.SENT_RC, tgr.SENT_U32
OUT_OF_DATA, INVALID_INPUT = tg.OUT_OF_DATA, tg.INVALID_INPUT
PAIRS = ("nested", "viewport")
_CASES = {}


def case(torch, name):
    """Once per geometry: the masters of batch 0 encoded on the device at the lossless quota, and per pair the output block of ONE
    recut_roi_torch call -- (2 n, stride) rows, the held cuts in rows 0 .. n - 1 and the wanted cuts in rows n .. 2 n - 1 -- with
    its sizes.  nested: cuts (shift 0, S // 4) and (shift 0, S // 2 + S // 8) of the n masters.  viewport: the cut
    (shift 3, S // 4) of the masters taken twice, with the `segment` rectangle the first time and the `border` one the second."""
    if name in _CASES:
        return _CASES[name]
    g, specs, m = rc.GEOMETRIES[name], rc.BATCHES[name][0], rc.model(name)
    n, S = len(specs), g.samples
    enc, r = tg.encoder(g, rc.MAX_FRAMES[0]), tg.recutter(g)
    masters, sizes, enc_rcs = tg.encode_masters(torch, enc, tl.device_frames(ebc.batch(g, specs)), rc.quotas(name)[0])
    assert [int(x) for x in enc_rcs.cpu()] == [0 if rc.has_stream(s) else -1 for s in specs]
    enc.close()
    stride = (S // 2 + S // 8 + 5) | 1
    blocks = {}
    for pair in PAIRS:
        out = torch.full((2 * n, stride), SENT, dtype=torch.uint8, device="cuda")
        osz = torch.zeros(2 * n, dtype=torch.int64, device="cuda")
        rcs, kept, fg = (torch.zeros(2 * n, dtype=torch.int32, device="cuda") for _ in range(3))
        if pair == "nested":
            r.recut_roi_torch(masters, sizes, rois_on_the_stream(torch, [rc.rectangle(m, "full")] * n),
                              [(0, S // 4, 0), (0, S // 2 + S // 8, 0)], out, osz, rcs, kept, fg)
        else:
            rects = [rc.rectangle(m, "segment")] * n + [rc.rectangle(m, "border")] * n
            offsets = (torch.arange(n, dtype=torch.int64, device="cuda") * masters.stride(0)).repeat(2)
            r.recut_roi_torch(masters, sizes.repeat(2), rois_on_the_stream(torch, rects), [(0, S // 4, 3)], out, osz, rcs, kept, fg,
                              offsets=offsets)
        blocks[pair] = (out, osz)
    _CASES[name] = (g, specs, m, r, blocks)
    return _CASES[name]


def rows_of(block, sizes):
    host, sz = block.cpu().numpy(), sizes.cpu().numpy()
    return [host[k, : int(sz[k])].tobytes() for k in range(host.shape[0])]


def combine(torch, r, data, op, lens_a, lens_b, stride, **kw):
    """combine_torch into n + 1 rows / entries and 2 n + 2 counts filled with a sentinel.  Returns the device tensors (out, sizes) of
    the n frames and res[f] = (rc, stream, packets, from A, size) after checking the buffer promises; a frame with
    ICER_OUTPUT_BUF_TOO_SMALL has b"" for a stream and an untouched row"""
    n = int(lens_a.shape[0])
    keep = data.clone()
    out = torch.full((n + 1, stride), SENT, dtype=torch.uint8, device="cuda")
    sizes = torch.full((n + 1,), SENT_SIZE, dtype=torch.int64, device="cuda")
    rcs = torch.full((n + 1,), SENT_RC, dtype=torch.int32, device="cuda")
    counts = torch.full((2 * n + 2,), SENT_U32, dtype=torch.int32, device="cuda")
    r.combine_torch(data, op, lens_a, lens_b, out[:n], sizes[:n], rcs[:n], counts[: 2 * n], **kw)
    torch.cuda.synchronize()
    assert torch.equal(data, keep), "the blob was modified on the device"
    return (out[:n], sizes[:n]), read(out, sizes, rcs, counts, n)


def read(out, sizes, rcs, counts, n):
    stride = out.shape[1]
    out, sizes, rcs, counts = out.cpu().numpy(), sizes.cpu().numpy(), rcs.cpu().numpy(), counts.cpu().numpy()
    assert (out[n] == SENT).all() and int(sizes[n]) == SENT_SIZE and int(rcs[n]) == SENT_RC, "written past the n rows / entries"
    assert (counts[2 * n:] == SENT_U32).all(), "counts written past 2 n"
    res = []
    for f in range(n):
        code, s = int(rcs[f]), int(sizes[f])
        if code == cm.TOO_SMALL:
            assert s > stride and (out[f] == SENT).all(), f"frame {f}: a row that is too small was written"
            res.append((code, b"", int(counts[2 * f]), int(counts[2 * f + 1]), s))
            continue
        assert 0 <= s <= stride and (out[f, s:] == SENT).all(), f"frame {f}: bytes written behind its stream of {s} bytes"
        res.append((code, out[f, :s].tobytes(), int(counts[2 * f]), int(counts[2 * f + 1]), s))
    return res


def difference_then_union(torch, name, pair):
    """-> (g, specs, m, H, W, (inc tensors, inc results), (union tensors, union results)): DIFFERENCE on the re-cut's output block as
    it is, UNION on a blob of the held rows and the increments"""
    g, specs, m, r, blocks = case(torch, name)
    block, osz = blocks[pair]
    n, stride = len(specs), block.shape[1]
    both = rows_of(block, osz)
    H, W = both[:n], both[n:]
    inc = combine(torch, r, block, cm.DIFFERENCE, osz[:n], osz[n:], stride, base_b=n * stride)
    (inc_rows, inc_sizes), _ = inc
    held_and_inc = torch.cat([block[:n], inc_rows])
    uni = combine(torch, r, held_and_inc, cm.UNION, osz[:n], inc_sizes, stride, base_b=n * stride)
    return g, specs, m, H, W, inc, uni


# ---- 1. both ops on both pairs, against the model ------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", list(rc.GEOMETRIES))
def test_difference_and_union_equal_the_model(torch, name):
    for pair in PAIRS:
        g, specs, m, H, W, (_, inc), (_, uni) = difference_then_union(torch, name, pair)
        stride = (g.samples // 2 + g.samples // 8 + 5) | 1
        grew = 0
        for f, spec in enumerate(specs):
            tag = f"{name} {pair} frame {f} {spec}"
            if not rc.has_stream(spec):
                assert H[f] == W[f] == b"" and inc[f] == uni[f] == (OUT_OF_DATA, b"", 0, 0, 0), tag
                continue
            want = cm.combine(m, H[f], W[f], cm.DIFFERENCE, out_stride=stride)
            assert inc[f] == want, (tag, inc[f][0], inc[f][2:], want[0], want[2:], ebc.first_difference(inc[f][1], want[1]))
            want = cm.combine(m, H[f], inc[f][1], cm.UNION, out_stride=stride)
            assert uni[f] == want, (tag, uni[f][0], uni[f][2:], want[0], want[2:], ebc.first_difference(uni[f][1], want[1]))
            assert uni[f][0] == 0 and cm.units(m, uni[f][1]) == cm.units(m, H[f]) | cm.units(m, W[f]), tag
            grew += inc[f][2] > 0
            if pair == "nested":
                assert uni[f][1] == W[f] and inc[f][4] == len(W[f]) - len(H[f]), f"{tag}: the union is not the wanted cut"
            elif name == "G4" and f == 0:
                uh, uw = cm.units(m, H[f]), cm.units(m, W[f])
                assert (len(uh), len(uw), inc[f][2], len(uh - uw), uni[f][2], uni[f][3]) == (412, 409, 102, 105, 514, 412), tag
        if name in ("G1", "G3"):
            # the host convenience: bytes in, bytes out (G3: with the frame that has no stream)
            r = case(torch, name)[3]
            assert r.combine(H, W, cm.DIFFERENCE) == [x[:4] for x in inc], f"{name} {pair}: Recutter.combine, difference"
            assert r.combine(H, [x[1] for x in inc], cm.UNION) == [x[:4] for x in uni], f"{name} {pair}: Recutter.combine, union"
        # (one segment: every unit is foreground whatever the rectangle, so both viewports give one stream and nothing is missing)
        assert grew or (pair == "viewport" and g.segments == 1), f"{name} {pair}: no frame has an increment"
        assert not (grew and pair == "viewport" and g.segments == 1), f"{name}: one segment and the viewports differ"


# ---- 2. held cut + increment -> the decoder -------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", ["G2", "G3"])
def test_held_cut_and_increment_decode_as_the_union(torch, oracle, name):
    for pair in PAIRS:
        g, specs, m, H, W, ((inc_rows, inc_sizes), inc), ((uni_rows, uni_sizes), uni) = difference_then_union(torch, name, pair)
        _, _, _, _, blocks = case(torch, name)
        block, osz = blocks[pair]
        ok = [f for f, s in enumerate(specs) if rc.has_stream(s)]
        n = len(ok)
        # the increment behind the held cut, per frame, on the device
        parts, offsets, at = [], [], 0
        for f in ok:
            offsets.append(at)
            parts += [block[f, : len(H[f])], inc_rows[f, : inc[f][4]]]
            at += len(H[f]) + inc[f][4]
        appended = torch.cat(parts)
        lens = torch.tensor([len(H[f]) + inc[f][4] for f in ok], dtype=torch.int64, device="cuda")
        dec = decoder.Decoder(g.channels, g.stages, g.filt, g.segments, bits=g.bits)
        dt = torch.int16 if g.bits == 16 else torch.uint8
        images = []
        for data, kw in ((appended, dict(offsets=torch.tensor(offsets, dtype=torch.int64, device="cuda"))),
                         (uni_rows[ok].contiguous(), {})):
            planes = torch.full((n, g.channels, g.w * g.h), 0x5A, dtype=dt, device="cuda")
            rcs = torch.full((n,), 77, dtype=torch.int32, device="cuda")
            ws, hs = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda")
            dec.decode_torch(data, lens if kw else uni_sizes[ok].contiguous(), planes, rcs, ws, hs, **kw)
            torch.cuda.synchronize()
            assert rcs.cpu().tolist() == [0] * n and ws.cpu().tolist() == [g.w] * n and hs.cpu().tolist() == [g.h] * n, (name, pair)
            images.append(planes.cpu().numpy().view(np.uint16 if g.bits == 16 else np.uint8))
        dec.close()
        for k, f in enumerate(ok):
            tag = f"{name} {pair} frame {f} {specs[f]}"
            union = cm.combine(m, H[f], W[f], cm.UNION)[1]
            assert uni[f][1] == union, tag
            want = oracle_decode(oracle, union, g.channels, g.stages, g.filt, g.segments, g.w * g.h, g.bits)
            assert want[:3] == (0, g.w, g.h), tag
            assert all(np.array_equal(images[1][k, c], want[3][c]) for c in range(g.channels)), f"{tag}: the union's decode"
            # (where a chain of the union reads on into the bytes behind its packet, the order of the packets shows in the decode:
            # the documented exception of tests/reduced_model.py; the held cut with the increment behind it is then its own stream)
            if reads_on(oracle, g, union, 0):
                want = oracle_decode(oracle, H[f] + inc[f][1], g.channels, g.stages, g.filt, g.segments, g.w * g.h, g.bits)
            assert all(np.array_equal(images[0][k, c], want[3][c]) for c in range(g.channels)), f"{tag}: held cut + increment"


# ---- 3. lens written on the stream, two calls in flight --------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_lens_on_the_stream_and_two_calls_in_flight(torch):
    name = "G4"
    g, specs, m, r, blocks = case(torch, name)
    n = len(specs)
    alone = {}
    for pair in PAIRS:
        block, osz = blocks[pair]
        alone[pair] = [combine(torch, r, block, op, osz[:n], osz[n:], block.shape[1], base_b=n * block.shape[1])[1]
                       for op in (cm.DIFFERENCE, cm.UNION)]
    assert alone["viewport"][0][0][2] == 102
    before = len(r._combine_workspaces)
    runs = []
    for pair, st in zip(PAIRS, (torch.cuda.Stream(), torch.cuda.Stream())):
        block, osz = blocks[pair]
        stride = block.shape[1]
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            for op in (cm.DIFFERENCE, cm.UNION):
                out = torch.full((n + 1, stride), SENT, dtype=torch.uint8, device="cuda")
                sizes = torch.full((n + 1,), SENT_SIZE, dtype=torch.int64, device="cuda")
                rcs = torch.full((n + 1,), SENT_RC, dtype=torch.int32, device="cuda")
                counts = torch.full((2 * n + 2,), SENT_U32, dtype=torch.int32, device="cuda")
                torch.cuda._sleep(int(10e-3 * 2.1e9))
                lens = (osz * 3 + 7 - 7) // 3                  # (out of a torch kernel on this stream, just before the call)
                r.combine_torch(block, op, lens[:n], lens[n:], out[:n], sizes[:n], rcs[:n], counts[: 2 * n], base_b=n * stride)
                runs.append((pair, op, out, sizes, rcs, counts, lens))
    assert len(r._combine_workspaces) >= before + 2
    torch.cuda.synchronize()
    for pair, op, out, sizes, rcs, counts, _ in runs:
        assert read(out, sizes, rcs, counts, n) == alone[pair][op == cm.UNION], f"two streams: {pair} op {op}"


# ---- 4. refused calls, a row that is too small ------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_refused_calls_and_short_rows_write_nothing(torch):
    name = "G1"
    g, specs, m, r, blocks = case(torch, name)
    block, osz = blocks["nested"]
    n, stride = len(specs), block.shape[1]
    _, full = combine(torch, r, block, cm.UNION, osz[:n], osz[n:], stride, base_b=n * stride)
    assert all(x[0] == 0 and x[4] > 28 for x in full)
    # a row one byte short of the longest result: that frame gets the bytes it needs and an untouched row, the others their streams
    short = max(x[4] for x in full) - 1
    _, got = combine(torch, r, block, cm.UNION, osz[:n], osz[n:], short, base_b=n * stride)
    for f in range(n):
        assert got[f] == ((cm.TOO_SMALL, b"") + full[f][2:] if full[f][4] > short else full[f]), f
    assert sum(x[0] == cm.TOO_SMALL for x in got) >= 1 and sum(x[0] == 0 for x in got) >= 1
    # refused calls
    out = torch.full((n, stride), SENT, dtype=torch.uint8, device="cuda")
    sizes = torch.full((n,), SENT_SIZE, dtype=torch.int64, device="cuda")
    rcs = torch.full((n,), SENT_RC, dtype=torch.int32, device="cuda")
    counts = torch.full((2 * n,), SENT_U32, dtype=torch.int32, device="cuda")
    need = r.combine_workspace_bytes(n, block.numel())
    work = torch.full((need,), 0xCD, dtype=torch.uint8, device="cuda")
    la, lb = osz[:n].contiguous(), osz[n:].contiguous()
    st = torch.cuda.current_stream().cuda_stream

    def call(**kw):
        a = dict(n=n, op=cm.UNION, d_data=block.data_ptr(), data_bytes=block.numel(), d_offsets_a=None, base_a=0, d_lens_a=la.data_ptr(),
                 d_offsets_b=None, base_b=n * stride, d_lens_b=lb.data_ptr(), stream_stride=stride, d_out=out.data_ptr(), out_stride=stride,
                 d_sizes=sizes.data_ptr(), d_rcs=rcs.data_ptr(), d_counts=counts.data_ptr(), d_workspace=work.data_ptr(),
                 workspace_bytes=need, stream=st)
        a.update(kw)
        return r.combine_device_async_ptrs(**a)

    cases = {
        "op 2": dict(op=2), "op -1": dict(op=-1), "no frames": dict(n=0), "too many frames": dict(n=65536), "null data": dict(d_data=None),
        "null lens a": dict(d_lens_a=None), "null lens b": dict(d_lens_b=None), "null out": dict(d_out=None), "null sizes": dict(d_sizes=None),
        "null rcs": dict(d_rcs=None), "null counts": dict(d_counts=None), "null workspace": dict(d_workspace=None),
        "workspace one byte short": dict(workspace_bytes=need - 1),
    }
    for what, kw in cases.items():
        assert call(**kw) == INVALID_INPUT, what
    torch.cuda.synchronize()
    assert (out == SENT).all().item() and (sizes == SENT_SIZE).all().item() and (rcs == SENT_RC).all().item(), "a refused call wrote"
    assert (counts == SENT_U32).all().item() and (work == 0xCD).all().item(), "a refused call wrote"
    assert call() == 0
    torch.cuda.synchronize()
    assert sizes.cpu().tolist() == [x[4] for x in full] and rcs.cpu().tolist() == [0] * n
