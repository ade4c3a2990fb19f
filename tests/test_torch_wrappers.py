"""The six torch wrappers of icer_compression_amd/decoder.py -- Decoder.decode_torch / decode_display_torch and
Recutter.recut_torch / recut_cuts_torch / recut_roi_torch / combine_torch -- as wrappers: what they check before the library
is reached, what they hand to the library, how they keep their per-stream workspace and how they report a refused call.  What
the calls compute is covered by the tests of each call; here a valid call only has to equal the matching *_ptrs call made with
a workspace allocated by hand.  The argument checks run on the CPU against a mock build of decoder.hip (CPU tensors never reach
it); everything else needs an MI355X."""
import numpy as np
import pytest

from icer_compression_amd import api, decoder, synth
from tests.test_recut_mock import mock_lib                  # noqa: F401  (fixture)

W, H, STAGES, FILT, SEGMENTS = 64, 48, 2, 0, 2               # the gray 16-bit masters
CW, CH = 48, 32                                              # the three-channel frames of the display call
QUOTAS = [400, 900]
SENT = 0xA5
INVALID_INPUT = -11


class Call:
    """One wrapper: how to make its object, a valid set of arguments for n frames, the same call through *_ptrs."""
    method = c_name = cache = shape_message = ""
    named = ()                   # the tensors the wrapper checks by name, in its order
    outputs = ()                 # the tensors the call writes
    offset_names = ("offsets",)

    def make(self, lib=None):
        return decoder.Recutter(W, H, 1, STAGES, SEGMENTS, lib=lib, max_reduce=1)

    def run(self, obj, a):
        return getattr(obj, self.method)(**a)

    def rows(self, a):
        return len(a.get("quotas") or a.get("cuts")) * int(a["lens"].shape[0])


def _recut_outputs(torch, a, rows, stride, dev, extra=()):
    a["out"] = torch.full((rows, stride), SENT, dtype=torch.uint8, device=dev)
    a["sizes"] = torch.full((rows,), 77, dtype=torch.int64, device=dev)
    for name in ("rcs",) + tuple(extra):
        a[name] = torch.full((rows,), 77, dtype=torch.int32, device=dev)
    return a


class DecodeCall(Call):
    method, c_name, cache = "decode_torch", "icerx_decode_device_async", "_workspaces"
    named, outputs = ("data", "lens", "rcs", "ws", "hs", "out"), ("out", "rcs", "ws", "hs")
    shape_message = "out must hold n * channels * frame_stride samples"
    channels, w, h, masters = 1, W, H, "gray"

    def make(self, lib=None):
        return decoder.Decoder(self.channels, STAGES, FILT, SEGMENTS, lib=lib)

    def out(self, torch, n, dev):
        return torch.full((n, self.channels, self.w * self.h), 0x5A5A, dtype=torch.int16, device=dev)

    def args(self, torch, e, n):
        data, sizes = e[self.masters]
        dev = data.device
        return dict(data=data[:n], lens=sizes[:n].clone(), out=self.out(torch, n, dev),
                    rcs=torch.full((n,), 77, dtype=torch.int32, device=dev),
                    ws=torch.zeros(n, dtype=torch.int64, device=dev), hs=torch.zeros(n, dtype=torch.int64, device=dev))

    def bad_shape(self, torch, a):
        a["out"] = torch.zeros(a["out"].numel() + 1, dtype=a["out"].dtype, device=a["out"].device)

    def refuse(self, obj, a):
        obj.close()                                              # a null decoder: ICER_INVALID_INPUT before anything is enqueued

    def need(self, obj, a):
        n = int(a["lens"].shape[0])
        return obj.workspace_bytes(n, a["data"].numel(), a["out"].numel() // (n * self.channels))

    def ptrs(self, obj, a, work, st):
        n, off = int(a["lens"].shape[0]), a.get("offsets")
        return obj.decode_device_async_ptrs(n, a["data"].data_ptr(), a["data"].numel(), off.data_ptr() if off is not None else None,
                                            0 if off is not None else a["data"].stride(0), a["lens"].data_ptr(), a["out"].data_ptr(),
                                            a["out"].numel() // (n * self.channels), a["rcs"].data_ptr(), a["ws"].data_ptr(),
                                            a["hs"].data_ptr(), work.data_ptr(), work.numel(), st)


class DisplayCall(DecodeCall):
    method, c_name, cache = "decode_display_torch", "icerx_decode_device_display_async", "_display_workspaces"
    shape_message = "out must hold n * frame_stride * channels bytes"
    channels, w, h, masters = 3, CW, CH, "color"

    def out(self, torch, n, dev):
        return torch.full((n, self.h, self.w, 3), SENT, dtype=torch.uint8, device=dev)

    def need(self, obj, a):
        n = int(a["lens"].shape[0])
        return obj.display_workspace_bytes(n, a["data"].numel(), a["out"].numel() // (n * self.channels))

    def ptrs(self, obj, a, work, st):
        n, off = int(a["lens"].shape[0]), a.get("offsets")
        return obj.decode_display_async_ptrs(n, a["data"].data_ptr(), a["data"].numel(), off.data_ptr() if off is not None else None,
                                             0 if off is not None else a["data"].stride(0), a["lens"].data_ptr(), a["out"].data_ptr(),
                                             a["out"].numel() // (n * self.channels), a["rcs"].data_ptr(), a["ws"].data_ptr(),
                                             a["hs"].data_ptr(), work.data_ptr(), work.numel(), st)


class RecutCall(Call):
    method, c_name, cache = "recut_torch", "icerx_recut_device_async", "_workspaces"
    named, outputs = ("data", "lens", "out", "sizes", "rcs"), ("out", "sizes", "rcs")
    shape_message = "out must be (Q * n, out_stride), sizes and rcs Q * n entries"

    def args(self, torch, e, n):
        data, sizes = e["gray"]
        a = dict(data=data[:n], lens=sizes[:n].clone(), quotas=list(QUOTAS))
        return _recut_outputs(torch, a, len(QUOTAS) * n, max(QUOTAS) + 1, data.device)

    def bad_shape(self, torch, a):
        a["sizes"] = torch.zeros(a["sizes"].numel() + 1, dtype=torch.int64, device=a["sizes"].device)

    def refuse(self, obj, a):
        import torch
        a["quotas"] = [60] * (decoder.MAX_LADDER + 1)            # 17 quotas, one above MAX_LADDER
        _recut_outputs(torch, a, self.rows(a), 61, a["data"].device)

    def need(self, obj, a):
        return obj.workspace_bytes(int(a["lens"].shape[0]), a["data"].numel(), len(a["quotas"]))

    def ptrs(self, obj, a, work, st):
        n, off = int(a["lens"].shape[0]), a.get("offsets")
        return obj.recut_device_async_ptrs(n, a["data"].data_ptr(), a["data"].numel(), off.data_ptr() if off is not None else None,
                                           0 if off is not None else a["data"].stride(0), a["lens"].data_ptr(), a["quotas"],
                                           a["out"].data_ptr(), a["out"].shape[-1], a["sizes"].data_ptr(), a["rcs"].data_ptr(),
                                           work.data_ptr(), work.numel(), st)


class CutsCall(RecutCall):
    method, c_name, cache = "recut_cuts_torch", "icerx_recut_device_cuts_async", "_cuts_workspaces"
    CUTS = [(0, 400), (1, 300)]

    def args(self, torch, e, n):
        data, sizes = e["gray"]
        a = dict(data=data[:n], lens=sizes[:n].clone(), cuts=list(self.CUTS))
        return _recut_outputs(torch, a, len(self.CUTS) * n, 401, data.device)

    def refuse(self, obj, a):
        import torch
        a["cuts"] = [(0, 60)] * (decoder.MAX_LADDER + 1)
        _recut_outputs(torch, a, self.rows(a), 61, a["data"].device)

    def need(self, obj, a):
        return obj.cuts_workspace_bytes(int(a["lens"].shape[0]), a["data"].numel(), len(a["cuts"]))

    def ptrs(self, obj, a, work, st):
        n, off = int(a["lens"].shape[0]), a.get("offsets")
        return obj.recut_cuts_device_async_ptrs(n, a["data"].data_ptr(), a["data"].numel(), off.data_ptr() if off is not None else None,
                                                0 if off is not None else a["data"].stride(0), a["lens"].data_ptr(),
                                                [c[0] for c in a["cuts"]], [c[1] for c in a["cuts"]], a["out"].data_ptr(),
                                                a["out"].shape[-1], a["sizes"].data_ptr(), a["rcs"].data_ptr(), work.data_ptr(),
                                                work.numel(), st)


class RoiCall(RecutCall):
    method, c_name, cache = "recut_roi_torch", "icerx_recut_device_roi_async", "_roi_workspaces"
    named, outputs = ("data", "lens", "out", "sizes", "rcs", "kept", "foreground", "rois"), ("out", "sizes", "rcs", "kept", "foreground")
    shape_message = "out must be (Q * n, out_stride), sizes, rcs, kept and foreground Q * n entries"
    CUTS = [(0, 400, 0), (1, 300, 3)]

    def args(self, torch, e, n):
        data, sizes = e["gray"]
        a = dict(data=data[:n], lens=sizes[:n].clone(), cuts=list(self.CUTS),
                 rois=torch.tensor([[8, 8, 24, 16]] * n, dtype=torch.int32, device=data.device))
        return _recut_outputs(torch, a, len(self.CUTS) * n, 401, data.device, ("kept", "foreground"))

    def refuse(self, obj, a):
        a["cuts"] = [(0, 400, 17), (1, 300, 3)]                  # a shift above ICERX_MAX_ROI_SHIFT

    def need(self, obj, a):
        return obj.roi_workspace_bytes(int(a["lens"].shape[0]), a["data"].numel(), len(a["cuts"]))

    def ptrs(self, obj, a, work, st):
        n, off = int(a["lens"].shape[0]), a.get("offsets")
        return obj.recut_roi_device_async_ptrs(n, a["data"].data_ptr(), a["data"].numel(), off.data_ptr() if off is not None else None,
                                               0 if off is not None else a["data"].stride(0), a["lens"].data_ptr(), a["rois"].data_ptr(),
                                               [c[0] for c in a["cuts"]], [c[2] for c in a["cuts"]], [c[1] for c in a["cuts"]],
                                               a["out"].data_ptr(), a["out"].shape[-1], a["sizes"].data_ptr(), a["rcs"].data_ptr(),
                                               a["kept"].data_ptr(), a["foreground"].data_ptr(), work.data_ptr(), work.numel(), st)


class CombineCall(Call):
    method, c_name, cache = "combine_torch", "icerx_combine_device_async", "_combine_workspaces"
    named, outputs = ("data", "lens_a", "lens_b", "out", "sizes", "rcs", "counts"), ("out", "sizes", "rcs", "counts")
    offset_names = ("offsets_a", "offsets_b")
    shape_message = "out must be (n, out_stride), lens, offsets, sizes and rcs n entries, counts 2 n"

    def args(self, torch, e, n):
        block, osz = e["cuts"][n]                                # (2 n, stride): the held cuts, then the wanted cuts
        dev, stride = block.device, block.shape[1]
        return dict(data=block, op=decoder.COMBINE_DIFFERENCE, lens_a=osz[:n].clone(), lens_b=osz[n:].clone(), base_b=n * stride,
                    out=torch.full((n, stride), SENT, dtype=torch.uint8, device=dev),
                    sizes=torch.full((n,), 77, dtype=torch.int64, device=dev), rcs=torch.full((n,), 77, dtype=torch.int32, device=dev),
                    counts=torch.full((n, 2), 77, dtype=torch.int32, device=dev))

    def bad_shape(self, torch, a):
        a["counts"] = torch.zeros(a["counts"].numel() + 1, dtype=torch.int32, device=a["counts"].device)

    def refuse(self, obj, a):
        a["op"] = 2

    def need(self, obj, a):
        return obj.combine_workspace_bytes(int(a["lens_a"].shape[0]), a["data"].numel())

    def ptrs(self, obj, a, work, st):
        n, oa, ob = int(a["lens_a"].shape[0]), a.get("offsets_a"), a.get("offsets_b")
        return obj.combine_device_async_ptrs(n, a["op"], a["data"].data_ptr(), a["data"].numel(), oa.data_ptr() if oa is not None else None,
                                             a.get("base_a", 0), a["lens_a"].data_ptr(), ob.data_ptr() if ob is not None else None,
                                             a.get("base_b", 0), a["lens_b"].data_ptr(),
                                             0 if oa is not None and ob is not None else a["data"].stride(-2), a["out"].data_ptr(),
                                             a["out"].shape[-1], a["sizes"].data_ptr(), a["rcs"].data_ptr(), a["counts"].data_ptr(),
                                             work.data_ptr(), work.numel(), st)


CALLS = [DecodeCall(), DisplayCall(), RecutCall(), CutsCall(), RoiCall(), CombineCall()]
IDS = [c.method for c in CALLS]


def with_offsets(torch, call, a):
    """the same call with its streams named by offsets instead of a stride"""
    n, dev = a["out"].shape[0] if call.method == "combine_torch" else int(a["lens"].shape[0]), a["data"].device
    rows = torch.arange(2 * n, dtype=torch.int64, device=dev) * a["data"].stride(-2)
    if call.method == "combine_torch":
        a.update(offsets_a=rows[:n].contiguous(), offsets_b=rows[n:].contiguous())
        a.pop("base_b")
    else:
        a["offsets"] = rows[:n].contiguous()
    return a


# ---------------------------------------------------------------------------------------------------- the CPU half
class _NoLibrary:
    """stands in for the library: any use of it fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f"the library was reached ({name})")


def _host_env(torch):
    blob = torch.zeros((4, 2048), dtype=torch.uint8)
    sizes = torch.full((4,), 100, dtype=torch.int64)
    return {"gray": (blob, sizes), "color": (blob, sizes), "cuts": {n: (blob[: 2 * n], sizes[: 2 * n]) for n in (1, 2)}}


@pytest.mark.parametrize("call", CALLS, ids=IDS)
def test_host_tensors_and_flat_blobs_never_reach_the_library(mock_lib, call):             # noqa: F811
    import torch
    obj = call.make(lib=mock_lib)
    lib, obj.lib = obj.lib, _NoLibrary()
    try:
        a = call.args(torch, _host_env(torch), 2)
        with pytest.raises(ValueError) as err:
            call.run(obj, a)
        assert str(err.value).startswith("data: a contiguous cuda"), str(err.value)
        a["data"] = a["data"].reshape(-1)
        with pytest.raises(ValueError) as err:
            call.run(obj, a)
        assert str(err.value) == "a 1-D blob needs offsets or stream_stride"
        assert not getattr(obj, call.cache)
    finally:
        obj.lib = lib
        obj.close()


# ---------------------------------------------------------------------------------------------------- the GPU half
@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    assert torch.cuda.is_available()
    decoder.load_library()
    return torch


def _encode(torch, frames, w, h, channels):
    n, quota = frames.shape[0], 2 * w * h * channels + 16384          # (room for the 28-byte headers of every packet as well)
    enc = api.Encoder(w, h, channels, STAGES, FILT, SEGMENTS, max_frames=n)
    out = torch.zeros((n, quota), dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(n, dtype=torch.int64, device="cuda")
    rcs = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    enc.encode_torch(torch.from_numpy(frames.view(np.int16)).cuda(), quota, out, sizes, rcs)
    torch.cuda.synchronize()
    enc.close()
    assert rcs.cpu().tolist() == [0] * n                      # lossless masters
    return out, sizes


@pytest.fixture(scope="module")
def env(torch_gpu):
    """the masters, encoded once: two gray 64 x 48 frames, two three-channel 48 x 32 frames, and for n = 1, 2 the output block of
    one recut_torch call at two quotas (the operands of the combine call)"""
    torch = torch_gpu
    e = {"gray": _encode(torch, np.stack([synth.gray_frame(W, H, 12345 + k) for k in range(2)]), W, H, 1),
         "color": _encode(torch, np.stack([np.stack(synth.color_frame_yuv(CW, CH, 777 + k)) for k in range(2)]), CW, CH, 3), "cuts": {}}
    r, call = RecutCall().make(), RecutCall()
    for n in (1, 2):
        a = call.args(torch, e, n)
        call.run(r, a)
        torch.cuda.synchronize()
        assert set(a["rcs"].cpu().tolist()) <= {0, -5}
        e["cuts"][n] = (a["out"], a["sizes"])
    r.close()
    return e


@pytest.mark.gpu
@pytest.mark.parametrize("call", CALLS, ids=IDS)
def test_argument_checks(torch_gpu, env, call):
    torch = torch_gpu
    obj = call.make()
    names = call.named + call.offset_names
    for name in names:                                        # a wrong dtype, each named tensor in turn
        a = with_offsets(torch, call, call.args(torch, env, 2))
        a[name] = a[name].to(torch.float32)
        with pytest.raises(ValueError) as err:
            call.run(obj, a)
        assert str(err.value).startswith(name + ": "), (name, str(err.value))
    a = call.args(torch, env, 2)                              # a non-contiguous out
    wide = torch.zeros(tuple(a["out"].shape[:-1]) + (2 * a["out"].shape[-1],), dtype=a["out"].dtype, device="cuda")
    a["out"] = wide[..., ::2]
    assert a["out"].shape == wide[..., : wide.shape[-1] // 2].shape and not a["out"].is_contiguous()
    with pytest.raises(ValueError) as err:
        call.run(obj, a)
    assert str(err.value).startswith("out: "), str(err.value)
    a = call.args(torch, env, 2)                              # a wrong shape: the method's own message
    call.bad_shape(torch, a)
    with pytest.raises(ValueError) as err:
        call.run(obj, a)
    assert str(err.value) == call.shape_message
    assert not getattr(obj, call.cache)                       # none of these calls came as far as the workspace
    obj.close()


@pytest.mark.gpu
@pytest.mark.parametrize("offsets", [False, True], ids=["stride", "offsets"])
@pytest.mark.parametrize("call", CALLS, ids=IDS)
def test_valid_call_equals_the_ptrs_call(torch_gpu, env, call, offsets):
    torch = torch_gpu
    obj = call.make()
    a, b = call.args(torch, env, 2), call.args(torch, env, 2)
    if offsets:
        a, b = with_offsets(torch, call, a), with_offsets(torch, call, b)
    call.run(obj, a)
    work = torch.empty(max(call.need(obj, b), 1), dtype=torch.uint8, device="cuda")
    assert call.ptrs(obj, b, work, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert set(a["rcs"].cpu().tolist()) <= {0, -5} and 77 not in a["rcs"].cpu().tolist()
    for name in call.outputs:
        assert torch.equal(a[name], b[name]), name
    assert not torch.equal(a["out"], call.args(torch, env, 2)["out"]), "nothing was written"
    obj.close()


@pytest.mark.gpu
@pytest.mark.parametrize("call", CALLS, ids=IDS)
def test_workspace_cache(torch_gpu, env, call):
    torch = torch_gpu
    obj = call.make()
    cache = getattr(obj, call.cache)
    key = torch.cuda.current_stream().cuda_stream
    call.run(obj, call.args(torch, env, 1))
    first = cache[key]
    call.run(obj, call.args(torch, env, 1))                   # again on the same stream: the same entry
    assert len(cache) == 1 and cache[key].data_ptr() == first.data_ptr() and cache[key] is first
    small = first.numel()
    assert small >= call.need(obj, call.args(torch, env, 1))
    torch.cuda.synchronize()
    big = call.args(torch, env, 2)                            # a larger call: a larger tensor in the entry's place
    assert call.need(obj, big) > small
    call.run(obj, big)
    assert len(cache) == 1 and cache[key].numel() == call.need(obj, big) > small
    side = torch.cuda.Stream()                                # a second stream: an entry of its own
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call.run(obj, call.args(torch, env, 1))
    assert len(cache) == 2 and set(cache) == {key, side.cuda_stream} and cache[side.cuda_stream].numel() >= small
    torch.cuda.synchronize()
    others = [c.cache for c in CALLS if c.cache != call.cache and hasattr(obj, c.cache)]
    assert others and not any(getattr(obj, c) for c in others)      # each call keeps a cache of its own
    obj.close()


@pytest.mark.gpu
@pytest.mark.parametrize("call", CALLS, ids=IDS)
def test_refused_call_raises_with_the_c_name_and_rc(torch_gpu, env, call):
    torch = torch_gpu
    obj = call.make()
    a = call.args(torch, env, 2)
    call.refuse(obj, a)
    with pytest.raises(RuntimeError) as err:
        call.run(obj, a)
    assert str(err.value).startswith(f"{call.c_name}: {INVALID_INPUT}"), str(err.value)
    torch.cuda.synchronize()
    obj.close()
