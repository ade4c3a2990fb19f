"""Host-side mirror of the reference's DECODING interface over the C ABI of libicer_hip_dec.so
(include/icer_hip_dec.h).

STATUS: the device code behind it is checked against the decoder oracle in its CPU builds (tests/test_emu_decoder.py) and,
on an MI355X, by tests/test_gpu_decoder.py (gray / YUV, 16 / 8 bit, damaged streams, golden digests, the batch object;
all in the default `pytest -m gpu` run, HISTORY.md 6b (summary: DESIGN.md 8)).

The reference's callers do (example/src/example_decode.c, example/src/icer_util.c `decompress`)
    icer_get_image_dimensions(stream, len, &w, &h);  buf = malloc(w * h * 2);
    rc = icer_decompress_image_uint16(buf, &w, &h, w * h, stream, len, stages, filt, segments);
The functions below keep those names, argument order and return codes, numpy arrays standing in for the pointers.
There is no CPU fallback: every decompress call needs libicer_hip_dec.so and a HIP device and fails loudly otherwise.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from ._abi import DECODER, c_array, declare

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG, "libicer_hip_dec.so")
ICER_DECODER_OUT_OF_DATA = -7
ICER_DECODED_INVALID_DATA = -8
WINDOW_INFO = 6                  # uint32 per frame of a window decode: x0, y0, ww, wh, chains run, chains of the plain call

_lib = None
_sz = C.c_size_t


def bind(path: str) -> C.CDLL:
    """dlopen a build of the decoder library (RTLD_LOCAL: it exports the same icer_* names as the reference) and declare
    its entry points.  (tests/test_emu_decoder.py binds a CPU mock build of decoder.hip's host pipeline this way; a build
    without some of the entry points still serves the others.)"""
    return declare(C.CDLL(path, mode=os.RTLD_LOCAL), DECODER)


def _need(lib, name):
    if not hasattr(lib, name):
        raise RuntimeError(f"this build of the decoder library has no {name}")
    return getattr(lib, name)


def _check(lib, name, rc):
    if rc != 0:
        raise RuntimeError(f"{name}: {rc} {lib.icerx_decoder_last_error().decode()}")


# ---- the one path behind the *_torch methods --------------------------------------------------------------------------
def _stream_stride(data, stream_stride, offsets, any_rows=False) -> int:
    """stream_stride as given; else 0 when every operand has offsets; else the row stride of a blob with rows (a 2-D blob;
    any_rows: a blob of two or more dimensions, its stride(-2))"""
    if stream_stride is not None:
        return int(stream_stride)
    for o in offsets:
        if o is None:
            if data.dim() < 2 or (data.dim() != 2 and not any_rows):
                raise ValueError("a 1-D blob needs offsets or stream_stride")
            return data.stride(-2)
    return 0


def _need_tensors(*named):
    """(name, tensor, dtype or dtypes) in turn: a contiguous cuda tensor of one of the dtypes; None (offsets not given) passes"""
    for name, t, dts in named:
        dts = dts if isinstance(dts, tuple) else (dts,)
        if t is not None and (not t.is_cuda or not t.is_contiguous() or t.dtype not in dts):
            raise ValueError(f"{name}: a contiguous cuda {dts[0]} tensor is needed")


def _enqueue(lib, name, cache, need, device, ptrs_call, *args):
    """ptrs_call(*args, workspace, its bytes, stream) on torch's current stream, tensors among args as their data_ptr(): the
    stream's workspace comes out of `cache`, grown to max(need, 1) bytes here, on the host; a refused call raises"""
    import torch
    st = torch.cuda.current_stream(device)
    work = cache.get(st.cuda_stream)
    if work is None or work.numel() < max(need, 1):
        work = cache[st.cuda_stream] = torch.empty(max(need, 1), dtype=torch.uint8, device=device)
    work.record_stream(st)
    args = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
    _check(lib, name, ptrs_call(*args, work.data_ptr(), work.numel(), st.cuda_stream))


def _bytes_through(streams, rows, stride, call):
    """bytes in, bytes out: the streams in one blob on the current device, zeroed outputs of `rows` rows of `stride` bytes,
    call(blob, lens, offsets, out, sizes, rcs), a wait, and -> [(rc, stream)] per row"""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    lens = [len(s) for s in streams]
    blob = np.frombuffer(b"".join(streams), dtype=np.uint8).copy() if sum(lens) else np.zeros(1, np.uint8)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    out = torch.zeros((rows, stride), dtype=torch.uint8, device=dev)
    sizes = torch.zeros(rows, dtype=torch.int64, device=dev)
    rcs = torch.zeros(rows, dtype=torch.int32, device=dev)
    call(torch.from_numpy(blob).to(dev), torch.tensor(lens, dtype=torch.int64, device=dev), torch.from_numpy(offs).to(dev), out, sizes, rcs)
    torch.cuda.current_stream(dev).synchronize()
    out, sizes, rcs = out.cpu().numpy(), sizes.cpu().numpy(), rcs.cpu().numpy()
    return [(int(rcs[k]), out[k, : int(sizes[k])].tobytes()) for k in range(rows)]


def _pack(streams):
    """byte strings -> (blob, offsets, lens): the streams back to back in one host array, and where each lies, as size_t arrays"""
    lens = [len(s) for s in streams]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64) if streams else np.zeros(0, np.uint64)
    blob = np.frombuffer(b"".join(streams), dtype=np.uint8).copy() if sum(lens) else np.zeros(1, np.uint8)
    n = len(streams)
    return blob, (_sz * n)(*[int(o) for o in offs]), (_sz * n)(*lens)


def _per_frame(n: int, offsets, lens, call, sizes=None):
    """the per-frame host arrays of a synchronous call, at least one entry each, packed once for every driver: call(offsets, lens,
    rcs, ws, hs) -> (its rc, rcs, ws, hs as lists of n); sizes: (w, h) per frame, what ws / hs hold going in (default 0)"""
    m = max(n, 1)
    offs, ln = (_sz * m)(*[int(o) for o in offsets]), (_sz * m)(*[int(x) for x in lens])
    sizes = sizes or [(0, 0)] * n
    rcs, ws, hs = (C.c_int * m)(), (_sz * m)(*[int(s[0]) for s in sizes]), (_sz * m)(*[int(s[1]) for s in sizes])
    rc = call(offs, ln, rcs, ws, hs)
    return rc, list(rcs)[:n], list(ws)[:n], list(hs)[:n]


def load_library() -> C.CDLL:
    """libicer_hip_dec.so of this package"""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(f"{LIB_PATH} is missing: run `python -m icer_compression_amd.build` (there is no CPU fallback)")
        _lib = bind(LIB_PATH)
    return _lib


def icer_get_image_dimensions(stream: bytes, lib=None):
    """-> (rc, w, h)"""
    lib = lib or load_library()
    buf = np.frombuffer(stream, dtype=np.uint8).copy() if len(stream) else np.zeros(1, np.uint8)
    w, h = _sz(0), _sz(0)
    rc = lib.icer_get_image_dimensions(buf, len(stream), C.byref(w), C.byref(h))
    return rc, w.value, h.value


def reduced_size(w: int, h: int, r: int):
    """the size of a w x h image decoded at 1/2^r resolution: (ceil(w / 2^r), ceil(h / 2^r)) (icerx_reduced_size)"""
    return (w + (1 << r) - 1) >> r, (h + (1 << r) - 1) >> r


def decompress(stream: bytes, channels: int, stages: int, filt: int, segments: int, bufsize: int | None = None, bits: int = 16,
               lib=None, reduce: int = 0, reconstruct: int = 0, window=None):
    """icer_decompress_image_[yuv_]uint16 / _uint8 on a host stream -> (rc, w, h, [flat planes of bufsize samples]).
    window = (x, y, w, h) in pixels of the delivered image: icerx_decompress_window, only that rectangle, stored compactly, and
    only the chains it depends on -> (rc, w, h, [flat planes], info) with info = [x0, y0, ww, wh, chains run, chains of the
    plain call]; bufsize then counts samples of the window (default: the window clipped to the image the stream announces).
    reduce = r > 0: icerx_decompress_reduced, the image at 1/2^r size; bufsize then counts samples of the reduced image.
    reconstruct = k in 1..4: icerx_decompress_reconstructed, truncated non-zero coefficients rebuilt k eighths of the way into
    their interval (3 is the recommended value; 0 is the reference's decode)."""
    lib = lib or load_library()
    if channels not in (1, 3):
        raise ValueError("channels must be 1 or 3")
    if bufsize is None:                                      # (the image the stream announces, or the window clipped to it)
        rc0, w0, h0 = icer_get_image_dimensions(stream, lib)
        w0, h0 = (reduced_size(w0, h0, reduce) if reduce > 0 else (w0, h0)) if rc0 == 0 else (0, 0)
        bufsize = w0 * h0
        if window is not None:
            x0, y0 = min(int(window[0]), w0), min(int(window[1]), h0)
            bufsize = min(int(window[2]), w0 - x0) * min(int(window[3]), h0 - y0)
    buf = np.frombuffer(stream, dtype=np.uint8).copy() if len(stream) else np.zeros(1, np.uint8)
    planes = [np.zeros(max(bufsize, 1), np.uint16 if bits == 16 else np.uint8) for _ in range(channels)]
    ptrs = (C.c_void_p * channels)(*[p.ctypes.data for p in planes])
    w, h = _sz(0), _sz(0)
    image = (C.byref(w), C.byref(h), bufsize, buf, len(stream), stages, filt, segments)
    if window is not None:
        win, info = np.asarray(window, np.uint32).copy(), np.zeros(WINDOW_INFO, np.uint32)
        rc = _need(lib, "icerx_decompress_window")(ptrs, channels, *image, bits, reduce, reconstruct, win.ctypes.data, info.ctypes.data)
        return rc, w.value, h.value, planes, [int(x) for x in info]
    if reconstruct != 0:
        rc = _need(lib, "icerx_decompress_reconstructed")(ptrs, channels, *image, bits, reduce, reconstruct)
    elif reduce != 0:
        rc = _need(lib, "icerx_decompress_reduced")(ptrs, channels, *image, bits, reduce)
    else:
        fn = getattr(lib, "icer_decompress_image_" + ("yuv_" if channels == 3 else "") + ("uint16" if bits == 16 else "uint8"))
        rc = fn(*[p.ctypes.data for p in planes], *image)
    return rc, w.value, h.value, planes


def decompress_display(stream: bytes, channels: int, stages: int, filt: int, segments: int, lib=None, reconstruct: int = 0):
    """icerx_decompress_display on a host 16-bit stream -> (rc, image): uint8 (h, w) for channels 1 (gray8), (h, w, 3) for
    channels 3 (RGB888), the image the reference's `icer_util decompress` writes; an empty array when nothing was decoded.
    reconstruct = k in 1..4: through a Decoder with that setting (icerx_decode_host_display)."""
    lib = lib or load_library()
    fn = _need(lib, "icerx_decompress_display")
    rc0, w0, h0 = icer_get_image_dimensions(stream, lib)
    bufsize = w0 * h0 if rc0 == 0 else 0
    if reconstruct != 0:
        if channels not in (1, 3):
            return -11, np.zeros((0, 0), np.uint8)
        dec = Decoder(channels, stages, filt, segments, lib=lib, reconstruct=reconstruct)
        try:
            rc, res = dec.decode_display_host([stream], bufsize)
        finally:
            dec.close()
        rc_k, w_k, h_k, row = res[0]
        rc = rc if rc != 0 else rc_k
        if w_k * h_k == 0 or w_k * h_k > bufsize:
            return rc, np.zeros((0, 0) if channels != 3 else (0, 0, 3), np.uint8)
        row = row[: channels * w_k * h_k]
        return rc, row.reshape((h_k, w_k) if channels == 1 else (h_k, w_k, 3))
    buf = np.frombuffer(stream, dtype=np.uint8).copy() if len(stream) else np.zeros(1, np.uint8)
    image = np.zeros(max(bufsize * max(channels, 1), 1), np.uint8)
    w, h = _sz(0), _sz(0)
    rc = fn(image.ctypes.data, C.byref(w), C.byref(h), bufsize, buf, len(stream), stages, filt, segments, channels)
    if channels not in (1, 3) or w.value * h.value == 0 or w.value * h.value > bufsize:
        return rc, np.zeros((0, 0) if channels != 3 else (0, 0, 3), np.uint8)
    image = image[: channels * w.value * h.value]
    return rc, image.reshape((h.value, w.value) if channels == 1 else (h.value, w.value, 3))


def planes_to_display_torch(planes):
    """icerx_planes_to_display_device on torch's current stream, without waiting: planes = a contiguous cuda tensor
    (..., channels, h, w) with channels 1 or 3, or (h, w) gray, of int16 / uint16 or uint8 samples taken as unsigned and as
    they are -> a cuda uint8 tensor (..., h, w) gray8 or (..., h, w, 3) RGB888."""
    import torch
    fn = _need(load_library(), "icerx_planes_to_display_device")
    if planes.dim() == 2:
        planes = planes[None]
    want = (torch.int16, getattr(torch, "uint16", torch.int16), torch.uint8)
    if not planes.is_cuda or not planes.is_contiguous() or planes.dtype not in want or planes.dim() < 3 or planes.shape[-3] not in (1, 3):
        raise ValueError("planes: a contiguous cuda int16 / uint16 / uint8 tensor (..., 1 or 3, h, w) is needed")
    ch, h, w = (int(x) for x in planes.shape[-3:])
    n = planes.numel() // max(ch * h * w, 1) if h * w else 0
    lead = tuple(planes.shape[:-3])
    out = torch.empty(lead + ((h, w) if ch == 1 else (h, w, 3)), dtype=torch.uint8, device=planes.device)
    if n:
        st = torch.cuda.current_stream(planes.device)
        rc = fn(planes.data_ptr(), n, ch, w, h, h * w, 8 if planes.dtype == torch.uint8 else 16, out.data_ptr(), h * w, st.cuda_stream)
        _check(load_library(), "icerx_planes_to_display_device", rc)
    return out


class Decoder:
    """Batch / device-resident extension (icerx_decoder_*, include/icer_hip_dec.h Part 2)."""

    def __init__(self, channels: int, stages: int, filt: int, segments: int, bits: int = 16, device: int = -1, lib=None,
                 reduce: int = 0, reconstruct: int = 0):
        """reduce = r > 0: a decoder for streams made with `stages` that delivers every image at 1/2^r size
        (icerx_decoder_create_reduced): strides and buffer sizes count samples of the reduced image, ws / hs report its size.
        reconstruct = k in 1..4: truncated non-zero coefficients are rebuilt k eighths of the way into their interval in every
        call of this decoder (icerx_decoder_set_reconstruction; 3 is the recommended value, 0 the reference's decode)"""
        self.lib = lib or load_library()
        self.channels, self.bits, self.reduce = channels, bits, 0
        self._workspaces = {}                # decode_torch: one cached workspace per torch stream
        self._display_workspaces = {}        # decode_display_torch: the same, sized for the display call
        self._window_workspaces = {}         # decode_window_torch: the same, sized for the window calls
        self.handle = C.c_void_p()
        if reduce != 0:
            fn = _need(self.lib, "icerx_decoder_create_reduced")
            _check(self.lib, "icerx_decoder_create_reduced", fn(C.byref(self.handle), device, channels, stages, filt, segments, bits, reduce))
            self.reduce = int(self.lib.icerx_decoder_reduce(self.handle))
        else:
            rc = self.lib.icerx_decoder_create(C.byref(self.handle), device, channels, stages, filt, segments, bits)
            _check(self.lib, "icerx_decoder_create", rc)
        if reconstruct != 0:
            self.set_reconstruction(reconstruct)

    @property
    def reconstruct(self) -> int:
        """the decoder's reconstruction point in eighths (icerx_decoder_reconstruction; 0 on a build without it)"""
        if not hasattr(self.lib, "icerx_decoder_reconstruction"):
            return 0
        return int(self.lib.icerx_decoder_reconstruction(self.handle))

    def set_reconstruction(self, eighths: int) -> None:
        """icerx_decoder_set_reconstruction: 0..4, for every call enqueued from now on"""
        rc = _need(self.lib, "icerx_decoder_set_reconstruction")(self.handle, eighths)
        if rc != 0:
            raise ValueError(f"icerx_decoder_set_reconstruction({eighths}): {rc}")

    def close(self):
        if self.handle:
            self.lib.icerx_decoder_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    _pack = staticmethod(_pack)

    def _sync(self, fn, n: int, data: int, offsets, lens, out, frame_stride: int):
        """one of the four synchronous calls -> (rc, rcs, ws, hs)"""
        return _per_frame(n, offsets, lens, lambda offs, ln, rcs, ws, hs: fn(self.handle, n, data, offs, ln, out, frame_stride, rcs, ws, hs))

    def _sync_host(self, fn, streams, frame_stride: int, arrays):
        """the same for streams in host memory, written to the host arrays `arrays` (in frame order)"""
        blob, offs, lens = self._pack(streams)
        ptrs = (C.c_void_p * max(len(arrays), 1))(*[a.ctypes.data for a in arrays])
        return self._sync(fn, len(streams), blob.ctypes.data, offs, lens, ptrs, frame_stride)

    def decode_host(self, streams, frame_stride: int):
        """-> (rc, [(rc_k, w_k, h_k, [flat planes])]) for a list of streams in host memory"""
        n, ch = len(streams), self.channels
        planes = [np.zeros(max(frame_stride, 1), np.uint16 if self.bits == 16 else np.uint8) for _ in range(n * ch)]
        rc, rcs, ws, hs = self._sync_host(self.lib.icerx_decode_host, streams, frame_stride, planes)
        return rc, [(rcs[k], ws[k], hs[k], planes[k * ch: (k + 1) * ch]) for k in range(n)]

    def decode_device(self, n: int, d_data: int, offsets, lens, d_out: int, frame_stride: int):
        """raw device pointers (e.g. torch tensors' data_ptr()); -> (rc, rcs, ws, hs)"""
        return self._sync(self.lib.icerx_decode_device, n, d_data, offsets, lens, d_out, frame_stride)

    def workspace_bytes(self, n: int, data_bytes: int, frame_stride: int) -> int:
        """icerx_decode_workspace_bytes: the device workspace one decode_device_async_ptrs call needs"""
        return int(self.lib.icerx_decode_workspace_bytes(self.handle, n, data_bytes, frame_stride))

    def decode_device_async_ptrs(self, n: int, d_data: int, data_bytes: int, d_offsets, stream_stride: int, d_lens: int, d_out: int,
                                 frame_stride: int, d_rcs: int, d_ws: int, d_hs: int, d_workspace: int, workspace_bytes: int,
                                 stream: int = 0) -> int:
        """icerx_decode_device_async on raw device pointers (d_offsets None: stream k starts at k * stream_stride; offsets,
        lens, ws, hs: uint64 / int64; rcs: int32).  Enqueues on `stream` and returns the call's rc without waiting."""
        return self.lib.icerx_decode_device_async(self.handle, n, d_data, data_bytes, d_offsets, stream_stride, d_lens, d_out,
                                                  frame_stride, d_rcs, d_ws, d_hs, d_workspace, workspace_bytes, stream)

    # ---- straight to 8-bit display images: gray8 / packed RGB888 (include/icer_hip_dec.h) ----
    def decode_display_host(self, streams, frame_stride: int):
        """icerx_decode_host_display -> (rc, [(rc_k, w_k, h_k, image)]): image = flat uint8 of channels * frame_stride bytes,
        its first channels * w_k * h_k bytes the gray8 / RGB888 image of frame k"""
        fn = _need(self.lib, "icerx_decode_host_display")
        images = [np.zeros(max(self.channels * frame_stride, 1), np.uint8) for _ in streams]
        rc, rcs, ws, hs = self._sync_host(fn, streams, frame_stride, images)
        return rc, list(zip(rcs, ws, hs, images))

    def decode_display_device(self, n: int, d_data: int, offsets, lens, d_out: int, frame_stride: int):
        """icerx_decode_device_display on raw device pointers; frame k's image at d_out + k * channels * frame_stride bytes
        -> (rc, rcs, ws, hs)"""
        return self._sync(_need(self.lib, "icerx_decode_device_display"), n, d_data, offsets, lens, d_out, frame_stride)

    def display_workspace_bytes(self, n: int, data_bytes: int, frame_stride: int) -> int:
        """icerx_decode_display_workspace_bytes: the device workspace one decode_display_async_ptrs call needs"""
        return int(_need(self.lib, "icerx_decode_display_workspace_bytes")(self.handle, n, data_bytes, frame_stride))

    def decode_display_async_ptrs(self, n: int, d_data: int, data_bytes: int, d_offsets, stream_stride: int, d_lens: int, d_out: int,
                                  frame_stride: int, d_rcs: int, d_ws: int, d_hs: int, d_workspace: int, workspace_bytes: int,
                                  stream: int = 0) -> int:
        """icerx_decode_device_display_async on raw device pointers (arguments as decode_device_async_ptrs; d_out: uint8 images)"""
        return _need(self.lib, "icerx_decode_device_display_async")(self.handle, n, d_data, data_bytes, d_offsets, stream_stride, d_lens,
                                                                    d_out, frame_stride, d_rcs, d_ws, d_hs, d_workspace, workspace_bytes,
                                                                    stream)

    def decode_display_torch(self, data, lens, out, rcs, ws, hs, offsets=None, stream_stride=None) -> None:
        """decode_torch with 8-bit images for output (icerx_decode_device_display_async), on torch's current stream, without
        waiting.  out: a contiguous cuda uint8 tensor of n * frame_stride * channels bytes, e.g. (n, h, w, 3) or (n, h, w);
        frame k's image is its first channels * ws[k] * hs[k] bytes of row k.  Everything else as decode_torch; the workspace
        (which holds the working planes) is cached per stream, apart from decode_torch's."""
        import torch
        n = int(lens.shape[0])
        stream_stride = _stream_stride(data, stream_stride, (offsets,))
        _need_tensors(("data", data, torch.uint8), ("lens", lens, torch.int64), ("rcs", rcs, torch.int32), ("ws", ws, torch.int64),
                      ("hs", hs, torch.int64), ("out", out, torch.uint8), ("offsets", offsets, torch.int64))
        if n and out.numel() % (n * self.channels):
            raise ValueError("out must hold n * frame_stride * channels bytes")
        frame_stride = out.numel() // (n * self.channels) if n else 0
        need = self.display_workspace_bytes(n, data.numel(), frame_stride) if n else 0
        _enqueue(self.lib, "icerx_decode_device_display_async", self._display_workspaces, need, data.device, self.decode_display_async_ptrs,
                 n, data, data.numel(), offsets, stream_stride, lens, out, frame_stride, rcs, ws, hs)

    # ---- window decode: a rectangle of each image, without the chains it does not depend on (include/icer_hip_dec_window.h) ----
    def _sync_window(self, fn, n: int, data: int, offsets, lens, windows, out, frame_stride: int, full_stride: int):
        """one of the three synchronous window calls; windows: n x 4 (x, y, w, h) -> (rc, rcs, ws, hs, info as n lists of 6)"""
        win = np.zeros((max(n, 1), 4), np.uint32)
        win[:n] = np.asarray(windows, np.uint32).reshape(n, 4)
        info = np.zeros((max(n, 1), WINDOW_INFO), np.uint32)
        res = _per_frame(n, offsets, lens, lambda offs, ln, rcs, ws, hs: fn(self.handle, n, data, offs, ln, win.ctypes.data, out, frame_stride,
                                                                           full_stride, rcs, ws, hs, info.ctypes.data))
        return (*res, [[int(x) for x in row] for row in info[:n]])

    def decode_window_host(self, streams, windows, frame_stride: int, full_stride: int):
        """icerx_decode_host_window -> (rc, [(rc_k, w_k, h_k, [flat planes of frame_stride samples], info_k)]): the first
        ww * wh samples of each plane are the window, row by row"""
        fn = _need(self.lib, "icerx_decode_host_window")
        n, ch = len(streams), self.channels
        planes = [np.zeros(max(frame_stride, 1), np.uint16 if self.bits == 16 else np.uint8) for _ in range(n * ch)]
        blob, offs, lens = self._pack(streams)
        ptrs = (C.c_void_p * max(n * ch, 1))(*[a.ctypes.data for a in planes])
        rc, rcs, ws, hs, info = self._sync_window(fn, n, blob.ctypes.data, offs, lens, windows, ptrs, frame_stride, full_stride)
        return rc, [(rcs[k], ws[k], hs[k], planes[k * ch: (k + 1) * ch], info[k]) for k in range(n)]

    def decode_window_device(self, n: int, d_data: int, offsets, lens, windows, d_out: int, frame_stride: int, full_stride: int,
                             display: bool = False):
        """icerx_decode_device_window / _display on raw device pointers (windows: a host sequence) -> (rc, rcs, ws, hs, info)"""
        fn = _need(self.lib, "icerx_decode_device_window_display" if display else "icerx_decode_device_window")
        return self._sync_window(fn, n, d_data, offsets, lens, windows, d_out, frame_stride, full_stride)

    def window_workspace_bytes(self, n: int, data_bytes: int, full_stride: int, display: bool = False) -> int:
        """icerx_decode_window_workspace_bytes / _display_workspace_bytes: what one decode_window_async_ptrs call needs"""
        name = "icerx_decode_window_display_workspace_bytes" if display else "icerx_decode_window_workspace_bytes"
        return int(_need(self.lib, name)(self.handle, n, data_bytes, full_stride))

    def decode_window_async_ptrs(self, n: int, d_data: int, data_bytes: int, d_offsets, stream_stride: int, d_lens: int, d_windows: int,
                                 d_out: int, frame_stride: int, full_stride: int, d_rcs: int, d_ws: int, d_hs: int, d_info: int,
                                 d_workspace: int, workspace_bytes: int, stream: int = 0, display: bool = False) -> int:
        """icerx_decode_device_window_async / _display_async on raw device pointers (as decode_device_async_ptrs; d_windows:
        n x 4 uint32 and d_info: n x 6 uint32 in device memory)"""
        fn = _need(self.lib, "icerx_decode_device_window_display_async" if display else "icerx_decode_device_window_async")
        return fn(self.handle, n, d_data, data_bytes, d_offsets, stream_stride, d_lens, d_windows, d_out, frame_stride, full_stride, d_rcs,
                  d_ws, d_hs, d_info, d_workspace, workspace_bytes, stream)

    def decode_window_torch(self, data, lens, out, rcs, ws, hs, windows, info, full_stride: int, offsets=None, stream_stride=None,
                            display: bool = False) -> None:
        """decode_torch (display=True: decode_display_torch) for a rectangle per frame, on torch's current stream, without waiting.

        windows: a cuda int32 / uint32 tensor (n, 4) of x, y, w, h in pixels of the delivered image, read on the stream (write
        it there with any torch op just before; nothing waits); info: cuda int32 (n, 6), written with x0, y0, ww, wh of the
        clipped window, the chains run and the chains the plain call runs.  out holds n * channels * frame_stride samples (bytes
        for display): the window of frame k, ww * wh samples row by row, at the start of each of its planes (of its row).
        full_stride: samples of a full-size working plane (in the workspace), at least the largest image.  Only the chains a
        window depends on are run."""
        import torch
        n = int(lens.shape[0])
        stream_stride = _stream_stride(data, stream_stride, (offsets,))
        want = (torch.uint8,) if display or self.bits == 8 else (torch.int16, getattr(torch, "uint16", torch.int16))
        i32 = (torch.int32, getattr(torch, "uint32", torch.int32))
        _need_tensors(("data", data, torch.uint8), ("lens", lens, torch.int64), ("rcs", rcs, torch.int32), ("ws", ws, torch.int64),
                      ("hs", hs, torch.int64), ("out", out, want), ("offsets", offsets, torch.int64), ("windows", windows, i32),
                      ("info", info, i32))
        if tuple(windows.shape) != (n, 4) or info.numel() != n * WINDOW_INFO:
            raise ValueError("windows must be (n, 4) and info n * 6 entries")
        if n and out.numel() % (n * self.channels):
            raise ValueError("out must hold n * channels * frame_stride samples")
        frame_stride = out.numel() // (n * self.channels) if n else 0
        need = self.window_workspace_bytes(n, data.numel(), full_stride, display) if n else 0
        name = "icerx_decode_device_window_display_async" if display else "icerx_decode_device_window_async"

        def call(n_, data_, bytes_, offs_, sstride_, lens_, win_, out_, fs_, full_, rcs_, ws_, hs_, info_, work_, work_bytes_, stream_):
            return self.decode_window_async_ptrs(n_, data_, bytes_, offs_, sstride_, lens_, win_, out_, fs_, full_, rcs_, ws_, hs_, info_,
                                                 work_, work_bytes_, stream_, display)
        _enqueue(self.lib, name, self._window_workspaces, need, data.device, call, n, data, data.numel(), offsets, stream_stride, lens,
                 windows, out, frame_stride, int(full_stride), rcs, ws, hs, info)

    def decode_torch(self, data, lens, out, rcs, ws, hs, offsets=None, stream_stride=None) -> None:
        """Decode n streams of a cuda uint8 tensor on torch's current stream, without waiting (icerx_decode_device_async).

        data: the blob, 1-D, or 2-D (n, stride) with stream k in row k; lens / offsets: cuda int64 (n,), offsets None: stream
        k starts at k * stream_stride (default: data.stride(0) of a 2-D blob); out: cuda int16 / uint16 (uint8 for an 8-bit decoder),
        n * channels * frame_stride samples, e.g. (n, channels, frame_stride); rcs: cuda int32 (n,); ws / hs: cuda int64 (n,),
        read as the sizes kept by a stream without a valid packet and written with each frame's size.  The workspace is
        cached per stream and grown here, on the host, before the call is enqueued.

        The encoder's output goes in as it is, with nothing copied to the host:
            enc.encode_torch(frames, quota, out=streams, sizes=sizes, rcs=enc_rcs)          # streams: (n, out_stride) uint8
            dec.decode_torch(streams, sizes, planes, rcs, ws, hs)                            # offsets = k * out_stride
            torch.cuda.current_stream().synchronize()
        """
        import torch
        n = int(lens.shape[0])
        stream_stride = _stream_stride(data, stream_stride, (offsets,))
        want = (torch.int16, getattr(torch, "uint16", torch.int16)) if self.bits == 16 else (torch.uint8,)
        _need_tensors(("data", data, torch.uint8), ("lens", lens, torch.int64), ("rcs", rcs, torch.int32), ("ws", ws, torch.int64),
                      ("hs", hs, torch.int64), ("out", out, want), ("offsets", offsets, torch.int64))
        if n and out.numel() % (n * self.channels):
            raise ValueError("out must hold n * channels * frame_stride samples")
        frame_stride = out.numel() // (n * self.channels) if n else 0
        need = self.workspace_bytes(n, data.numel(), frame_stride) if n else 0
        _enqueue(self.lib, "icerx_decode_device_async", self._workspaces, need, data.device, self.decode_device_async_ptrs,
                 n, data, data.numel(), offsets, stream_stride, lens, out, frame_stride, rcs, ws, hs)


class Session:
    """A progressive decode session of a Decoder (icerx_session_*, include/icer_hip_dec_session.h): n_slots held frames of
    frame_stride samples per channel whose coefficient state stays on the device; a feed decodes only the bit planes its
    packets add and delivers the whole refined image of every fed slot.  The calls are synchronous; the decoder must outlive
    the session.

        ses = Session(dec, n_slots, frame_stride)
        ses.feed_torch(cut_a, lens_a, out)                 # the held cut
        rec.combine_torch(blob, COMBINE_DIFFERENCE, lens_a, lens_b, inc, sizes, rcs, counts)
        ses.feed_torch(inc, sizes.cpu(), out)              # only the planes cut B adds are decoded
    """

    def __init__(self, dec: "Decoder", n_slots: int, frame_stride: int):
        self.dec, self.lib, self.n_slots, self.frame_stride = dec, dec.lib, n_slots, frame_stride
        self.channels, self.bits = dec.channels, dec.bits
        self.handle = C.c_void_p()
        fn = _need(self.lib, "icerx_session_create")
        _check(self.lib, "icerx_session_create", fn(C.byref(self.handle), dec.handle, n_slots, frame_stride))

    def close(self):
        if self.handle:
            self.lib.icerx_session_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, slot: int = -1) -> None:
        """forget what `slot` holds (-1: every slot)"""
        rc = self.lib.icerx_session_reset(self.handle, slot)
        if rc != 0:
            raise ValueError(f"icerx_session_reset({slot}): {rc}")

    def planes_held(self, slot: int, chan: int, level: int, subband: int, segment: int) -> int:
        """bit planes the chain holds, from the top; -1: stopped for good; -2: no such slot or chain"""
        return int(self.lib.icerx_session_planes_held(self.handle, slot, chan, level, subband, segment))

    def stats(self):
        """[chains resumed in the wave-per-plane kernel, chains run in the thread-per-chain kernel, planes decoded, packets
        dropped] since creation"""
        out = (C.c_uint64 * 4)()
        _check(self.lib, "icerx_session_stats", self.lib.icerx_session_stats(self.handle, out))
        return [int(x) for x in out]

    def _feed(self, fn, n: int, slots, data: int, offsets, lens, out, sizes=None):
        """one of the three feed calls -> (rc, rcs, ws, hs)"""
        slots = c_array(C.c_int, slots)
        return _per_frame(n, offsets, lens, lambda offs, ln, rcs, ws, hs: fn(self.handle, n, slots, data, offs, ln, out, rcs, ws, hs), sizes)

    def feed_host(self, feeds, slots=None, sizes=None):
        """feeds: a list of byte strings in host memory, feed k for slot slots[k] (None: 0 .. n - 1); sizes: (w, h) per feed,
        used while the slot has seen no valid packet -> (rc, [(rc_k, w_k, h_k, [flat planes of frame_stride samples])])"""
        n, ch = len(feeds), self.channels
        blob, offs, lens = _pack(feeds)
        planes = [np.zeros(max(self.frame_stride, 1), np.uint16 if self.bits == 16 else np.uint8) for _ in range(n * ch)]
        ptrs = (C.c_void_p * max(n * ch, 1))(*[a.ctypes.data for a in planes])
        rc, rcs, ws, hs = self._feed(self.lib.icerx_session_feed_host, n, slots, blob.ctypes.data, offs, lens, ptrs, sizes)
        return rc, [(rcs[k], ws[k], hs[k], planes[k * ch: (k + 1) * ch]) for k in range(n)]

    def feed_device(self, n: int, d_data: int, offsets, lens, d_out: int, slots=None, sizes=None, display: bool = False):
        """raw device pointers; d_out as icerx_decode_device (display: as icerx_decode_device_display) for n frames of
        frame_stride -> (rc, rcs, ws, hs)"""
        fn = self.lib.icerx_session_feed_device_display if display else self.lib.icerx_session_feed_device
        return self._feed(fn, n, slots, d_data, offsets, lens, d_out, sizes)

    def feed_torch(self, data, lens, out, offsets=None, stream_stride=None, slots=None, sizes=None, display: bool = False):
        """Feed n increments of a cuda uint8 tensor and wait.  data: the blob, 1-D, or 2-D (n, stride) with feed k in row k;
        lens / offsets: host sequences (offsets None: feed k starts at k * stream_stride, default data.stride(0)); out: a
        contiguous cuda tensor of n * channels * frame_stride samples -- int16 / uint16 (uint8 for an 8-bit decoder), or, with
        display, uint8 gray8 / RGB888 rows -> (rcs, ws, hs).  A refused call raises."""
        import torch
        n = len(lens)
        want = (torch.uint8,) if display or self.bits == 8 else (torch.int16, getattr(torch, "uint16", torch.int16))
        _need_tensors(("data", data, torch.uint8), ("out", out, want))
        if out.numel() != n * self.channels * self.frame_stride:
            raise ValueError("out must hold n * channels * frame_stride samples")
        stream_stride = _stream_stride(data, stream_stride, (offsets,))
        if offsets is None:
            offsets = [k * stream_stride for k in range(n)]
        if any(int(o) + int(x) > data.numel() for o, x in zip(offsets, lens)):
            raise ValueError("a feed leaves the blob")
        with torch.cuda.device(data.device):
            torch.cuda.current_stream().synchronize()        # (the call runs on the null stream: what made `data` is complete)
            rc, rcs, ws, hs = self.feed_device(n, data.data_ptr(), offsets, lens, out.data_ptr(), slots, sizes, display)
        _check(self.lib, "icerx_session_feed_device", rc)
        return rcs, ws, hs


MAX_LADDER = 16                  # ICERX_MAX_LADDER
COMBINE_UNION, COMBINE_DIFFERENCE = 0, 1         # ICERX_COMBINE_UNION / ICERX_COMBINE_DIFFERENCE


class Recutter:
    """Stored streams re-cut to smaller byte quotas on the device, without the pixels and without re-coding
    (icerx_recutter_* / icerx_recut_device_async, include/icer_hip_dec.h): from a master of a frame made at quota Qm, the
    stream the encoder makes at any quota Q <= Qm (any Q for a complete master), byte for byte.  One recutter per geometry
    the masters were made with.

    max_reduce = R > 0 (icerx_recutter_create_reduced): the recutter also cuts by resolution -- recut_cuts_torch / recut_cuts
    take cuts (reduce r, quota) with r in 0 .. R and give, from the same masters, streams of the image at 1/2^r size that
    any decoder made for stages - r decodes (the re-cut of the master's derived stream, include/icer_hip_dec.h)."""

    def __init__(self, w: int, h: int, channels: int, stages: int, segments: int, bits: int = 16, device: int = -1, lib=None,
                 max_reduce: int = 0, filt=None):
        self.lib = lib or load_library()
        _need(self.lib, "icerx_recut_device_async")
        self.w, self.h, self.channels, self.bits = w, h, channels, bits
        L = self.lib
        self._target_workspaces, self._budget_workspaces = {}, {}        # recut_target_torch / recut_budget_torch: a cache each, as below
        self._workspaces = {}                # recut_torch: one cached workspace per torch stream
        self._cuts_workspaces = {}           # recut_cuts_torch: the same, sized for the cuts call
        self._roi_workspaces = {}            # recut_roi_torch: the same, sized for the ROI call
        self._combine_workspaces = {}        # combine_torch: the same, sized for the combine call
        self.handle = C.c_void_p()
        self.max_reduce = 0
        self.filt = filt
        if filt is not None:                 # a quality recutter: it knows the filter, and cuts by distortion sidecars as well
            fn = _need(L, "icerx_recutter_create_quality")
            _check(L, "icerx_recutter_create_quality", fn(C.byref(self.handle), device, w, h, channels, stages, filt, segments, bits, max_reduce))
            self.max_reduce = int(L.icerx_recutter_max_reduce(self.handle))
            return
        if max_reduce != 0:
            fn = _need(L, "icerx_recutter_create_reduced")
            _check(L, "icerx_recutter_create_reduced", fn(C.byref(self.handle), device, w, h, channels, stages, segments, bits, max_reduce))
            self.max_reduce = int(L.icerx_recutter_max_reduce(self.handle))
            return
        _check(L, "icerx_recutter_create", L.icerx_recutter_create(C.byref(self.handle), device, w, h, channels, stages, segments, bits))

    def close(self):
        if self.handle:
            self.lib.icerx_recutter_destroy(self.handle)
            self.handle = C.c_void_p()
        self._workspaces.clear()
        self._cuts_workspaces.clear()
        self._roi_workspaces.clear()
        self._combine_workspaces.clear()
        self._target_workspaces.clear()
        self._budget_workspaces.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def workspace_bytes(self, n: int, data_bytes: int, n_quotas: int) -> int:
        """icerx_recut_workspace_bytes: the device workspace one recut_device_async_ptrs call needs"""
        return int(self.lib.icerx_recut_workspace_bytes(self.handle, n, data_bytes, n_quotas))

    def recut_device_async_ptrs(self, n: int, d_data: int, data_bytes: int, d_offsets, stream_stride: int, d_lens: int, quotas,
                                d_out: int, out_stride: int, d_sizes: int, d_rcs: int, d_workspace: int, workspace_bytes: int,
                                stream: int = 0, n_quotas=None) -> int:
        """icerx_recut_device_async on raw device pointers (d_offsets None: master k starts at k * stream_stride; offsets, lens,
        sizes: uint64 / int64; rcs: int32; quotas: a host sequence, None for a null pointer).  Frame f at quota q is row
        q * n + f of d_out and entry q * n + f of d_sizes / d_rcs.  Enqueues on `stream` and returns the call's rc without
        waiting."""
        nq = n_quotas if n_quotas is not None else (len(quotas) if quotas is not None else 0)
        return self.lib.icerx_recut_device_async(self.handle, n, d_data, data_bytes, d_offsets, stream_stride, d_lens, c_array(_sz, quotas),
                                                 nq, d_out, out_stride, d_sizes, d_rcs, d_workspace, workspace_bytes, stream)

    def recut_torch(self, data, lens, quotas, out, sizes, rcs, offsets=None, stream_stride=None) -> None:
        """Re-cut n masters of a cuda uint8 tensor to every quota of `quotas` on torch's current stream, without waiting.

        data: the blob, 1-D, or 2-D (n, stride) with master k in row k; lens / offsets: cuda int64 (n,), offsets None: master
        k starts at k * stream_stride (default: data.stride(0) of a 2-D blob); out: cuda uint8 (Q, n, out_stride) or
        (Q * n, out_stride), out_stride at least the largest quota; sizes: cuda int64 and rcs: cuda int32 of Q * n entries.
        Row and entry q * n + f hold frame f at quotas[q], as encode_ladder leaves them, so out[q] / sizes[q] go into
        Decoder.decode_torch as they are.  The workspace is cached per stream and grown here, on the host, before the call
        is enqueued."""
        import torch
        n, Q = int(lens.shape[0]), len(quotas)
        stream_stride = _stream_stride(data, stream_stride, (offsets,))
        _need_tensors(("data", data, torch.uint8), ("lens", lens, torch.int64), ("out", out, torch.uint8), ("sizes", sizes, torch.int64),
                      ("rcs", rcs, torch.int32), ("offsets", offsets, torch.int64))
        if out.dim() < 2 or out.numel() != Q * n * out.shape[-1] or sizes.numel() != Q * n or rcs.numel() != Q * n:
            raise ValueError("out must be (Q * n, out_stride), sizes and rcs Q * n entries")
        _enqueue(self.lib, "icerx_recut_device_async", self._workspaces, self.workspace_bytes(n, data.numel(), Q), data.device,
                 self.recut_device_async_ptrs, n, data, data.numel(), offsets, stream_stride, lens, list(quotas), out, out.shape[-1], sizes, rcs)

    def recut(self, streams, quotas):
        """bytes in, bytes out: res[q][f] = (rc, stream) of master streams[f] re-cut to quotas[q] (copies to the device and back,
        and waits: a convenience, not the fast path)"""
        n, Q = len(streams), len(quotas)
        rows = _bytes_through(streams, Q * n, max(max(int(q) for q in quotas), 1), lambda blob, lens, offs, out, sizes, rcs:
                              self.recut_torch(blob, lens, quotas, out, sizes, rcs, offsets=offs))
        return [rows[q * n: (q + 1) * n] for q in range(Q)]

    # ---- cuts by resolution as well as by byte quota (icerx_recut_device_cuts_async) ----
    def cuts_workspace_bytes(self, n: int, data_bytes: int, n_cuts: int) -> int:
        """icerx_recut_cuts_workspace_bytes: the device workspace one recut_cuts_device_async_ptrs call needs"""
        return int(_need(self.lib, "icerx_recut_cuts_workspace_bytes")(self.handle, n, data_bytes, n_cuts))

    def recut_cuts_device_async_ptrs(self, n: int, d_data: int, data_bytes: int, d_offsets, stream_stride: int, d_lens: int, reduces,
                                     quotas, d_out: int, out_stride: int, d_sizes: int, d_rcs: int, d_workspace: int,
                                     workspace_bytes: int, stream: int = 0, n_cuts=None) -> int:
        """icerx_recut_device_cuts_async on raw device pointers (arguments as recut_device_async_ptrs; reduces and quotas: host
        sequences of one length, None for a null pointer).  Frame f at cut c is row c * n + f of d_out and entry c * n + f of
        d_sizes / d_rcs.  Enqueues on `stream` and returns the call's rc without waiting."""
        fn = _need(self.lib, "icerx_recut_device_cuts_async")
        nc = n_cuts if n_cuts is not None else (len(quotas) if quotas is not None else 0)
        return fn(self.handle, n, d_data, data_bytes, d_offsets, stream_stride, d_lens, c_array(C.c_int, reduces), c_array(_sz, quotas), nc,
                  d_out, out_stride, d_sizes, d_rcs, d_workspace, workspace_bytes, stream)

    def recut_cuts_torch(self, data, lens, cuts, out, sizes, rcs, offsets=None, stream_stride=None) -> None:
        """recut_torch with cuts = [(reduce, quota), ...] in place of the quotas: row and entry c * n + f hold frame f at cuts[c],
        a stream of the image at 1/2^reduce size, so out[c] / sizes[c] go into decode_torch of a Decoder made for
        stages - reduce as they are.  Everything else as recut_torch; the workspace is cached per stream, apart from
        recut_torch's."""
        import torch
        n, Q = int(lens.shape[0]), len(cuts)
        stream_stride = _stream_stride(data, stream_stride, (offsets,))
        _need_tensors(("data", data, torch.uint8), ("lens", lens, torch.int64), ("out", out, torch.uint8), ("sizes", sizes, torch.int64),
                      ("rcs", rcs, torch.int32), ("offsets", offsets, torch.int64))
        if out.dim() < 2 or out.numel() != Q * n * out.shape[-1] or sizes.numel() != Q * n or rcs.numel() != Q * n:
            raise ValueError("out must be (Q * n, out_stride), sizes and rcs Q * n entries")
        _enqueue(self.lib, "icerx_recut_device_cuts_async", self._cuts_workspaces, self.cuts_workspace_bytes(n, data.numel(), Q), data.device,
                 self.recut_cuts_device_async_ptrs, n, data, data.numel(), offsets, stream_stride, lens, [c[0] for c in cuts],
                 [c[1] for c in cuts], out, out.shape[-1], sizes, rcs)

    def recut_cuts(self, streams, cuts):
        """bytes in, bytes out: res[c][f] = (rc, stream) of master streams[f] at cuts[c] = (reduce, quota) (copies to the device
        and back, and waits: a convenience, not the fast path)"""
        n, Q = len(streams), len(cuts)
        rows = _bytes_through(streams, Q * n, max(max(int(q) for _, q in cuts), 1), lambda blob, lens, offs, out, sizes, rcs:
                              self.recut_cuts_torch(blob, lens, cuts, out, sizes, rcs, offsets=offs))
        return [rows[c * n: (c + 1) * n] for c in range(Q)]

    # ---- cuts by region of interest, at any resolution (icerx_recut_device_roi_async) ----
    def roi_workspace_bytes(self, n: int, data_bytes: int, n_cuts: int) -> int:
        """icerx_recut_roi_workspace_bytes: the device workspace one recut_roi_device_async_ptrs call needs"""
        return int(_need(self.lib, "icerx_recut_roi_workspace_bytes")(self.handle, n, data_bytes, n_cuts))

    def recut_roi_device_async_ptrs(self, n: int, d_data: int, data_bytes: int, d_offsets, stream_stride: int, d_lens: int, d_rois: int,
                                    reduces, shifts, quotas, d_out: int, out_stride: int, d_sizes: int, d_rcs: int, d_kept: int,
                                    d_foreground: int, d_workspace: int, workspace_bytes: int, stream: int = 0, n_cuts=None) -> int:
        """icerx_recut_device_roi_async on raw device pointers (arguments as recut_cuts_device_async_ptrs; d_rois: n x 4 uint32
        x, y, w, h in device memory; reduces, shifts and quotas: host sequences of one length, None for a null pointer --
        reduces None: every reduce 0; d_kept / d_foreground: uint32, entry c * n + f as d_sizes).  Enqueues on `stream` and
        returns the call's rc without waiting."""
        fn = _need(self.lib, "icerx_recut_device_roi_async")
        nc = n_cuts if n_cuts is not None else (len(quotas) if quotas is not None else 0)
        return fn(self.handle, n, d_data, data_bytes, d_offsets, stream_stride, d_lens, d_rois, c_array(C.c_int, reduces),
                  c_array(C.c_int, shifts), c_array(_sz, quotas), nc, d_out, out_stride, d_sizes, d_rcs, d_kept, d_foreground, d_workspace,
                  workspace_bytes, stream)

    def recut_roi_torch(self, data, lens, rois, cuts, out, sizes, rcs, kept, foreground, offsets=None, stream_stride=None) -> None:
        """recut_cuts_torch with cuts = [(reduce, quota, shift), ...] and a rectangle per frame: rois, a cuda int32 / uint32 tensor
        (n, 4) of x, y, w, h in pixels of the full frame, read on torch's current stream (write it there with any torch op
        just before; nothing waits).  Row and entry c * n + f hold frame f at cuts[c]: the stream of the image at 1/2^reduce
        size whose byte quota is spent inside the rectangle first; kept / foreground: cuda int32 of Q * n entries (the uint32
        K and foreground units).  out[c] / sizes[c] go into decode_torch of a Decoder made for stages - reduce as they are.
        Everything else as recut_cuts_torch; the workspace is cached per stream, apart from the other calls'."""
        import torch
        n, Q = int(lens.shape[0]), len(cuts)
        stream_stride = _stream_stride(data, stream_stride, (offsets,))
        _need_tensors(("data", data, torch.uint8), ("lens", lens, torch.int64), ("out", out, torch.uint8), ("sizes", sizes, torch.int64),
                      ("rcs", rcs, torch.int32), ("kept", kept, torch.int32), ("foreground", foreground, torch.int32),
                      ("offsets", offsets, torch.int64))
        if not rois.is_cuda or not rois.is_contiguous() or rois.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or \
                tuple(rois.shape) != (n, 4):
            raise ValueError("rois: a contiguous cuda int32 / uint32 tensor (n, 4) is needed")
        if out.dim() < 2 or out.numel() != Q * n * out.shape[-1] or any(t.numel() != Q * n for t in (sizes, rcs, kept, foreground)):
            raise ValueError("out must be (Q * n, out_stride), sizes, rcs, kept and foreground Q * n entries")
        _enqueue(self.lib, "icerx_recut_device_roi_async", self._roi_workspaces, self.roi_workspace_bytes(n, data.numel(), Q), data.device,
                 self.recut_roi_device_async_ptrs, n, data, data.numel(), offsets, stream_stride, lens, rois, [c[0] for c in cuts],
                 [c[2] for c in cuts], [c[1] for c in cuts], out, out.shape[-1], sizes, rcs, kept, foreground)

    # ---- cuts by distortion target or shared byte budget, from masters and their distortion sidecars (include/icer_hip_dec_quality.h) ----
    @property
    def sidecar_entries(self) -> int:
        """icerx_recut_sidecar_entries: the uint64 words of a sidecar row (Encoder.sidecar_entries of the geometry); 0 for a plain recutter"""
        return int(_need(self.lib, "icerx_recut_sidecar_entries")(self.handle))

    def target_threshold(self, mse: float, reduce: int = 0) -> int:
        """icerx_recut_target_threshold: floor(mse * samples at 1/2^reduce size * 16), saturated; at reduce 0 Encoder.target_threshold"""
        return int(_need(self.lib, "icerx_recut_target_threshold")(self.handle, float(mse), int(reduce)))

    def target_workspace_bytes(self, n: int, data_bytes: int, n_cuts: int) -> int:
        """icerx_recut_target_workspace_bytes: the device workspace one recut_target_device_async_ptrs call needs"""
        return int(_need(self.lib, "icerx_recut_target_workspace_bytes")(self.handle, n, data_bytes, n_cuts))

    def recut_target_device_async_ptrs(self, n: int, d_data: int, data_bytes: int, d_offsets, stream_stride: int, d_lens: int, d_sidecar: int,
                                       sidecar_stride: int, reduces, targets_mse, byte_cap: int, d_out: int, out_stride: int, d_sizes: int,
                                       d_rcs: int, d_reached: int, d_dist: int, d_equiv_quota: int, d_workspace: int, workspace_bytes: int,
                                       stream: int = 0, n_cuts=None) -> int:
        """icerx_recut_device_target_async on raw device pointers (masters and outputs as recut_cuts_device_async_ptrs; d_sidecar:
        uint64 rows sidecar_stride words apart; reduces: a host sequence or None for every reduce 0; targets_mse: a host
        sequence, None for a null pointer; d_reached: int32, d_dist / d_equiv_quota: uint64, entry c * n + f as d_sizes).
        Enqueues on `stream` and returns the call's rc without waiting."""
        fn = _need(self.lib, "icerx_recut_device_target_async")
        nc = n_cuts if n_cuts is not None else (len(targets_mse) if targets_mse is not None else 0)
        return fn(self.handle, n, d_data, data_bytes, d_offsets, stream_stride, d_lens, d_sidecar, sidecar_stride, c_array(C.c_int, reduces),
                  c_array(C.c_double, targets_mse), nc, byte_cap, d_out, out_stride, d_sizes, d_rcs, d_reached, d_dist, d_equiv_quota,
                  d_workspace, workspace_bytes, stream)

    def _quality_tensors(self, n, Q, data, lens, sidecar, out, offsets, int64s, int32s):
        import torch
        _need_tensors(("data", data, torch.uint8), ("lens", lens, torch.int64), ("sidecar", sidecar, torch.int64), ("out", out, torch.uint8),
                      ("offsets", offsets, torch.int64), *[(k, t, torch.int64) for k, t in int64s.items()],
                      *[(k, t, torch.int32) for k, t in int32s.items()])
        if sidecar.dim() != 2 or sidecar.shape[0] < n:
            raise ValueError("sidecar must be (n, stride) int64 words")
        if out.dim() < 2 or out.numel() != Q * n * out.shape[-1] or any(t.numel() != Q * n for t in (*int64s.values(), *int32s.values())):
            raise ValueError("out must be (Q * n, out_stride), " + ", ".join((*int64s, *int32s)) + " Q * n entries")

    def recut_target_torch(self, data, lens, sidecar, cuts, byte_cap: int, out, sizes, rcs, reached, dist, equiv, offsets=None,
                           stream_stride=None) -> None:
        """recut_cuts_torch with cuts = [(reduce, mse), ...] and the masters' distortion sidecars: row and entry c * n + f hold frame
        f cut where the mean squared error mse is met at 1/2^reduce size, or at byte_cap -- at reduce 0 what
        Encoder.encode_target_torch gives on the original frames.  sidecar: cuda int64 (n, stride >= sidecar_entries), row f
        the sidecar of master f (Encoder.distortion_sidecar_torch); reached: cuda int32, dist / equiv: cuda int64 of Q * n
        entries.  Needs a quality recutter (filt given).  Everything else as recut_cuts_torch; the workspace is cached per
        stream, apart from the other calls'."""
        n, Q = int(lens.shape[0]), len(cuts)
        stream_stride = _stream_stride(data, stream_stride, (offsets,))
        self._quality_tensors(n, Q, data, lens, sidecar, out, offsets, dict(sizes=sizes, dist=dist, equiv=equiv), dict(rcs=rcs, reached=reached))
        _enqueue(self.lib, "icerx_recut_device_target_async", self._target_workspaces, self.target_workspace_bytes(n, data.numel(), Q),
                 data.device, self.recut_target_device_async_ptrs, n, data, data.numel(), offsets, stream_stride, lens, sidecar, sidecar.shape[1],
                 [c[0] for c in cuts], [c[1] for c in cuts], int(byte_cap), out, out.shape[-1], sizes, rcs, reached, dist, equiv)

    def budget_workspace_bytes(self, n: int, data_bytes: int, n_budgets: int) -> int:
        """icerx_recut_budget_workspace_bytes: the device workspace one recut_budget_device_async_ptrs call needs"""
        return int(_need(self.lib, "icerx_recut_budget_workspace_bytes")(self.handle, n, data_bytes, n_budgets))

    def recut_budget_device_async_ptrs(self, n: int, d_data: int, data_bytes: int, d_offsets, stream_stride: int, d_lens: int, d_sidecar: int,
                                       sidecar_stride: int, reduce: int, budgets, byte_cap: int, d_out: int, out_stride: int, d_sizes: int,
                                       d_rcs: int, d_at_cap: int, d_dist: int, d_equiv_quota: int, d_threshold: int, d_total: int,
                                       d_workspace: int, workspace_bytes: int, stream: int = 0, n_budgets=None) -> int:
        """icerx_recut_device_budget_async on raw device pointers (as recut_target_device_async_ptrs; one reduce for the call;
        budgets: a host sequence, None for a null pointer; d_threshold / d_total: uint64, entry b).  Enqueues on `stream` and
        returns the call's rc without waiting."""
        fn = _need(self.lib, "icerx_recut_device_budget_async")
        nb = n_budgets if n_budgets is not None else (len(budgets) if budgets is not None else 0)
        return fn(self.handle, n, d_data, data_bytes, d_offsets, stream_stride, d_lens, d_sidecar, sidecar_stride, reduce,
                  c_array(C.c_uint64, budgets), nb, byte_cap, d_out, out_stride, d_sizes, d_rcs, d_at_cap, d_dist, d_equiv_quota, d_threshold,
                  d_total, d_workspace, workspace_bytes, stream)

    def recut_budget_torch(self, data, lens, sidecar, budgets, byte_cap: int, out, sizes, rcs, at_cap, dist, equiv, threshold, total, reduce: int = 0,
                           offsets=None, stream_stride=None) -> None:
        """recut_target_torch with byte budgets in place of the targets: row and entry b * n + f hold frame f when the n masters
        share budgets[b] bytes at one distortion threshold, no stream above byte_cap, all at 1/2^reduce size -- at reduce 0 what
        Encoder.encode_budget_torch gives on the original frames.  at_cap: cuda int32 of B * n entries; threshold / total: cuda
        int64 (B,).  The workspace is cached per stream, apart from the other calls'."""
        import torch
        n, Q = int(lens.shape[0]), len(budgets)
        stream_stride = _stream_stride(data, stream_stride, (offsets,))
        self._quality_tensors(n, Q, data, lens, sidecar, out, offsets, dict(sizes=sizes, dist=dist, equiv=equiv), dict(rcs=rcs, at_cap=at_cap))
        _need_tensors(("threshold", threshold, torch.int64), ("total", total, torch.int64))
        if threshold.numel() != Q or total.numel() != Q:
            raise ValueError("threshold and total must have an entry per budget")
        _enqueue(self.lib, "icerx_recut_device_budget_async", self._budget_workspaces, self.budget_workspace_bytes(n, data.numel(), Q),
                 data.device, self.recut_budget_device_async_ptrs, n, data, data.numel(), offsets, stream_stride, lens, sidecar, sidecar.shape[1],
                 int(reduce), [int(b) for b in budgets], int(byte_cap), out, out.shape[-1], sizes, rcs, at_cap, dist, equiv, threshold, total)

    def _quality_through(self, streams, sidecars, Q, byte_cap, call):
        """bytes and sidecar rows in; call(blob, lens, offs, sidecar, out, sizes, rcs, flag, dist, equiv); -> per row a dict"""
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        n = len(streams)
        side = torch.from_numpy(np.ascontiguousarray(np.asarray(sidecars, np.uint64).reshape(n, -1)).view(np.int64)).to(dev)
        flag = torch.zeros(Q * n, dtype=torch.int32, device=dev)
        dist, equiv = (torch.zeros(Q * n, dtype=torch.int64, device=dev) for _ in range(2))
        rows = _bytes_through(streams, Q * n, max(int(byte_cap), 1), lambda blob, lens, offs, out, sizes, rcs:
                              call(blob, lens, offs, side, out, sizes, rcs, flag, dist, equiv))
        flag, dist, equiv = flag.cpu().numpy(), dist.cpu().numpy().view(np.uint64), equiv.cpu().numpy().view(np.uint64)
        return [dict(rc=rc, stream=s, flag=int(flag[k]), dist=int(dist[k]), equiv=int(equiv[k])) for k, (rc, s) in enumerate(rows)]

    def recut_target(self, streams, sidecars, cuts, byte_cap: int):
        """bytes in, bytes out: res[c][f] = dict(rc, stream, reached, dist, equiv) of master streams[f] with sidecar row sidecars[f]
        (uint64 words) at cuts[c] = (reduce, mse) under byte_cap (copies to the device and back, and waits: a convenience, not the
        fast path)"""
        n, Q = len(streams), len(cuts)
        rows = self._quality_through(streams, sidecars, Q, byte_cap, lambda blob, lens, offs, side, out, sizes, rcs, flag, dist, equiv:
                                     self.recut_target_torch(blob, lens, side, cuts, byte_cap, out, sizes, rcs, flag, dist, equiv, offsets=offs))
        for row in rows:
            row["reached"] = row.pop("flag")
        return [rows[c * n: (c + 1) * n] for c in range(Q)]

    def recut_budget(self, streams, sidecars, budgets, byte_cap: int, reduce: int = 0):
        """bytes in, bytes out: (res, thresholds, totals) with res[b][f] = dict(rc, stream, at_cap, dist, equiv) of master streams[f]
        when the masters share budgets[b] bytes (copies to the device and back, and waits: a convenience, not the fast path)"""
        import torch
        n, Q = len(streams), len(budgets)
        dev = torch.device("cuda", torch.cuda.current_device())
        threshold, total = (torch.zeros(Q, dtype=torch.int64, device=dev) for _ in range(2))
        rows = self._quality_through(streams, sidecars, Q, byte_cap, lambda blob, lens, offs, side, out, sizes, rcs, flag, dist, equiv:
                                     self.recut_budget_torch(blob, lens, side, budgets, byte_cap, out, sizes, rcs, flag, dist, equiv, threshold,
                                                             total, reduce=reduce, offsets=offs))
        for row in rows:
            row["at_cap"] = row.pop("flag")
        return ([rows[b * n: (b + 1) * n] for b in range(Q)], [int(t) for t in threshold.cpu().numpy().view(np.uint64)],
                [int(t) for t in total.cpu().numpy().view(np.uint64)])

    # ---- refinement increments: the difference and the union of two stored streams (icerx_combine_device_async) ----
    def combine_workspace_bytes(self, n: int, data_bytes: int) -> int:
        """icerx_combine_workspace_bytes: the device workspace one combine_device_async_ptrs call needs"""
        return int(_need(self.lib, "icerx_combine_workspace_bytes")(self.handle, n, data_bytes))

    def combine_device_async_ptrs(self, n: int, op: int, d_data: int, data_bytes: int, d_offsets_a, base_a: int, d_lens_a: int, d_offsets_b,
                                  base_b: int, d_lens_b: int, stream_stride: int, d_out: int, out_stride: int, d_sizes: int, d_rcs: int,
                                  d_counts: int, d_workspace: int, workspace_bytes: int, stream: int = 0) -> int:
        """icerx_combine_device_async on raw device pointers.  Both operands lie in the blob d_data: frame k of operand X is
        [off, off + lens_x[k]) with off = offsets_x[k], or base_x + k * stream_stride when d_offsets_x is None (offsets, lens,
        sizes: uint64 / int64; rcs: int32; counts: uint32, entries 2 k and 2 k + 1 = packets written, of them from A).  Frame k
        is row k of d_out.  Enqueues on `stream` and returns the call's rc without waiting."""
        fn = _need(self.lib, "icerx_combine_device_async")
        return fn(self.handle, n, op, d_data, data_bytes, d_offsets_a, base_a, d_lens_a, d_offsets_b, base_b, d_lens_b, stream_stride, d_out,
                  out_stride, d_sizes, d_rcs, d_counts, d_workspace, workspace_bytes, stream)

    def combine_torch(self, data, op, lens_a, lens_b, out, sizes, rcs, counts, offsets_a=None, offsets_b=None, base_a=0, base_b=0,
                      stream_stride=None) -> None:
        """The union (COMBINE_UNION) or the difference (COMBINE_DIFFERENCE: the packets of B that A lacks) of two stored streams
        per frame, on torch's current stream, without waiting.

        data: one cuda uint8 tensor that holds both operands, of any shape; lens_a / lens_b (and offsets_a / offsets_b, if given):
        cuda int64 (n,).  Without offsets frame k of operand X starts at base_x + k * stream_stride bytes (default:
        data.stride(-2) of a blob with rows), so the output of one recut_*_torch call with the held cut c and the wanted cut d
        goes in as it is: data = out, base_a = c * n * out_stride, base_b = d * n * out_stride, lens sizes[c] and sizes[d].
        out: cuda uint8 (n, out_stride); sizes: cuda int64 (n,); rcs: cuda int32 (n,); counts: cuda int32 (n, 2) or 2 n entries.
        A frame whose result is longer than out_stride gets ICER_OUTPUT_BUF_TOO_SMALL, the bytes needed in sizes and an untouched
        row.  The workspace is cached per stream, apart from the other calls'."""
        import torch
        n = int(lens_a.shape[0])
        stream_stride = _stream_stride(data, stream_stride, (offsets_a, offsets_b), any_rows=True)
        _need_tensors(("data", data, torch.uint8), ("lens_a", lens_a, torch.int64), ("lens_b", lens_b, torch.int64), ("out", out, torch.uint8),
                      ("sizes", sizes, torch.int64), ("rcs", rcs, torch.int32), ("counts", counts, torch.int32),
                      ("offsets_a", offsets_a, torch.int64), ("offsets_b", offsets_b, torch.int64))
        if out.dim() != 2 or out.shape[0] != n or any(t.numel() != n for t in (lens_b, sizes, rcs)) or counts.numel() != 2 * n or \
                any(t is not None and t.numel() != n for t in (offsets_a, offsets_b)):
            raise ValueError("out must be (n, out_stride), lens, offsets, sizes and rcs n entries, counts 2 n")
        _enqueue(self.lib, "icerx_combine_device_async", self._combine_workspaces, self.combine_workspace_bytes(n, data.numel()), data.device,
                 self.combine_device_async_ptrs, n, op, data, data.numel(), offsets_a, int(base_a), lens_a, offsets_b, int(base_b), lens_b,
                 stream_stride, out, out.shape[-1], sizes, rcs, counts)

    def combine(self, streams_a, streams_b, op):
        """bytes in, bytes out: res[f] = (rc, stream, packets written, of them from A) of streams_a[f] and streams_b[f] under `op`
        (copies to the device and back, and waits: a convenience, not the fast path)"""
        import torch
        if len(streams_a) != len(streams_b):
            raise ValueError("one stream of each operand per frame")
        n = len(streams_a)
        counts = torch.zeros((n, 2), dtype=torch.int32, device=torch.device("cuda", torch.cuda.current_device()))
        rows = _bytes_through(list(streams_a) + list(streams_b), n, max(max(len(a) + len(b) for a, b in zip(streams_a, streams_b)), 1),
                              lambda blob, lens, offs, out, sizes, rcs:
                              self.combine_torch(blob, op, lens[:n].contiguous(), lens[n:].contiguous(), out, sizes, rcs, counts,
                                                 offsets_a=offs[:n].contiguous(), offsets_b=offs[n:].contiguous()))
        counts = counts.cpu().numpy()
        return [row + (int(counts[f, 0]), int(counts[f, 1])) for f, row in enumerate(rows)]


# ---- standalone wavelet transform, inverse (include/icer_hip_dec.h; the forward is in api.py) -------------------------
def inverse_wavelet_transform(data: np.ndarray, filt: int, stages: int = 1, kind: str = "stages", image_w=None, image_h=None,
                              rowstride=None, N=None, stride: int = 1) -> int:
    """icer_inverse_wavelet_transform_{stages,2d,1d}_{uint16,uint8} on a host array, in place; arguments as
    api.wavelet_transform.  Returns the reference's icer_status."""
    from . import api
    return api._wavelet_host(load_library(), True, data, filt, stages, kind, image_w, image_h, rowstride, N, stride)


def wavelet_inverse_torch(planes, stages: int, filt: int):
    """icerx_wavelet_inverse_device on a cuda tensor (..., h, w) in place, on torch's current stream; returns the
    per-plane icer_status as a cuda int32 tensor (see api.wavelet_forward_torch)."""
    from . import api
    return api._wavelet_torch(load_library().icerx_wavelet_inverse_device, planes, stages, filt)
