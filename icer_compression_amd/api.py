"""Host-side mirror of the reference interface for the encode path, over the C ABI of
libicer_hip.so (include/icer_hip.h).

The reference is a C library (lib_icer); its own callers do
    icer_init(); icer_init_output_struct(&out, buf, len, quota);
    rc = icer_compress_image_uint16(img, w, h, stages, filt, segments, &out);
    fwrite(out.rearrange_start, out.size_used)
(example/src/example_encode.c:36-77, example/src/icer_util.c:186-227).  The functions below keep the
same names, argument order, in-place side effect on the image and return codes, with numpy arrays
standing in for the raw pointers.  `Encoder` wraps the batched / device-resident extension
(icerx_*), which is what bench.py times.

There is no CPU fallback: importing works anywhere, but every compress call needs libicer_hip.so
and a HIP device and fails loudly otherwise.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from ._abi import ENCODER, c_array, declare, icer_output_data_buf_typedef  # noqa: F401  (the struct is part of this module's interface)

PKG = os.path.dirname(os.path.abspath(__file__))
# (ICER_HIP_LIB: another build of the same library, e.g. one made with different tuning flags -- measurements only)
LIB_PATH = os.environ.get("ICER_HIP_LIB") or os.path.join(PKG, "libicer_hip.so")

# enum icer_status (lib_icer/inc/icer.h:92-105)
ICER_RESULT_OK = 0
ICER_INTEGER_OVERFLOW = -1
ICER_OUTPUT_BUF_TOO_SMALL = -2
ICER_TOO_MANY_SEGMENTS = -3
ICER_TOO_MANY_STAGES = -4
ICER_BYTE_QUOTA_EXCEEDED = -5
ICER_BITPLANE_OUT_OF_RANGE = -6
ICER_PACKET_COUNT_EXCEEDED = -9
ICER_FATAL_ERROR = -10
ICER_INVALID_INPUT = -11
# enum icer_filter_types (icer.h:107-115)
ICER_FILTER_A, ICER_FILTER_B, ICER_FILTER_C, ICER_FILTER_D, ICER_FILTER_E, ICER_FILTER_F, ICER_FILTER_Q = range(7)
ICERX_NUM_STAGES = 4
STAGE_NAMES = ("dwt", "ll_mean+sign_magnitude", "code_units", "scan+gather")


class IcerHipError(RuntimeError):
    pass


_lib = None


def load_library() -> C.CDLL:
    """dlopen libicer_hip.so (RTLD_LOCAL: it exports the same icer_* names as the reference)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise IcerHipError(f"{LIB_PATH} is missing: build it with `python -m icer_compression_amd.build` "
                           "(hipcc, gfx950).  There is no CPU fallback.")
    _lib = declare(C.CDLL(LIB_PATH, mode=os.RTLD_LOCAL), ENCODER)
    return _lib


# ---- lib_icer-shaped entry points --------------------------------------------------------------
def icer_init() -> int:
    return load_library().icer_init()


def icer_init_output_struct(out: icer_output_data_buf_typedef, data: np.ndarray, buf_len: int, byte_quota: int) -> int:
    return load_library().icer_init_output_struct(C.byref(out), data.ctypes.data, buf_len, byte_quota)


def _check_plane(a: np.ndarray, w: int, h: int, dtype=np.uint16) -> None:
    if a.dtype != dtype or not a.flags["C_CONTIGUOUS"] or a.size != w * h:
        raise ValueError(f"image planes must be C-contiguous {np.dtype(dtype).name} arrays of w*h elements")


def icer_compress_image_uint16(image: np.ndarray, image_w: int, image_h: int, stages: int, filt: int, segments: int,
                               output_data: icer_output_data_buf_typedef) -> int:
    _check_plane(image, image_w, image_h)
    return load_library().icer_compress_image_uint16(image.ctypes.data, image_w, image_h, stages, filt, segments,
                                                     C.byref(output_data))


def icer_compress_image_yuv_uint16(y: np.ndarray, u: np.ndarray, v: np.ndarray, image_w: int, image_h: int, stages: int,
                                   filt: int, segments: int, output_data: icer_output_data_buf_typedef) -> int:
    for p in (y, u, v):
        _check_plane(p, image_w, image_h)
    return load_library().icer_compress_image_yuv_uint16(y.ctypes.data, u.ctypes.data, v.ctypes.data, image_w, image_h,
                                                         stages, filt, segments, C.byref(output_data))


def icer_compress_image_uint8(image: np.ndarray, image_w: int, image_h: int, stages: int, filt: int, segments: int,
                              output_data: icer_output_data_buf_typedef) -> int:
    _check_plane(image, image_w, image_h, np.uint8)
    return load_library().icer_compress_image_uint8(image.ctypes.data, image_w, image_h, stages, filt, segments,
                                                    C.byref(output_data))


def icer_compress_image_yuv_uint8(y: np.ndarray, u: np.ndarray, v: np.ndarray, image_w: int, image_h: int, stages: int,
                                  filt: int, segments: int, output_data: icer_output_data_buf_typedef) -> int:
    for p in (y, u, v):
        _check_plane(p, image_w, image_h, np.uint8)
    return load_library().icer_compress_image_yuv_uint8(y.ctypes.data, u.ctypes.data, v.ctypes.data, image_w, image_h,
                                                        stages, filt, segments, C.byref(output_data))


def compress_u8(planes, stages: int, filt: int, segments: int, byte_quota: int):
    """As compress(), through the uint8 twins (planes: (h, w) uint8 arrays, int8 storage)."""
    icer_init()
    work = [np.ascontiguousarray(p, dtype=np.uint8).copy() for p in planes]
    h, w = work[0].shape
    buf = np.zeros(2 * byte_quota + 64, dtype=np.uint8)
    out = icer_output_data_buf_typedef()
    rc = icer_init_output_struct(out, buf, buf.size, byte_quota)
    if rc != ICER_RESULT_OK:
        return rc, b"", work
    if len(work) == 1:
        rc = icer_compress_image_uint8(work[0], w, h, stages, filt, segments, out)
    else:
        rc = icer_compress_image_yuv_uint8(work[0], work[1], work[2], w, h, stages, filt, segments, out)
    return rc, bytes(buf[byte_quota: byte_quota + out.size_used]), work


def compress(planes, stages: int, filt: int, segments: int, byte_quota: int):
    """Convenience wrapper used by the tests: same call sequence as the reference's CLI
    (example/src/icer_util.c:186-227).  Returns (rc, stream bytes, planes as left by the call)."""
    icer_init()
    work = [np.ascontiguousarray(p, dtype=np.uint16).copy() for p in planes]
    h, w = work[0].shape
    buf = np.zeros(2 * byte_quota + 64, dtype=np.uint8)
    out = icer_output_data_buf_typedef()
    rc = icer_init_output_struct(out, buf, buf.size, byte_quota)
    if rc != ICER_RESULT_OK:
        return rc, b"", work
    if len(work) == 1:
        rc = icer_compress_image_uint16(work[0], w, h, stages, filt, segments, out)
    else:
        rc = icer_compress_image_yuv_uint16(work[0], work[1], work[2], w, h, stages, filt, segments, out)
    return rc, bytes(buf[byte_quota: byte_quota + out.size_used]), work


# ---- batched / device-resident extension ----------------------------------------------------------
def _check(name: str, rc: int, detail=None) -> None:
    """rc -> IcerHipError; detail: the text behind the code, by default the library's last error"""
    if rc != 0:
        raise IcerHipError(f"{name} rc={rc}" + (": " + load_library().icerx_last_error().decode() if detail is None else detail))


def _cut_outputs(frames, rows: int, stride: int, int64s: int = 1, int32s: int = 1):
    """the outputs of a call that cuts every frame `rows` times, on the frames' device: the streams, uint8 (rows, n, stride), and
    lists of int64 and of int32 tensors (rows, n)"""
    import torch
    n, dev = frames.shape[0], frames.device
    return (torch.empty((rows, n, int(stride)), dtype=torch.uint8, device=dev),
            [torch.empty((rows, n), dtype=torch.int64, device=dev) for _ in range(int64s)],
            [torch.empty((rows, n), dtype=torch.int32, device=dev) for _ in range(int32s)])


class Encoder:
    """icerx_encoder: frames of one geometry, many per call, buffers resident on one GPU."""

    def __init__(self, w: int, h: int, channels: int = 1, stages: int = 4, filt: int = ICER_FILTER_A, segments: int = 10,
                 max_frames: int = 1, device: int = 0, sample_bits: int = 16):
        self.lib = load_library()
        self.w, self.h, self.channels, self.max_frames, self.device = w, h, channels, max_frames, device
        self.sample_bits = sample_bits
        self.handle = C.c_void_p()
        rc = self.lib.icerx_encoder_create_ex(C.byref(self.handle), device, w, h, channels, stages, filt, segments, max_frames,
                                              sample_bits)
        self.create_rc = rc
        if rc != 0:
            self.handle = C.c_void_p()
            if rc == ICER_FATAL_ERROR:
                raise IcerHipError(f"icerx_encoder_create failed: {self.lib.icerx_last_error().decode()}")

    def close(self):
        if getattr(self, "handle", None) and self.handle.value:
            self.lib.icerx_encoder_destroy(self.handle)
            self.handle = C.c_void_p()

    __del__ = close

    def encode_device_ptrs(self, d_frames: int, n_frames: int, byte_quota: int, d_out: int, out_stride: int, d_sizes: int,
                           d_rcs: int, stream: int = 0) -> None:
        rc = self.lib.icerx_encode_device(self.handle, d_frames, n_frames, byte_quota, d_out, out_stride, d_sizes, d_rcs,
                                          stream)
        _check("icerx_encode_device", rc)

    def encode_device_async_ptrs(self, d_frames: int, n_frames: int, byte_quota: int, d_out: int, out_stride: int, d_sizes: int,
                                 d_rcs: int, stream: int = 0) -> None:
        """first half of encode_device_ptrs: returns once everything is enqueued; wait() completes it"""
        rc = self.lib.icerx_encode_device_async(self.handle, d_frames, n_frames, byte_quota, d_out, out_stride, d_sizes, d_rcs, stream)
        _check("icerx_encode_device_async", rc)

    def wait(self) -> None:
        rc = self.lib.icerx_encoder_wait(self.handle)
        _check("icerx_encoder_wait", rc)

    def encode_torch(self, frames, byte_quota: int, out, sizes, rcs) -> None:
        """frames: cuda int16/uint16 tensor (n, channels, h, w) or (n, h, w); out: cuda uint8 (n, stride);
        sizes: cuda int64 (n,); rcs: cuda int32 (n,).  Runs on torch's current stream."""
        import torch
        n = frames.shape[0]
        st = torch.cuda.current_stream(frames.device).cuda_stream
        self.encode_device_ptrs(frames.data_ptr(), n, byte_quota, out.data_ptr(), out.stride(0), sizes.data_ptr(),
                                rcs.data_ptr(), st)

    def encode_ladder_ptrs(self, d_frames: int, n_frames: int, quotas, d_out: int, out_stride: int, d_sizes: int, d_rcs: int,
                           stream: int = 0) -> None:
        """icerx_encode_device_ladder: the frames at every quota of `quotas` (at most ICERX_MAX_LADDER) in one call; frame f at
        quotas[q] goes to row q * n_frames + f of d_out and entry q * n_frames + f of d_sizes / d_rcs"""
        rc = self.lib.icerx_encode_device_ladder(self.handle, d_frames, n_frames, c_array(C.c_size_t, quotas), len(quotas), d_out, out_stride,
                                                 d_sizes, d_rcs, stream)
        _check("icerx_encode_device_ladder", rc)

    def encode_ladder_torch(self, frames, quotas, out=None, sizes=None, rcs=None):
        """frames: cuda tensor (n, channels, h, w) or (n, h, w) -- int16/uint16, or uint8 (int8 storage) for an encoder of
        sample_bits 8.  Codes them once at every quota of `quotas` on torch's current stream.  out: cuda uint8 (Q, n, stride),
        sizes: cuda int64 (Q, n), rcs: cuda int32 (Q, n), allocated (stride = the largest quota) when not given.  Returns
        (out, sizes, rcs)."""
        import torch
        n, Q = frames.shape[0], len(quotas)
        dev = frames.device
        if out is None or sizes is None or rcs is None:
            own_out, (own_sizes,), (own_rcs,) = _cut_outputs(frames, Q, max(int(q) for q in quotas) if out is None else 0)
            out, sizes, rcs = (own_out if out is None else out), (own_sizes if sizes is None else sizes), (own_rcs if rcs is None else rcs)
        if out.dim() != 3 or tuple(out.shape[:2]) != (Q, n) or out.stride(2) != 1 or out.stride(0) != n * out.stride(1):
            raise ValueError("out must be a uint8 tensor (Q, n, stride) whose rows are stride bytes apart")
        if tuple(sizes.shape) != (Q, n) or tuple(rcs.shape) != (Q, n) or not sizes.is_contiguous() or not rcs.is_contiguous():
            raise ValueError("sizes and rcs must be contiguous tensors (Q, n)")
        st = torch.cuda.current_stream(dev).cuda_stream
        self.encode_ladder_ptrs(frames.data_ptr(), n, quotas, out.data_ptr(), out.stride(1), sizes.data_ptr(), rcs.data_ptr(), st)
        return out, sizes, rcs

    def encode_roi_ptrs(self, d_frames: int, n_frames: int, d_rois: int, shift: int, quotas, d_out: int, out_stride: int, d_sizes: int,
                        d_rcs: int, d_kept: int, d_foreground: int, stream: int = 0) -> None:
        """icerx_encode_device_roi: the ladder's call with every frame's quota spent first inside its rectangle (d_rois: device,
        n_frames x 4 uint32 x, y, w, h), the foreground `shift` bit planes ahead; outputs quota-major as the ladder's, K to entry
        q * n_frames + f of d_kept, the frames' foreground units to d_foreground"""
        rc = self.lib.icerx_encode_device_roi(self.handle, d_frames, n_frames, d_rois, int(shift), c_array(C.c_size_t, quotas), len(quotas),
                                              d_out, out_stride, d_sizes, d_rcs, d_kept, d_foreground, stream)
        _check("icerx_encode_device_roi", rc)

    def encode_roi_torch(self, frames, rois, shift: int, quotas):
        """frames: as encode_ladder_torch takes them.  rois: cuda int32 or uint32 tensor (n, 4) on the frames' device -- x, y, w, h
        of every frame's rectangle, read on torch's current stream (no synchronisation needed after the kernel that wrote it).
        Returns cuda tensors (out uint8 (Q, n, largest quota), sizes int64 (Q, n), rcs int32 (Q, n), kept int32 (Q, n) holding the
        uint32 K, foreground int32 (n,))."""
        import torch
        n, Q, dev = frames.shape[0], len(quotas), frames.device
        if rois.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or tuple(rois.shape) != (n, 4) or rois.device != dev or \
                not rois.is_contiguous():
            raise ValueError("rois must be a contiguous int32 or uint32 tensor (n, 4) on the frames' device")
        out, (sizes,), (rcs, kept) = _cut_outputs(frames, Q, max(int(q) for q in quotas), int32s=2)
        foreground = torch.empty((n,), dtype=torch.int32, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        self.encode_roi_ptrs(frames.data_ptr(), n, rois.data_ptr(), shift, quotas, out.data_ptr(), out.stride(1), sizes.data_ptr(), rcs.data_ptr(),
                             kept.data_ptr(), foreground.data_ptr(), st)
        return out, sizes, rcs, kept, foreground

    def encode_target_ptrs(self, d_frames: int, n_frames: int, targets_mse, byte_cap: int, d_out: int, out_stride: int, d_sizes: int,
                           d_rcs: int, d_reached: int, d_dist: int, d_equiv_quota: int, stream: int = 0) -> None:
        """icerx_encode_device_target: every frame cut where each mean-squared-error target of `targets_mse` (at most
        ICERX_MAX_LADDER) is met, or at byte_cap; frame f at targets_mse[t] goes to row / entry t * n_frames + f of the outputs"""
        rc = self.lib.icerx_encode_device_target(self.handle, d_frames, n_frames, c_array(C.c_double, targets_mse), len(targets_mse), byte_cap,
                                                 d_out, out_stride, d_sizes, d_rcs, d_reached, d_dist, d_equiv_quota, stream)
        _check("icerx_encode_device_target", rc)

    def encode_target_torch(self, frames, targets, byte_cap: int, psnr: bool = False):
        """frames: as encode_ladder_torch takes them.  targets: mean squared errors per sample, or with psnr=True peak
        signal-to-noise ratios in dB against the encoder's sample peak (2^sample_bits - 1), converted on the host.  Returns cuda
        tensors (out uint8 (T, n, byte_cap), sizes int64 (T, n), rcs int32 (T, n), reached int32 (T, n), dist int64 (T, n) holding
        the uint64 distortions, equiv_quota int64 (T, n)), on torch's current stream."""
        import torch
        peak = float((1 << self.sample_bits) - 1)
        mse = [peak * peak / 10.0 ** (float(t) / 10.0) for t in targets] if psnr else [float(t) for t in targets]
        n, T, dev = frames.shape[0], len(mse), frames.device
        out, (sizes, dist, equiv), (rcs, reached) = _cut_outputs(frames, T, byte_cap, int64s=3, int32s=2)
        st = torch.cuda.current_stream(dev).cuda_stream
        self.encode_target_ptrs(frames.data_ptr(), n, mse, int(byte_cap), out.data_ptr(), out.stride(1), sizes.data_ptr(), rcs.data_ptr(),
                                reached.data_ptr(), dist.data_ptr(), equiv.data_ptr(), st)
        return out, sizes, rcs, reached, dist, equiv

    def encode_budget_ptrs(self, d_frames: int, n_frames: int, budgets, byte_cap: int, d_out: int, out_stride: int, d_sizes: int, d_rcs: int,
                           d_at_cap: int, d_dist: int, d_equiv_quota: int, d_threshold: int, d_total: int, stream: int = 0) -> None:
        """icerx_encode_device_budget: for each byte budget of `budgets` (at most ICERX_MAX_LADDER) the frames share it at one
        distortion threshold, no stream above byte_cap; frame f at budgets[b] goes to row / entry b * n_frames + f of the
        per-stream outputs, the threshold and the sum of the sizes to entry b of d_threshold / d_total"""
        rc = self.lib.icerx_encode_device_budget(self.handle, d_frames, n_frames, c_array(C.c_uint64, budgets), len(budgets), byte_cap, d_out,
                                                 out_stride, d_sizes, d_rcs, d_at_cap, d_dist, d_equiv_quota, d_threshold, d_total, stream)
        _check("icerx_encode_device_budget", rc)

    def encode_budget_torch(self, frames, budgets, byte_cap: int):
        """frames: as encode_ladder_torch takes them.  budgets: byte budgets for the whole batch.  Returns cuda tensors (out uint8
        (B, n, byte_cap), sizes int64 (B, n), rcs int32 (B, n), at_cap int32 (B, n), dist int64 (B, n) holding the uint64
        distortions, equiv_quota int64 (B, n), threshold int64 (B,) holding the uint64 thresholds, total int64 (B,)), on torch's
        current stream."""
        import torch
        n, nb, dev = frames.shape[0], len(budgets), frames.device
        out, (sizes, dist, equiv), (rcs, at_cap) = _cut_outputs(frames, nb, byte_cap, int64s=3, int32s=2)
        threshold, total = (torch.empty((nb,), dtype=torch.int64, device=dev) for _ in range(2))
        st = torch.cuda.current_stream(dev).cuda_stream
        self.encode_budget_ptrs(frames.data_ptr(), n, budgets, int(byte_cap), out.data_ptr(), out.stride(1), sizes.data_ptr(), rcs.data_ptr(),
                                at_cap.data_ptr(), dist.data_ptr(), equiv.data_ptr(), threshold.data_ptr(), total.data_ptr(), st)
        return out, sizes, rcs, at_cap, dist, equiv, threshold, total

    def target_threshold(self, target_mse: float) -> int:
        """the integer threshold a target becomes (icerx_target_threshold): floor(target_mse * samples * 16)"""
        return int(self.lib.icerx_target_threshold(self.handle, float(target_mse)))

    def distortion_table(self, frame: int = 0, families: int | None = None) -> np.ndarray:
        """the families' residual energies of `frame` in the last target or budget call (icerx_get_distortion_table): uint64 (families, P + 1).
        families: the rows of the table; by default units / P, which holds unless a subband has fewer samples than there are
        segments -- its planes then keep the rectangles of whichever packet comes before them in the priority order, every
        distinct rectangle is a family (csrc/plan.hpp, quirk P1), and the caller has to give the count."""
        planes = 7 if self.sample_bits == 8 else 9
        if families is None:
            families = self.info()["units_per_frame"] // planes      # (a family = the coded planes of one rectangle, csrc/plan.hpp)
        dst = np.zeros((families, planes + 1), np.uint64)
        rc = self.lib.icerx_get_distortion_table(self.handle, frame, dst.ctypes.data, dst.size)
        _check("icerx_get_distortion_table", rc, ": no target call yet, or the frame was not part of the last one")
        return dst

    @property
    def sidecar_entries(self) -> int:
        """icerx_distortion_sidecar_entries: the uint64 words of a frame's distortion sidecar, families * (P + 1) + 1"""
        return int(self.lib.icerx_distortion_sidecar_entries(self.handle))

    def distortion_sidecar_torch(self, n_frames: int | None = None, out=None):
        """the distortion sidecars of the first n_frames frames (default: max_frames) of the last target or budget call
        (icerx_get_distortion_sidecar_device): a cuda int64 tensor (n_frames, sidecar_entries) holding the uint64 words -- a
        frame's energy table as distortion_table gives it, then one word with its LL means --, written on torch's current
        stream without a host copy.  out: a cuda int64 tensor (n_frames, stride) with stride >= sidecar_entries and unit
        stride along a row, to write into; the words behind a row's entries are left alone.  Store a row beside the frame's
        master: decoder.Recutter re-cuts the master to a distortion target or a shared byte budget by it."""
        import torch
        n = self.max_frames if n_frames is None else int(n_frames)
        dev = torch.device("cuda", self.device)
        if out is None:
            out = torch.empty((n, self.sidecar_entries), dtype=torch.int64, device=dev)
        if not out.is_cuda or out.dtype != torch.int64 or out.dim() != 2 or out.shape[0] < n or out.stride(1) != 1:
            raise ValueError("out must be a cuda int64 tensor (n_frames, stride) with rows of consecutive words")
        rc = self.lib.icerx_get_distortion_sidecar_device(self.handle, n, out.data_ptr(), out.stride(0) if out.shape[0] > 1 else out.shape[1],
                                                          torch.cuda.current_stream(dev).cuda_stream)
        _check("icerx_get_distortion_sidecar_device", rc, ": no target or budget call yet, more frames than it had, or rows too short")
        return out

    def encode_torch_s8(self, planes, byte_quota: int):
        """uint8 twins: planes = cuda uint8 tensor (n, h, w) or (n, channels, h, w), int8 storage; the encoder must have
        been created with sample_bits=8.  Returns [(rc, stream bytes)] per frame."""
        import torch
        n = planes.shape[0]
        stride = byte_quota + 64
        out = torch.empty((n, stride), dtype=torch.uint8, device=planes.device)
        sizes = torch.empty(n, dtype=torch.int64, device=planes.device)
        rcs = torch.empty(n, dtype=torch.int32, device=planes.device)
        st = torch.cuda.current_stream(planes.device).cuda_stream
        rc = self.lib.icerx_encode_device_s8(self.handle, planes.data_ptr(), n, byte_quota, out.data_ptr(), stride,
                                             sizes.data_ptr(), rcs.data_ptr(), st)
        _check("icerx_encode_device_s8", rc)
        sz, rr, host = sizes.cpu().numpy(), rcs.cpu().numpy(), out.cpu().numpy()
        return [(int(rr[k]), bytes(host[k, : int(sz[k])])) for k in range(n)]

    def encode_torch_frontend(self, raw, byte_quota: int, out, sizes, rcs) -> None:
        """raw: cuda uint8 tensor, (n, h, w) gray for a 1-channel encoder or (n, h, w, 3) packed RGB for a
        3-channel one; converted on the device (icerx_encode_device_u8 / _rgb8)."""
        import torch
        fn = self.lib.icerx_encode_device_u8 if self.channels == 1 else self.lib.icerx_encode_device_rgb8
        st = torch.cuda.current_stream(raw.device).cuda_stream
        rc = fn(self.handle, raw.data_ptr(), raw.shape[0], byte_quota, out.data_ptr(), out.stride(0), sizes.data_ptr(),
                rcs.data_ptr(), st)
        _check("front-end encode", rc)

    def encode_host(self, frames: np.ndarray, byte_quota: int):
        """frames: uint16 array (n, channels, h, w) or (n, h, w).  Returns list of (rc, stream bytes)."""
        frames = np.ascontiguousarray(frames, dtype=np.uint16)
        n = frames.shape[0]
        stride = byte_quota
        out = np.zeros((n, stride), dtype=np.uint8)
        sizes = np.zeros(n, dtype=np.uint64)
        rcs = np.zeros(n, dtype=np.int32)
        rc = self.lib.icerx_encode_host(self.handle, frames.ctypes.data, n, byte_quota, out.ctypes.data, stride,
                                        sizes.ctypes.data, rcs.ctypes.data)
        _check("icerx_encode_host", rc)
        return [(int(rcs[i]), bytes(out[i, : int(sizes[i])])) for i in range(n)]

    def encode_host_into(self, frames: np.ndarray, byte_quota: int, out: np.ndarray, sizes: np.ndarray, rcs: np.ndarray) -> None:
        """the same into caller-owned arrays (out: uint8 (n, stride), sizes: uint64 (n,), rcs: int32 (n,)) -- nothing is
        allocated or copied on the Python side, so this is what a C caller of icerx_encode_host sees"""
        n = frames.shape[0]
        rc = self.lib.icerx_encode_host(self.handle, frames.ctypes.data, n, byte_quota, out.ctypes.data, out.shape[1],
                                        sizes.ctypes.data, rcs.ctypes.data)
        _check("icerx_encode_host", rc)

    def coefficients(self, frame: int = 0, channel: int = 0) -> np.ndarray:
        dst = np.zeros((self.h, self.w), dtype=np.uint16)
        rc = self.lib.icerx_get_coefficients(self.handle, frame, channel, dst.ctypes.data)
        _check("icerx_get_coefficients", rc, "")
        return dst

    def timing_enable(self, on: bool = True) -> None:
        self.lib.icerx_timing_enable(self.handle, 1 if on else 0)

    def timing_read(self, reset: bool = True):
        ms = (C.c_double * ICERX_NUM_STAGES)()
        calls = C.c_uint64(0)
        rc = self.lib.icerx_timing_read(self.handle, ms, C.byref(calls), 1 if reset else 0)
        _check("icerx_timing_read", rc, "")
        return {n: ms[i] for i, n in enumerate(STAGE_NAMES)}, int(calls.value)

    def stats(self):
        out = (C.c_uint64 * 4)()
        self.lib.icerx_encoder_stats(self.handle, out)
        return {"unit_timeouts": out[0], "fallback_batches": out[1], "slot_retries": out[2], "coder_mode": out[3]}

    def routing(self):
        """coding units that went to the small workgroup coder beside the pipeline kernel, and the calls that routed"""
        out = (C.c_uint64 * 2)()
        self.lib.icerx_encoder_routing(self.handle, out)
        return {"routed_units": out[0], "routed_calls": out[1]}

    def launch_info(self):
        """shape of the last launch (icerx_encoder_launch_info)"""
        out = (C.c_uint32 * 4)()
        self.lib.icerx_encoder_launch_info(self.handle, out)
        return {"split": bool(out[0]), "sub_range_workgroups": int(out[1]), "pipeline_waves": int(out[2]), "window_coder_beside": bool(out[3])}

    def parts(self) -> int:
        """parts the last call was enqueued in (icerx_encoder_parts)"""
        return int(self.lib.icerx_encoder_parts(self.handle))

    def info(self):
        u, b, s = C.c_uint32(), C.c_uint32(), C.c_uint64()
        self.lib.icerx_info(self.handle, C.byref(u), C.byref(b), C.byref(s))
        return {"units_per_frame": u.value, "slot_bits_per_pixel": b.value, "slot_bytes_per_frame": s.value}


def compress_batch(frames: np.ndarray, stages: int, filt: int, segments: int, byte_quota: int, out: np.ndarray, sizes: np.ndarray,
                   rcs: np.ndarray, devices=None) -> int:
    """icerx_compress_batch_uint16[_devices]: frames uint16 (n, h, w) or (n, channels, h, w) in host memory (page-locked for
    DMA: pin_host), out uint8 (n, stride), sizes uint64 (n,), rcs int32 (n,); devices = list of HIP devices, None = all.
    Returns the call's return code (0 = every frame coded; per-frame codes in rcs)."""
    L = load_library()
    n = frames.shape[0]
    ch = 1 if frames.ndim == 3 else frames.shape[1]
    h, w = frames.shape[-2:]
    assert frames.dtype == np.uint16 and frames.flags["C_CONTIGUOUS"] and out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"]
    if devices is None:
        return L.icerx_compress_batch_uint16(frames.ctypes.data, n, w, h, ch, stages, filt, segments, byte_quota, out.ctypes.data,
                                             out.shape[1], sizes.ctypes.data, rcs.ctypes.data, 0)
    dv = (C.c_int * len(devices))(*devices)
    return L.icerx_compress_batch_uint16_devices(frames.ctypes.data, n, w, h, ch, stages, filt, segments, byte_quota, out.ctypes.data,
                                                 out.shape[1], sizes.ctypes.data, rcs.ctypes.data, dv, len(devices))


def process_stats():
    """unit time-outs / batches re-coded by the barrier-only coder / slot re-runs, summed over every encoder of the process"""
    out = (C.c_uint64 * 4)()
    load_library().icerx_process_stats(out)
    return {"unit_timeouts": out[0], "fallback_batches": out[1], "slot_retries": out[2]}


def pin_host(arr) -> bool:
    """page-lock a numpy array (icerx_pin_host); returns False if the runtime refuses"""
    return load_library().icerx_pin_host(arr.ctypes.data, arr.nbytes) == 0


def unpin_host(arr) -> None:
    load_library().icerx_unpin_host(arr.ctypes.data)


# ---- standalone wavelet transform (include/icer_hip.h; the inverse twins are in decoder.py) --------------------------
_WL_KINDS = ("stages", "2d", "1d")


def _wavelet_host(lib, inverse: bool, data: np.ndarray, filt: int, stages: int, kind: str, image_w, image_h, rowstride, N, stride) -> int:
    if kind not in _WL_KINDS:
        raise ValueError(f"kind must be one of {_WL_KINDS}")
    if data.dtype not in (np.uint16, np.uint8) or not data.flags["C_CONTIGUOUS"]:
        raise ValueError("data must be a C-contiguous uint16 or uint8 array (changed in place)")
    bits = 16 if data.dtype == np.uint16 else 8
    pre = ("icer_inverse_wavelet_transform_" if inverse else "icer_wavelet_transform_") + kind + ("_uint16" if bits == 16 else "_uint8")
    fn = getattr(lib, pre)
    ptr = C.c_void_p(data.ctypes.data)
    if kind == "1d":
        N = data.size if N is None else int(N)
        if N >= 1 and (N - 1) * stride + 1 > data.size:
            raise ValueError("N samples at `stride` run past the array")
        return fn(ptr, N, stride, filt)
    h, w = data.shape[-2:] if data.ndim >= 2 else (1, data.size)
    image_w = w if image_w is None else int(image_w)
    image_h = h if image_h is None else int(image_h)
    if kind == "stages":
        if image_w * image_h > data.size:
            raise ValueError("image_w * image_h runs past the array")
        return fn(ptr, image_w, image_h, stages, filt)
    rowstride = w if rowstride is None else int(rowstride)
    if image_h >= 1 and image_w >= 1 and (image_h - 1) * rowstride + image_w > data.size:
        raise ValueError("the image_w x image_h region at `rowstride` runs past the array")
    return fn(ptr, image_w, image_h, rowstride, filt)


def wavelet_transform(data: np.ndarray, filt: int, stages: int = 1, kind: str = "stages", image_w=None, image_h=None,
                      rowstride=None, N=None, stride: int = 1) -> int:
    """icer_wavelet_transform_{stages,2d,1d}_{uint16,uint8} on a host array, in place (the dtype picks the twin):
    kind "stages" (image_w x image_h, default the array's shape), "2d" (one level on an image_w x image_h region of rows
    `rowstride` apart) or "1d" (N samples `stride` apart).  Returns the reference's icer_status."""
    return _wavelet_host(load_library(), False, data, filt, stages, kind, image_w, image_h, rowstride, N, stride)


def _wavelet_torch(fn, planes, stages: int, filt: int):
    import torch
    if not planes.is_cuda or not planes.is_contiguous() or planes.dtype not in (torch.int16, getattr(torch, "uint16", torch.int16), torch.int8, torch.uint8):
        raise ValueError("planes must be a contiguous cuda tensor of int16/uint16 (or int8/uint8 for the uint8 twins)")
    if planes.dim() < 2 or planes.shape[-1] == 0 or planes.shape[-2] == 0 or planes.numel() == 0:
        raise ValueError("planes must be a non-empty tensor (..., h, w)")
    bits = 16 if planes.element_size() == 2 else 8
    h, w = planes.shape[-2:]
    n = planes.numel() // (h * w)
    lib = load_library()
    ws = torch.empty(int(lib.icerx_wavelet_workspace_bytes(w, h, n, bits)), dtype=torch.uint8, device=planes.device)
    rcs = torch.zeros(n, dtype=torch.int32, device=planes.device)
    with torch.cuda.device(planes.device):
        st = torch.cuda.current_stream(planes.device).cuda_stream
        rc = fn(planes.data_ptr(), n, w, h, w * h, stages, filt, bits, ws.data_ptr(), rcs.data_ptr(), st)
    _check("wavelet transform", rc, "")
    return rcs


def wavelet_forward_torch(planes, stages: int, filt: int):
    """icerx_wavelet_forward_device on a cuda tensor (..., h, w) in place, on torch's current stream, with no host
    synchronisation; returns the per-plane icer_status as a cuda int32 tensor.  ICER_TOO_MANY_STAGES /
    ICER_INVALID_INPUT raise IcerHipError before anything runs."""
    return _wavelet_torch(load_library().icerx_wavelet_forward_device, planes, stages, filt)
