"""The ctypes declarations of the two product libraries, each function once: ENCODER for libicer_hip.so (include/icer_hip.h),
DECODER for libicer_hip_dec.so (include/icer_hip_dec.h), name -> (restype, [argtypes]).  api.load_library() and decoder.bind()
apply them with declare(); nothing else in the package declares.  tests/test_abi.py holds every entry against its prototype:
with ctypes an undeclared size_t, pointer or uint64_t parameter travels as a 32-bit int and nothing warns."""
import ctypes as C

import numpy as np


class icer_output_data_buf_typedef(C.Structure):       # icer.h:307-312
    _fields_ = [("size_used", C.c_size_t), ("size_allocated", C.c_size_t),
                ("data_start", C.c_void_p), ("rearrange_start", C.c_void_p)]


i, u, u8, sz, u64, dbl, p, text = C.c_int, C.c_uint, C.c_uint8, C.c_size_t, C.c_uint64, C.c_double, C.c_void_p, C.c_char_p
szp, ip, handle = C.POINTER(sz), C.POINTER(i), C.POINTER(p)
u8p = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")
outp = C.POINTER(icer_output_data_buf_typedef)

_gray, _yuv = [p, sz, sz, u8, i, u8, outp], [p, p, p, sz, sz, u8, i, u8, outp]      # icer_compress_image_*
_create = [handle, i, sz, sz, i, i, i, i, i]
_encode = [p, p, i, sz, p, sz, p, p, p]                                             # icerx_encode_device and its twins
_batch = [p, i, sz, sz, i, i, i, i, sz, p, sz, p, p]
_wl_stages, _wl_2d, _wl_1d = [p, sz, sz, u8, i], [p, sz, sz, sz, i], [p, sz, sz, i]
_wl_device = [p, i, sz, sz, sz, i, i, i, p, p, p]


def _wavelets(prefix):
    return {f"{prefix}_{kind}_{t}": (i, a) for kind, a in (("stages", _wl_stages), ("2d", _wl_2d), ("1d", _wl_1d))
            for t in ("uint16", "uint8")}


ENCODER = {
    "icer_init": (i, []),
    "icer_init_output_struct": (i, [outp, p, sz, sz]),
    "icer_compress_image_uint16": (i, _gray),
    "icer_compress_image_yuv_uint16": (i, _yuv),
    "icer_compress_image_uint8": (i, _gray),
    "icer_compress_image_yuv_uint8": (i, _yuv),
    "icerx_encoder_create": (i, _create),
    "icerx_encoder_create_ex": (i, _create + [i]),
    "icerx_encoder_destroy": (None, [p]),
    "icerx_encode_device": (i, _encode),
    "icerx_encode_device_async": (i, _encode),
    "icerx_encode_device_u8": (i, _encode),
    "icerx_encode_device_rgb8": (i, _encode),
    "icerx_encode_device_s8": (i, _encode),
    "icerx_encoder_wait": (i, [p]),
    "icerx_encode_device_ladder": (i, [p, p, i, szp, i, p, sz, p, p, p]),
    "icerx_encode_device_target": (i, [p, p, i, C.POINTER(dbl), i, sz, p, sz, p, p, p, p, p, p]),
    "icerx_encode_device_budget": (i, [p, p, i, C.POINTER(u64), i, sz, p, sz, p, p, p, p, p, p, p, p]),
    "icerx_encode_device_roi": (i, [p, p, i, p, i, szp, i, p, sz, p, p, p, p, p]),
    "icerx_target_threshold": (u64, [p, dbl]),
    "icerx_get_distortion_table": (i, [p, i, p, sz]),
    # the distortion sidecar: a frame's energy table and LL means in device memory (include/icer_hip_sidecar.h)
    "icerx_distortion_sidecar_entries": (sz, [p]),
    "icerx_get_distortion_sidecar_device": (i, [p, i, p, sz, p]),
    "icerx_encode_host": (i, [p, p, i, sz, p, sz, p, p]),
    "icerx_device_count": (i, []),
    "icerx_compress_batch_uint16": (i, _batch + [i]),
    "icerx_compress_batch_uint16_devices": (i, _batch + [ip, i]),
    "icerx_batch_release": (None, []),
    "icerx_pin_host": (i, [p, sz]),
    "icerx_unpin_host": (i, [p]),
    "icerx_get_coefficients": (i, [p, i, i, p]),
    "icerx_timing_enable": (i, [p, i]),
    "icerx_timing_read": (i, [p, C.POINTER(dbl), C.POINTER(u64), i]),
    "icerx_info": (i, [p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(u64)]),
    "icerx_encoder_stats": (i, [p, C.POINTER(u64)]),
    "icerx_encoder_routing": (i, [p, C.POINTER(u64)]),
    "icerx_encoder_launch_info": (i, [p, C.POINTER(C.c_uint32)]),
    "icerx_encoder_parts": (i, [p]),
    "icerx_process_stats": (i, [C.POINTER(u64)]),
    **_wavelets("icer_wavelet_transform"),
    "icer_to_sign_magnitude_int16": (None, [p, sz]),
    "icer_to_sign_magnitude_int8": (None, [p, sz]),
    "icerx_wavelet_workspace_bytes": (sz, [sz, sz, i, i]),
    "icerx_wavelet_forward_device": (i, _wl_device),
    "icerx_last_error": (text, []),
}

_image = [szp, szp, sz, u8p, sz, u8, i, u8]                      # icer_decompress_image_*, behind the planes
_sync = [p, i, p, szp, szp, p, sz, ip, szp, szp]                 # icerx_decode_host / _device and their display twins
_async = [p, i, p, sz, p, sz, p, p, sz, p, p, p, p, sz, p]       # icerx_decode_device_async and its display twin
_masters = [p, i, p, sz, p, sz, p]                               # recutter, n, blob, its bytes, offsets, stride, lens
_cut_out = [p, sz, p, p]                                         # out, its stride, sizes, rcs
_work = [p, sz, p]                                               # workspace, its bytes, stream
_sync_win = [p, i, p, szp, szp, p, p, sz, sz, ip, szp, szp, p]   # the synchronous window calls (icer_hip_dec_window.h)
_async_win = [p, i, p, sz, p, sz, p, p, p, sz, sz, p, p, p, p] + _work
_feed = [p, i, ip, p, szp, szp, p, ip, szp, szp]                 # session, n, slots, data, offsets, lens, out, rcs, ws, hs

DECODER = {
    "icer_get_image_dimensions": (i, [u8p, sz, szp, szp]),
    "icer_decompress_image_uint16": (i, [p] + _image),
    "icer_decompress_image_yuv_uint16": (i, [p, p, p] + _image),
    "icer_decompress_image_uint8": (i, [p] + _image),
    "icer_decompress_image_yuv_uint8": (i, [p, p, p] + _image),
    "icerx_decoder_create": (i, [handle, i, i, i, i, u, i]),
    "icerx_decoder_destroy": (None, [p]),
    "icerx_decode_host": (i, _sync),
    "icerx_decode_device": (i, _sync),
    "icerx_decode_workspace_bytes": (sz, [p, i, sz, sz]),
    "icerx_decode_device_async": (i, _async),
    # straight to 8-bit display images
    "icerx_decode_host_display": (i, _sync),
    "icerx_decode_device_display": (i, _sync),
    "icerx_decode_display_workspace_bytes": (sz, [p, i, sz, sz]),
    "icerx_decode_device_display_async": (i, _async),
    "icerx_planes_to_display_device": (i, [p, i, i, sz, sz, sz, i, p, sz, p]),
    "icerx_decompress_display": (i, [p] + _image + [i]),
    # decoding at 1/2^r resolution
    "icerx_decoder_create_reduced": (i, [handle, i, i, i, i, u, i, i]),
    "icerx_decoder_reduce": (i, [p]),
    "icerx_reduced_size": (None, [sz, sz, i, szp, szp]),
    "icerx_decompress_reduced": (i, [handle, i] + _image + [i, i]),
    # truncated coefficients rebuilt inside their interval
    "icerx_decoder_set_reconstruction": (i, [p, i]),
    "icerx_decoder_reconstruction": (i, [p]),
    "icerx_decompress_reconstructed": (i, [handle, i, szp, szp, sz, u8p, sz, i, i, u, i, i, i]),
    # re-cutting stored streams: by byte quota, by resolution, by region of interest
    "icerx_recutter_create": (i, [handle, i, sz, sz, i, i, u, i]),
    "icerx_recutter_create_reduced": (i, [handle, i, sz, sz, i, i, u, i, i]),
    "icerx_recutter_destroy": (None, [p]),
    "icerx_recutter_max_reduce": (i, [p]),
    "icerx_recut_workspace_bytes": (sz, [p, i, sz, i]),
    "icerx_recut_device_async": (i, _masters + [szp, i] + _cut_out + _work),
    "icerx_recut_cuts_workspace_bytes": (sz, [p, i, sz, i]),
    "icerx_recut_device_cuts_async": (i, _masters + [ip, szp, i] + _cut_out + _work),
    "icerx_recut_roi_workspace_bytes": (sz, [p, i, sz, i]),
    "icerx_recut_device_roi_async": (i, _masters + [p, ip, ip, szp, i] + _cut_out + [p, p] + _work),
    # re-cutting to a distortion target or a shared byte budget, by the masters' distortion sidecars (include/icer_hip_dec_quality.h)
    "icerx_recutter_create_quality": (i, [handle, i, sz, sz, i, i, i, u, i, i]),
    "icerx_recut_sidecar_entries": (sz, [p]),
    "icerx_recut_target_threshold": (u64, [p, dbl, i]),
    "icerx_recut_target_workspace_bytes": (sz, [p, i, sz, i]),
    "icerx_recut_device_target_async": (i, _masters + [p, sz, ip, C.POINTER(dbl), i, sz] + _cut_out + [p, p, p] + _work),
    "icerx_recut_budget_workspace_bytes": (sz, [p, i, sz, i]),
    "icerx_recut_device_budget_async": (i, _masters + [p, sz, i, C.POINTER(u64), i, sz] + _cut_out + [p, p, p, p, p] + _work),
    # refinement increments: the difference and the union of two stored streams
    "icerx_combine_workspace_bytes": (sz, [p, i, sz]),
    "icerx_combine_device_async": (i, [p, i, i, p, sz, p, sz, p, p, sz, p, sz] + _cut_out + [p] + _work),
    # window decode: a rectangle of each image, without the chains it does not depend on (include/icer_hip_dec_window.h)
    "icerx_decode_host_window": (i, _sync_win),
    "icerx_decode_device_window": (i, _sync_win),
    "icerx_decode_device_window_display": (i, _sync_win),
    "icerx_decode_window_workspace_bytes": (sz, [p, i, sz, sz]),
    "icerx_decode_device_window_async": (i, _async_win),
    "icerx_decode_window_display_workspace_bytes": (sz, [p, i, sz, sz]),
    "icerx_decode_device_window_display_async": (i, _async_win),
    "icerx_decompress_window": (i, [handle, i, szp, szp, sz, u8p, sz, i, i, u, i, i, i, p, p]),
    # progressive decode sessions: held frames refined from new packets (include/icer_hip_dec_session.h)
    "icerx_session_create": (i, [handle, p, i, sz]),
    "icerx_session_destroy": (None, [p]),
    "icerx_session_reset": (i, [p, i]),
    "icerx_session_feed_host": (i, _feed),
    "icerx_session_feed_device": (i, _feed),
    "icerx_session_feed_device_display": (i, _feed),
    "icerx_session_planes_held": (i, [p, i, i, i, i, i]),
    "icerx_session_stats": (i, [p, C.POINTER(u64)]),
    "icerx_decoder_last_error": (text, []),
    **_wavelets("icer_inverse_wavelet_transform"),
    "icer_from_sign_magnitude_int16": (None, [p, sz]),
    "icer_from_sign_magnitude_int8": (None, [p, sz]),
    "icerx_wavelet_inverse_device": (i, _wl_device),
}


def c_array(ctype, seq):
    """a host sequence -> a C array of `ctype` (at least one entry), None -> None: a null pointer"""
    if seq is None:
        return None
    conv = float if ctype is C.c_double else int
    return (ctype * max(len(seq), 1))(*[conv(x) for x in seq])


def declare(lib, table):
    """restype and argtypes of every entry of `table` whose symbol `lib` exports (the CPU mock builds of decoder.hip lack some)"""
    for name, (restype, argtypes) in table.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, list(argtypes)
    return lib
