"""The refused and degenerate calls of the synchronous decode entry points -- plain, display, window (include/icer_hip_dec.h,
icer_hip_dec_window.h) and session feeds (icer_hip_dec_session.h), host and device flavour -- as one table: the return code
each gives, the text of icerx_decoder_last_error() where the call fails with one, and that nothing is written to the
outputs.  Where a call breaks two rules at once the table records which one answers.  Runs against the mock build of
tests/test_display_mock.py.  CPU only."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests.test_display_mock import DECODER_HIP, MOCK_FLAGS

OK, FATAL, INVALID = 0, -10, -11
JUNK = 0xA5
N, CH, STRIDE = 2, 3, 16
FAR = 0xFFFFFFFF - 64                           # the first stream end the 32-bit offsets refuse
WIDE = 1 << 32                                  # the first stride the 32-bit indices refuse
BATCH_FAR = f"batch of {FAR} stream bytes: 32-bit offsets only"
FEEDS_FAR = f"feeds of {FAR} bytes: 32-bit offsets only"
FRAMES_WIDE = f"frames of {WIDE} samples: 32-bit indices only"
_sz = C.c_size_t


@pytest.fixture(scope="module")
def rig(tmp_path_factory):
    from icer_compression_amd import decoder
    lib_path = str(tmp_path_factory.mktemp("mock_refusals") / "libdecoder_mock_refusals.so")
    subprocess.check_call(["g++"] + MOCK_FLAGS + ["-O2", "-fPIC", "-shared", "-o", lib_path, DECODER_HIP])
    lib = decoder.bind(lib_path)
    dec = decoder.Decoder(CH, 3, 0, 2, bits=16, lib=lib)
    ses = decoder.Session(dec, N, STRIDE)
    yield lib, dec, ses
    ses.close()
    dec.close()


class Args:
    """the arguments of one call, every output filled with junk; host: `out` is an array of pointers into the junk"""

    def __init__(self, rows, host):
        self.blob = np.zeros(64, np.uint8)
        self.data = self.blob.ctypes.data
        self.offsets, self.lens = (_sz * N)(0, 0), (_sz * N)(0, 0)
        self.rcs, self.ws, self.hs = (C.c_int * N)(77, 77), (_sz * N)(5, 5), (_sz * N)(6, 6)
        self.windows = (C.c_uint32 * (4 * N))(*[0, 0, 2, 2] * N)
        self.info = (C.c_uint32 * (6 * N))(*[JUNK] * (6 * N))
        self.slots = None
        self.mem = np.full(rows * STRIDE * 2, JUNK, np.uint8)
        self.ptrs = (C.c_void_p * rows)(*[self.mem.ctypes.data + k * STRIDE * 2 for k in range(rows)])
        self.out = self.ptrs if host else self.mem.ctypes.data
        self.n, self.frame_stride, self.full_stride = N, STRIDE, STRIDE
        self.made = self.rcs, self.ws, self.hs, self.info         # (a change may null the attribute: the arrays are checked all the same)

    def untouched(self):
        rcs, ws, hs, info = self.made
        return (bool((self.mem == JUNK).all()) and list(rcs) == [77] * N and list(ws) == [5] * N and list(hs) == [6] * N
                and list(info) == [JUNK] * (6 * N))


def far(a):
    a.offsets[1] = FAR


def needs_data(a):
    a.lens[1] = 1
    a.data = None


def null_entry(a):
    a.ptrs[1] = None


def null(*names):
    def change(a):
        for name in names:
            setattr(a, name, None)
    change.__name__ = "null_" + "_".join(names)
    return change


def put(**values):
    def change(a):
        for name, v in values.items():
            setattr(a, name, v)
    change.__name__ = "_".join(f"{k}_{v}" for k, v in values.items())
    return change


def both(*changes):
    def change(a):
        for c in changes:
            c(a)
    change.__name__ = "_and_".join(c.__name__ for c in changes)
    return change


ALL_NULL = both(put(n=0), null("data", "offsets", "lens", "out", "rcs", "ws", "hs", "windows", "info", "slots"))
ALL_NULL.__name__ = "n_0_every_pointer_null"

# (change, return code, last error) -- what every driver refuses in the same way
COMMON = [(null("handle"), INVALID, None), (put(n=-1), INVALID, None), (ALL_NULL, OK, None)] + \
         [(null(name), INVALID, None) for name in ("offsets", "lens", "rcs", "ws", "hs", "out")] + \
         [(needs_data, INVALID, None),
          # two at once: the null data is seen in the loop that adds the lengths up, a null output before either
          (both(needs_data, far), INVALID, None), (both(null("out"), far), INVALID, None)]
PLAIN = COMMON + [(far, FATAL, BATCH_FAR), (put(frame_stride=WIDE), FATAL, FRAMES_WIDE),
                  (both(far, put(frame_stride=WIDE)), FATAL, BATCH_FAR), (both(null("handle"), put(frame_stride=WIDE)), INVALID, None)]
WINDOW = COMMON + [(null("windows"), INVALID, None), (null("info"), INVALID, None), (far, FATAL, BATCH_FAR),
                   (put(frame_stride=WIDE), FATAL, FRAMES_WIDE), (put(full_stride=WIDE), FATAL, FRAMES_WIDE),
                   (put(frame_stride=WIDE, full_stride=WIDE + 8), FATAL, f"frames of {WIDE + 8} samples: 32-bit indices only"),
                   (both(far, put(full_stride=WIDE)), FATAL, BATCH_FAR), (both(null("info"), put(full_stride=WIDE)), INVALID, None)]
SESSION = COMMON + [(put(slots=[0, 0]), INVALID, None), (put(slots=[0, 2]), INVALID, None), (put(slots=[-1, 1]), INVALID, None),
                    (put(n=3), INVALID, None), (far, FATAL, FEEDS_FAR),
                    # two at once: too many feeds and a bad slot answer before the offsets are looked at
                    (both(put(n=3), far), INVALID, None), (both(put(slots=[1, 1]), far), INVALID, None),
                    (both(put(slots=[1, 0]), far), FATAL, FEEDS_FAR)]
# a host call with a null pointer among its outputs (icerx_decode_host and the session's host feed do not look)
NULL_ENTRY = [(null_entry, INVALID, None), (both(null_entry, far), INVALID, None), (both(null_entry, put(frame_stride=WIDE)), INVALID, None)]

# entry point -> (family, host flavour, rows of its output, table)
ENTRIES = {
    "icerx_decode_host": ("plain", True, N * CH, PLAIN),
    "icerx_decode_device": ("plain", False, N * CH, PLAIN),
    "icerx_decode_host_display": ("plain", True, N, PLAIN + NULL_ENTRY),
    "icerx_decode_device_display": ("plain", False, N, PLAIN),
    "icerx_decode_host_window": ("window", True, N * CH, WINDOW + NULL_ENTRY),
    "icerx_decode_device_window": ("window", False, N * CH, WINDOW),
    "icerx_decode_device_window_display": ("window", False, N, WINDOW),
    "icerx_session_feed_host": ("session", True, N * CH, SESSION),
    "icerx_session_feed_device": ("session", False, N * CH, SESSION),
    "icerx_session_feed_device_display": ("session", False, N, SESSION),
}
CASES = [pytest.param(name, change, rc, text, id=f"{name}-{change.__name__}")
         for name, (_, _, _, table) in ENTRIES.items() for change, rc, text in table]


@pytest.mark.parametrize("name,change,want_rc,want_text", CASES)
def test_refused_and_degenerate_calls(rig, name, change, want_rc, want_text):
    from icer_compression_amd._abi import c_array
    lib, dec, ses = rig
    family, host, rows, _ = ENTRIES[name]
    a = Args(rows, host)
    a.handle = ses.handle if family == "session" else dec.handle
    change(a)
    fn = getattr(lib, name)
    if family == "plain":
        rc = fn(a.handle, a.n, a.data, a.offsets, a.lens, a.out, a.frame_stride, a.rcs, a.ws, a.hs)
    elif family == "window":
        rc = fn(a.handle, a.n, a.data, a.offsets, a.lens, a.windows, a.out, a.frame_stride, a.full_stride, a.rcs, a.ws, a.hs, a.info)
    else:
        rc = fn(a.handle, a.n, c_array(C.c_int, a.slots), a.data, a.offsets, a.lens, a.out, a.rcs, a.ws, a.hs)
    assert rc == want_rc
    if want_text is not None:
        assert lib.icerx_decoder_last_error().decode() == want_text
    assert a.untouched()
    if family == "session":
        assert ses.stats() == [0, 0, 0, 0] and ses.planes_held(0, 0, 1, 1, 0) == 0


def test_one_shot_calls_refuse_before_they_make_a_decoder(rig):
    """the three one-shot entry points: their own argument checks, nothing written"""
    lib = rig[0]
    planes = [np.full(STRIDE, JUNK * 0x0101, np.uint16) for _ in range(CH)]
    ptrs = (C.c_void_p * CH)(*[p.ctypes.data for p in planes])
    image = np.full(CH * STRIDE, JUNK, np.uint8)
    blob = np.zeros(8, np.uint8)
    w, h = _sz(5), _sz(6)
    win, info = (C.c_uint32 * 4)(0, 0, 2, 2), (C.c_uint32 * 6)(*[JUNK] * 6)

    def recon(planes_=ptrs, ch=CH, w_=C.byref(w), data=blob, length=8, stages=3, eighths=0):
        return lib.icerx_decompress_reconstructed(planes_, ch, w_, C.byref(h), STRIDE, data, length, stages, 0, 2, 16, 0, eighths)

    def window(planes_=ptrs, ch=CH, w_=C.byref(w), data=blob, length=8, stages=3, eighths=0, win_=win, info_=info):
        return lib.icerx_decompress_window(planes_, ch, w_, C.byref(h), STRIDE, data, length, stages, 0, 2, 16, 0, eighths, win_, info_)

    def display(image_=image.ctypes.data, ch=CH, w_=C.byref(w), data=blob, length=8, stages=3):
        return lib.icerx_decompress_display(image_, w_, C.byref(h), STRIDE, data, length, stages, 0, 2, ch)
    holed = (C.c_void_p * CH)(planes[0].ctypes.data, None, planes[2].ctypes.data)
    for call in (recon, window):
        for kw in (dict(planes_=None), dict(ch=2), dict(w_=None), dict(eighths=5), dict(eighths=-1), dict(planes_=holed),
                   dict(planes_=holed, stages=0)):
            assert call(**kw) == INVALID, (call.__name__, kw)
        assert call(stages=0) == -4 and call(stages=7) == -4, call.__name__           # ICER_TOO_MANY_STAGES, from the decoder's creation
    assert window(win_=None) == INVALID and window(info_=None) == INVALID and window(info_=None, stages=0) == INVALID
    for kw in (dict(image_=None), dict(ch=2), dict(w_=None), dict(image_=None, stages=0)):
        assert display(**kw) == INVALID, kw
    assert display(stages=0) == -4
    assert all((p == JUNK * 0x0101).all() for p in planes) and (image == JUNK).all() and list(info) == [JUNK] * 6
    assert (w.value, h.value) == (5, 6)
