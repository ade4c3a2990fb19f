"""icerx_combine_device_async end to end on the CPU (the mock build of tests/test_recut_mock.py), through
decoder.Recutter.combine_device_async_ptrs, against tests/combine_model.py: the union and the difference of the oracle's nested
cuts and of ROI cuts with different rectangles; operands addressed by odd offsets and by base + stride; an operand that is a
concatenation; empty, alien and out-of-blob operands; a row one byte short; the buffer promises; the refusals.  CPU only."""
import numpy as np
import pytest

from tests import combine_model as cm
from tests import encoder_batch_cases as ebc
from tests import reduced_model as red
from tests import roi_cases as rc
from tests import test_recut_mock as trm
from tests.test_combine_model import CLASSES, model_of, moved_viewport, nested_frames
from tests.test_recut_mock import GEOMETRIES, expected, mock_lib        # noqa: F401  (fixtures: the oracle's streams, the mock build)

SENT, SENT_SIZE, SENT_RC, SENT_U32 = trm.SENT, trm.SENT_SIZE, trm.SENT_RC, 0x5A5A5A5A
INVALID_INPUT, FATAL = trm.INVALID_INPUT, trm.FATAL
GUARD = trm.GUARD


def combine_call(r, op, blob, n, lens_a, lens_b, offsets_a=None, offsets_b=None, base_a=0, base_b=0, stream_stride=0, stride=None,
                 ws_bytes=None, **override):
    """icerx_combine_device_async on host arrays (the mock's device memory) into n + 1 sentinel rows of an odd stride, n + 1
    entries and 2 n + 2 counts, and a workspace of exactly combine_workspace_bytes with a guard tail
    -> (rc of the call, res[f] = (rc, stream, packets written, of them from A, size)) after checking the buffer promises; the
    stream of a frame with ICER_OUTPUT_BUF_TOO_SMALL is b"" and its row is checked to be untouched"""
    stride = stride if stride is not None else (max(int(a) + int(b) for a, b in zip(lens_a, lens_b)) + 5) | 1
    out = np.full((n + 1, max(stride, 1)), SENT, np.uint8)
    sizes = np.full(n + 1, SENT_SIZE, np.uint64)
    rcs = np.full(n + 1, SENT_RC, np.int32)
    counts = np.full(2 * n + 2, SENT_U32, np.uint32)
    la, lb = np.asarray(lens_a, np.uint64), np.asarray(lens_b, np.uint64)
    oa = np.asarray(offsets_a, np.uint64) if offsets_a is not None else None
    ob = np.asarray(offsets_b, np.uint64) if offsets_b is not None else None
    keep = blob.copy()
    need = r.combine_workspace_bytes(n, len(blob))
    work = np.full(need + GUARD, 0xCD, np.uint8)
    args = dict(n=n, op=op, d_data=blob.ctypes.data, data_bytes=len(blob), d_offsets_a=oa.ctypes.data if oa is not None else None,
                base_a=base_a, d_lens_a=la.ctypes.data, d_offsets_b=ob.ctypes.data if ob is not None else None, base_b=base_b,
                d_lens_b=lb.ctypes.data, stream_stride=stream_stride, d_out=out.ctypes.data, out_stride=stride, d_sizes=sizes.ctypes.data,
                d_rcs=rcs.ctypes.data, d_counts=counts.ctypes.data, d_workspace=work.ctypes.data,
                workspace_bytes=need if ws_bytes is None else ws_bytes, stream=None)
    if "n_arg" in override:                                             # (the frame count as passed, whatever the rows are sized for)
        override["n"] = override.pop("n_arg")
    args.update(override)
    rc = r.combine_device_async_ptrs(**args)
    assert (work[need:] == 0xCD).all(), "written behind the workspace"
    assert np.array_equal(blob, keep), "the blob was modified"
    if rc != 0:
        assert (out == SENT).all() and (sizes == SENT_SIZE).all() and (rcs == SENT_RC).all() and (counts == SENT_U32).all(), "a refused call wrote"
        assert (work == 0xCD).all(), "a refused call wrote to the workspace"
        return rc, None
    assert (out[n] == SENT).all() and sizes[n] == SENT_SIZE and rcs[n] == SENT_RC, "written past the n rows"
    assert (counts[2 * n:] == SENT_U32).all(), "counts written past 2 n"
    res = []
    for f in range(n):
        code, s = int(rcs[f]), int(sizes[f])
        if code == cm.TOO_SMALL:
            assert s > stride and (out[f] == SENT).all(), f"frame {f}: a row that is too small was written"
            res.append((code, b"", int(counts[2 * f]), int(counts[2 * f + 1]), s))
            continue
        assert 0 <= s <= stride, (f, s, stride)
        assert (out[f, s:] == SENT).all(), f"frame {f}: bytes written behind its stream of {s} bytes"
        res.append((code, out[f, :s].tobytes(), int(counts[2 * f]), int(counts[2 * f + 1]), s))
    return rc, res


def pack_two(rng, A, B):
    """both operands in one blob at odd offsets: (blob, offsets of A, offsets of B), the frames of B first and interleaved"""
    order = [(1, k) for k in range(len(B))] + [(0, k) for k in range(len(A))]
    rng.shuffle(order)
    blob, offsets = trm.pack_odd(rng, [(A, B)[x][k] for x, k in order])
    oa, ob = [0] * len(A), [0] * len(B)
    for (x, k), o in zip(order, offsets):
        (oa, ob)[x][k] = o
    return blob, oa, ob


def pack_block(A, B):
    """the layout of a two-cut re-cut call: n rows of A, then n rows of B, of one odd stride -> (blob, stride, base_b)"""
    n = len(A)
    stride = (max(len(s) for s in A + B) + 6) | 1
    blob = np.full(2 * n * stride, 0x5B, np.uint8)
    for k, s in enumerate(A + B):
        blob[k * stride: k * stride + len(s)] = np.frombuffer(s, np.uint8)
    return blob, stride, n * stride


def both_layouts(r, rng, op, A, B, **kw):
    """the call on both layouts -> [(what, rc, res)]"""
    n, la, lb = len(A), [len(s) for s in A], [len(s) for s in B]
    blob, oa, ob = pack_two(rng, A, B)
    rows, stride, base_b = pack_block(A, B)
    return [("odd offsets",) + combine_call(r, op, blob, n, la, lb, offsets_a=oa, offsets_b=ob, **kw),
            ("base + stride",) + combine_call(r, op, rows, n, la, lb, base_b=base_b, stream_stride=stride, **kw)]


def check(m, got, A, B, op, what, stride=None):
    for f, (a, b) in enumerate(zip(A, B)):
        want = cm.combine(m, a, b, op, out_stride=stride if stride is not None else len(a) + len(b) + 5)
        assert got[f][0] == want[0] and got[f][2:] == want[2:], (what, f, got[f][0], got[f][2:], want[0], want[2:])
        assert got[f][1] == want[1], f"{what} frame {f}: first difference at byte {ebc.first_difference(got[f][1], want[1])}"


# ------------------------------------------------------------------------------------------------ nested cuts
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_nested_cuts(mock_lib, expected, name):
    g, specs = GEOMETRIES[name]
    m = model_of(g)
    rng = np.random.default_rng(sum(map(ord, name)))
    frames = nested_frames(expected, g, specs)
    r = trm.recutter(mock_lib, g)
    for i in range(len(CLASSES)):
        for j in range(i + 1, len(CLASSES)):
            H, W = [s[i] for _, s in frames], [s[j] for _, s in frames]
            incs = []
            for what, code, got in both_layouts(r, rng, cm.DIFFERENCE, H, W):
                assert code == 0
                check(m, got, H, W, cm.DIFFERENCE, f"{name} {CLASSES[i]} < {CLASSES[j]} difference, {what}")
                assert all(0 < x[4] == len(w) - len(h) and x[3] == 0 for x, h, w in zip(got, H, W))
                incs = [x[1] for x in got]
            for what, code, got in both_layouts(r, rng, cm.UNION, H, incs):
                assert code == 0
                check(m, got, H, incs, cm.UNION, f"{name} {CLASSES[i]} < {CLASSES[j]} union, {what}")
                assert [x[1] for x in got] == W, what
            # an operand that is a concatenation: the held stream with the increment behind it holds everything already
            cat = [h + x for h, x in zip(H, incs)]
            for what, code, got in both_layouts(r, rng, cm.DIFFERENCE, cat, W):
                assert code == 0 and [x[:4] for x in got] == [(0, b"", 0, 0)] * len(W), what
            for what, code, got in both_layouts(r, rng, cm.UNION, H, cat):
                assert code == 0 and [x[1] for x in got] == W and all(x[3] == 0 for x in got), what
    # the same stream twice, and a zero-length A
    X = [s[1] for _, s in frames]
    for what, code, got in both_layouts(r, rng, cm.UNION, X, X):
        assert code == 0 and [x[1] for x in got] == X and all(x[3] == 0 for x in got), what
    for what, code, got in both_layouts(r, rng, cm.DIFFERENCE, X, X):
        assert code == 0 and [x[:4] for x in got] == [(0, b"", 0, 0)] * len(X), what
    for op in (cm.UNION, cm.DIFFERENCE):
        for what, code, got in both_layouts(r, rng, op, [b""] * len(X), X):
            assert code == 0 and [x[:2] for x in got] == [(0, x) for x in X], (what, op)
    r.close()


# ------------------------------------------------------------------------------------------------ moved viewport
@pytest.mark.parametrize("name", ["G1", "G2", "G3", "G4"])
def test_moved_viewport(mock_lib, expected, name):
    g = rc.GEOMETRIES[name]
    m, H, W = moved_viewport(expected, name)
    rng = np.random.default_rng(sum(map(ord, name)))
    r = trm.recutter(mock_lib, g)
    A, B = [H, W], [W, H]                                        # (both directions in one call)
    for op in (cm.DIFFERENCE, cm.UNION):
        for what, code, got in both_layouts(r, rng, op, A, B):
            assert code == 0
            check(m, got, A, B, op, f"{name} op {op}, {what}")
            if op == cm.DIFFERENCE:
                assert got[0][2] > 0 and got[1][2] > 0
                if name == "G4":
                    assert (got[0][2], got[1][2]) == (102, 105)
            else:
                assert 0 < got[0][3] < got[0][2] and cm.units(m, got[0][1]) == cm.units(m, got[1][1])
    r.close()


# ------------------------------------------------------------------------------------------------ damage
def test_a_damaged_copy_gets_its_packet_again(mock_lib, expected):
    g, specs = GEOMETRIES["yuv16"]
    m = model_of(g)
    rng = np.random.default_rng(9)
    spec, (_, H, W) = nested_frames(expected, g, specs)[0]
    hurt = red.flip_in_packet(H, max(red.levels_of(H)), False, which=1)
    header = red.flip_in_packet(H, 1, True, which=0)
    A, B = [H, hurt, header], [W, W, W]
    r = trm.recutter(mock_lib, g)
    for what, code, got in both_layouts(r, rng, cm.DIFFERENCE, A, B):
        assert code == 0
        check(m, got, A, B, cm.DIFFERENCE, what)
        assert got[1][2] == got[0][2] + 1 == got[2][2], what
    r.close()


# ------------------------------------------------------------------------------------------------ statuses, a short row, refusals
def test_bad_frames_a_short_row_and_refused_calls(mock_lib, expected):
    g, specs = GEOMETRIES["gray16"]
    m = model_of(g)
    other = ebc.Geometry(256, 192, 1, 2, 3, 2)
    rng = np.random.default_rng(5)
    (_, (P, H, W)), = nested_frames(expected, g, specs)[:1]
    alien = expected(other, ("smooth", 0), ebc.quota(other, "cut"))[1]
    junk = rng.integers(0, 256, 3000).astype(np.uint8).tobytes()
    A = [H, alien, H, b"", junk, P, H]
    B = [W, W, alien, b"", b"", H, W]
    blob, oa, ob = pack_two(rng, A, B)
    la, lb = [len(s) for s in A], [len(s) for s in B]
    # two more frames: A leaves the blob, B leaves the blob
    oa, la = oa + [len(blob) - 10, oa[0]], la + [11, la[0]]
    ob, lb = ob + [ob[0], len(blob) + 1], lb + [lb[0], 0]
    n = len(la)
    r = trm.recutter(mock_lib, g)
    bad = lambda code: (code, b"", 0, 0, 0)
    for op in (cm.UNION, cm.DIFFERENCE):
        code, got = combine_call(r, op, blob, n, la, lb, offsets_a=oa, offsets_b=ob)
        assert code == 0
        check(m, got[:7], A, B, op, f"op {op}")
        assert [got[f] for f in (1, 2, 3, 4, 7, 8)] == [bad(cm.INVALID_INPUT), bad(cm.INVALID_INPUT), bad(cm.OUT_OF_DATA), bad(cm.OUT_OF_DATA),
                                                         bad(cm.INVALID_INPUT), bad(cm.INVALID_INPUT)], op
        assert got[0][0] == 0 == got[5][0] == got[6][0] and got[0][1] == got[6][1]
        # a row one byte short of frame 5's result: that frame alone is refused, with the bytes it needs
        short = got[5][4] - 1
        code, again = combine_call(r, op, blob, n, la, lb, offsets_a=oa, offsets_b=ob, stride=short)
        assert code == 0
        for f in range(n):
            if got[f][4] > short:
                assert again[f] == (cm.TOO_SMALL, b"") + got[f][2:], (op, f)
            else:
                assert again[f] == got[f], (op, f)
        assert again[5][0] == cm.TOO_SMALL
        check(m, again[:7], A, B, op, f"op {op}, short rows", stride=short)
    # refused calls write nothing (combine_call checks that)
    need = r.combine_workspace_bytes(n, len(blob))
    cases = {
        "op 2": dict(op=2), "op -1": dict(op=-1), "no frames": dict(n=0), "negative frames": dict(n=-1), "too many frames": dict(n=65536),
        "null data": dict(d_data=None), "null lens a": dict(d_lens_a=None), "null lens b": dict(d_lens_b=None), "null out": dict(d_out=None),
        "null sizes": dict(d_sizes=None), "null rcs": dict(d_rcs=None), "null counts": dict(d_counts=None),
        "null workspace": dict(d_workspace=None), "workspace one byte short": dict(ws_bytes=need - 1),
    }
    for what, kw in cases.items():
        op = kw.pop("op", cm.UNION)
        if "n" in kw:
            kw["n_arg"] = kw.pop("n")
        assert combine_call(r, op, blob, n, la, lb, offsets_a=oa, offsets_b=ob, **kw)[0] == INVALID_INPUT, what
    assert combine_call(r, cm.UNION, blob, n, la, lb, offsets_a=oa, offsets_b=ob, data_bytes=0xFFFFFFFF - 64)[0] == FATAL
    assert r.lib.icerx_combine_device_async(None, n, 0, blob.ctypes.data, len(blob), None, 0, None, None, 0, None, 0, None, 0, None, None, None,
                                            None, 0, None) == INVALID_INPUT
    assert r.combine_workspace_bytes(0, len(blob)) == 0 == r.combine_workspace_bytes(65536, len(blob))
    # the existing calls of the same recutter are what they were
    assert trm.recut_call(r, blob, oa[:1], la[:1], [60])[0] == 0
    r.close()
