"""The definition of icerx_combine_device_async (include/icer_hip_dec.h, "Refinement increments") in plain Python: the union
and the difference of two stored streams of one frame.  An operand is walked as a decoder walks it (reduced_model.walk: every
CRC-valid packet, an accepted packet stepped over whole); a packet stands for the unit of the plan that its header names
(Model.unit_index), the last one of a unit wins, and one that names no unit of the plan is dropped.  Per unit u:
    UNION        kept when A or B has a packet of u; B's if B has one, else A's
    DIFFERENCE   kept when B has a packet of u and A has none; B's
The kept packets follow one another verbatim in the plan's final order (roi_model.final_order)."""
from tests import reduced_model as red
from tests import roi_model as rm

UNION, DIFFERENCE = 0, 1
OK, TOO_SMALL, OUT_OF_DATA, INVALID_INPUT = 0, -2, -7, -11


def table(m, stream):
    """({unit index: packet bytes}, any valid packet, a valid packet of another image size) of one operand"""
    stream = bytes(stream)
    index, packets, other = m.unit_index(), {}, False
    for off, n in red.walk(stream):
        hdr = stream[off: off + red.HEADER]
        other |= (int.from_bytes(hdr[8:12], "little"), int.from_bytes(hdr[12:16], "little")) != (m.w, m.h)
        key = (hdr[7] >> 4 if m.channels == 3 else 0, hdr[4], hdr[5], hdr[7] & 15, hdr[6])
        if key in index:
            packets[index[key]] = stream[off: off + n]
    return packets, any(True for _ in red.walk(stream)), other


def combine(m, a, b, op, out_stride=None, inside=True):
    """-> (rc, stream, packets written, of them from A[, bytes needed]); `inside` False: an operand leaves the blob.  With an
    out_stride the result is (rc, stream, packets, from A, size): a result longer than out_stride has TOO_SMALL, no stream and
    the bytes needed for size"""
    (pa, any_a, other_a), (pb, any_b, other_b) = table(m, a), table(m, b)
    bad = INVALID_INPUT if not inside or other_a or other_b else \
        OUT_OF_DATA if not (any_b or (op == UNION and any_a)) else OK
    if bad != OK:
        return (bad, b"", 0, 0) + ((0,) if out_stride is not None else ())
    kept = [(pb[u], 0) if u in pb and (op == UNION or u not in pa) else (pa[u], 1) if op == UNION and u in pa else None
            for u in rm.final_order(m)]
    kept = [x for x in kept if x is not None]
    stream, from_a = b"".join(p for p, _ in kept), sum(f for _, f in kept)
    if out_stride is None:
        return OK, stream, len(kept), from_a
    if len(stream) > out_stride:
        return TOO_SMALL, b"", len(kept), from_a, len(stream)
    return OK, stream, len(kept), from_a, len(stream)


def units(m, stream):
    """the set of the plan's units that `stream` holds a valid packet of"""
    return set(table(m, stream)[0])
