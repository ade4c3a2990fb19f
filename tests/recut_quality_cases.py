"""What tests/test_recut_quality_mock.py and tests/test_gpu_recut_quality.py share: the model's view of a master and its
distortion sidecar (tests/target_model.py), at full size and at 1/2^r size."""
import numpy as np

from tests import reduced_model as red
from tests import target_model as tm


def model_of(g):
    return tm.Model(g.w, g.h, g.channels, g.stages, g.filt, g.segments, g.bits)


def sidecar_row(model, E, means):
    """a sidecar row as the encoder exports it: E[family][b], then one word with the 16-bit LL means (None: none, zero)"""
    word = sum((int(m) & 0xFFFF) << (16 * c) for c, m in enumerate(means or []))
    return np.concatenate([np.asarray(E, np.uint64).ravel(), np.array([word], np.uint64)])


def unit_bits(model, stream):
    """payload bits of the units in priority order from the packets of a stream; a unit without a packet does not fit"""
    where = model.unit_index()
    bits = [tm.TOO_BIG] * model.n_units
    for (ch, lv, sb, lsb, sg, b) in tm.parse_stream(stream):
        bits[where[(ch, lv, sb, lsb, sg)]] = b
    return bits


def reduced_view(master_model, g, r):
    """the model of the geometry at 1/2^r size and, per family of it, the master's family it is: family (ch, lv, sb, sg)
    there is the master's (ch, lv + r, sb, sg)"""
    rw, rh = red.reduced_size(g.w, g.h, r)
    m = tm.Model(rw, rh, g.channels, g.stages - r, g.filt, g.segments, g.bits)
    of_key = {(u[0], u[1], u[2], u[4]): u[5] for u in master_model.units}
    fam_map = {u[5]: of_key[(u[0], u[1] + r, u[2], u[4])] for u in m.units}
    return m, [fam_map[f] for f in range(m.n_families)]


def check_target(got, want, what, flag="flag"):
    """one row of a target call against tm.target_walk's tuple"""
    K, used, rc, reached, dK, equiv, _ = want
    assert (got["rc"], len(got["stream"]), got[flag], got["dist"], got["equiv"]) == (rc, used, reached, dK, equiv), \
        f"{what}: got rc {got['rc']} size {len(got['stream'])} reached {got[flag]} dist {got['dist']} equiv {got['equiv']}, want {want}"


def header_means(stream, channels):
    """the LL mean field (header bytes 2 .. 3) of the last LL packet of every channel"""
    out, at = [0] * channels, 0
    while at + tm.HEADER <= len(stream):
        w = np.frombuffer(stream[at: at + tm.HEADER], np.uint32)
        if (int(w[1]) >> 8) & 0xFF == tm.LL:
            out[(int(w[1]) >> 28) & 0xF] = int(w[0]) >> 16
        at += tm.unit_len(int(w[4]))
    return out
