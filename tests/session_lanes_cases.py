"""What the tests of a decode session's lane-per-plane route share (tests/test_session_lanes_mock.py on the mock HIP runtime,
tests/test_gpu_session_lanes.py on the GPU), on top of tests/session_cases.py: a case whose level-1 chains are taller than the
kernel's row ring, the failing-plane scenario as that route reports it, and the load rule -- enough slots of one small noise
frame in one call that the plain decode's rule (csrc/decoder_route.hpp dwant_planes) leaves the wave-per-plane kernel."""
from tests import combine_model as cm
from tests import encoder_batch_cases as ebc
from tests import reduced_model as red
from tests import session_cases as sc
from tests import session_model as sm
from tests.sweep_cut_cases import reads_on

# one stage, one segment: four chains of 64 x 64 -- the ring of a 16-bit chain has 13 rows, so slots are recycled and reloaded
TALL = ("gray16_tall", (ebc.Geometry(128, 128, 1, 1, 0, 1), ("smooth", 7)))
# 16 chains of 8 x 8 per frame, every packet of which is above 16 bits: every chain may take the wave-per-plane kernel
LOAD = ("gray16_load", (ebc.Geometry(32, 32, 1, 1, 0, 4), ("noise8", 11)))
FAST_BITS = 16                                  # csrc/decoder_core.hpp kFastPacketBits
CHAINS_PER_CU = 12                              # csrc/decoder_route.hpp dwant_planes


def register(monkeypatch, case):
    """the case among those of tests/session_cases.py for the length of a test"""
    monkeypatch.setitem(sc.CASES, case[0], case[1])
    return case[0]


def run_failing_plane(rig, expected, orc, name="gray16_A4"):
    """tests/session_cases.py run_failing_plane for a session whose chains all take the lane-per-plane kernel: that kernel reports
    where the chain stopped, so no chain is counted on the thread route"""
    from tests.decoder_batch_cases import oracle_decode
    g, master, cuts, incs = sc.ladder(expected, name)
    crafted, key = sc.failing_plane(expected, orc, name)
    ses, _ = rig.open(name)
    fed = b""
    for i, data in enumerate((cuts[0], crafted, incs[2])):
        fed += data
        want = oracle_decode(orc, fed, g.channels, g.stages, g.filt, g.segments, g.w * g.h, g.bits)
        sc.check_step(g, rig.feed(ses, [data]), 0, want, (name, "failing plane, step", i))
        if i == 0:
            assert 0 < ses.planes_held(0, *key[:4]) <= (9 if g.bits == 16 else 7) - 1 - key[4], "the failing packet's chain holds nothing above it"
    assert ses.planes_held(0, *key[:4]) == -1, "the chain has not stopped"
    assert ses.stats()[:2] == [0, 0] and ses.stats()[3] > 0, ses.stats()
    return ses


def chains_of(stream):
    """{(level, subband, segment): [bits of each packet]} of a one-channel stream"""
    out = {}
    for off, _ in red.walk(stream):
        out.setdefault(bytes(stream[off + 4: off + 7]), []).append(int.from_bytes(stream[off + 16: off + 20], "little"))
    return out


def load_feeds(expected, orc, name, n_cus):
    """(g, cut, increment to the lossless stream, slots) such that both feeds of `slots` slots bring more than CHAINS_PER_CU fast
    chains per compute unit, counted here from the packets' lengths"""
    g, spec = sc.CASES[name]
    rc, master = expected(g, spec, ebc.quota(g, "lossless"))[:2]
    assert rc == 0
    cut = expected(g, spec, len(master) // 2)[1]
    m = sc.model_of(g)
    assert cm.units(m, cut) < cm.units(m, master) and not reads_on(orc, g, cut, 0) and not reads_on(orc, g, master, 0)
    inc = cm.combine(m, cut, master, cm.DIFFERENCE)[1]
    per_call = []
    for s in (cut, inc):
        chains = chains_of(s)
        assert chains and all(b >= FAST_BITS for v in chains.values() for b in v), "a chain of the load frame has a short packet"
        per_call.append(len(chains))
    slots = CHAINS_PER_CU * n_cus // min(per_call) + 1
    assert slots * min(per_call) > CHAINS_PER_CU * n_cus
    return g, cut, inc, slots


def run_load(rig, expected, orc, name, n_cus):
    """the cut, then its increment, into `slots` slots in one call each -> the session; every row is the model's image"""
    g, cut, inc, slots = load_feeds(expected, orc, name, n_cus)
    ses, _ = rig.open(name, n_slots=slots)
    mod = sm.SessionModel(orc, g.channels, g.stages, g.filt, g.segments, g.w * g.h, g.bits, 0, 0, 1)
    for step, data in enumerate((cut, inc)):
        got = rig.feed(ses, [data] * slots)
        want = mod.feed(0, data)
        assert want[0] == 0 and want[3] is not None
        for k in range(slots):
            sc.check_step(g, got, k, want, (name, "load", step))
    return ses, slots
