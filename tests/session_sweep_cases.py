"""The geometry sweep of the decode sessions: the cases, scenarios and conditions shared by tests/test_session_sweep_mock.py (the
host pipeline and the serial forms of the chain bodies, on the mock HIP runtime) and tests/test_gpu_session_sweep.py (the three
resumable chain decoders on the GPU).  Nothing here runs on a device: a scenario drives a `rig` as those of
tests/session_cases.py do, plus rig.plain(case, stream, **options) -> (rc, w, h, planes), the plain decode of one stream by a
second decoder of the rig's library with the same options, and rig.kind, the library's name.

Cases: every geometry of tests/geometry_sweep_cases.py with one frame spec -- the first of its three, dense one first, whose
lossless master the oracle codes with rc 0 and whose master and cuts at L/6, L/3 and 2L/3 do not read on behind their packets
(sweep_cut_cases.reads_on: such a stream decodes to what follows each packet, which a feed and the model's stream do not share,
so there is nothing to compare), else a smooth frame -- and two wide frames whose level-1 chains are 2560 samples wide: too wide
for the lane-per-plane kernel's row ring, so that one call mixes chains whose ring fits with chains whose ring does not.

Scenarios, each under ICER_DEC_WAVE unset, 0, 1 and 2 (MODES):
  A  run_ladder     the cut at L/6 and the DIFFERENCE increments to L/3, 2L/3 and the master, then an empty feed;
  B  run_staggered  the master split into one feed per bit plane, fed to three slots one call apart in permuted slot order:
                    one launch mixes chains that hold nothing, k planes and k + 1 planes, and every chain is resumed with a
                    single new plane at every depth;
  C  run_ladder with one of four decoder option sets (OPTION_SETS), unset and 1 only, no P1 geometry; with a reconstruction
     setting every step is compared with the plain decode of the model's stream by the same library (the header's definition),
     not with tests/recon_model.py, whose domain is an open question;
  D  run_wide       the wide frames in five feeds: planes 8 .. 6, 5, 4 .. 2, 1, 0;
  E  run_wide over levels_apart: the three-stage wide frame in three feeds that end level 1 and the deeper levels on different
                    planes, so that the status words of the lane-per-plane and the thread-per-chain route differ in one call.
Every step is compared with tests/session_model.py sample for sample, and the session's counts with the conditions of
check_counts / check_wide_counts: they were fixed with the oracle and the mock (256 compute units, as the MI355X) and are
conditions, not measurements -- a sample that misses one gets another seed."""
import numpy as np

from tests import combine_model as cm
from tests import encoder_batch_cases as ebc
from tests import geometry_sweep_cases as gsc
from tests import reduced_model as red
from tests import session_cases as sc
from tests import session_model as sm
from tests.session_cases import check_step
from tests.sweep_cut_cases import reads_on

MODES = (None, "0", "1", "2")                   # ICER_DEC_WAVE: by load, threads only, lanes only, pinned to the wave-per-plane kernel
WIDE = ((ebc.Geometry(5120, 10, 1, 1, 0, 1), ("smooth", 4)),       # four chains of 2560 x 5: no ring fits
        # level 1 as above; levels 2 and 3 fit, in two ring classes (17 rows: the least height the codec takes with three stages)
        (ebc.Geometry(5120, 17, 1, 3, 0, 1), ("smooth", 4)))
WIDE_FEEDS = ((8, 7, 6), (5,), (4, 3, 2), (1,), (0,))
MIN_THREADS_BESIDE_PLANES = 10                  # scenario B, unset: geometries with chains on the thread route beside the planes kernel
_CASES, _DECODES = {}, {"case": None, "memo": {}}


class Case:
    """name, geometry, spec; the master, its three cuts and the ladder's four feeds"""

    def __init__(self, expected, g, spec, own):
        self.name, self.g, self.spec, self.own, self.p1 = gsc.case_id(g), g, spec, own, gsc.is_p1(g)
        self.planes = 9 if g.bits == 16 else 7
        self.master = expected(g, spec, ebc.quota(g, "lossless"))[1]
        L = len(self.master)
        self.cuts = [expected(g, spec, q)[1] for q in (L // 6, L // 3, (2 * L) // 3)] + [self.master]
        m = sc.model_of(g)
        u = [cm.units(m, c) for c in self.cuts]
        assert u[0] <= u[1] <= u[2] <= u[3] and len(u[3]) == gsc.n_units(g), (self.name, [len(x) for x in u])
        self.incs = [self.cuts[0]] + [increment(m, self.cuts[i], self.cuts[i + 1]) for i in range(3)]
        assert [len(x) for x in self.incs[1:]] == [len(self.cuts[i + 1]) - len(self.cuts[i]) for i in range(3)], self.name


def increment(m, held, wanted):
    """the DIFFERENCE increment from one cut to the next (of a cut without a packet: nothing)"""
    rc, inc = cm.combine(m, held, wanted, cm.DIFFERENCE)[:2]
    assert rc == cm.OK or (rc == cm.OUT_OF_DATA and not list(red.walk(wanted))), rc
    return inc


def contained(expected, g, spec):
    """the lossless master has rc 0, and neither it nor a cut of the ladder reads on behind its packets"""
    rc, master = expected(g, spec, ebc.quota(g, "lossless"))[:2]
    L = len(master)
    return rc == 0 and not any(reads_on(expected.orc, g, s, 0) for s in [master] + [expected(g, spec, q)[1] for q in (L // 6, L // 3, (2 * L) // 3)])


def case_of(expected, g, specs):
    if g not in _CASES:
        own = next((s for s in specs if contained(expected, g, s)), None)
        spec = own or (("smooth6", 0) if g.bits == 8 else ("smooth", 0))
        assert own or contained(expected, g, spec), (gsc.case_id(g), "no spec without a chain that reads on")
        _CASES[g] = Case(expected, g, spec, own is not None)
    return _CASES[g]


def sample_cases(expected):
    """a case per geometry of the sample: none may be left out"""
    cases = [case_of(expected, g, specs) for g, specs in gsc.cases()]
    assert len(cases) == len(gsc.cases())
    return cases


def wide_case(expected, i):
    g, spec = WIDE[i]
    return case_of(expected, g, [spec])


def option_sets(g):
    return [dict(reduce=min(1, g.stages - 1)), dict(reconstruct=3), dict(display=True), dict(reduce=g.stages - 1, reconstruct=3)]


def chains_of(g):
    """(channel, level, subband, segment) of every chain of the geometry"""
    return [(ch, lv, sb, sg) for ch in range(g.channels) for lv in range(1, g.stages + 1) for sb in range(0 if lv == g.stages else 1, 4)
            for sg in range(g.segments)]


def by_plane(stream, lsbs):
    """the packets of `stream` whose lsb is one of `lsbs`, in stream order"""
    return b"".join(stream[o: o + n] for o, n in red.walk(stream) if (stream[o + 7] & 15) in lsbs)


# ------------------------------------------------------------------------------------------------ the model of a run
class Model(sm.SessionModel):
    """SessionModel whose decodes are made once per case -- the routing modes feed the same streams -- and, with a reconstruction
    setting, by the plain decode of the rig's library"""

    def __init__(self, rig, case, n_slots=1, reduce=0, reconstruct=0):
        g = case.g
        rw, rh = red.reduced_size(g.w, g.h, reduce)
        super().__init__(rig.orc, g.channels, g.stages, g.filt, g.segments, rw * rh, g.bits, reduce, reconstruct, n_slots)
        self.rig, self.case = rig, case
        if _DECODES["case"] != case.name:
            _DECODES["case"], _DECODES["memo"] = case.name, {}

    def decode(self, slot, w0=0, h0=0):
        key = (self.rig.kind if self.k else "", self.r, self.k, w0, h0, self.stream_of(slot))
        memo = _DECODES["memo"]
        if key not in memo:
            if self.k:
                memo[key] = self.rig.plain(self.case, key[5], reduce=self.r, reconstruct=self.k)
            else:
                memo[key] = super().decode(slot, w0, h0)
        return memo[key]


def same_image(a, b):
    return a[:3] == b[:3] and all(np.array_equal(x[: a[1] * a[2]], y[: a[1] * a[2]]) for x, y in zip(a[3], b[3]))


def oracle_image(rig, case, stream):
    from tests.decoder_batch_cases import oracle_decode
    g = case.g
    key = ("oracle", stream)
    if _DECODES["case"] != case.name:
        _DECODES["case"], _DECODES["memo"] = case.name, {}
    if key not in _DECODES["memo"]:
        _DECODES["memo"][key] = oracle_decode(rig.orc, stream, g.channels, g.stages, g.filt, g.segments, g.w * g.h, g.bits)
    return _DECODES["memo"][key]


def open_session(rig, case, n_slots=1, **options):
    ses, _ = rig.open(case.name, n_slots=n_slots, **options)
    return ses, Model(rig, case, n_slots, options.get("reduce", 0), options.get("reconstruct", 0))


def check_held(case, ses, mod, n_slots, tag):
    for slot in range(n_slots):
        for chain in chains_of(case.g):
            if chain[1] > mod.r:
                assert ses.planes_held(slot, *chain) == mod.planes_held(slot, *chain), (tag, slot, chain)


# ------------------------------------------------------------------------------------------------ conditions on the counts
def check_counts(case, mode, ses, mod, tag, routes=True):
    """[chains resumed in the wave-per-plane kernel, chains on the thread route, planes decoded, packets dropped] of a scenario
    on the sample.  routes=False (a decoder option that leaves few small chains): the two mode conditions that need a fast
    chain to be resumed are not owed"""
    resumed, threads, decoded, dropped = ses.stats()
    assert dropped == 0 and [decoded, dropped] == [mod.decoded, mod.dropped], (tag, ses.stats(), mod.decoded, mod.dropped)
    if mode == "0":
        assert resumed == 0 and threads > 0, (tag, ses.stats())
    elif mode == "1":
        assert [resumed, threads] == [0, 0], (tag, ses.stats())           # (every ring of the sample fits)
    elif mode == "2":
        assert (resumed > 0 or not routes) and threads == 0, (tag, ses.stats())
    else:
        assert resumed > 0 or not routes, (tag, ses.stats())


def check_wide_counts(case, mode, ses, mod, tag):
    resumed, threads, decoded, dropped = ses.stats()
    assert [decoded, dropped] == [mod.decoded, mod.dropped] and dropped == 0, (tag, ses.stats(), mod.decoded, mod.dropped)
    if mode == "0":
        assert resumed == 0 and threads == mod.runs, (tag, ses.stats(), mod.runs)
    elif mode == "1":
        # no ring of a level-1 chain fits: those chains take the thread route; the deeper levels' rings fit and take the lanes
        assert resumed == 0 and threads > 0, (tag, ses.stats())
        if case.g.stages > 1:
            assert threads < mod.runs, (tag, ses.stats(), mod.runs)
    else:
        # (the level-1 chains ask for about 72 KB of dynamic LDS in the wave-per-plane kernel; a runtime may refuse that, and
        # the chains then take the thread route)
        assert resumed + threads > 0, (tag, ses.stats())


# ------------------------------------------------------------------------------------------------ scenarios
def run_ladder(rig, case, mode, **options):
    """A (and C, with options): the ladder's four feeds and an empty one -> (session, model)"""
    g, display = case.g, options.get("display", False)
    plain = not options.get("reduce") and not options.get("reconstruct")
    ses, mod = open_session(rig, case, **options)
    for i, inc in enumerate(case.incs + [b""]):
        tag = (case.name, mode, options, "step", i)
        got = rig.feed(ses, [inc], display=display)
        want = mod.feed(0, inc)
        if plain:                                           # (the model itself: T is the cut, packet for packet)
            assert same_image(oracle_image(rig, case, case.cuts[min(i, 3)]), want), tag
        check_step(g, got, 0, want, tag, display)
    check_held(case, ses, mod, 1, (case.name, mode, options))
    check_counts(case, mode, ses, mod, (case.name, mode, options), routes=not options.get("reduce"))
    return ses, mod


def run_staggered(rig, case, mode):
    """B: plane by plane into three slots, staggered -> (session, model)"""
    g, P = case.g, case.planes
    feeds = [by_plane(case.master, (P - 1 - j,)) for j in range(P)]
    assert sum(len(f) for f in feeds) == len(case.master)
    order = [2, 0, 1]
    ses, mod = open_session(rig, case, n_slots=3)
    for t in range(P + 2):
        mine = [feeds[t - s] if 0 <= t - s < P else b"" for s in range(3)]
        got = rig.feed(ses, mine, slots=order)
        for s, slot in enumerate(order):
            empty_slot = not mod.slots[slot].T and not mine[s]
            want = mod.feed(slot, mine[s])
            assert not empty_slot or want[1] * want[2] == 0            # (check_step: such a row must be untouched)
            check_step(g, got, s, want, (case.name, mode, "call", t, "slot", slot))
            if t == P + 1:
                assert want[0] == (-3 if case.p1 else 0) and same_image(oracle_image(rig, case, case.master), want), (case.name, mode, slot)
        if t in (0, P // 2, P + 1):
            check_held(case, ses, mod, 3, (case.name, mode, "call", t))
    assert all(mod.planes_held(slot, *chain) == P for slot in range(3) for chain in chains_of(g)), case.name
    check_counts(case, mode, ses, mod, (case.name, mode, "staggered"))
    return ses, mod


def run_wide(rig, case, mode, feeds=None):
    """D: a wide frame in five feeds of whole bit planes (or in `feeds`) -> (session, model)"""
    g = case.g
    ses, mod = open_session(rig, case)
    for i, data in enumerate(feeds or [by_plane(case.master, lsbs) for lsbs in WIDE_FEEDS]):
        check_step(g, rig.feed(ses, [data]), 0, mod.feed(0, data), (case.name, mode, "feed", i))
        check_held(case, ses, mod, 1, (case.name, mode, "feed", i))
    assert same_image(oracle_image(rig, case, case.master), mod.feed(0, b"")) and mod.decoded == gsc.n_units(g)
    check_held(case, ses, mod, 1, (case.name, mode))
    check_wide_counts(case, mode, ses, mod, (case.name, mode, "wide"))
    return ses, mod


def levels_apart(case):
    """E: three feeds of a wide frame of several stages in which level 1 (the thread route under ICER_DEC_WAVE=1) and the deeper
    levels (the lanes) end on different planes -- level 1 above the others in the first feed, below them in the second -- so that
    a status word read for a chain of the other route says that the chain stopped"""
    s, P = case.master, case.planes
    pick = lambda fine, deep: b"".join(s[o: o + n] for o, n in red.walk(s) if (s[o + 7] & 15) in (fine if s[o + 4] == 1 else deep))
    return [pick(range(5, P), range(3, P)), pick(range(0, 5), (2,)), pick((), (1, 0))]
