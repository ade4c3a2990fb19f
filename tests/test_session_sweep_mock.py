"""The geometry sweep of the decode sessions on the CPU (tests/session_sweep_cases.py): decoder.hip on the mock HIP runtime, built
and driven as tests/test_session_mock.py does it, over every geometry of tests/geometry_sweep_cases.py and two wide frames, in all
four settings of ICER_DEC_WAVE.  What runs here is the host pipeline -- the packet walk, session_accept, the routing, the status
words -- and the serial forms of the three chain bodies; tests/test_gpu_session_sweep.py runs the same scenarios on the device
forms.  The conditions the sample must meet for the sweep to cover what it claims are asserted in a test of their own.
CPU only."""
import pytest

from tests import geometry_sweep_cases as gsc
from tests import session_lanes_cases as slc
from tests import session_sweep_cases as ssc
from tests import test_session_mock as tsm
from tests.test_session_mock import expected, mock_lib                      # noqa: F401  (fixtures)

CASES = gsc.cases()
IDS = [gsc.case_id(g) for g, _ in CASES]
_STAGGERED = {}                                  # case name -> stats() of scenario B with ICER_DEC_WAVE unset


class Rig(tsm.Rig):
    kind = "mock"

    def plain(self, case, stream, reduce=0, reconstruct=0):
        return plain_decode(self.lib, case, stream, reduce, reconstruct)


def plain_decode(lib, case, stream, reduce, reconstruct):
    """(rc, w, h, planes) of the plain decode of one stream by a decoder of its own"""
    from icer_compression_amd import decoder
    from tests import reduced_model as red
    g = case.g
    rw, rh = red.reduced_size(g.w, g.h, reduce)
    dec = decoder.Decoder(g.channels, g.stages, g.filt, g.segments, bits=g.bits, lib=lib, reduce=reduce, reconstruct=reconstruct)
    try:
        rc, res = dec.decode_host([stream], rw * rh)
        assert rc == 0
        return res[0]
    finally:
        dec.close()


def set_mode(monkeypatch, mode):
    if mode is None:
        monkeypatch.delenv("ICER_DEC_WAVE", raising=False)
    else:
        monkeypatch.setenv("ICER_DEC_WAVE", mode)


def staggered_unset(rig, case, monkeypatch):
    if case.name not in _STAGGERED:
        set_mode(monkeypatch, None)
        _STAGGERED[case.name] = ssc.run_staggered(rig, case, None)[0].stats()
    return _STAGGERED[case.name]


def registered(monkeypatch, expected, i):                                   # noqa: F811
    g, specs = CASES[i]
    case = ssc.case_of(expected, g, specs)
    slc.register(monkeypatch, (case.name, (case.g, case.spec)))
    return case


@pytest.mark.timeout(300)
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_ladder_to_lossless(mock_lib, expected, oracle, monkeypatch, i):    # noqa: F811
    case, rig = registered(monkeypatch, expected, i), Rig(mock_lib, oracle)
    seen = []
    for mode in ssc.MODES:
        set_mode(monkeypatch, mode)
        seen.append(ssc.run_ladder(rig, case, mode)[0].stats()[2:])
    assert seen == [seen[0]] * 4, (case.name, seen)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_plane_by_plane_into_three_staggered_slots(mock_lib, expected, oracle, monkeypatch, i):        # noqa: F811
    case, rig = registered(monkeypatch, expected, i), Rig(mock_lib, oracle)
    seen = [staggered_unset(rig, case, monkeypatch)[2:]]
    for mode in ssc.MODES[1:]:
        set_mode(monkeypatch, mode)
        seen.append(ssc.run_staggered(rig, case, mode)[0].stats()[2:])
    assert seen == [seen[0]] * 4, (case.name, seen)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("i", [i for i, (g, _) in enumerate(CASES) if not gsc.is_p1(g)], ids=[x for x, (g, _) in zip(IDS, CASES) if not gsc.is_p1(g)])
def test_ladder_with_decoder_options(mock_lib, expected, oracle, monkeypatch, i):                      # noqa: F811
    case, rig = registered(monkeypatch, expected, i), Rig(mock_lib, oracle)
    for mode in (None, "1"):
        set_mode(monkeypatch, mode)
        ssc.run_ladder(rig, case, mode, **ssc.option_sets(case.g)[i % 4])


@pytest.mark.timeout(300)
@pytest.mark.parametrize("i", range(len(ssc.WIDE)), ids=[gsc.case_id(g) for g, _ in ssc.WIDE])
def test_wide_chains(mock_lib, expected, oracle, monkeypatch, i):           # noqa: F811
    case = ssc.wide_case(expected, i)
    slc.register(monkeypatch, (case.name, (case.g, case.spec)))
    rig = Rig(mock_lib, oracle)
    for mode in ssc.MODES:
        set_mode(monkeypatch, mode)
        ssc.run_wide(rig, case, mode)
        if case.g.stages > 1:
            ssc.run_wide(rig, case, mode, ssc.levels_apart(case))


@pytest.mark.timeout(600)
def test_the_sample_meets_the_sweeps_conditions(mock_lib, expected, oracle, monkeypatch):              # noqa: F811
    """no geometry is left out; the sample has its failing grids, its rows narrower than a wavefront and its odd sides; and
    with the variable unset enough geometries of scenario B run chains on the thread route beside the wave-per-plane kernel"""
    cases = ssc.sample_cases(expected)
    assert len(cases) == len(CASES) and [c.g for c in cases] == [g for g, _ in CASES]
    assert sum(c.p1 for c in cases) >= 3 and sum(c.g.w < 64 for c in cases) >= 2 and sum(c.g.w % 2 or c.g.h % 2 for c in cases) >= 4
    rig, beside = Rig(mock_lib, oracle), []
    for case in cases:
        slc.register(monkeypatch, (case.name, (case.g, case.spec)))
        resumed, threads = staggered_unset(rig, case, monkeypatch)[:2]
        assert resumed > 0, case.name
        beside += [case.name] if threads > 0 else []
    assert len(beside) >= ssc.MIN_THREADS_BESIDE_PLANES, beside
