"""The geometry sweep of the decode sessions on the GPU (tests/session_sweep_cases.py): the three resumable chain decoders --
decode_chains_planes_resume_kernel (a wave per plane behind a loader wave), decode_chains_wave_resume_kernel (a lane per plane over
a row ring preloaded from, and recycled into, the state plane) and decode_chains_resume_kernel (a thread per chain) -- over every
geometry of tests/geometry_sweep_cases.py and two wide frames, in all four settings of ICER_DEC_WAVE: 1 to 6 stages, all seven
filters, 1 to 32 segments, gray and YUV, 16 and 8 bits, odd sides, rows narrower than a wavefront, grids that fail (quirk P1),
chains too wide for the row ring.  Per geometry one test runs the quota ladder to lossless, the plane-by-plane feed of three
staggered slots and the ladder under one set of decoder options; every image is compared with tests/session_model.py sample for
sample and the counts with the conditions tests/test_session_sweep_mock.py meets on the CPU.  Streams are the CPU oracle's; the
only device objects are decoder.Decoder and decoder.Session."""
import pytest

from icer_compression_amd import decoder
from tests import encoder_batch_cases as ebc
from tests import geometry_sweep_cases as gsc
from tests import reduced_model as red
from tests import session_lanes_cases as slc
from tests import session_sweep_cases as ssc
from tests import test_gpu_session as tgs
from tests.test_gpu_recut import torch                      # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

CASES = gsc.cases()
IDS = [gsc.case_id(g) for g, _ in CASES]


@pytest.fixture(scope="module")
def expected(oracle):
    return ebc.Expected(oracle)


class Rig(tgs.Rig):
    kind = "gpu"

    def plain(self, case, stream, reduce=0, reconstruct=0):
        """(rc, w, h, planes) of the plain decode of one stream by a decoder of its own"""
        g = case.g
        rw, rh = red.reduced_size(g.w, g.h, reduce)
        dec = decoder.Decoder(g.channels, g.stages, g.filt, g.segments, bits=g.bits, reduce=reduce, reconstruct=reconstruct)
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


def closed(run):
    """the counts of a scenario's session, the session closed"""
    ses, _ = run
    stats = ses.stats()
    ses.close()
    return stats


@pytest.mark.timeout(300)
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_ladder_staggered_slots_and_options(torch, expected, oracle, monkeypatch, i):      # noqa: F811
    g, specs = CASES[i]
    case = ssc.case_of(expected, g, specs)
    slc.register(monkeypatch, (case.name, (case.g, case.spec)))
    rig = Rig(torch, oracle)
    ladder, staggered = [], []
    for mode in ssc.MODES:
        set_mode(monkeypatch, mode)
        ladder.append(closed(ssc.run_ladder(rig, case, mode))[2:])
        staggered.append(closed(ssc.run_staggered(rig, case, mode))[2:])
        if mode in (None, "1") and not case.p1:
            closed(ssc.run_ladder(rig, case, mode, **ssc.option_sets(g)[i % 4]))
    assert ladder == [ladder[0]] * 4 and staggered == [staggered[0]] * 4, (case.name, ladder, staggered)
    for dec in rig.keep:
        dec.close()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("i", range(len(ssc.WIDE)), ids=[gsc.case_id(g) for g, _ in ssc.WIDE])
def test_wide_chains(torch, expected, oracle, monkeypatch, i):                             # noqa: F811
    case = ssc.wide_case(expected, i)
    slc.register(monkeypatch, (case.name, (case.g, case.spec)))
    rig = Rig(torch, oracle)
    for mode in ssc.MODES:
        set_mode(monkeypatch, mode)
        closed(ssc.run_wide(rig, case, mode))
        if case.g.stages > 1:
            closed(ssc.run_wide(rig, case, mode, ssc.levels_apart(case)))
    for dec in rig.keep:
        dec.close()
