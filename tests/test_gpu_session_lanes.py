"""The lane-per-plane route of a decode session on the GPU (csrc/decoder_session.hpp decode_chains_wave_resume_kernel,
csrc/decoder_wave.hpp decode_chain_wave_resume), with the rig of tests/test_gpu_session.py: under ICER_DEC_WAVE=1 the ladders of
two cases of tests/session_cases.py and of a case whose chains are taller than the kernel's row ring, the failing-plane and the
damaged-increment scenarios -- every image the oracle's, no chain counted in the wave-per-plane kernel or on the thread route --
and the load rule: with the variable unset, a call that brings more than 12 fast chains per compute unit leaves the wave-per-plane
kernel.  tests/test_session_lanes_mock.py runs the same on the CPU."""
import pytest

from tests import encoder_batch_cases as ebc
from tests import session_cases as sc
from tests import session_lanes_cases as slc
from tests.test_gpu_recut import torch                      # noqa: F401  (fixture)
from tests.test_gpu_session import Rig

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def expected(oracle):
    return ebc.Expected(oracle)


@pytest.fixture
def lanes(monkeypatch):
    monkeypatch.setenv("ICER_DEC_WAVE", "1")


def only_lanes(ses, tag):
    resumed, threads, planes, _ = ses.stats()
    assert resumed == 0 and threads == 0 and planes > 0, (tag, ses.stats())


@pytest.mark.parametrize("name", ["gray16_A4", "yuv8", slc.TALL[0]])
def test_ladder_of_three_steps(torch, expected, oracle, lanes, monkeypatch, name):
    slc.register(monkeypatch, slc.TALL)
    ses, _ = sc.run_ladder(Rig(torch, oracle), expected, oracle, name)
    only_lanes(ses, name)


def test_damaged_packet_in_an_increment(torch, expected, oracle, lanes):
    ses, _ = sc.run_damaged_increment(Rig(torch, oracle), expected)
    only_lanes(ses, "damaged increment")


def test_a_plane_that_fails_stops_its_chain_for_good(torch, expected, oracle, lanes):
    slc.run_failing_plane(Rig(torch, oracle), expected, oracle)


def test_a_call_above_the_load_threshold_leaves_the_wave_per_plane_kernel(torch, expected, oracle, monkeypatch):
    name = slc.register(monkeypatch, slc.LOAD)
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    # the precondition: pinned to the wave-per-plane kernel, the second feed resumes more than 12 chains per compute unit there
    monkeypatch.setenv("ICER_DEC_WAVE", "2")
    ses, slots = slc.run_load(Rig(torch, oracle), expected, oracle, name, n_cus)
    assert ses.stats()[0] > slc.CHAINS_PER_CU * n_cus and ses.stats()[1] == 0, (slots, ses.stats())
    pinned = ses.stats()
    # by load: none of them does, and no chain is left for the thread route (every ring fits)
    monkeypatch.delenv("ICER_DEC_WAVE")
    ses, _ = slc.run_load(Rig(torch, oracle), expected, oracle, name, n_cus)
    assert ses.stats()[:2] == [0, 0] and ses.stats()[2:] == pinned[2:], (ses.stats(), pinned)
