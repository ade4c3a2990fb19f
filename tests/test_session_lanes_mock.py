"""The lane-per-plane route of a decode session (csrc/decoder_session.hpp decode_chains_wave_resume_kernel, csrc/decoder_wave.hpp
decode_chain_wave_resume) and its routing on the CPU: decoder.hip on the mock HIP runtime, built and driven as
tests/test_session_mock.py does it.  Under ICER_DEC_WAVE=1 every chain of every scenario of tests/session_cases.py takes that kernel,
and the counts say so: no chain resumed in the wave-per-plane kernel, none on the thread route.  With the variable unset a feed
routes by load like the plain decode: a call that brings more than 12 fast chains per compute unit (the mock has 256) leaves the
wave-per-plane kernel.  tests/test_gpu_session_lanes.py runs the same on the GPU.  CPU only."""
import pytest

from tests import session_cases as sc
from tests import session_lanes_cases as slc
from tests.test_session_mock import Rig, expected, mock_lib                      # noqa: F401  (fixtures)

MOCK_CUS = 256                                  # icerx_decoder::n_cus where no device is asked


@pytest.fixture
def lanes(monkeypatch):
    monkeypatch.setenv("ICER_DEC_WAVE", "1")


def only_lanes(ses, tag):
    resumed, threads, planes, _ = ses.stats()
    assert resumed == 0 and threads == 0 and planes > 0, (tag, ses.stats())


@pytest.mark.parametrize("name", list(sc.CASES))
def test_ladder_of_three_steps(mock_lib, expected, oracle, lanes, name):
    ses, _ = sc.run_ladder(Rig(mock_lib, oracle), expected, oracle, name)
    only_lanes(ses, name)


def test_ladder_of_chains_taller_than_the_ring(mock_lib, expected, oracle, lanes, monkeypatch):
    name = slc.register(monkeypatch, slc.TALL)
    ses, _ = sc.run_ladder(Rig(mock_lib, oracle), expected, oracle, name)
    only_lanes(ses, name)


def test_ladder_through_the_host_call(mock_lib, expected, oracle, lanes):
    ses, _ = sc.run_ladder(Rig(mock_lib, oracle, host=True), expected, oracle, "gray16_A4")
    only_lanes(ses, "host call")


def test_roi_cut_then_quota_cut(mock_lib, expected, oracle, lanes):
    ses, _ = sc.run_roi_then_quota(Rig(mock_lib, oracle), expected)
    only_lanes(ses, "roi")


def test_slots_reset_size_mismatch_duplicate(mock_lib, expected, oracle, lanes):
    ses, _ = sc.run_slots(Rig(mock_lib, oracle), expected)
    only_lanes(ses, "slots")


def test_damaged_packet_in_an_increment(mock_lib, expected, oracle, lanes):
    ses, _ = sc.run_damaged_increment(Rig(mock_lib, oracle), expected)
    only_lanes(ses, "damaged increment")


def test_a_plane_that_fails_stops_its_chain_for_good(mock_lib, expected, oracle, lanes):
    """tests/session_cases.py run_failing_plane, but for its count of chains on the thread route: here the lane-per-plane kernel
    reports the stop (slc.run_failing_plane)"""
    slc.run_failing_plane(Rig(mock_lib, oracle), expected, oracle)


def test_a_call_above_the_load_threshold_leaves_the_wave_per_plane_kernel(mock_lib, expected, oracle, monkeypatch):
    name = slc.register(monkeypatch, slc.LOAD)
    # the precondition: pinned to the wave-per-plane kernel, the second feed resumes more than 12 chains per compute unit there
    monkeypatch.setenv("ICER_DEC_WAVE", "2")
    ses, slots = slc.run_load(Rig(mock_lib, oracle), expected, oracle, name, MOCK_CUS)
    assert ses.stats()[0] > slc.CHAINS_PER_CU * MOCK_CUS and ses.stats()[1] == 0, (slots, ses.stats())
    pinned = ses.stats()
    # by load: none of them does, and no chain is left for the thread route (every ring fits)
    monkeypatch.delenv("ICER_DEC_WAVE")
    ses, _ = slc.run_load(Rig(mock_lib, oracle), expected, oracle, name, MOCK_CUS)
    assert ses.stats()[:2] == [0, 0] and ses.stats()[2:] == pinned[2:], (ses.stats(), pinned)
