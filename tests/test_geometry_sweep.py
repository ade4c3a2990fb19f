"""The geometry sweep on the CPU (tests/geometry_sweep_cases.py): the sample meets its coverage conditions; for every swept
geometry the plain model of tests/target_model.py -- units, rectangles and families, quirk P1 included -- equals the planner
(csrc/plan.hpp through the emulator build) and the packets of the oracle's stream; the re-cut of the oracle's lossless masters
through the mock runtime equals the oracle at every quota class, byte for byte; and the emulated energy pass over the model's
family rectangles equals numpy on the oracle's coefficient planes.  The same geometries run on the GPU in
tests/test_gpu_geometry_sweep.py."""
import ctypes as C

import numpy as np
import pytest

from tests import encoder_batch_cases as ebc
from tests import geometry_sweep_cases as gsc
from tests import target_model as tm
from tests.test_emu_target import emu as distortion_emu            # noqa: F401  (the fixture that binds emu_family_energy)
from tests.test_emu_target import words16
from tests.test_recut_mock import mock_lib, pack_odd, recut_call, recutter, wanted   # noqa: F401  (mock_lib: a fixture)

CASES = gsc.cases()
sweep = pytest.mark.parametrize("case", CASES, ids=[gsc.case_id(g) for g, _ in CASES])
PLAN_ROWS = 8000                                                      # (what the emu fixture's plan_units gives back at most)


@pytest.fixture(scope="module")
def expected(oracle):
    return ebc.Expected(oracle)


def model_of(g, bits=None):
    return tm.Model(g.w, g.h, g.channels, g.stages, g.filt, g.segments, bits or g.bits)


# ---- 1. the sample ----------------------------------------------------------------------------------------------------------------
def test_sample_meets_its_coverage_conditions(oracle):
    gs = [g for g, _ in CASES]
    print({name: have for name, (have, _) in gsc.coverage(gs).items()})
    assert gsc.unmet(gs) == []
    assert 20 <= len(gs) <= 30 and len(set(gs)) == len(gs)
    for g, specs in CASES:
        assert 9 <= g.w <= 200 and 9 <= g.h <= 200 and g.w * g.h <= gsc.MAX_SAMPLES
        assert 1 <= g.stages <= 6 and 0 <= g.filt <= 6 and 1 <= g.segments <= 32 and g.channels in (1, 3) and g.bits in (16, 8)
        assert len(specs) == 3
        kinds = [k for kind, _ in specs for k in ebc.channel_kinds(g, kind)]
        if g.bits == 16:
            assert set(kinds) <= set(ebc.CODED16) and specs[0][0] in ("noise8", "wide")
        else:
            assert set(kinds) <= set(ebc.KINDS8) - {"full8"} and ("noise6" not in kinds or g.filt == 0)
        assert gsc.coded_by(oracle, g, specs)
    # the conditions on P1 and on the unit counts, from the model itself
    p1 = [g for g in gs if model_of(g).stale]
    assert p1 == [g for g in gs if gsc.is_p1(g)] and len(p1) >= 3
    assert all(model_of(g).n_units == gsc.n_units(g) for g in gs)
    assert gsc.sample(oracle, target=3)[:3] == list(CASES[:3])        # (the same seed, the same sample)


def test_geometries_the_sampler_must_not_keep(oracle, emu):
    """the first packet's grid fails: refused by the planner, the oracle and the model alike.  A kept grid that leaves the
    plane (9 x 9, 1 stage, 17 segments: HH keeps the 4 x 5 grid of HL at (5, 5)): the model shows it, the sampler keeps such a
    geometry away from the oracle, and no swept geometry is one"""
    for (w, h, ch, st, seg) in ((24, 24, 1, 3, 10), (40, 40, 3, 3, 26), (48, 24, 1, 3, 19)):
        assert emu.plan_units(w, h, ch, st, seg)[0] == -3
        assert oracle.compress([np.zeros((h, w), np.uint16)] * ch, st, 0, seg, 1 << 20)[:2] == (-3, b"")
        with pytest.raises(tm.Refused):
            tm.Model(w, h, ch, st, 0, seg)
    for (w, h, ch, st, seg, bits) in ((9, 9, 1, 1, 17, 16), (9, 9, 3, 1, 20, 8), (11, 9, 1, 1, 21, 16)):
        m = tm.Model(w, h, ch, st, 0, seg, bits)
        assert m.stale and any(x + rw > w or y + rh > h for (_, x, y, rw, rh, _) in m.families)
        assert gsc.leaves_plane(ebc.Geometry(w, h, ch, st, 0, seg, bits=bits))
    assert not any(gsc.leaves_plane(g) for g, _ in CASES)
    # the P1 geometry of the first probe stays inside the plane and is coded
    g = ebc.Geometry(17, 17, 1, 3, 0, 6)
    m = model_of(g)
    assert m.stale and not gsc.leaves_plane(g)
    assert emu.plan_units(17, 17, 1, 3, 6)[0] == m.n_units
    assert oracle.compress(ebc.oracle_planes(g, ("noise8", 0)), 3, 0, 6, ebc.quota(g, "lossless"))[0] == 0


# ---- 2. the model against the planner and the oracle's packets ------------------------------------------------------------------------
@sweep
def test_model_units_equal_the_planner(emu, expected, case):
    g, specs = case
    # (the emulator's planner is the 16-bit one: nine planes; the 8-bit plan differs in the plane count alone)
    m = model_of(g, 16)
    n, rows = emu.plan_units(g.w, g.h, g.channels, g.stages, g.segments)
    assert n == m.n_units == gsc.n_units(g._replace(bits=16))
    assert all(0 <= x and x + rw <= g.w and 0 <= y and y + rh <= g.h and rw * rh >= 1 for (_, x, y, rw, rh, _) in m.families)
    want = np.array([m.families[f][1:5] + (ch, lv, sb, lsb, sg) for (ch, lv, sb, lsb, sg, f, _) in m.units], np.uint32)
    assert len(rows) == min(n, PLAN_ROWS)
    assert np.array_equal(rows, want[: len(rows)]), np.argwhere(rows != want[: len(rows)])[:4].tolist()
    # the families: the planner's index of every unit's family (emu_plan_orders gives it in launch order)
    L = emu.lib
    L.emu_plan_orders.argtypes = [C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_int, C.POINTER(C.c_uint32)]
    order, nf = np.zeros((n, 3), np.uint32), C.c_uint32()
    assert L.emu_plan_orders(g.w, g.h, g.channels, g.stages, g.segments, 0, order.ctypes.data, n, C.byref(nf)) == n
    assert nf.value == m.n_families and sorted(order[:, 0].tolist()) == list(range(n))
    fam = np.array([u[5] for u in m.units], np.uint32)
    assert np.array_equal(order[:, 1], fam[order[:, 0]])
    assert m.n_families >= n // 9 and (m.stale or m.n_families == n // 9)      # (P1 alone splits a segment number's planes)
    # the model of the geometry's own bit depth against the packets of the oracle's complete stream
    m = model_of(g)
    rc, stream, _ = expected(g, specs[0], ebc.quota(g, "lossless"))
    assert rc == 0
    got = [p[:5] for p in tm.parse_stream(stream)]
    assert len(got) == m.n_units and sorted(got) == sorted(u[:5] for u in m.units)


# ---- 3. the re-cut through the mock runtime ----------------------------------------------------------------------------------------
@sweep
def test_recut_mock_equals_oracle(mock_lib, expected, case):       # noqa: F811
    g, specs = case
    rng = np.random.default_rng(g.w * 1000 + g.h)
    mq = ebc.quota(g, "lossless")
    masters = [expected(g, s, mq) for s in specs]
    assert all(m[0] == 0 for m in masters)
    quotas = [int(ebc.quota(g, c)) for c in ebc.QUOTA_CLASSES]
    r = recutter(mock_lib, g)
    streams = [m[1] for m in masters]
    blob, offsets = pack_odd(rng, streams)
    rc, got = recut_call(r, blob, offsets, [len(s) for s in streams], quotas)
    assert rc == 0
    for q, quota in enumerate(quotas):
        for f, spec in enumerate(specs):
            ebc.check_frame(*got[q][f], wanted(expected, g, spec, masters[f], mq, quota), f"{gsc.case_id(g)}: quota {quota} frame {f} {spec}")
    r.close()


# ---- 4. the energy pass over the model's families -----------------------------------------------------------------------------------
@sweep
def test_energy_pass_over_the_model_families(distortion_emu, expected, case):     # noqa: F811
    g, specs = case
    m = model_of(g)
    rc, _, coef = expected(g, specs[0], ebc.quota(g, "lossless"))
    assert rc == 0
    planes = [np.ascontiguousarray(p) for p in words16(g, coef)]
    want = m.energy_table(planes)
    assert int(want[:, m.P].sum()) > 0
    for ch in range(g.channels):
        fams = [f for f, fam in enumerate(m.families) if fam[0] == ch]
        rects = np.array([m.families[f][1:5] for f in fams], np.uint32).ravel()
        for seed in (0, 7):
            E = np.full((len(fams), m.P + 1), 12345, np.uint64)
            n_wg = distortion_emu.emu_family_energy(planes[ch], g.w, rects, len(fams), m.P, seed, E)
            assert n_wg == sum((m.families[f][3] * m.families[f][4] + 4095) // 4096 for f in fams)
            assert np.array_equal(E, want[fams]), (ch, seed, np.argwhere(E != want[fams])[:4].tolist())
