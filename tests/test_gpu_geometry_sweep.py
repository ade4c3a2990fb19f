"""The geometry sweep on the GPU (tests/geometry_sweep_cases.py): for every swept geometry -- 1 to 6 stages, all seven
filters, 1 to 32 segments, gray and YUV, 16 and 8 bits, grids kept under quirk P1, rows shorter than a wavefront, from 28 to
several thousand units -- one encoder runs the rate ladder against the oracle, re-cuts its own lossless masters to the same
quotas against the oracle, makes the quality-targeted encode under two byte caps against the plain model (energy table, D[K],
the cut rule, the separate call at the equivalent quota), and feeds one re-cut quota block to the decoder beside the oracle's
streams, both compared with the decoder oracle.  Every comparison is exact.  The CPU side of the same sample is
tests/test_geometry_sweep.py."""
import numpy as np
import pytest

from icer_compression_amd import api, decoder
from tests import encoder_batch_cases as ebc
from tests import geometry_sweep_cases as gsc
from tests import target_model as tm
from tests import test_gpu_ladder as tl
from tests.test_gpu_recut import encode_masters, recut, recutter, torch          # noqa: F401  (torch: a fixture)
from tests.test_gpu_target import HUGE, check_call, frame_means, target

pytestmark = pytest.mark.gpu

CASES = gsc.cases()


@pytest.fixture(scope="module")
def expected(oracle):
    return ebc.Expected(oracle)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("case", CASES, ids=[gsc.case_id(g) for g, _ in CASES])
def test_ladder_recut_target_and_chain(torch, oracle, expected, case):            # noqa: F811
    g, specs = case
    what = gsc.case_id(g)
    n = len(specs)
    rng = np.random.default_rng(g.w * 1000 + g.h)
    model = tm.Model(g.w, g.h, g.channels, g.stages, g.filt, g.segments, g.bits)
    enc = api.Encoder(g.w, g.h, g.channels, g.stages, g.filt, g.segments, max_frames=3, sample_bits=g.bits)
    r = recutter(g)
    assert model.n_units == enc.info()["units_per_frame"] == gsc.n_units(g)
    t = tl.device_frames(ebc.batch(g, specs))
    quotas = tl.class_ladder(g, rng)
    big = ebc.quota(g, "lossless")

    # the ladder against the oracle
    got = tl.ladder(enc, t, quotas)
    for q, quota in enumerate(quotas):
        for f, spec in enumerate(specs):
            ebc.check_frame(*got[q][f], expected(g, spec, quota), f"{what} ladder: quota {quota} frame {f} {spec}")

    # the encoder's lossless masters re-cut to the same quotas
    masters, sizes, enc_rcs = encode_masters(torch, enc, t, big)
    assert [int(x) for x in enc_rcs.cpu()] == [0] * n
    cut = recut(torch, r, masters, sizes, quotas)
    for q, quota in enumerate(quotas):
        for f, spec in enumerate(specs):
            ebc.check_frame(*cut[q][f], expected(g, spec, quota), f"{what} re-cut: quota {quota} frame {f} {spec}")

    # the quality target: nothing, a distortion met half way through frame 0's units, everything
    tables = None
    inside = 0
    for cap_class in ("lossless", "progressive"):
        cap = ebc.quota(g, cap_class)
        if tables is None:                                       # (the first call gives the energy table the target is taken from)
            target(enc, t, [HUGE], cap)
            tables = enc.distortion_table(0, model.n_families)
            D0 = model.distortions(tables, frame_means(oracle, g, specs[0]))
            mid = D0[model.n_units // 2] / (16 * g.samples)
            assert D0[0] > D0[model.n_units // 2], f"{what}: the first half of frame 0's units takes no distortion out"
        targets = [0.0, mid, HUGE]
        res = target(enc, t, targets, cap)
        met, at_cap, _ = check_call(oracle, enc, g, model, specs, t, targets, cap, res, f"{what} target, cap {cap_class}")
        for f in range(n):
            hg = res[2][f]
            assert (hg["stream"], hg["reached"], hg["rc"]) == (b"", 1, tm.QUOTA_EXCEEDED), (what, cap_class, f)
        inside += sum(1 for (q, f) in met if q == 1 and 0 < len(res[q][f]["stream"]) < len(at_cap[f][1]))
        if cap_class == "lossless":                              # frame 0 meets its own mid target strictly inside its stream
            K = len(tm.parse_stream(res[1][0]["stream"]))
            assert res[1][0]["reached"] == 1 and 0 < K < model.n_units, (what, K, model.n_units)
    assert inside >= 1, f"{what}: no target was met below the cap"

    # one quota block of a re-cut into the decoder, beside the oracle's streams at that quota
    quota = ebc.quota(g, "cut")
    d = decoder.Decoder(g.channels, g.stages, g.filt, g.segments, bits=g.bits)
    try:
        out = torch.zeros((1, n, quota + 3), dtype=torch.uint8, device="cuda")
        cut_sizes = torch.zeros((1, n), dtype=torch.int64, device="cuda")
        cut_rcs = torch.zeros((1, n), dtype=torch.int32, device="cuda")
        r.recut_torch(masters, sizes, [quota], out, cut_sizes, cut_rcs)
        planes = torch.full((n, g.channels, g.w * g.h), 0x5A, dtype=torch.int16 if g.bits == 16 else torch.uint8, device="cuda")
        rcs = torch.full((n,), 77, dtype=torch.int32, device="cuda")
        ws, hs = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda")
        d.decode_torch(out[0], cut_sizes[0], planes, rcs, ws, hs)
        torch.cuda.synchronize()
        rc, want = d.decode_host([expected(g, s, quota)[1] for s in specs], g.w * g.h)
        assert rc == 0
        for f in range(n):
            assert (int(rcs[f]), int(ws[f]), int(hs[f])) == want[f][:3], (what, f, int(rcs[f]), want[f][:3])
            # both against the decoder oracle on the oracle's stream (a kept grid of quirk P1 ends it with rc -3, the words stay)
            orc = oracle.decompress(expected(g, specs[f], quota)[1], g.channels, g.stages, g.filt, g.segments, bufsize=g.w * g.h, bits=g.bits)
            assert want[f][:3] == orc[:3] == (-3 if gsc.is_p1(g) else 0, g.w, g.h), (what, f, want[f][:3], orc[:3])
            for c in range(g.channels):
                p = planes[f, c].cpu().numpy()
                assert np.array_equal(p.view(np.uint16) if g.bits == 16 else p, want[f][3][c]), (what, f, c)
                assert np.array_equal(want[f][3][c], orc[3][c]), (what, f, c, "decode_host differs from the decoder oracle")
    finally:
        d.close()
    assert enc.stats()["unit_timeouts"] == 0
    enc.close()
    r.close()
