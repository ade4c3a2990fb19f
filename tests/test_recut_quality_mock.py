"""icerx_recut_device_target_async / icerx_recut_device_budget_async end to end on the CPU (csrc/recut_quality.hpp in the mock
build of tests/test_recut_mock.py).  Masters are oracle streams; a sidecar row is tm.Model.energy_table of the oracle's
coefficient planes and the tm.ll_means word.  The cuts are held to the definitions in plain Python -- tm.target_walk and
budget_model.allocate on the master's parsed packet table --, the streams to the byte-quota re-cut at the equivalent quota the
call reports (and, for complete masters, to the oracle at that quota).  CPU only."""
import numpy as np
import pytest

from tests import budget_model as bm
from tests import encoder_batch_cases as ebc
from tests import geometry_sweep_cases as gsc
from tests import reduced_model as red
from tests import target_model as tm
from tests.recut_quality_cases import check_target, model_of, reduced_view, sidecar_row, unit_bits
from tests.test_emu_target import words16
from tests.test_recut_mock import (FATAL, GUARD, INVALID_INPUT, OUT_OF_DATA, QUOTA_EXCEEDED, SENT, SENT_RC, SENT_SIZE, expected, mock_lib,  # noqa: F401
                                   pack_odd, pack_rows, recut_call)

SENT64 = 0x5555555555555555
BASE = ebc.Geometry(96, 80, 3, 3, 1, 3)                          # 90 families, 810 units: more than one 64-lane round of every scan
BASE_SPECS = [("smooth", 0), ("noise8", 1), (("sparse", "dot", "wide"), 2), ("flat", 3)]       # (flat: LL means above one byte)


def quality_recutter(lib, g, max_reduce=0):
    from icer_compression_amd import decoder
    return decoder.Recutter(g.w, g.h, g.channels, g.stages, g.segments, bits=g.bits, lib=lib, max_reduce=max_reduce, filt=g.filt)


class Master:
    """one frame: the oracle's complete stream, its sidecar row and the model's view of both"""

    def __init__(self, expected, g, spec, model):
        self.g, self.spec, self.model = g, spec, model
        rc, self.stream, coef = expected(g, spec, ebc.quota(g, "lossless"))
        assert rc == 0
        self.means = tm.ll_means(expected.orc, ebc.oracle_planes(g, spec), g.stages, g.filt) if g.bits == 16 else None
        self.E = model.energy_table(words16(g, coef))
        self.row = sidecar_row(model, self.E, self.means)


def sidecars_of(rows, pad=3):
    """the rows in a 2-D array of a padded stride, the padding a sentinel"""
    side = np.full((len(rows), len(rows[0]) + pad), SENT64, np.uint64)
    for k, row in enumerate(rows):
        side[k, :len(row)] = row
    return side


def quality_call(r, kind, blob, offsets, lens, side, cuts, cap, stream_stride=0, reduce=0, **override):
    """the target (cuts = [(reduce, mse)]) or budget (cuts = budgets) call on host arrays into Q * n + 1 sentinel rows, with a
    workspace of exactly the bytes asked for and a guard tail -> (rc, res[c][f] dict, thresholds, totals) after checking the
    buffer promises"""
    n, Q = len(lens), len(cuts)
    stride = (cap + 5) | 1
    out = np.full((Q * n + 1, stride), SENT, np.uint8)
    sizes, dist, equiv = (np.full(Q * n + 1, SENT_SIZE, np.uint64) for _ in range(3))
    rcs, flag = (np.full(Q * n + 1, SENT_RC, np.int32) for _ in range(2))
    thr, tot = (np.full(Q + 1, SENT_SIZE, np.uint64) for _ in range(2))
    offs = np.asarray(offsets, np.uint64) if offsets is not None else None
    ln = np.asarray(lens, np.uint64)
    keep, keep_side = blob.copy(), side.copy()
    need = (r.target_workspace_bytes if kind == "target" else r.budget_workspace_bytes)(n, len(blob), Q)
    assert need > 0
    work = np.full(need + GUARD, 0xCD, np.uint8)
    args = dict(n=n, d_data=blob.ctypes.data, data_bytes=len(blob), d_offsets=offs.ctypes.data if offs is not None else None,
                stream_stride=stream_stride, d_lens=ln.ctypes.data, d_sidecar=side.ctypes.data, sidecar_stride=side.shape[1], byte_cap=cap,
                d_out=out.ctypes.data, out_stride=stride, d_sizes=sizes.ctypes.data, d_rcs=rcs.ctypes.data, d_dist=dist.ctypes.data,
                d_equiv_quota=equiv.ctypes.data, d_workspace=work.ctypes.data, workspace_bytes=need, stream=None)
    if kind == "target":
        args.update(reduces=[c[0] for c in cuts], targets_mse=[c[1] for c in cuts], d_reached=flag.ctypes.data)
        fn = r.recut_target_device_async_ptrs
    else:
        args.update(reduce=reduce, budgets=list(cuts), d_at_cap=flag.ctypes.data, d_threshold=thr.ctypes.data, d_total=tot.ctypes.data)
        fn = r.recut_budget_device_async_ptrs
    args.update(override)
    rc = fn(**args)
    assert (work[need:] == 0xCD).all(), "written behind the workspace"
    assert np.array_equal(blob, keep) and np.array_equal(side, keep_side), "the masters or sidecars were modified"
    everything = (out, sizes, dist, equiv, rcs, flag, thr, tot)
    if rc != 0:
        assert all((a == s).all() for a, s in zip(everything, (SENT, SENT_SIZE, SENT_SIZE, SENT_SIZE, SENT_RC, SENT_RC, SENT_SIZE, SENT_SIZE))), \
            "a refused call wrote"
        return rc, None, None, None
    assert (out[Q * n] == SENT).all() and all(a[Q * n] == s for a, s in ((sizes, SENT_SIZE), (dist, SENT_SIZE), (equiv, SENT_SIZE),
                                                                          (rcs, SENT_RC), (flag, SENT_RC))), "written past the Q * n rows"
    assert thr[Q] == SENT_SIZE and tot[Q] == SENT_SIZE and (kind == "budget" or ((thr == SENT_SIZE).all() and (tot == SENT_SIZE).all()))
    res = []
    for c in range(Q):
        row = []
        for f in range(n):
            k = c * n + f
            s = int(sizes[k])
            assert 0 <= s <= cap and (out[k, s:] == SENT).all(), f"cut {c} frame {f}: bytes behind its stream of {s} bytes"
            row.append(dict(rc=int(rcs[k]), stream=out[k, :s].tobytes(), flag=int(flag[k]), dist=int(dist[k]), equiv=int(equiv[k])))
        res.append(row)
    return rc, res, [int(t) for t in thr[:Q]], [int(t) for t in tot[:Q]]


NO_STREAM = dict(stream=b"", flag=0, dist=0)


def check_no_stream(got, rc, cap, what):
    assert got == dict(NO_STREAM, rc=rc, equiv=cap), f"{what}: {got['rc']}, {len(got['stream'])} bytes"


@pytest.fixture(scope="module")
def base(mock_lib, expected):
    model = model_of(BASE)
    masters = [Master(expected, BASE, s, model) for s in BASE_SPECS]
    return model, masters, quality_recutter(mock_lib, BASE)


def targets_for(model, D_list):
    """mean squared errors in no particular order with a repeat: two in the middle of the frames' curves, 0 (which a frame
    with D_n > 0 does not reach) and one every frame meets with nothing kept"""
    mid = sorted(D[len(D) // 3] for D in D_list)[len(D_list) // 2]
    low = sorted(D[2 * len(D) // 3] for D in D_list)[0]
    scale = float(model.samples * 16)
    return [mid / scale, 0.0, low / scale, 1e9, mid / scale]


def test_target_equals_the_walk_and_the_byte_quota_recut(base, expected):
    model, masters, r = base
    assert r.sidecar_entries == model.n_families * (model.P + 1) + 1 == len(masters[0].row)
    rng = np.random.default_rng(11)
    streams = [m.stream for m in masters]
    bits = [unit_bits(model, s) for s in streams]
    D = [model.distortions(m.E, m.means) for m in masters]
    mses = targets_for(model, D)
    T = [model.threshold(x) for x in mses]
    assert all(r.target_threshold(x) == t for x, t in zip(mses, T)) and r.target_threshold(-1.0) == 0 == r.target_threshold(float("nan"))
    assert any(D[f][-1] > 0 for f in range(len(masters))), "target 0 is reached by every frame"
    side = sidecars_of([m.row for m in masters])
    blob, offsets = pack_odd(rng, streams)
    rows, stride = pack_rows(streams)
    lens = [len(s) for s in streams]
    for cap in (ebc.quota(BASE, "lossless"), min(lens) // 2):         # (the second one binds)
        cuts = [(0, x) for x in mses]
        for what, (rc, got, _, _) in (("odd offsets", quality_call(r, "target", blob, offsets, lens, side, cuts, cap)),
                                      ("stride", quality_call(r, "target", rows, None, lens, side, cuts, cap, stream_stride=stride))):
            assert rc == 0, what
            flags = set()
            for c in range(len(cuts)):
                for f in range(len(masters)):
                    want = tm.target_walk(bits[f], D[f], T[c], cap)
                    check_target(got[c][f], want, f"{what}, cap {cap}, target {c} frame {f}")
                    flags.add((want[3], want[6]))
                    if what == "stride":
                        ebc.check_frame(got[c][f]["rc"], got[c][f]["stream"], expected(BASE, masters[f].spec, got[c][f]["equiv"]),
                                        f"cap {cap}, target {c} frame {f}: the oracle at the equivalent quota")
            assert (1, False) in flags and (0, True) in flags, "both a reached target and a cap-made cut"
        # the equivalent quota: the byte-quota call on the same masters makes the same streams
        quotas = sorted({row["equiv"] for cut in got for row in cut})
        rc, again = recut_call(r, blob, offsets, lens, quotas)
        assert rc == 0
        for c in range(len(cuts)):
            for f in range(len(masters)):
                assert again[quotas.index(got[c][f]["equiv"])][f] == (got[c][f]["rc"], got[c][f]["stream"]), (cap, c, f)


def frames_for_budget(model, masters, statuses=None):
    out = []
    for f, m in enumerate(masters):
        if statuses and statuses.get(f):
            out.append(([], [0], statuses[f]))
        else:
            out.append((unit_bits(model, m.stream), model.distortions(m.E, m.means), False))
    return out


def check_budget(r, blob, offsets, lens, side, frames, budgets, cap, what, reduce=0):
    rc, got, thr, tot = quality_call(r, "budget", blob, offsets, lens, side, budgets, cap, reduce=reduce)
    assert rc == 0, what
    for b, B in enumerate(budgets):
        want, T, total = bm.allocate(frames, B, cap)
        assert (thr[b], tot[b]) == (T, total) and total <= max(B, 0), f"{what}: budget {B}: threshold {thr[b]} total {tot[b]}, want {T} {total}"
        for f, w in enumerate(want):
            g = got[b][f]
            assert (g["rc"], len(g["stream"]), g["flag"], g["dist"], g["equiv"]) == (w["rc"], w["size"], w["at_cap"], w["dist"], w["equiv"]), \
                f"{what}: budget {B} frame {f}: got {g['rc']} {len(g['stream'])} {g['flag']} {g['dist']} {g['equiv']}, want {w}"
    return got


def test_budget_equals_the_allocation(base):
    model, masters, r = base
    rng = np.random.default_rng(12)
    streams = [m.stream for m in masters]
    lens = [len(s) for s in streams]
    blob, offsets = pack_odd(rng, streams)
    side = sidecars_of([m.row for m in masters])
    frames = frames_for_budget(model, masters)
    total = sum(lens)
    for cap in (ebc.quota(BASE, "lossless"), max(lens) // 2):
        budgets = [total // 3, 27, total + 5, 0, total // 7, total]
        got = check_budget(r, blob, offsets, lens, side, frames, budgets, cap, f"cap {cap}")
        quotas = sorted({row["equiv"] for cut in got for row in cut})
        rc, again = recut_call(r, blob, offsets, lens, quotas)
        assert rc == 0
        for b in range(len(budgets)):
            for f in range(len(masters)):
                assert again[quotas.index(got[b][f]["equiv"])][f] == (got[b][f]["rc"], got[b][f]["stream"]), (cap, b, f)
        assert all(row["stream"] == b"" for row in got[1] + got[3]), "a budget below one packet header keeps nothing"


def test_budget_of_70_small_frames(mock_lib, expected):
    g = ebc.Geometry(32, 24, 1, 2, 0, 1)
    model = model_of(g)
    kinds = ("smooth", "noise8", "sparse", "wide", "flat", "dot", "blank")
    masters = [Master(expected, g, (kinds[k % len(kinds)], k), model) for k in range(70)]
    r = quality_recutter(mock_lib, g)
    streams = [m.stream for m in masters]
    lens = [len(s) for s in streams]
    blob, offsets = pack_odd(np.random.default_rng(13), streams)
    side = sidecars_of([m.row for m in masters], pad=0)
    total = sum(lens)
    check_budget(r, blob, offsets, lens, side, frames_for_budget(model, masters), [total // 2, total // 9, 2 * total], max(lens) + 40, "70 frames")
    r.close()


def test_reduced_cuts_equal_the_model_and_the_definition(mock_lib, expected):
    g = ebc.Geometry(61, 45, 3, 3, 2, 2)
    model = model_of(g)
    masters = [Master(expected, g, s, model) for s in (("noise8", 0), ("smooth", 1), (("wide", "sparse", "smooth"), 2))]
    r = quality_recutter(mock_lib, g, max_reduce=2)
    assert r.max_reduce == 2
    streams = [m.stream for m in masters]
    lens = [len(s) for s in streams]
    blob, offsets = pack_odd(np.random.default_rng(14), streams)
    side = sidecars_of([m.row for m in masters])
    cap = ebc.quota(g, "lossless")
    views = {0: (model, list(range(model.n_families)))}
    views.update({k: reduced_view(model, g, k) for k in (1, 2)})
    derived = {k: [red.derive(s, k) for s in streams] for k in (0, 1, 2)}
    bits = {k: [unit_bits(views[k][0], s) for s in derived[k]] for k in views}
    D = {k: [views[k][0].distortions(m.E[views[k][1]], m.means) for m in masters] for k in views}
    cuts = []
    for k in (2, 0, 1):
        Ds = sorted(d[len(d) // 2] for d in D[k])
        cuts += [(k, Ds[1] / float(views[k][0].samples * 16)), (k, 0.0)]
    assert all(r.target_threshold(x, k) == views[k][0].threshold(x) for k, x in cuts)
    rc, got, _, _ = quality_call(r, "target", blob, offsets, lens, side, cuts, cap)
    assert rc == 0
    for c, (k, x) in enumerate(cuts):
        for f in range(len(masters)):
            check_target(got[c][f], tm.target_walk(bits[k][f], D[k][f], views[k][0].threshold(x), cap), f"cut {c} (reduce {k}) frame {f}")
    # the equivalent quota, through the cuts call
    for c, (k, _) in enumerate(cuts):
        for f in range(len(masters)):
            out = np.zeros((1, cap + 8), np.uint8)
            sizes, rcs = np.zeros(1, np.uint64), np.zeros(1, np.int32)
            one = np.frombuffer(streams[f], np.uint8).copy()
            ln = np.array([len(one)], np.uint64)
            work = np.zeros(r.cuts_workspace_bytes(1, len(one), 1), np.uint8)
            assert r.recut_cuts_device_async_ptrs(1, one.ctypes.data, len(one), None, 0, ln.ctypes.data, [k], [got[c][f]["equiv"]], out.ctypes.data,
                                                  out.shape[1], sizes.ctypes.data, rcs.ctypes.data, work.ctypes.data, len(work)) == 0
            assert (int(rcs[0]), out[0, :int(sizes[0])].tobytes()) == (got[c][f]["rc"], got[c][f]["stream"]), (c, f)
    # the definition: a reduce-0 call of a quality recutter of the reduced geometry, on the derived streams, rows re-indexed
    for k in (1, 2):
        rw, rh = red.reduced_size(g.w, g.h, k)
        gk = ebc.Geometry(rw, rh, g.channels, g.stages - k, g.filt, g.segments)
        rk = quality_recutter(mock_lib, gk)
        side_k = sidecars_of([sidecar_row(views[k][0], m.E[views[k][1]], m.means) for m in masters])
        blob_k, offsets_k = pack_odd(np.random.default_rng(15 + k), derived[k])
        mine = [(c, x) for c, (kk, x) in enumerate(cuts) if kk == k]
        rc, want, _, _ = quality_call(rk, "target", blob_k, offsets_k, [len(s) for s in derived[k]], side_k, [(0, x) for _, x in mine], cap)
        assert rc == 0
        for j, (c, _) in enumerate(mine):
            assert want[j] == got[c], f"reduce {k}, cut {c}"
        # and the budget call at this reduce
        frames = [(bits[k][f], D[k][f], False) for f in range(len(masters))]
        total = sum(len(s) for s in derived[k])
        check_budget(r, blob, offsets, lens, side, frames, [total // 2, total + 1, 30], cap, f"budget at reduce {k}", reduce=k)
        rk.close()
    r.close()


def test_master_and_sidecar_cases(base, expected):
    model, masters, r = base
    rng = np.random.default_rng(16)
    m0, m1 = masters[1], masters[0]
    lossless = len(m0.stream)
    third = expected(BASE, m0.spec, lossless // 3)
    assert third[0] == QUOTA_EXCEEDED
    # a mid-chain packet removed: the first packet of bit plane 4 of the first family
    packets, at, gone = tm.parse_stream(m1.stream), 0, None
    for (ch, lv, sb, lsb, sg, b) in packets:
        if gone is None and lsb == 4 and b > 0:
            gone = (at, at + tm.unit_len(b))
        at += tm.unit_len(b)
    holed = m1.stream[:gone[0]] + m1.stream[gone[1]:]
    other = ebc.Geometry(64, 48, 3, 3, 1, 3)
    alien = expected(other, ("smooth", 0), ebc.quota(other, "lossless"))[1]
    bad_mono, bad_bound = m1.row.copy(), m1.row.copy()
    bad_mono[5 * (model.P + 1) + 3] = bad_mono[5 * (model.P + 1) + 4] + np.uint64(1)
    fam = model.families[7]
    bad_bound[7 * (model.P + 1) + model.P] = np.uint64(fam[3] * fam[4] * 32767 * 32767 + 1)
    garbage = rng.integers(0, 2 ** 63, len(m1.row)).astype(np.uint64)
    streams = [third[1], holed, alien, m1.stream, b"", m1.stream, m1.stream, m0.stream]
    rows = [m0.row, m1.row, m1.row, m1.row, garbage, bad_mono, bad_bound, m0.row]
    blob, offsets = pack_odd(rng, streams)
    lens = [len(s) for s in streams]
    offsets += [len(blob) - 10]                                         # a frame that leaves the blob
    lens += [11]
    rows.append(m0.row)
    side = sidecars_of(rows)
    status = {2: INVALID_INPUT, 4: OUT_OF_DATA, 5: INVALID_INPUT, 6: INVALID_INPUT, 8: INVALID_INPUT}
    cap = lossless + 100
    D0, D1 = model.distortions(m0.E, m0.means), model.distortions(m1.E, m1.means)
    views = {0: (unit_bits(model, third[1]), D0), 1: (unit_bits(model, holed), D1), 3: (unit_bits(model, m1.stream), D1),
             7: (unit_bits(model, m0.stream), D0)}
    assert tm.TOO_BIG in views[0][0] and views[1][0].count(tm.TOO_BIG) == 1
    mses = [0.0, D1[model.n_units // 2] / float(model.samples * 16)]
    rc, got, _, _ = quality_call(r, "target", blob, offsets, lens, side, [(0, x) for x in mses], cap)
    assert rc == 0
    for c, x in enumerate(mses):
        for f in range(len(lens)):
            if f in status:
                check_no_stream(got[c][f], status[f], cap, f"target {c} frame {f}")
            else:
                check_target(got[c][f], tm.target_walk(views[f][0], views[f][1], model.threshold(x), cap), f"target {c} frame {f}")
    assert got[0][0]["stream"] == third[1] and got[0][0]["equiv"] == cap and got[0][0]["flag"] == 0      # (the cut master itself: the cap is above it)
    frames = [(views[f][0], views[f][1], False) if f in views else ([], [0], status[f]) for f in range(len(lens))]
    total = sum(len(streams[f]) for f in views)
    check_budget(r, blob, offsets, lens, side, frames, [total // 2, total, 20], cap, "frames with a status among the others")


def test_refused_calls_write_nothing(base, mock_lib):
    model, masters, r = base
    streams = [m.stream for m in masters[:2]]
    lens = [len(s) for s in streams]
    blob, offsets = pack_odd(np.random.default_rng(17), streams)
    side = sidecars_of([m.row for m in masters[:2]], pad=0)
    cap = max(lens)
    n, entries = len(lens), side.shape[1]
    cuts, budgets = [(0, 1.0), (0, 0.0)], [1000, 5000]
    short = np.ascontiguousarray(side[:, :entries - 1])
    both = {"no frames": dict(n=0), "negative frames": dict(n=-1), "too many frames": dict(n=65536), "null data": dict(d_data=None),
            "null lens": dict(d_lens=None), "null sidecar": dict(d_sidecar=None), "null out": dict(d_out=None), "null sizes": dict(d_sizes=None),
            "null rcs": dict(d_rcs=None), "null dist": dict(d_dist=None), "null equiv": dict(d_equiv_quota=None),
            "null workspace": dict(d_workspace=None), "stride below the cap": dict(out_stride=cap - 1),
            "sidecar stride below the entries": dict(d_sidecar=short.ctypes.data, sidecar_stride=entries - 1)}
    target = dict(both, **{"no cuts": dict(n_cuts=0), "17 cuts": dict(reduces=[0] * 17, targets_mse=[1.0] * 17), "null targets": dict(targets_mse=None, n_cuts=2),
                           "null reached": dict(d_reached=None), "a reduce above max_reduce": dict(reduces=[0, 1]),
                           "a negative reduce": dict(reduces=[-1, 0]), "a negative target": dict(targets_mse=[1.0, -0.5]),
                           "a NaN target": dict(targets_mse=[float("nan"), 1.0])})
    budget = dict(both, **{"no budgets": dict(n_budgets=0), "17 budgets": dict(budgets=[100] * 17), "null budgets": dict(budgets=None, n_budgets=2),
                           "null at_cap": dict(d_at_cap=None), "null threshold": dict(d_threshold=None), "null total": dict(d_total=None),
                           "a reduce above max_reduce": dict(reduce=1), "a negative reduce": dict(reduce=-1)})
    for kind, cases, c in (("target", target, cuts), ("budget", budget, budgets)):
        need = (r.target_workspace_bytes if kind == "target" else r.budget_workspace_bytes)(n, len(blob), 2)
        cases = dict(cases, **{"a workspace one byte short": dict(workspace_bytes=need - 1)})
        for what, kw in cases.items():
            assert quality_call(r, kind, blob, offsets, lens, side, c, cap, **kw)[0] == INVALID_INPUT, f"{kind}: {what}"
        assert quality_call(r, kind, blob, offsets, lens, side, c, cap, data_bytes=0xFFFFFFFF - 64)[0] == FATAL, kind
        assert quality_call(r, kind, blob, offsets, lens, side, c, cap)[0] == 0, kind
    # reduces = NULL: every reduce 0
    rc, a, _, _ = quality_call(r, "target", blob, offsets, lens, side, cuts, cap, reduces=None, n_cuts=2)
    assert rc == 0 and a == quality_call(r, "target", blob, offsets, lens, side, cuts, cap)[1]
    # a plain recutter: no sidecar entries, no workspace figure, every call refused
    from icer_compression_amd import decoder
    plain = decoder.Recutter(BASE.w, BASE.h, BASE.channels, BASE.stages, BASE.segments, lib=mock_lib)
    assert plain.sidecar_entries == 0 and plain.target_workspace_bytes(n, len(blob), 2) == 0 == plain.budget_workspace_bytes(n, len(blob), 2)
    work = np.zeros(r.budget_workspace_bytes(n, len(blob), 2), np.uint8)
    for kind, c in (("target", cuts), ("budget", budgets)):
        fn = r.target_workspace_bytes if kind == "target" else r.budget_workspace_bytes
        # (quality_call sizes the workspace by the recutter it is given: hand it the quality recutter's figure)
        plain.target_workspace_bytes = plain.budget_workspace_bytes = fn
        assert quality_call(plain, kind, blob, offsets, lens, side, c, cap, d_workspace=work.ctypes.data, workspace_bytes=len(work))[0] == INVALID_INPUT
    plain.close()
    assert mock_lib.icerx_recut_sidecar_entries(None) == 0 and mock_lib.icerx_recut_target_threshold(None, 1.0, 0) == 0


def test_create_quality_refusals(mock_lib):
    from icer_compression_amd import decoder
    for kw in (dict(filt=7), dict(filt=-1), dict(max_reduce=3), dict(max_reduce=-1)):
        args = dict(dict(filt=0, max_reduce=0), **kw)
        with pytest.raises(RuntimeError, match="icerx_recutter_create_quality: -11 "):
            decoder.Recutter(64, 64, 1, 3, 4, lib=mock_lib, **args)
    # a subband with fewer samples than segments (quirk P1): the families of a reduced geometry are not the master's
    # -- here from reduce 2 on, where the planes of a chain keep grids of different packets
    p1 = ebc.Geometry(113, 64, 3, 4, 1, 29, bits=8)
    assert gsc.is_p1(p1)
    quality_recutter(mock_lib, p1, max_reduce=1).close()
    with pytest.raises(RuntimeError, match="icerx_recutter_create_quality: -11 .*fewer samples than segments"):
        quality_recutter(mock_lib, p1, max_reduce=2)
    # what the plain create refuses, with its code
    with pytest.raises(RuntimeError, match="icerx_recutter_create_quality: -4 "):
        decoder.Recutter(16, 16, 1, 4, 1, lib=mock_lib, filt=0)


SWEEP = [gsc.cases()[int(k)] for k in np.random.default_rng(gsc.SEED).choice(len(gsc.cases()), 12, replace=False)]


@pytest.mark.parametrize("g,specs", SWEEP, ids=[gsc.case_id(g) for g, _ in SWEEP])
def test_geometry_sweep_target(mock_lib, expected, g, specs):
    model = model_of(g)
    masters = [Master(expected, g, s, model) for s in specs]
    r = quality_recutter(mock_lib, g)
    assert r.sidecar_entries == len(masters[0].row)
    streams = [m.stream for m in masters]
    lens = [len(s) for s in streams]
    blob, offsets = pack_odd(np.random.default_rng(18), streams)
    side = sidecars_of([m.row for m in masters])
    bits = [unit_bits(model, s) for s in streams]
    D = [model.distortions(m.E, m.means) for m in masters]
    mses = targets_for(model, D)
    for cap in (ebc.quota(g, "lossless"), max(max(lens) // 3, 30)):
        rc, got, _, _ = quality_call(r, "target", blob, offsets, lens, side, [(0, x) for x in mses], cap)
        assert rc == 0
        for c, x in enumerate(mses):
            for f in range(len(masters)):
                check_target(got[c][f], tm.target_walk(bits[f], D[f], model.threshold(x), cap), f"cap {cap} target {c} frame {f}")
    r.close()
