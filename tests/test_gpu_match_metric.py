"""GPU: the segment AP on the device (csrc/metric.hip behind vsc_match_metric) and everything built on it --
`match_metric_table`, `evaluate_matching_track(on_device=True)`, the CLI flag, `DeviceMatcher.segment_ap`.

The contract is exact: `ap` and the curve equal `match_metric` over the float64 tables bit for bit (`==`, `np.array_equal`);
the group-end sums equal the numpy restatement of tests/match_metric_ref.py (itself pinned against `match_metric` in
tests/test_match_metric_host.py).  Every generated case is small: at most ~5 000 rows on the host side."""
import functools
import io

import numpy as np
import pytest

import match_metric_ref as mm
from helpers import METRIC_CANARY as CANARY
from helpers import check_match_metric_case as _check_case
from helpers import g8_inputs, load
from helpers import match_metric_raw as _raw
from helpers import match_metric_table_result as _device

pytestmark = pytest.mark.gpu

@pytest.mark.parametrize("case", range(4))
def test_goldens(gpu, case):
    from vsc2022_amd.vsc.metrics import Match, MatchTable

    fx = load("g7_metrics")

    def rows(arr):
        return MatchTable.from_matches([Match(f"Q{int(a):06d}", f"R{int(b):06d}", *(float(x) for x in rest)) for a, b, *rest in arr])

    gt, pred = rows(fx[f"c{case}_gt"]), rows(fx[f"c{case}_pred"])
    got = _device(gt, pred)
    assert mm.same(got, mm.host_metric(gt, pred))
    assert abs(got[0] - float(fx[f"c{case}_segment_ap"])) < 1e-12
    assert np.allclose(got[1], fx[f"c{case}_curve_p"], atol=1e-12) and np.allclose(got[2], fx[f"c{case}_curve_r"], atol=1e-12)


def test_golden_end_to_end_rows(gpu):
    from vsc2022_amd.vsc.metrics import Match, MatchTable, match_metric_table

    fx = load("g6_end_to_end")
    gt = MatchTable.from_matches([Match(str(q), str(r), 1.0, *row) for q, r, row in zip(fx["gt_q"], fx["gt_r"], fx["gt_rows"])])
    pred = MatchTable.from_matches([Match(str(q), str(r), row[0], *row[1:]) for q, r, row in
                                    zip(fx["match_m_q"], fx["match_m_r"], fx["match_m_rows"])])
    # (the fixture stores rows as float64 while the reference accumulated np.float32 timestamps: test_host_logic's 1e-6)
    assert abs(match_metric_table(gt, pred).ap - float(fx["segment_ap"])) < 1e-6
    assert mm.same(_device(gt, pred), mm.host_metric(gt, pred))


@pytest.mark.parametrize("how", mm.SCORES)
@pytest.mark.parametrize("shape", range(len(mm.SHAPES)))
def test_coarse_family(gpu, shape, how):
    n_pred, n_gt, n_pairs = mm.SHAPES[shape]
    gt, pred = mm.coarse_case(shape, n_pairs, n_pred, n_gt, how)
    if how == "equal" and n_pairs > 1:
        assert len(set(pred.score)) == 1 and len(set(zip(pred.query_id, pred.ref_id))) > 1  # one group that spans the pairs
    _check_case(gt, pred)


@pytest.mark.parametrize("born32", [False, True], ids=["float64", "float32-born"])
@pytest.mark.parametrize("how", mm.SCORES)
@pytest.mark.parametrize("shape", range(len(mm.SHAPES)))
def test_fine_family(gpu, shape, how, born32):
    n_pred, n_gt, n_pairs = mm.SHAPES[shape]
    gt, pred = mm.fine_case(mm.FINE_SEEDS[shape], n_pairs, n_pred, n_gt, how, born32=born32)
    if born32:
        assert np.array_equal(pred.query_start, pred.query_start.astype(np.float32).astype(np.float64))
    ap = _check_case(gt, pred)
    assert 0.2 < ap < 0.95, ap  # not a comparison of zeros


def test_zero_length_predictions_that_are_not_ranked_first(gpu):
    gt, pred = mm.coarse_case(5, 4, 7, 2, "distinct", zero_length=True)
    points = pred.query_start == pred.query_end
    assert points.any() and pred.score[points].max() < pred.score[~points].min()
    _check_case(gt, pred)


def test_float32_tables_are_scored_in_float64(gpu):
    import dataclasses

    gt, pred = mm.fine_case(3, 5, 3, 2, "distinct", born32=True)
    f32 = {f: getattr(pred, f).astype(np.float32) for f in ("query_start", "query_end", "ref_start", "ref_end")}
    pred32 = dataclasses.replace(pred, score=pred.score.astype(np.float32), **f32)
    assert mm.same(_device(gt, pred32), mm.host_metric(gt, pred32))


def test_no_predictions_and_sides_without_the_other(gpu):
    from vsc2022_amd.vsc.metrics import match_metric_table

    gt, pred = mm.coarse_case(1, 6, 2, 1, "alphabet")
    none = pred.take(np.zeros(0, dtype=np.int64))
    res = match_metric_table(gt, none)
    assert res.ap == 0.0 and len(res.pr_curve.scores) == 0
    assert mm.same(_device(gt, none), mm.host_metric(gt, none))
    # ... and the entry point itself with n_pred = 0 (cap = 0): only the ground truth's lengths are produced
    from vsc2022_amd import _lib

    gp, pp, n_pairs, n_gt_pairs = mm.pair_ordinals(gt, none)
    ref = mm.group_sums(gp, mm.times_of(gt), pp, none.score, mm.times_of(none), n_pairs, n_gt_pairs)
    for device_mem in (False, True):
        rc, n_groups, scores, sums, gt_len, stats = _raw(gt, none, device_mem)
        assert rc == _lib.VSC_OK and n_groups == 0 and len(ref[0]) == 0, _lib.lib().vsc_last_error()
        assert np.array_equal(gt_len, ref[2]) and (gt_len > 0).all()
        assert (scores == CANARY).all() and (sums == CANARY).all()
        assert stats[:4].tolist() == [n_pairs, 0, 0, 0]
    # ground-truth-only and prediction-only pairs are part of every family (pairs 2, 5, ... / 1, 4, ...): say so
    gt_pairs, pred_pairs = set(zip(gt.query_id, gt.ref_id)), set(zip(pred.query_id, pred.ref_id))
    assert gt_pairs - pred_pairs and pred_pairs - gt_pairs and gt_pairs & pred_pairs


def test_an_area_that_underflows_leaves_the_segment_asleep(gpu):
    """Widths of 1e-200 on both axes: the area is 0.0 in double and the host says "no overlap"; `w > 0 && h > 0` would
    wake the segment and add 1e-200 to the intersection.  Widths of 1e-100 (area 1e-200 > 0) are the control."""
    for eps, asleep in ((1e-200, True), (1e-100, False)):
        assert (eps * eps == 0.0) == asleep
        gt = mm.table([(0, 1.0, -eps, eps, -eps, eps), (1, 1.0, 5.0, 6.0, 5.0, 6.0)])
        pred = mm.table([(0, 0.9, 0.0, 2 * eps, 0.0, 2 * eps), (1, 0.8, 5.5, 7.0, 5.5, 7.0)])
        assert mm.same(_device(gt, pred), mm.host_metric(gt, pred))
        rc, n_groups, scores, sums, _, _ = _raw(gt, pred)
        assert n_groups == 2 and sums[0, 2] == 2 * eps
        assert sums[0, 0] == (0.0 if asleep else eps) and sums[0, 1] == sums[0, 0]


def test_a_pair_beyond_the_lds_budget_runs_from_hbm(gpu):
    rng = np.random.default_rng(11)
    gt, pred = mm.fine_case(21, 1, 1500, 40, "distinct")
    small_gt, small_pred = mm.fine_case(22, 3, 2, 1, "distinct")
    shift = lambda t, k: mm.table([(int(r[1:]) + k, s, a, b, c, d) for r, s, a, b, c, d in
                                   zip(t.ref_id, t.score, t.query_start, t.query_end, t.ref_start, t.ref_end)])
    from vsc2022_amd.vsc.metrics import MatchTable

    gt, pred = MatchTable.concat([shift(small_gt, 10), gt]), MatchTable.concat([shift(small_pred, 10), pred])
    pred = pred.take(rng.permutation(len(pred)))
    assert 0.2 < _check_case(gt, pred, want_hbm=True, restatement=False) < 0.95  # (against the host: the restatement's
    # plain loops take seconds at 1 500 prefixes)


@pytest.mark.parametrize("n_pred, hbm", [(300, False), (301, True)], ids=["320 rows", "321 rows"])
def test_the_edge_of_the_lds_budget(gpu, n_pred, hbm):
    """One pair of 20 segments and 300 / 301 predictions: 320 rows are the last that fit LDS, 321 the first on the slab."""
    gt, pred = mm.fine_case(31, 1, n_pred, 20, "distinct")
    assert len(gt) + len(pred) == 320 + hbm
    _check_case(gt, pred, want_hbm=hbm)


def test_a_pair_beyond_the_documented_bound_is_refused(gpu):
    from vsc2022_amd import _lib
    from vsc2022_amd.vsc.metrics import match_metric_table

    gt, pred = mm.coarse_case(3, 1, _lib.METRIC_MAX_PAIR_ROWS - 1, 2, "equal")
    assert len(gt) + len(pred) == _lib.METRIC_MAX_PAIR_ROWS + 1 and len(set(pred.ref_id)) == 1
    rc, _, scores, sums, _, _ = _raw(gt, pred)
    assert rc == _lib.VSC_ERR_INVALID and b"VSC_METRIC_MAX_PAIR_ROWS" in _lib.lib().vsc_last_error()
    assert (scores == CANARY).all() and (sums == CANARY).all()
    with pytest.raises(ValueError):
        match_metric_table(gt, pred)
    small_gt, small_pred = mm.coarse_case(3, 2, 5, 2, "equal")
    assert mm.same(_device(small_gt, small_pred), mm.host_metric(small_gt, small_pred))  # ... and the next call is right


def test_errors(gpu):
    import dataclasses

    from vsc2022_amd.vsc.metrics import Match, match_metric, match_metric_table

    gt, pred = mm.coarse_case(2, 5, 3, 1, "distinct")

    def with_(table, field, k, value):
        col = getattr(table, field).copy()
        col[k] = value
        return dataclasses.replace(table, **{field: col})

    bad_pred = [with_(pred, "score", 4, np.nan), with_(pred, "score", 0, np.inf), with_(pred, "ref_end", 2, np.nan),
                with_(pred, "query_end", 3, pred.query_start[3] - 0.25)]
    bad_gt = [with_(gt, "ref_end", 1, gt.ref_start[1] - 0.25), with_(gt, "query_start", 0, -np.inf)]
    for g, p in [(gt, b) for b in bad_pred] + [(b, pred) for b in bad_gt]:
        with pytest.raises(ValueError):
            match_metric_table(g, p)
    empty_gt = gt.take(np.zeros(0, dtype=np.int64))
    with pytest.raises(ZeroDivisionError):
        match_metric_table(empty_gt, pred)
    with pytest.raises(ZeroDivisionError):  # the host over Python floats (numpy scalars would only warn and yield nan)
        match_metric([], [Match(m.query_id, m.ref_id, *(float(x) for x in m[2:])) for m in pred.to_matches()])
    assert mm.same(_device(gt, pred), mm.host_metric(gt, pred))  # ... and the next call is right


def test_a_wrong_pair_ordinal_is_refused_and_the_outputs_stay_untouched(gpu):
    from vsc2022_amd import _lib

    gt, pred = mm.coarse_case(4, 5, 65, 2, "alphabet")
    spoils = {"prediction == n_pairs": lambda ins: ins[2].__setitem__(7, 1 << 20), "prediction -1": lambda ins: ins[2].__setitem__(0, -1),
              "ground truth -5": lambda ins: ins[0].__setitem__(1, -5), "ground truth beyond": lambda ins: ins[0].__setitem__(0, 12345)}
    for device_mem in (False, True):
        for name, spoil in spoils.items():
            rc, _, scores, sums, _, _ = _raw(gt, pred, device_mem, spoil=spoil)
            assert rc == _lib.VSC_ERR_INVALID, name
            assert (scores == CANARY).all() and (sums == CANARY).all(), name
            with pytest.raises(ValueError):
                _lib.check(rc)
    rc, n_groups, scores, sums, _, _ = _raw(gt, pred)
    assert rc == _lib.VSC_OK and n_groups == len(set((pred.score + 0.0).tolist()))
    rc, n_again, scores, sums, _, _ = _raw(gt, pred, cap=n_groups - 1)
    assert rc == _lib.VSC_ERR_CAPACITY and n_again == n_groups and (scores == CANARY).all() and (sums == CANARY).all()


def test_two_runs_and_both_memory_kinds_give_the_same_bits(gpu):
    from vsc2022_amd import _lib

    gt, pred = mm.fine_case(8, 4, 129, 33, "alphabet")
    runs = [_raw(gt, pred, device_mem) for device_mem in (False, False, True, True)]
    for rc, n_groups, scores, sums, gt_len, stats in runs:
        assert rc == _lib.VSC_OK and n_groups == runs[0][1] > 1
        for a, b in zip((scores, sums, gt_len), runs[0][2:5]):
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_the_stage_times_are_reported_while_the_accounting_is_on(gpu):
    from vsc2022_amd import _lib

    L = _lib.lib()
    gt, pred = mm.coarse_case(4, 5, 65, 2, "alphabet")
    assert (_raw(gt, pred)[5][4:] == 0).all()
    _lib.check(L.vsc_aux_profile(1))
    try:
        rc, _, _, _, _, stats = _raw(gt, pred)
    finally:
        _lib.check(L.vsc_aux_profile(0))
    assert rc == _lib.VSC_OK and (stats[4:7] > 0).all() and stats[7] == 0  # microseconds: sorts, pair kernels, ordered sums


def test_evaluate_matching_track_and_the_cli_line(gpu, tmp_path, capsys):
    from vsc2022_amd.cli import matching_eval
    from vsc2022_amd.vsc.metrics import evaluate_matching_track

    gt, pred = mm.fine_case(9, 40, 3, 2, "distinct")
    gt_file, pred_file = str(tmp_path / "gt.csv"), str(tmp_path / "matches.csv")
    gt.write_csv(gt_file)
    pred.write_csv(pred_file)
    host, dev = evaluate_matching_track(gt_file, pred_file), evaluate_matching_track(gt_file, pred_file, on_device=True)
    for a, b in ((host.segment_ap, dev.segment_ap), (host.pairwise_micro_ap, dev.pairwise_micro_ap)):
        assert a.ap == b.ap and a.simple_ap == b.simple_ap
        for f in ("precisions", "recalls", "scores"):
            assert np.array_equal(getattr(a.pr_curve, f), getattr(b.pr_curve, f))
    assert 0.2 < host.segment_ap.ap < 0.95
    lines = []
    for flags in ([], ["--on_device"]):
        matching_eval.main(["--predictions", pred_file, "--ground_truth", gt_file] + flags)
        lines.append(capsys.readouterr().out)
    assert lines[0] == lines[1] and lines[0].startswith("Matching track segment AP: 0.")


@functools.lru_cache(maxsize=None)
def _g8():
    from vsc2022_amd import synth
    from vsc2022_amd.vsc.index import VideoFeature

    q, r, noise, gts, _ = g8_inputs()
    return synth.to_video_features(q, VideoFeature), synth.to_video_features(r, VideoFeature), gts


def test_segment_ap_of_rows_still_in_hbm(gpu):
    from vsc2022_amd import engine
    from vsc2022_amd.vsc.index import VideoLayout
    from vsc2022_amd.vsc.metrics import Match, MatchTable, match_metric_table

    queries, refs, gts = _g8()

    def flat(videos_):
        layout = VideoLayout(videos_)
        return VideoLayout.features(videos_), layout.offsets, np.concatenate([v.timestamps for v in videos_], axis=0), layout.video_ids

    (qf, q_off, q_ts, q_ids), (rf, r_off, r_ts, r_ids) = flat(queries), flat(refs)
    m = engine.DeviceMatcher(rf, r_off, r_ts=r_ts)
    m.set_queries(qf, q_off, q_ts=q_ts)
    res = m.match(rows=True)
    assert res.n_matches >= 10
    rows = [Match(g.query_id, g.ref_id, 1.0, g.query_start, g.query_end, g.ref_start, g.ref_end) for g in gts]
    gt = MatchTable.from_matches(rows)
    # + a ground-truth pair that is no candidate, and one whose query video the matcher has never seen
    extra = MatchTable.from_matches([Match(q_ids[0], r_ids[-1], 1.0, 0.0, 3.0, 1.0, 4.0), Match("Q999999", r_ids[0], 1.0, 0.0, 2.0, 0.0, 2.0)])
    for truth in (gt, MatchTable.concat([gt.take(np.arange(3)), extra, gt.take(np.arange(3, len(gt)))])):
        got = m.segment_ap(res, truth, q_ids, r_ids)
        want = match_metric_table(truth, m.match_table(res, q_ids, r_ids))
        assert got.ap == want.ap and 0.0 < got.ap < 1.0
        for f in ("precisions", "recalls", "scores"):
            assert np.array_equal(getattr(got.pr_curve, f), getattr(want.pr_curve, f))
    assert m.last_metric_stats[1] == 0 and m.last_metric_stats[2] == res.n_matches
    with pytest.raises(ValueError, match="rows=True"):
        m.segment_ap(m.match(), gt, q_ids, r_ids)
