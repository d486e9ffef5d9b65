"""No GPU: the restatement of the segment AP that csrc/metric.hip implements (tests/match_metric_ref.py) is `match_metric`
bit for bit, and the host-side pieces of the table route -- `MatchTable.read_csv`, the pair ordinals, `pairwise_ap_table`,
the vectorised tail and what it raises -- are the per-row routes' values."""
import io
import warnings

import numpy as np
import pytest

import match_metric_ref as mm
from helpers import load


def _g7(case):
    from vsc2022_amd.vsc.metrics import Match, MatchTable

    fx = load("g7_metrics")

    def rows(arr):
        return [Match(f"Q{int(a):06d}", f"R{int(b):06d}", *(float(x) for x in rest)) for a, b, *rest in arr]

    return MatchTable.from_matches(rows(fx[f"c{case}_gt"])), MatchTable.from_matches(rows(fx[f"c{case}_pred"])), fx


def _cases():
    for si, (n_pred, n_gt, n_pairs) in enumerate(mm.SHAPES):
        for how in mm.SCORES:
            yield ("coarse", si, how), lambda si=si, a=(n_pairs, n_pred, n_gt), how=how: mm.coarse_case(si, *a, how)
            for born32 in (False, True):
                yield ("fine32" if born32 else "fine", si, how), \
                    lambda si=si, a=(n_pairs, n_pred, n_gt), how=how, b=born32: mm.fine_case(mm.FINE_SEEDS[si], *a, how, born32=b)
    yield ("coarse-zero-length", 0, "distinct"), lambda: mm.coarse_case(5, 4, 7, 2, "distinct", zero_length=True)


@pytest.mark.parametrize("case", range(4))
def test_restatement_is_match_metric_on_the_goldens(case):
    gt, pred, fx = _g7(case)
    got = mm.metric(gt, pred)
    assert mm.same(got, mm.host_metric(gt, pred))
    assert abs(got[0] - float(fx[f"c{case}_segment_ap"])) < 1e-12


def test_restatement_is_match_metric_on_the_generated_families():
    raised, n = 0, 0
    for name, make in _cases():
        gt, pred = make()
        try:
            want = mm.host_metric(gt, pred)
        except (ZeroDivisionError, ValueError):
            raised += 1
            continue
        n += 1
        assert mm.same(mm.metric(gt, pred), want), name
        if name[0].startswith("fine"):
            assert 0.2 < want[0] < 0.95, (name, want[0])  # not a comparison of zeros
    assert raised == 0 and n == 9 * len(mm.SHAPES) + 1  # no case is lost to a host that raised


def test_zero_length_predictions_below_the_first_rank_are_covered():
    gt, pred = mm.coarse_case(5, 4, 7, 2, "distinct", zero_length=True)
    points = pred.query_start == pred.query_end
    assert points.any() and pred.score[points].max() < pred.score[~points].min()


def test_read_csv_is_from_matches_of_read_csv():
    from vsc2022_amd.vsc.metrics import Match, MatchTable

    gt, pred = mm.fine_case(3, 5, 3, 2, "alphabet")
    text = io.StringIO()
    pred.write_csv(text)
    numbered = "query_id,ref_id,score,query_start,query_end,ref_start,ref_end\n7,12,1,0,10,20,30\n8,3,2,5,6,7,8\n"
    shuffled = "ref_end,ref_id,query_id,score,query_start,query_end,ref_start\n3.5,R000001,Q000002,0.25,1.0,2.0,3.0\n"
    header = "query_id,ref_id,score,query_start,query_end,ref_start,ref_end\n"
    for body in (text.getvalue(), numbered, shuffled, header):
        for is_gt in (False, True):
            got = MatchTable.read_csv(io.StringIO(body), is_gt=is_gt)
            want = MatchTable.from_matches(Match.read_csv(io.StringIO(body), is_gt=is_gt))
            assert len(got) == len(want)
            for f in ("query_id", "ref_id", "score", "query_start", "query_end", "ref_start", "ref_end", "pair", "boxes"):
                a, b = getattr(got, f), getattr(want, f)
                assert a.dtype == b.dtype and a.shape == b.shape and a.tolist() == b.tolist(), (f, is_gt)
            assert [type(x) for x in got.query_id] == [type(x) for x in want.query_id]
    assert MatchTable.read_csv(io.StringIO(numbered)).query_id.tolist() == ["Q000007", "Q000008"]
    with pytest.raises(AssertionError):
        MatchTable.read_csv(io.StringIO(header + "R000001,R000001,1,0,1,0,1\n"))
    with pytest.raises(AssertionError):
        MatchTable.read_csv(io.StringIO(header + "Q000001,R000001,,0,1,0,1\n"))


def test_pair_ordinals_are_first_appearance_ground_truth_first():
    from vsc2022_amd.vsc.metrics import pair_ordinals

    for gt, pred in (mm.coarse_case(2, 9, 3, 2, "alphabet"), mm.fine_case(1, 257, 2, 1, "distinct")):
        got = pair_ordinals(gt, pred)
        want = mm.pair_ordinals(gt, pred)
        assert all(np.array_equal(a, b) for a, b in zip(got[:2], want[:2])) and got[2:] == want[2:]
        assert got[0].dtype == np.int32 and got[3] == len(set(zip(gt.query_id, gt.ref_id))) and got[3] < got[2]
    # the same query video with two references, the same reference with two queries: four pairs
    gt = mm.table([(0, 1.0, 0, 1, 0, 1)])
    pred = mm.table([(1, 0.5, 0, 1, 0, 1), (0, 0.4, 0, 1, 0, 1), (8, 0.3, 0, 1, 0, 1), (1, 0.2, 0, 1, 0, 1)])
    assert pair_ordinals(gt, pred)[1].tolist() == [1, 0, 2, 1]


def _same_ap(a, b):
    return a.ap == b.ap and a.simple_ap == b.simple_ap and all(
        np.array_equal(getattr(a.pr_curve, f), getattr(b.pr_curve, f)) for f in ("precisions", "recalls", "scores"))


def test_pairwise_ap_table_is_average_precision():
    from vsc2022_amd.vsc.metrics import CandidatePair, average_precision, pairwise_ap_table

    def host(gt, pred):
        return average_precision(CandidatePair.from_matches(gt.to_matches()), CandidatePair.from_matches(pred.to_matches()))

    for case in range(4):
        gt, pred, fx = _g7(case)
        got = pairwise_ap_table(gt, pred)
        assert _same_ap(got, host(gt, pred))
        assert abs(got.ap - float(fx[f"c{case}_uap"])) < 1e-12 and abs(got.simple_ap - float(fx[f"c{case}_simple_ap"])) < 1e-12
    tables = [mm.coarse_case(3, 40, 3, 1, how) for how in mm.SCORES]          # ties, -0.0 / 0.0, negative scores
    tables.append(mm.fine_case(4, 257, 2, 1, "distinct"))
    negative = mm.coarse_case(6, 30, 2, 1, "distinct")
    negative[1].score[:] -= 0.75                                               # most pairs' best score floors at 0.0
    tables.append(negative)
    for gt, pred in tables:
        assert _same_ap(pairwise_ap_table(gt, pred), host(gt, pred))
    assert (negative[1].score < 0).sum() > 20
    gt, pred = tables[0]
    empty = pred.take(np.zeros(0, dtype=np.int64))
    assert _same_ap(pairwise_ap_table(gt, empty), host(gt, empty))


def test_the_tail_raises_what_python_float_arithmetic_raises():
    """The host walk over Python floats (Match.read_csv's values) raises ZeroDivisionError for a divisor of 0.0 and
    ValueError for the square root of a negative product; over numpy scalars its divisions only warn.  The table route's
    tail raises like the former."""
    from vsc2022_amd.vsc.metrics import Match, match_metric, segment_ap_tail

    pred = [Match("Q000001", "R000001", 0.5, 0.0, 1.0, 0.0, 1.0)]
    with pytest.raises(ZeroDivisionError):
        match_metric([], pred)                                                  # no ground truth: length 0.0
    with pytest.raises(ZeroDivisionError):
        match_metric([Match("Q000001", "R000001", 1.0, 0.0, 1.0, 0.0, 1.0)], [pred[0]._replace(query_end=0.0)])  # covers 0.0
    one = np.array([0.5])
    with pytest.raises(ZeroDivisionError):
        segment_ap_tail(one, np.array([[0.0, 0.0, 1.0, 1.0]]), np.zeros(2))
    with pytest.raises(ZeroDivisionError):
        segment_ap_tail(one, np.array([[0.0, 1.0, 0.0, 1.0]]), np.ones(2))
    with pytest.raises(ValueError):
        segment_ap_tail(one, np.array([[-0.5, 1.0, 1.0, 1.0]]), np.ones(2))
    with pytest.raises(ValueError):  # the recall's square root comes before the precision's division
        segment_ap_tail(one, np.array([[-0.5, 1.0, 0.0, 1.0]]), np.ones(2))
    with pytest.raises(ZeroDivisionError):  # the first group in trouble decides
        segment_ap_tail(np.array([0.5, 0.25]), np.array([[0.5, 1.0, 0.0, 1.0], [-0.5, 1.0, 1.0, 1.0]]), np.ones(2))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = segment_ap_tail(np.array([0.5, 0.25]), np.array([[0.5, 0.5, 1.0, 1.0], [1.0, 1.0, 2.0, 2.0]]), np.ones(2))
    assert mm.same((got.ap, got.pr_curve.precisions, got.pr_curve.recalls, got.pr_curve.scores),
                   mm.tail(np.array([0.5, 0.25]), np.array([[0.5, 0.5, 1.0, 1.0], [1.0, 1.0, 2.0, 2.0]]), np.ones(2)))
    assert segment_ap_tail(np.zeros(0), np.zeros((0, 4)), np.zeros(2)).ap == 0.0


def test_the_tail_is_the_loop_on_every_generated_case():
    from vsc2022_amd.vsc.metrics import segment_ap_tail

    for name, make in list(_cases())[::7]:
        gt, pred = make()
        gp, pp, n_pairs, n_gt_pairs = mm.pair_ordinals(gt, pred)
        sums = mm.group_sums(gp, mm.times_of(gt), pp, pred.score, mm.times_of(pred), n_pairs, n_gt_pairs)
        got = segment_ap_tail(*sums)
        assert mm.same((got.ap, got.pr_curve.precisions, got.pr_curve.recalls, got.pr_curve.scores), mm.tail(*sums)), name
