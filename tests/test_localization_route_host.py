"""Host only: the pure-Python pieces of the localisation classes' one batch route (vsc/baseline/localization.py) on a
hand-built box table -- the box table -> `Match` conversion, and the splice of the pairs a kernel hands back, through
`localize_all` and `localize_table` alike with the launch, the match-rows stage and the reference's route stubbed."""
import numpy as np
import pytest

from vsc2022_amd.vsc.baseline import localization as L
from vsc2022_amd.vsc.index import VideoFeature
from vsc2022_amd.vsc.metrics import CandidatePair, Match, MatchTable

f32 = np.float32


def _video(vid, frames, t0, step):
    """Frame i lasts from t0 + i * step to t0 + (i + 1) * step (float32 pairs, every value exact)."""
    start = t0 + step * np.arange(frames, dtype=np.float32)
    return VideoFeature(video_id=vid, timestamps=np.stack([start, start + f32(step)], axis=1), feature=np.zeros((frames, 4), np.float32))


QUERIES = [_video("Q0", 6, 0.0, 0.5), _video("Q1", 5, 0.0, 0.5)]
REFS = [_video("R0", 8, 10.0, 1.0), _video("R1", 4, 100.0, 1.0)]
CANDS = [CandidatePair("Q0", "R0", 0.9), CandidatePair("Q1", "R0", 0.8), CandidatePair("Q0", "R1", 0.7)]


def _fill(table, status=(0, 0, 0)):
    """n_boxes = [2, 0, 1]; the slots beyond a pair's count hold corners far outside every video."""
    table.n_boxes[:] = [2, 0, 1]
    table.boxes[:] = 1 << 30
    table.boxes[0, 0], table.boxes[0, 1], table.boxes[2, 0] = [0, 1, 2, 3], [3, 4, 5, 7], [1, 0, 4, 2]
    table.box_max[:] = -7.0
    table.box_max[0, 0], table.box_max[0, 1], table.box_max[2, 0] = 0.75, 0.5, 0.25
    table.status[:] = status
    return table


# what the per-pair, per-box loop gives for that table with the kernel's score: box [x1, y1, x2, y2] runs from the start of
# query frame x1 to the end of query frame x2, and from the start of reference frame y1 to the end of reference frame y2
ROWS = [Match("Q0", "R0", f32(0.75), f32(0.0), f32(1.5), f32(11.0), f32(14.0)),
        Match("Q0", "R0", f32(0.5), f32(1.5), f32(3.0), f32(14.0), f32(18.0)),
        Match("Q0", "R1", f32(0.25), f32(0.5), f32(2.5), f32(100.0), f32(103.0))]


class _Stubbed(L.VCSLLocalizationMaxSim):
    """The class without a device: a launch that writes the hand-built table, a reference route that knows two rows for
    pair 1, and the match-rows stage restated on the host."""

    def __init__(self, status=(0, 0, 0), device_route=True):
        self.queries, self.refs = {v.video_id: v for v in QUERIES}, {v.video_id: v for v in REFS}
        self._q_ordinal, self._r_ordinal = {"Q0": 0, "Q1": 1}, {"R0": 0, "R1": 1}
        self.status, self.device_route, self.calls = status, device_route, []

    def _device_route(self):
        return self._launch_stub if self.device_route else None

    def _pair_ordinals(self, candidates):
        self.calls.append("ordinals")
        return super()._pair_ordinals(candidates)

    def _launch_stub(self, candidates, table):
        self.calls.append("launch")
        assert table.pair_q.tolist() == [0, 1, 0] and table.pair_r.tolist() == [0, 0, 1]
        assert not table.n_boxes.any() and not table.boxes.any() and not table.box_max.any() and not table.status.any()
        _fill(table, self.status)

    def _device_rows(self, candidates, table):
        self.calls.append("rows")
        pair = np.repeat(np.arange(len(candidates)), table.n_boxes)
        slot = [b for n in table.n_boxes for b in range(n)]
        matches = L.box_matches(candidates, table.n_boxes, table.boxes, table.box_max, self._to_match, self._fused_score)
        return MatchTable.from_matches(matches, pair=pair, boxes=table.boxes[pair, slot])

    def _reference_rows(self, candidates, pair_index):
        self.calls.append(("reference", list(pair_index)))
        for k, candidate in zip(pair_index, candidates):
            assert candidate is CANDS[k]
            if k == 1:
                for box, score in (((0, 0, 1, 1), 0.125), ((2, 3, 4, 5), 0.0625)):
                    yield k, self._to_match(candidate, box)._replace(score=f32(score)), box


PAIR_1 = [Match("Q1", "R0", f32(0.125), f32(0.0), f32(1.0), f32(10.0), f32(12.0)),
          Match("Q1", "R0", f32(0.0625), f32(1.0), f32(2.5), f32(13.0), f32(16.0))]


def _same(got, want):
    assert got == want
    assert [[type(v) for v in m] for m in got] == [[type(v) for v in m] for m in want]


def test_box_table_to_matches():
    table = _fill(L.BoxTable.zeros(np.array([0, 1, 0], np.int32), np.array([0, 0, 1], np.int32)))
    assert table.boxes.shape == (3, 16, 4) and table.box_max.shape == (3, 16) and table.unfinished() == []
    loc = _Stubbed()
    got = L.box_matches(CANDS, table.n_boxes, table.boxes, table.box_max, loc._to_match, loc._fused_score)
    _same(got, ROWS)
    # the score hook sees the candidate: the retrieval score, a Python float, stays one
    got = L.box_matches(CANDS, table.n_boxes, table.boxes, table.box_max, loc._to_match, lambda candidate, box_max: candidate.score)
    _same(got, [m._replace(score=s) for m, s in zip(ROWS, (0.9, 0.9, 0.7))])
    assert L.box_matches([], table.n_boxes[:0], table.boxes[:0], table.box_max[:0], loc._to_match, loc._fused_score) == []


def test_unfinished_pair_is_spliced_in_candidate_order():
    want = ROWS[:2] + PAIR_1 + ROWS[2:]
    loc = _Stubbed(status=(0, 1, 0))
    matches = loc.localize_all(CANDS)
    assert loc.calls == ["ordinals", "launch", ("reference", [1])]  # one set of ordinals, one launch, pair 1 handed on
    _same(matches, want)
    loc.calls.clear()
    table = loc.localize_table(CANDS)
    assert loc.calls == ["ordinals", "launch", "rows", ("reference", [1])]
    assert table.pair.tolist() == [0, 0, 1, 1, 2] and table.pair.dtype == np.int64
    assert table.boxes.tolist() == [[0, 1, 2, 3], [3, 4, 5, 7], [0, 0, 1, 1], [2, 3, 4, 5], [1, 0, 4, 2]] and table.boxes.dtype == np.int32
    assert table.score.dtype == np.float32 and table.query_start.dtype == np.float32
    _same(table.to_matches(), matches)
    # the module-level pieces alone: the same list, the same table
    filled = _fill(L.BoxTable.zeros(*loc._pair_ordinals(CANDS)), (0, 1, 0))
    assert filled.unfinished() == [1]
    _same(L.box_matches(CANDS, filled.n_boxes, filled.boxes, filled.box_max, loc._to_match, loc._fused_score, {1: PAIR_1}), want)
    rows = [(1, PAIR_1[0], (0, 0, 1, 1)), (1, PAIR_1[1], (2, 3, 4, 5))]
    device = MatchTable.from_matches(ROWS, pair=[0, 0, 2], boxes=[[0, 1, 2, 3], [3, 4, 5, 7], [1, 0, 4, 2]])
    both = L.splice_rows(device, iter(rows))
    _same(both.to_matches(), want)
    assert both.pair.tolist() == [0, 0, 1, 1, 2]
    assert L.splice_rows(device, iter(())) is device


def test_every_pair_finished_asks_the_reference_route_for_nothing():
    loc = _Stubbed()
    _same(loc.localize_all(CANDS), ROWS)
    _same(loc.localize_table(CANDS).to_matches(), ROWS)
    assert loc.calls == ["ordinals", "launch", ("reference", []), "ordinals", "launch", "rows", ("reference", [])]


def test_without_a_device_route_every_pair_takes_the_reference_route():
    loc = _Stubbed(device_route=False)
    _same(loc.localize_all(CANDS), PAIR_1)
    table = loc.localize_table(CANDS)
    _same(table.to_matches(), PAIR_1)
    assert table.pair.tolist() == [1, 1] and table.boxes.tolist() == [[0, 0, 1, 1], [2, 3, 4, 5]]
    assert loc.calls == [("reference", [0, 1, 2])] * 2  # no ordinals, no launch, no match-rows stage


def test_empty_batches_touch_nothing():
    loc = _Stubbed()
    assert loc.localize_all([]) == [] and loc.localize_all(iter(())) == []
    assert len(loc.localize_table([])) == 0 and loc.localize_table([]).score.dtype == np.float64
    assert loc.calls == []


def test_unknown_id_is_a_key_error_before_the_launch():
    loc = _Stubbed()
    for run in (loc.localize_all, loc.localize_table):
        with pytest.raises(KeyError):
            run(CANDS + [CandidatePair("Q9", "R0", 0.5)])
    assert "launch" not in loc.calls
