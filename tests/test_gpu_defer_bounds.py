"""Deferred rescoring's two proofs at the inputs that come closest to their error bounds (tests/prefilter_bounds.py,
defer_floor_case and defer_radius_case; held to their purpose on the CPU by test_prefilter_bounds.py).

A pre-filtered batch leaves a candidate's exact score uncomputed when its fp16 score `low` proves the exact score to lie
in (radius, floor]: low > radius + e and low <= floor - e.  The band is coded twice -- `defer_band` of sim_f16p.hip (both
candidate emitters of the fp16 panel kernel) and the fp16 screen of rescore.hip (int8 batches) -- and on random rows,
whose fp16 error is a few per cent of e, a band with half the e, none, or the wrong sign returns the same results.
Here the planted pairs use 0.96 / 0.88 / 0.79 of the bound at D = 64 / 512 / 1000, all in one direction:

  floor case   exact = s just above the floor, low ~0.9 eps below it.  A narrower upper edge defers them, the next event
               is decided without D all the same, and they are missing from the result.
  radius case  exact = s just below the radius, low ~0.9 eps above it.  A narrower lower edge defers them, and the
               re-scoring of D at the end of the search finds pairs that do not pass the radius: the search raises.

Planted pairs lie in full and partial query panels, in interior column tiles and in the last, partial one.  Everything
is compared on integers and fp32 bit patterns: rows, references, score bits, radius and the number of events equal
those of defer = 0 and of the CPU oracle."""
import functools

import numpy as np
import pytest

import prefilter_bounds as pb

pytestmark = pytest.mark.gpu

ROUTES = {
    "f16-panel-64": (dict(prefilter=2, i8=0), 64),
    "f16-panel-512": (dict(prefilter=2, i8=0), 512),
    "i8-screen-64": (dict(prefilter=2, i8=2), 64),
    "i8-screen-512": (dict(prefilter=2, i8=2), 512),
    "i8-screen-1000": (dict(prefilter=2, i8=2), 1000),
}
STATS = ("deferred", "defer_forced", "defer_events_ok", "defer_events_forced")


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def case(side, d):
    """the rows of a case, built once and never modified"""
    c = pb.defer_floor_case(d) if side == "floor" else pb.defer_radius_case(d)
    c.q.setflags(write=False)
    c.r.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def reference(side, d):
    import oracle as orc

    c = case(side, d)
    return orc.global_threshold_search(c.q, c.r, c.K, 0, return_info=True)


def search(route, c, defer):
    from vsc2022_amd.vsc.index import FlatIndex

    idx = FlatIndex(c.d, options={k: float(v) for k, v in dict(ROUTES[route][0], defer=defer).items()})
    idx.profile(True)
    idx.add(c.r)
    i, j, s, radius = idx.global_topk(c.q, c.K)
    st = idx.profile_read(reset=True)
    st["n_rethreshold"] = int(idx.get_option("n_rethreshold"))
    # the intended kernel ran: the int8 pre-filter (whose deferring batches go through the fp16 screen), or the fp16
    # panel kernel alone
    if ROUTES[route][0]["i8"]:
        assert st["i8_launches"] > 0 and idx.get_option("i8_fallbacks") == 0, st
    else:
        assert st["f16_launches"] > 0 and st["i8_launches"] == 0, st
    return (i, j, s, np.float32(radius)), st


def same(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(bits(a[2]), bits(b[2]))
            and bits(a[3]) == bits(b[3]))


def pair_set(i, j):
    return set(zip(np.asarray(i).tolist(), np.asarray(j).tolist()))


def check(route, side, defer):
    """The search with `defer` equals defer = 0 and the oracle; returns its result, its statistics and the case."""
    c = case(side, ROUTES[route][1])
    oi, oj, os_, info = reference(side, c.d)
    want = (oi, oj, os_, np.float32(info["radius"]))
    off, st0 = search(route, c, 0)
    assert same(off, want), (route, side, "defer = 0 differs from the oracle")
    assert all(st0[k] == 0 for k in STATS), st0
    got, st = search(route, c, defer)      # (the radius case: a pair deferred without proof makes this raise)
    assert same(got, want), (route, side, defer, st, len(got[0]), len(want[0]))
    assert st["n_rethreshold"] == st0["n_rethreshold"] == info["n_rethreshold"], (st, st0, info)
    return got, st, c


@pytest.mark.parametrize("defer", [1, 2])
@pytest.mark.parametrize("route", list(ROUTES))
def test_floor_edge_at_the_bound(gpu, orc, route, defer):
    got, st, c = check(route, "floor", defer)
    # the oracle's result: the planted pairs and the plain 1.25 rows, the radius is the decoys' score
    rows, refs = c.pairs("planted", "plain125")
    assert pair_set(got[0], got[1]) == pair_set(rows, refs) and len(got[0]) == 192 + 64
    assert pair_set(*c.planted()) <= pair_set(got[0], got[1])
    assert st["n_rethreshold"] == 2
    # the event at row 32 precedes the floor; the one at row 224 is decided with D left out, and D (the plain 0.875 rows,
    # all of them and nothing else) is never scored
    assert st["defer_events_ok"] >= 1 and st["defer_events_forced"] == 0 and st["defer_forced"] == 0, st
    assert st["deferred"] == len(c.roles["plain0875"][0]) == 192, st


@pytest.mark.parametrize("defer", [1, 2])
@pytest.mark.parametrize("route", list(ROUTES))
def test_radius_edge_at_the_bound(gpu, orc, route, defer):
    got, st, c = check(route, "radius", defer)
    # the oracle's result: the plain rows; no planted pair passes the radius (the +1 decoys' score)
    rows, refs = c.pairs("plain125", "plain1125")
    assert pair_set(got[0], got[1]) == pair_set(rows, refs) and len(got[0]) == 128 + 96
    assert not (pair_set(*c.planted()) & pair_set(got[0], got[1]))
    assert st["n_rethreshold"] == 1
    # no event follows the floor: D (the plain 1.125 rows, all of them and nothing else) is outstanding at the end and
    # re-scored there, and every pair of it passes the radius
    assert st["deferred"] == st["defer_forced"] == len(c.roles["plain1125"][0]) == 96, st
    assert st["defer_events_ok"] == 0 and st["defer_events_forced"] == 0, st
