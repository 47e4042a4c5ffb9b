"""The unit planners (edgegraph3d_amd/csrc/eg3d_unit_plan.h: plan_seed_units, cut_bounded) without a GPU. They decide how
every eg3d_match_* call is cut into the units its lanes run, and are plain host arithmetic: tests/unitplan/unit_plan_check.cpp
includes the header alone, reads one case from stdin and prints the units. Checked here: the cut of eg3d_match_polyline_sets
on the bound families against sets_cases.units_expected and the declared unit counts (the triples
tests/test_gpu_polyline_sets.py checks on the device), and on fixed inputs the invariants of every planner — the units cover
the range contiguously, each non-empty; no seed unit above 16 384 seeds; a set / item unit above its bound holds one set /
item; one lane and no unit count give the fixed 16 384-seed batches; asking for k units gives at least min(k, e - b)."""
import os
import subprocess

import numpy as np
import pytest

import sets_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED_BATCH = 16384


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("unitplan") / "unit_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "edgegraph3d_amd", "csrc"),
                           os.path.join(ROOT, "tests", "unitplan", "unit_plan_check.cpp"), "-o", exe])
    return exe


def _plan(exe, kind, b, e, prefix, lanes=1, units=0, ramp=0.6, bound=0):
    prefix = np.asarray(prefix, np.int64)
    text = "%s %d %d %d %d %r %d %d\n%s\n" % (kind, b, e, lanes, units, ramp, bound, len(prefix), " ".join(map(str, prefix.tolist())))
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (kind, b, e, out.stderr)
    return [tuple(int(x) for x in line.split()) for line in out.stdout.splitlines()]


def _covers(units, b, e):
    """contiguous from b to e, every unit non-empty (an empty range has no unit)"""
    at = b
    for u0, u1 in units:
        assert u0 == at and u1 > u0, (units[:8], b, e)
        at = u1
    assert at == e, (units[-8:], b, e)


# ---------------------------------------------------------------------------------------------------------------- sets --
@pytest.mark.parametrize("family", ["bound_lo", "bound_hi"])
def test_sets_cut_matches_its_restatement_on_the_bound_families(checker, family):
    case = cases.FAMILIES[family]()
    n, row_off, _ = case.csr()
    V, mx = case.V, case.meta["max_items"]
    assert mx == (cases.MAX_ITEMS_HI if V >= 64 else cases.MAX_ITEMS_LO)
    prefix = row_off[::V]  # prefix(i) = row_off[i * V]: the polyline ids in front of set i
    assert len(prefix) == n + 1 and len(case.units) == 6
    for b, e, declared in case.units:
        units = _plan(checker, "bounded", b, e, prefix, lanes=1, units=0, bound=mx)
        _covers(units, b, e)
        assert len(units) == cases.units_expected(row_off, V, b, e, mx) == declared, (family, b, e, units)
        for u0, u1 in units:
            assert int(prefix[u1] - prefix[u0]) <= mx or u1 - u0 == 1, (family, u0, u1)


# (prefix, bound): an all-empty run; one item above the bound; exactly the bound, and the bound + 1, in two neighbours
BOUNDED_INPUTS = {
    "empty_run": (np.concatenate([[0], np.cumsum([5, 0, 0, 0, 0, 0, 0, 0, 7, 0, 0, 3])]), 8),
    "all_empty": (np.zeros(41, np.int64), 8),
    "one_above": (np.concatenate([[0], np.cumsum([3, 2, 100, 1, 4, 2])]), 10),
    "bound_and_bound_plus_1": (np.concatenate([[0], np.cumsum([6, 4, 1, 6, 5, 1, 10, 11])]), 10),
}


@pytest.mark.parametrize("name", sorted(BOUNDED_INPUTS))
@pytest.mark.parametrize("lanes,units", [(1, 0), (3, 0), (1, 2), (3, 5), (2, 4096)])
def test_bounded_cut_invariants(checker, name, lanes, units):
    prefix, bound = BOUNDED_INPUTS[name]
    n = len(prefix) - 1
    for b, e in ((0, n), (1, n), (0, n - 1), (2, 2), (n // 2, n // 2 + 1)):
        got = _plan(checker, "bounded", b, e, prefix, lanes=lanes, units=units, bound=bound)
        _covers(got, b, e)
        for u0, u1 in got:
            assert int(prefix[u1] - prefix[u0]) <= bound or u1 - u0 == 1, (name, u0, u1)
        assert len(got) >= min(units if units else lanes, e - b), (name, b, e, got)
    if name == "bound_and_bound_plus_1" and lanes == 1 and not units:
        # 6 + 4 = the bound: one unit; 6 + 5 = the bound + 1: two; an item above the bound is never joined to another
        assert _plan(checker, "bounded", 0, 2, prefix, bound=bound) == [(0, 2)]
        assert _plan(checker, "bounded", 3, 5, prefix, bound=bound) == [(3, 4), (4, 5)]
        assert _plan(checker, "bounded", 6, 8, prefix, bound=bound) == [(6, 7), (7, 8)]
        assert _plan(checker, "bounded", 0, 8, prefix, bound=bound) == [(0, 2), (2, 4), (4, 6), (6, 7), (7, 8)]
    if name == "one_above" and lanes == 1 and not units:
        assert _plan(checker, "bounded", 0, 6, prefix, bound=bound) == [(0, 2), (2, 3), (3, 6)]


# --------------------------------------------------------------------------------------------------------------- seeds --
def _tracks(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, np.int64))])


def _skewed(n=4000):
    rest = np.full(n - 1, 2, np.int64)
    return _tracks(np.concatenate([[int(rest.sum())], rest]))  # the first seed carries half of all track entries


# name: (trk_off, b, e, lanes, units, ramp)
SEED_INPUTS = {
    "empty": (_tracks([3, 4, 5]), 1, 1, 3, 0, 0.6),
    "one": (_tracks([3, 4, 5]), 1, 2, 3, 0, 0.6),
    "127_on_3": (_tracks(np.arange(127) % 5 + 2), 0, 127, 3, 0, 0.6),
    "128_on_3": (_tracks(np.arange(128) % 5 + 2), 0, 128, 3, 0, 0.6),
    "129_on_3": (_tracks(np.arange(129) % 5 + 2), 0, 129, 3, 0, 0.6),
    "16384_on_1": (_tracks(np.full(16384, 3)), 0, 16384, 1, 0, 0.6),
    "16385_on_1": (_tracks(np.full(16385, 3)), 0, 16385, 1, 0, 0.6),
    "40000_short_on_3": (_tracks(np.ones(40000)), 0, 40000, 3, 0, 0.6),
    "first_seed_half": (_skewed(), 0, 4000, 3, 0, 0.6),
}


@pytest.mark.parametrize("name", sorted(SEED_INPUTS))
def test_seed_cut_invariants(checker, name):
    trk, b, e, lanes, units, ramp = SEED_INPUTS[name]
    got = _plan(checker, "seeds", b, e, trk, lanes=lanes, units=units, ramp=ramp)
    _covers(got, b, e)
    assert all(u1 - u0 <= SEED_BATCH for u0, u1 in got), name
    if lanes <= 1 and not units:
        assert got == [(s, min(e, s + SEED_BATCH)) for s in range(b, e, SEED_BATCH)], name
    for k in (1, 2, 7, 300):
        asked = _plan(checker, "seeds", b, e, trk, lanes=lanes, units=k, ramp=ramp)
        _covers(asked, b, e)
        assert all(u1 - u0 <= SEED_BATCH for u0, u1 in asked), (name, k)
        assert len(asked) >= min(k, e - b), (name, k, len(asked))
    # what the cases are there for
    if name == "empty":
        assert got == []
    elif name == "one":
        assert got == [(1, 2)]
    elif name == "127_on_3":
        assert len(got) == 1  # under 128 seeds per unit a range is not worth cutting
    elif name in ("128_on_3", "129_on_3"):
        assert len(got) == 1  # (n / 128 = 1 unit; 3 lanes need 384 seeds)
    elif name == "16384_on_1":
        assert got == [(0, 16384)]
    elif name == "16385_on_1":
        assert got == [(0, 16384), (16384, 16385)]
    elif name == "40000_short_on_3":
        # 3 units of shares 1 : 0.6 : 0.36 = 20 408, 12 245 and 7 347 seeds; the first is above the batch bound and cut in two
        assert len(got) == 4 and abs((got[0][1] - got[0][0]) - (got[1][1] - got[1][0])) <= 1, got
    elif name == "first_seed_half":
        # 3 units; the first holds the heavy seed (half the weight) and its share 1 / 1.96 = 51 %: a few dozen seeds more
        assert len(got) == 3 and got[0][0] == 0 and 1 < got[0][1] < 200, got
