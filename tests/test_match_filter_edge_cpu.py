"""CPU tests (-m "not gpu"): the oracle's match filters PINNED to the reference's own kernels on the planted cases of tests/filter_cases.py - the very
inputs tests/test_match_filter_edge_gpu.py holds the HIP kernels to - and the proof that those cases are not vacuous (computed from the oracle alone).
Everything is bit for bit (tol = 0): both sides evaluate +, -, *, /, sqrt only."""
from collections import Counter

import numpy as np
import pytest

from tests import filter_cases as fc
from tests import ref_api

KABSCH_PARAMS = ((5, 0.0004), (3, 1e-4), (8, 1e-3))          # (min_matches, max_res2): the default and the two other settings the GPU test runs


@pytest.fixture(scope="module")
def kabsch(oracle):
    cases = fc.kabsch_cases()
    allkeys, idx, num_images = fc.pack(cases)
    Kinv = oracle.inverse44(fc.K)
    out = {p: [oracle.filter_matches(allkeys, g, c["dist"], c["n"], Kinv, *p) for c, g in zip(cases, idx)] for p in KABSCH_PARAMS}
    return cases, allkeys, idx, Kinv, out


def test_kabsch_cases_are_not_vacuous(kabsch):
    cases, allkeys, idx, Kinv, out = kabsch
    res = out[KABSCH_PARAMS[0]]
    split = Counter("0" if r[0] == 0 else "25" if r[0] == fc.MAX_FILT else "partial" for r in res)
    per_family = {}
    for c, r in zip(cases, res):
        per_family.setdefault(c["family"], Counter())["0" if r[0] == 0 else "25" if r[0] == fc.MAX_FILT else "partial"] += 1
    print(len(cases), dict(split), {k: dict(v) for k, v in per_family.items()})
    assert split["25"] >= 20 and split["partial"] >= 20 and split["0"] >= 20, split
    removed = 0
    for c, g, (n, kept, _, _) in zip(cases, idx, res):
        addable = fc.greedy_addable(allkeys, g, c["n"])
        removed += n > 0 and set(map(tuple, kept.tolist())) != set(addable[:n])      # not a prefix of what the 5 px rule alone keeps: a removal took place
    assert removed >= 10, removed
    n_nonfinite = 0
    for c, g, (n, kept, _, T) in zip(cases, idx, res):
        if c["family"] == "nonfinite" and not np.isfinite(c["bad_value"]):
            # a key with depth -inf / +inf / NaN among the first ten raw matches: every later fit has NaN residuals (the literal-sort fallback) and the pair ends
            # with 0.  (A depth of 0.0 is a finite point at the camera centre: an ordinary outlier, removed - those cases end with 25.)
            assert c["bad_pos"] < 10 and n == 0 and not np.isfinite(T).all(), c["name"]
            n_nonfinite += 1
        if "gap_case" in c:                           # raw match 1 lies 5.0 px from raw match 0: refused; at the next float above 5.0: kept
            has = tuple(g[1].tolist()) in set(map(tuple, kept.tolist()))
            assert has == (c["gap_case"][0] == "above5") and n >= 5, c["name"]
    assert n_nonfinite == 24
    # the other two settings change outcomes, so they are runs of their own
    for p in KABSCH_PARAMS[1:]:
        assert sum(a[0] != b[0] for a, b in zip(res, out[p])) >= 5, p


def _skip_without_reference():
    if not ref_api.available():
        pytest.skip("oracle/_ref/libbfref.so is absent and /root/reference is not here to build it")


def test_kabsch_filter_oracle_vs_reference_on_planted_cases(kabsch):
    _skip_without_reference()
    cases, allkeys, idx, Kinv, out = kabsch
    for p in KABSCH_PARAMS:
        for c, g, (no, io, do, To) in zip(cases, idx, out[p]):
            nr, ir, dr, Tr = ref_api.filter_matches(allkeys, g, c["dist"], c["n"], Kinv, *p)
            assert no == nr, (c["name"], p, no, nr)
            assert np.array_equal(io, ir) and np.array_equal(do.view(np.uint32), dr.view(np.uint32)), (c["name"], p)
            fo, fr = np.isfinite(To), np.isfinite(Tr)
            assert np.array_equal(fo, fr) and np.array_equal(To[fo].view(np.uint32), Tr[fr].view(np.uint32)), (c["name"], p, To, Tr)


def test_surface_area_oracle_vs_reference_on_planted_cases(oracle):
    _skip_without_reference()
    cases = fc.area_cases()
    allkeys, fidx, num_images = fc.pack(cases, "fidx")
    Kinv = oracle.inverse44(fc.K)
    cur = num_images - 1
    ref = ref_api.RefSiftManager(num_images, fc.MAX_KEYS)
    ref.set_keys(allkeys)
    flips = verdicts = 0
    seen = set()
    for p, (c, g) in enumerate(zip(cases, fidx)):
        n = len(g)
        _, areas = oracle.filter_surface_area(allkeys, g, Kinv)
        thresholds = [np.float32(0.032)]
        a = np.float32(max(areas)) if np.isfinite(areas).all() else None
        if a is not None:
            thresholds += [a, np.nextafter(a, np.float32(np.inf))]
        for k, thr in enumerate(thresholds):
            expect, _ = oracle.filter_surface_area(allkeys, g, Kinv, float(thr))
            if k:
                assert expect == (k == 1), (c["name"], float(a), float(thr))      # survives at the area, dropped at the next float
                flips += 1
            ref.set_filtered(p, n, g, np.zeros(n, np.float32), np.eye(4), np.eye(4))
            ref.filter_surface_area(cur, p, p + 1, Kinv, float(thr))
            assert (ref.filtered(p)[0] > 0) == expect, (c["name"], areas, float(thr))
            verdicts += 1
            if k == 0:
                seen.add((c["family"], expect))
    assert flips >= 60 and verdicts >= 100
    assert {(k, False) for k in ("collinear", "squeezed")} <= seen and ("spread", True) in seen and ("coplanar", True) in seen and ("nonfinite", True) in seen


_DENSE = {}


def _dense(oracle, geom):
    """frames, transforms and the oracle's cache frames (previous, current, no valid depth) of one cache size, computed once"""
    if "in" not in _DENSE:
        frames, Kin = fc.dense_inputs()
        _DENSE["in"] = (frames, Kin, fc.dense_transforms(frames))
    frames, Kin, transforms = _DENSE["in"]
    if geom not in _DENSE:
        W, H = geom
        _DENSE[geom] = [oracle.cache_store_frame(frames[i][0], frames[i][1], W, H, Kin) for i in (0, 1, 3)]
    return fc.cache_intrinsics(Kin, *geom), transforms, _DENSE[geom]


@pytest.mark.parametrize("geom", fc.DENSE_GEOMETRIES, ids=lambda g: "%dx%d" % g)
def test_dense_cases_are_not_vacuous(oracle, geom):
    W, H = geom
    Kc, transforms, of = _dense(oracle, geom)
    verdicts = set()
    for name, T in transforms:
        ok, err, corr = oracle.dense_verify(of[0], of[1], W, H, Kc, T)
        print(geom, name, ok, err, corr)
        assert np.isfinite(err) and err > 0 and corr > 0, (geom, name, err, corr)
        verdicts.add(ok)
        for et, ct, expect in fc.dense_flips(err, corr, ok):
            assert oracle.dense_verify(of[0], of[1], W, H, Kc, T, err_thresh=et, corr_thresh=ct)[0] == expect, (geom, name, err, corr, et, ct)
    assert verdicts == {True, False}, geom              # both verdicts occur at this cache size
    ok, err, corr = oracle.dense_verify(of[0], of[2], W, H, Kc, transforms[0][1], err_thresh=10.0, corr_thresh=0.0)
    assert not ok and np.isnan(err) and corr == 0.0      # no valid depth in the second frame: err = 0 / 0, rejected whatever the thresholds


@pytest.mark.parametrize("geom", fc.DENSE_GEOMETRIES, ids=lambda g: "%dx%d" % g)
def test_dense_verify_oracle_vs_reference_at_every_cache_size(oracle, geom):
    _skip_without_reference()
    W, H = geom
    Kc, transforms, of = _dense(oracle, geom)
    ref = ref_api.RefSiftManager(4, 64)
    for i in range(3):
        ref.set_cached_frame(i, of[i])
    for name, T in transforms:
        ok, err, corr = oracle.dense_verify(of[0], of[1], W, H, Kc, T)
        for et, ct, expect in fc.dense_flips(err, corr, ok):
            ref.set_filtered(0, 7, T=T, Tinv=oracle.inverse44(T))
            ref.filter_dense_verify(1, 0, 2, W, H, Kc, err_thresh=et, corr_thresh=ct)
            assert (ref.filtered(0)[0] > 0) == expect, (geom, name, err, corr, et, ct)
    T = transforms[0][1]
    ref.set_filtered(0, 7, T=T, Tinv=oracle.inverse44(T))
    ref.filter_dense_verify(2, 0, 3, W, H, Kc, err_thresh=10.0, corr_thresh=0.0)
    assert ref.filtered(0)[0] == 0
