"""CPU tests (-m "not gpu"): the planted matcher cases of tests/match_cases.py hold what they are named after (asserted on the oracle alone), and the oracle's
matcher is PINNED to the reference's own (SiftMatchGPU::GetSiftMatch through ref_api.RefSift.match, the path tests/test_ref_pin_cpu.py uses) on those
cases - the very inputs tests/test_match_edge_gpu.py holds k_match to.  Terms of the pin: the same count, the same SET of index pairs (the reference appends
by atomic arrival), distances within 1e-6 (acos: libm there, include/bf_detmath.h here); the tie cases therefore agree on the indices themselves.

Measured times of the emulated reference matcher (one host thread): 0.22 s for a pair of 1024 x 1024 keys, 0.07 s for 1024 x 256, 0.03 s for 300 x 300; all
109 planted pairs together 3.5 s, against 0.6 s for the oracle.  So every case is pinned, the 1024 x 1024 ones included, and the file runs in about ten
seconds."""
import numpy as np
import pytest

from tests import match_cases as mc
from tests import ref_api


def _run(oracle, c, sort=True, **kw):
    return oracle.sift_match(c["prev"], c["cur"], kw.get("dist_max", c["dist_max"]), kw.get("ratio_max", c["ratio_max"]), sort=sort)


@pytest.fixture(scope="module")
def cases():
    return mc.all_cases()


@pytest.fixture(scope="module")
def results(oracle, cases):
    """the oracle's output per case, unsorted (ascending current key) and sorted by distance: computed once, read only"""
    return [(_run(oracle, c, sort=False), _run(oracle, c, sort=True)) for c in cases]


def _by_family(cases, results, family):
    return [(c, r) for c, r in zip(cases, results) if c["family"] == family]


# ------------------------------------------------------------------------------------------------ the cases hold their properties
def test_every_case_returns_exactly_what_it_plants(cases, results):
    """count = the number of expected pairs (beyond 128 where the cap binds); the pairs kept are the expected ones with the 128 lowest current keys, emitted in
    ascending current-key order before the sort; the sorted output is a stable distance sort of that"""
    mc.layouts(cases)                                                   # bounds of every image and every expected index
    for c, ((n, idx, dist), (ns, idxs, dists)) in zip(cases, results):
        en, eidx = mc.expected_output(c, 0, 0)
        assert n == ns == en, (c["name"], n, en)
        assert np.array_equal(idx, eidx), c["name"]
        order = np.argsort(dist, kind="stable")
        assert np.array_equal(idxs, idx[order]) and np.array_equal(dists.view(np.uint32), dist[order].view(np.uint32)), c["name"]


def test_key_count_cases_cover_the_grid_and_match_first_and_last_keys(cases, results):
    kc = _by_family(cases, results, "key_counts")
    assert [(len(c["prev"]), len(c["cur"])) for c, _ in kc] == [(n1, n2) for n2 in mc.KEY_COUNTS_CUR for n1 in mc.KEY_COUNTS_PREV] and len(kc) == 84
    for c, ((n, idx, _), _) in kc + _by_family(cases, results, "strides"):
        n1, n2 = len(c["prev"]), len(c["cur"])
        assert n == min(n1, n2, 100), c["name"]
        rows, cols = set(idx[:, 0].tolist()), set(idx[:, 1].tolist())
        assert n1 - 1 in rows and n2 - 1 in cols, c["name"]            # the last key of both sides: the partial tile, the last slab
        if n >= 2:                                                      # (one partner is all a single-key image allows: it is the last key of the other side)
            assert 0 in rows and 0 in cols, c["name"]
    assert [(c["max_keys"], len(c["prev"]), len(c["cur"])) for c, _ in _by_family(cases, results, "strides")] == \
        [(mk, n1, n2) for mk, counts in mc.STRIDES for n2 in counts for n1 in counts]


def test_cap_cases_bind_where_they_should(cases, results):
    cap = _by_family(cases, results, "cap")
    assert [r[0][0] for _, r in cap] == [m for _, m in mc.CAP_CASES] == [127, 128, 129, 300, 200, 1024]
    for c, ((n, idx, dist), _) in cap:
        assert len(idx) == min(n, 128)
        if n > 128:                                                     # the kept ones are the 128 lowest current keys of the planted set
            assert idx[:, 1].max() < np.sort(c["expect"][:, 1])[128], c["name"]
        assert len(set(dist.view(np.uint32).tolist())) >= 20, c["name"]            # the sort has work to do ... and equal distances (the clamp at 2^18) to keep in order
        assert len(set(dist.view(np.uint32).tolist())) < len(dist), c["name"]


def test_equal_distance_case_has_one_distance(cases, results):
    (c, ((n, idx, dist), (_, idxs, dists))), = _by_family(cases, results, "equal")
    assert n == 100 and len(set(dists.view(np.uint32).tolist())) == 1
    assert np.array_equal(idxs, idx) and (np.diff(idxs[:, 1].astype(np.int64)) > 0).all()         # ascending current key: the tie rule of the sort alone
    assert (np.diff(idxs[:, 0].astype(np.int64)) < 0).any()                                        # (and not ascending previous key)


def test_tie_cases_show_the_traversal_order_rule(cases, results):
    (c125, ((n, idx, dist), _)), (c08, ((n0, _, _), _)) = _by_family(cases, results, "ties")
    assert c125["ratio_max"] == 1.25 and c08["ratio_max"] == 0.8
    assert n == 2 and idx.tolist() == [[129, 50], [70, 64]] and (dist > 0).all()
    assert sorted(c125["lowest_index_rule"]) == [(35, 50), (70, 33)]
    assert n0 == 0


def test_threshold_case_has_distinct_distances_and_a_strict_bound(oracle, cases, results):
    (c, (_, (n, idx, dist))), = _by_family(cases, results, "thresholds")
    assert n == 20 and (np.diff(dist) > 0).all() and dist[0] > 0
    below, at = mc.threshold_variants(c, idx, dist)
    for v, keep in ((below, mc.THRESH_RANK), (at, mc.THRESH_RANK + 1)):
        vn, vidx, vdist = _run(oracle, v)
        assert vn == keep and np.array_equal(vidx, idx[:keep]) and np.array_equal(vdist.view(np.uint32), dist[:keep].view(np.uint32)), v["name"]
        assert np.array_equal(mc.expected_output(v, 0, 0)[1], _run(oracle, v, sort=False)[1])


def test_saturated_keys_swallow_every_match_and_zero_keys_none(cases, results):
    (cz, ((nz, idxz, _), _)), (cs, ((ns, _, _), _)) = _by_family(cases, results, "saturated")
    assert nz == 30 and np.array_equal(idxz, cz["planted"]) and np.array_equal(cs["planted"], cz["planted"])
    assert ns == 0
    for c, want in ((cz, (1, 0)), (cs, (1, 1))):
        for d in (c["prev"], c["cur"]):
            assert ((d == 0).all(axis=1).sum(), (d == 255).all(axis=1).sum()) == want


def test_frame_images_share_partners_pairwise(oracle):
    imgs = mc.frame_images()
    assert tuple(len(d) for d in imgs) == mc.FRAME_COUNTS
    mc.check_bounds(imgs, 1024)
    for cur, prevs in ((5, (0, 2, 3, 4)), (2, (3, 4, 5)), (4, (0, 2, 3)), (3, (4, 5))):
        for p in prevs:
            assert oracle.sift_match(imgs[p], imgs[cur])[0] == min(len(imgs[p]), len(imgs[cur])), (p, cur)


# ------------------------------------------------------------------------------------------------ the oracle against the reference matcher
@pytest.fixture(scope="module")
def ref_sift():
    if not ref_api.available():
        pytest.skip("oracle/_ref/libbfref.so is absent and the reference sources are not here to build it")
    K = np.eye(4, dtype=np.float32); K[0, 0] = K[1, 1] = 100.0; K[0, 2], K[1, 2] = 31.5, 23.5
    return ref_api.RefSift(64, 48, K)                                   # (the detector's image size does not enter the matcher)


def test_oracle_vs_reference_matcher_on_planted_cases(oracle, ref_sift, cases, results):
    """Every planted case: the same count (beyond 128 too: the reference over-counts like the oracle, ProgramCU.cu:1909), the same set of index pairs,
    distances within 1e-6.  The tie cases are among them, so the reference takes (129, 50) and (70, 64) as well: the oracle's tie-break keys are the reference's
    traversal orders.  Where the cap binds the kept pairs are compared too: the serial block emulator runs ColMatch's threads in ascending column order, so its
    atomic arrival order IS ascending current key and it keeps the 128 lowest columns like the oracle (a property of the emulator; on a GPU the reference keeps
    whichever 128 arrive first)."""
    seen = set()
    for c, ((n, idx, dist), _) in zip(cases, results):
        rn, ridx, rdist = ref_sift.match(c["prev"], c["cur"], 0, 0, c["dist_max"], c["ratio_max"])
        assert rn == n, (c["name"], rn, n)
        om = {tuple(i): d for i, d in zip(idx.tolist(), dist.tolist())}
        assert sorted(om) == sorted(map(tuple, ridx.tolist())) and len(ridx) == min(n, mc.MAX_RAW), c["name"]
        assert all(abs(om[tuple(i)] - d) < 1e-6 for i, d in zip(ridx.tolist(), rdist.tolist())), c["name"]
        if c["family"] == "ties":
            assert sorted(map(tuple, ridx.tolist())) == sorted(map(tuple, c["expect"].tolist())), c["name"]
        seen.add(c["family"])
    assert seen == {"key_counts", "cap", "equal", "ties", "thresholds", "saturated", "strides"} and len(cases) == 109
    # the threshold variants: the reference applies dist_max with the same strict `<`
    (c, (_, (n, idx, dist))), = _by_family(cases, results, "thresholds")
    # dist_max is a distance of the ORACLE's; the reference's own acos may put its distance of that one match up to 1e-6 to either side of it, so that match may
    # go either way there; its neighbours in distance are more than 1e-5 away and may not
    k = mc.THRESH_RANK
    assert dist[k] - dist[k - 1] > 1e-5 and dist[k + 1] - dist[k] > 1e-5
    for v in mc.threshold_variants(c, idx, dist):
        rn, ridx, _ = ref_sift.match(v["prev"], v["cur"], 0, 0, v["dist_max"], v["ratio_max"])
        got = set(map(tuple, ridx.tolist()))
        assert rn == len(got) and set(map(tuple, idx[:k].tolist())) <= got <= set(map(tuple, idx[:k + 1].tolist())), v["name"]
