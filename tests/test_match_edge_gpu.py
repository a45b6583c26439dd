"""GPU tests (-m gpu): k_match and k_commit_pairs of siftmgr.hip held to the CPU oracle on the planted cases of tests/match_cases.py (the oracle is pinned to the
reference's own matcher on exactly these cases by tests/test_match_edge_cpu.py, which also asserts that every case returns what it plants).  One manager holds
one current image and several previous images, so one launch runs several cases.  Every comparison is bit for bit (tol = 0): the count, the first
min(count, 128) index pairs, the distances as uint32.  Every slot starts from sentinel contents, so what a launch leaves is what it wrote: the entries past
min(count, 128), and the slots outside the frame range, must still hold them.

No case addresses memory outside the key store: match_cases.layouts / check_bounds assert, before anything is uploaded, that every image fits its slot."""
import numpy as np
import pytest

from tests import match_cases as mc

pytestmark = pytest.mark.gpu

FAMILIES = ("key_counts", "cap", "equal", "ties", "thresholds", "saturated", "strides")
SENT_N = 77
SENT_IDX = ((np.arange(256, dtype=np.uint32).reshape(128, 2) * 7 + 3) % 16)            # key indices of image 0 at any stride: inside every key store
SENT_DIST = (0.5 + np.arange(128) / 256.0).astype(np.float32)
SENT_FILT = 7


def _manager(gpu, images, max_keys, valid=None):
    mc.check_bounds(images, max_keys)
    mgr = gpu.capi.SiftManager(len(images), max_keys)
    for d in images:
        mgr.add_image_host(np.zeros((len(d), 4), np.float32), d)
    _set_valid(mgr, [1] * len(images) if valid is None else valid)
    return mgr


def _set_valid(mgr, valid):
    for i, v in enumerate(valid):
        mgr.set_valid_image(i, v)
    mgr.update_gpu_valid_images()


def _fill_sentinels(mgr, slots):
    for p in slots:
        mgr.set_raw_matches(p, SENT_N, SENT_IDX, SENT_DIST)


def _assert_sentinel(mgr, p, what, n=SENT_N):
    """the lists untouched; the count `n` (SENT_N: untouched too)"""
    gn, idx, dist = mgr.raw_matches(p)
    assert gn == n and np.array_equal(idx, SENT_IDX) and np.array_equal(dist.view(np.uint32), SENT_DIST.view(np.uint32)), (what, p, gn)


def _assert_matches(got, exp, what, tail=True):
    n, idx, dist = got
    on, oidx, odist = exp
    assert n == on, (what, n, on)
    m = min(n, mc.MAX_RAW)
    assert len(oidx) == m and np.array_equal(idx[:m], oidx), what
    assert np.array_equal(dist[:m].view(np.uint32), odist.view(np.uint32)), what
    if tail:
        assert np.array_equal(idx[m:], SENT_IDX[m:]) and np.array_equal(dist[m:].view(np.uint32), SENT_DIST[m:].view(np.uint32)), what + ": written past the count"


def _oracle(oracle, imgs, prev, cur, max_keys=1024, **kw):
    return oracle.sift_match(imgs[prev], imgs[cur], off1=prev * max_keys, off2=cur * max_keys, **kw)


# ------------------------------------------------------------------------------------------------ the planted cases
@pytest.fixture(scope="module")
def cases():
    return mc.all_cases()


@pytest.mark.parametrize("family", FAMILIES)
def test_planted_cases_bit_exact(gpu, oracle, cases, family):
    mine = [c for c in cases if c["family"] == family]
    if family == "thresholds":                       # dist_max = one planted match's own distance, and the next float
        _, idx, dist = oracle.sift_match(mine[0]["prev"], mine[0]["cur"])
        mine = mine + mc.threshold_variants(mine[0], idx, dist)
    counts = []
    for g in mc.layouts(mine):
        mk, cur = g["max_keys"], len(g["cases"])
        imgs = [c["prev"] for c in g["cases"]] + [g["cur"]]
        mgr = _manager(gpu, imgs, mk)
        _fill_sentinels(mgr, range(cur + 1))
        mgr.match(cur, 0, cur + 1, dist_max=g["dist_max"], ratio_max=g["ratio_max"])
        for p, c in enumerate(g["cases"]):
            exp = _oracle(oracle, imgs, p, cur, mk, distmax=g["dist_max"], ratiomax=g["ratio_max"])
            en, eidx = mc.expected_output(c, p, cur)                     # what the case plants, at this manager's stride and slots
            assert exp[0] == en and sorted(map(tuple, exp[1].tolist())) == sorted(map(tuple, eidx.tolist())), c["name"]
            _assert_matches(mgr.raw_matches(p), exp, c["name"])
            counts.append(en)
        _assert_sentinel(mgr, cur, "the current image's own slot")
        mgr.close()
    print(family, "counts:", counts)
    assert len(counts) == {"key_counts": 84, "cap": 6, "equal": 1, "ties": 2, "thresholds": 3, "saturated": 2, "strides": 13}[family]


# ------------------------------------------------------------------------------------------------ frame ranges, recycled state, pair stage
@pytest.fixture(scope="module")
def six(gpu):
    imgs = mc.frame_images()
    return _manager(gpu, imgs, 1024), imgs


def test_frame_ranges_write_their_slots_only(oracle, six):
    mgr, imgs = six
    mgr.set_pair_stage(0, None, 0)
    _set_valid(mgr, [1, 1, 0, 1, 1, 1])
    # the frame loop's form: previous images 0 .. 4, the current image last; image 1 is empty, image 2 invalid
    _fill_sentinels(mgr, range(6))
    mgr.match(5, 0, 6)
    for p in (0, 3, 4):
        _assert_matches(mgr.raw_matches(p), _oracle(oracle, imgs, p, 5), "match(5, 0, 6) slot %d" % p)
    assert mgr.raw_matches(4)[0] == 129 and mgr.raw_matches(3)[0] == 17
    _assert_sentinel(mgr, 1, "empty previous image", n=0)
    _assert_sentinel(mgr, 2, "invalid previous image", n=0)
    _assert_sentinel(mgr, 5, "current image")
    # the revalidation form: the previous images come AFTER the current one (off1 > off2)
    _fill_sentinels(mgr, range(6))
    mgr.match(2, 3, 6)
    for p in (3, 4, 5):
        exp = _oracle(oracle, imgs, p, 2)
        assert exp[0] == min(len(imgs[p]), 300) and (exp[1][:, 0] > exp[1][:, 1]).all()
        _assert_matches(mgr.raw_matches(p), exp, "match(2, 3, 6) slot %d" % p)
    for p in (0, 1, 2):
        _assert_sentinel(mgr, p, "slot below startFrame")
    # a current image without keys: every slot of the range reads 0, nothing else is written
    mgr.match(1, 0, 6)
    for p in (0, 2, 3, 4, 5):
        n, idx, dist = mgr.raw_matches(p)
        assert n == 0, p
    for p in (0, 2):
        _assert_sentinel(mgr, p, "current image without keys", n=0)
    _assert_sentinel(mgr, 1, "current image")


def test_state_is_recycled_between_launches(oracle, six):
    """1024 keys, then 129, then 17 as the current image on one manager: the ticket counts from zero again, and the row / column verdicts a larger launch left
    beyond the new key counts are not read"""
    mgr, imgs = six
    mgr.set_pair_stage(0, None, 0)
    _set_valid(mgr, [1] * 6)
    _fill_sentinels(mgr, range(6))
    for cur, start, num in ((4, 0, 5), (5, 0, 6), (3, 4, 6)):
        first = None
        for rep in range(2):
            mgr.match(cur, start, num)
            got = [mgr.raw_matches(p) for p in range(start, num) if p != cur]
            for p, g in zip([p for p in range(start, num) if p != cur], got):
                _assert_matches(g, _oracle(oracle, imgs, p, cur), "match(%d, %d, %d) slot %d, call %d" % (cur, start, num, p, rep), tail=False)
            if first is None:
                first = got
            else:
                for a, b in zip(first, got):
                    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))
    assert mgr.raw_matches(4)[0] == 17 and mgr.raw_matches(5)[0] == 17


def test_pair_stage_matches_ahead_and_commit_clears_invalid_pairs(gpu, oracle, six):
    """Result set 1 on a side stream, speculative: invalid previous images are matched like valid ones; commit_pairs then zeroes the raw and filtered counts of
    the invalid images inside its range, and nothing else; set 0 is never touched."""
    import torch
    mgr, imgs = six
    side = torch.cuda.Stream()
    valid = [1, 1, 0, 0, 1, 0]                       # 2 and 3 invalid; the current image's own flag is 0 too: commit_pairs must skip it for being the current one
    mgr.set_pair_stage(0, None, 0)
    _set_valid(mgr, valid)
    _fill_sentinels(mgr, range(6))
    for p in range(6):
        mgr.set_filt_matches(p, SENT_FILT + 1)
    mgr.set_pair_stage(1, side.cuda_stream, 1)
    try:
        _fill_sentinels(mgr, range(6))               # (the setters name the selected set; they run on the manager's stream and wait for it)
        for p in range(6):
            mgr.set_filt_matches(p, SENT_FILT)
        mgr.match(5, 0, 6)
        side.synchronize()
        exp = {p: _oracle(oracle, imgs, p, 5) for p in (0, 2, 3, 4)}
        assert [exp[p][0] for p in (0, 2, 3, 4)] == [64, 129, 17, 129]
        for p in (0, 2, 3, 4):
            _assert_matches(mgr.raw_matches(p), exp[p], "speculative match, slot %d (valid %d)" % (p, valid[p]))
        _assert_sentinel(mgr, 1, "empty previous image", n=0)
        _assert_sentinel(mgr, 5, "current image")
        # set 0 in between
        mgr.set_pair_stage(0, None, 0)
        for p in range(6):
            _assert_sentinel(mgr, p, "set 0 after a launch on set 1")
            assert mgr.filt_matches(p)[0] == SENT_FILT + 1
        mgr.set_pair_stage(1, side.cuda_stream, 1)
        # commit [3, 6): slot 3 (invalid, in range) is cleared; slot 2 (invalid, below start), slot 4 (valid) and slot 5 (the current image) are not
        mgr.commit_pairs(5, 3, 6)
        want_n = {0: 64, 1: 0, 2: 129, 3: 0, 4: 129, 5: SENT_N}
        want_f = {0: SENT_FILT, 1: SENT_FILT, 2: SENT_FILT, 3: 0, 4: SENT_FILT, 5: SENT_FILT}
        for p in range(6):
            assert mgr.raw_matches(p)[0] == want_n[p] and mgr.filt_matches(p)[0] == want_f[p], ("commit_pairs(5, 3, 6)", p)
        # commit [0, 6): now slot 2 as well, and the empty image 1 stays as it is (valid)
        mgr.commit_pairs(5, 0, 6)
        want_n[2] = 0; want_f[2] = 0
        for p in range(6):
            assert mgr.raw_matches(p)[0] == want_n[p] and mgr.filt_matches(p)[0] == want_f[p], ("commit_pairs(5, 0, 6)", p)
        # only counts are cleared: the lists are what the matcher wrote
        for p in (2, 3):
            n, idx, dist = mgr.raw_matches(p)
            _assert_matches((exp[p][0], idx, dist), exp[p], "lists after commit, slot %d" % p)
    finally:
        mgr.set_pair_stage(0, None, 0)
    for p in range(6):
        _assert_sentinel(mgr, p, "set 0 at the end")
        assert mgr.filt_matches(p)[0] == SENT_FILT + 1
    # back on set 0 and not speculative: the invalid images read 0 again
    mgr.match(5, 0, 6)
    assert [mgr.raw_matches(p)[0] for p in range(5)] == [64, 0, 0, 0, 129]
