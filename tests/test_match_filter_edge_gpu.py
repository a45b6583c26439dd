"""GPU tests (-m gpu): the match filter chain of siftmgr.hip - k_filter_kabsch, k_filter_surface_area, k_filter_dense_verify / k_verify_trajectory,
k_add_residuals - held to the CPU oracle on the planted cases of tests/filter_cases.py (the oracle is pinned to the reference's own kernels on exactly
these cases by tests/test_match_filter_edge_cpu.py).  Match lists are put into the manager with set_raw_matches / set_filt_matches; one manager holds
one case per previous-image slot, so one launch filters all of them.  Every comparison is bit for bit (tol = 0).

No case addresses memory outside the key store: filter_cases.pack / check_indices assert it before anything is uploaded."""
import numpy as np
import pytest

from bundlefusion_amd.capi import BFError, ENTRYJ_DTYPE, intrinsics_matrix
from tests import filter_cases as fc

pytestmark = pytest.mark.gpu

PAD_IDX, PAD_DIST = 0xFFFFFFFF, np.float32(999.0)       # what k_filter_kabsch writes into the slots past the count


def _manager(gpu, allkeys, num_images, max_keys):
    mgr = gpu.capi.SiftManager(num_images, max_keys)
    descs = np.zeros((max_keys, 128), np.uint8)
    for i in range(num_images):
        mgr.add_image_host(allkeys[i * max_keys:(i + 1) * max_keys], descs)
        mgr.set_valid_image(i, 1)
    mgr.update_gpu_valid_images()
    return mgr


def _same_where_finite(got, exp, what):
    """bit equality; where the oracle's matrix has non-finite entries: the same finite mask and the bits of the finite entries (NaN payloads are not promised)"""
    fg, fe = np.isfinite(got), np.isfinite(exp)
    assert np.array_equal(fg, fe), (what, got, exp)
    assert np.array_equal(got[fg].view(np.uint32), exp[fe].view(np.uint32)), (what, got, exp)


def _assert_filtered(oracle, got, exp, what):
    n, idx, dist, T, Ti = got
    fn, fidx, fdist, fT = exp
    assert n == fn, (what, n, fn)
    assert np.array_equal(idx[:fn], fidx), what
    assert np.array_equal(dist[:fn].view(np.uint32), fdist.view(np.uint32)), what
    assert (idx[fn:] == PAD_IDX).all() and (dist[fn:] == PAD_DIST).all(), what
    _same_where_finite(T, fT, what + ": T")
    _same_where_finite(Ti, oracle.inverse44(fT), what + ": Tinv")


SENT = dict(n=7, idx=(np.arange(50, dtype=np.uint32).reshape(25, 2) * 3) % fc.MAX_KEYS, dist=(0.125 * np.arange(25)).astype(np.float32),
            T=(np.arange(16, dtype=np.float32) + 0.5).reshape(4, 4), Tinv=-(np.arange(16, dtype=np.float32) + 0.25).reshape(4, 4))


def _set_sentinel(mgr, p):
    mgr.set_filt_matches(p, SENT["n"], SENT["idx"], SENT["dist"], SENT["T"], SENT["Tinv"])


def _assert_sentinel(mgr, p, what):
    n, idx, dist, T, Ti = mgr.filt_matches(p)
    assert n == SENT["n"] and np.array_equal(idx, SENT["idx"]) and np.array_equal(dist, SENT["dist"]), (what, p)
    assert np.array_equal(T, SENT["T"]) and np.array_equal(Ti, SENT["Tinv"]), (what, p)


@pytest.fixture(scope="module")
def kab(gpu, oracle):
    cases = fc.kabsch_cases()
    allkeys, idx, num_images = fc.pack(cases)
    mgr = _manager(gpu, allkeys, num_images, fc.MAX_KEYS)
    return dict(cases=cases, allkeys=allkeys, idx=idx, num_images=num_images, mgr=mgr, Kinv=oracle.inverse44(fc.K))


def _inject_raw(k, order=None):
    """case order[p] into slot p (the indices are positions in the key store, so any slot may hold any case)"""
    mgr, B = k["mgr"], len(k["cases"])
    order = range(B) if order is None else order
    for p, c in enumerate(order):
        g = fc.check_indices(k["idx"][c], k["num_images"], fc.MAX_KEYS)
        mgr.set_raw_matches(p, k["cases"][c]["n"], g, k["cases"][c]["dist"])
    mgr.set_raw_matches(B, 0)                          # the current image's own slot


def _oracle_filter(oracle, k, c, min_matches, max_res2):
    return oracle.filter_matches(k["allkeys"], k["idx"][c], k["cases"][c]["dist"], k["cases"][c]["n"], k["Kinv"], min_matches, max_res2)


def test_kabsch_filter_planted_cases_bit_exact(oracle, kab):
    """every family, default parameters, one launch over all slots; every slot starts from sentinel contents, so what the kernel leaves is what it wrote"""
    mgr, cases, B = kab["mgr"], kab["cases"], len(kab["cases"])
    _inject_raw(kab)
    for p in range(B):
        _set_sentinel(mgr, p)
    mgr.filter_keypoint_matches(B, 0, B + 1, kab["Kinv"])
    split = {}
    for p in range(B):
        exp = _oracle_filter(oracle, kab, p, 5, 0.0004)
        _assert_filtered(oracle, mgr.filt_matches(p), exp, cases[p]["name"])
        s = split.setdefault(cases[p]["family"], [0, 0, 0]); s[0 if exp[0] == 0 else 2 if exp[0] == fc.MAX_FILT else 1] += 1
    print("kabsch cases per family (0, partial, 25):", split)
    # the raw lists are inputs only
    for p in (0, B // 2, B - 1):
        n, idx, dist = mgr.raw_matches(p)
        assert n == cases[p]["n"] and np.array_equal(idx, kab["idx"][p]) and np.array_equal(dist, cases[p]["dist"])


def test_kabsch_filter_start_frame_and_current_frame_slots_untouched(oracle, kab):
    """startFrame = 3 and curFrame in the middle of the range: the slots below 3 and the current frame's slot keep what was there; min_matches 3, max_res2 1e-4"""
    mgr, cases, B = kab["mgr"], kab["cases"], len(kab["cases"])
    _inject_raw(kab)
    mid = B // 2
    for p in range(B):
        _set_sentinel(mgr, p)
    mgr.filter_keypoint_matches(mid, 3, B + 1, kab["Kinv"], min_matches=3, max_res2=1e-4)
    for p in range(B):
        if p < 3 or p == mid:
            _assert_sentinel(mgr, p, "skipped slot written")
        else:
            _assert_filtered(oracle, mgr.filt_matches(p), _oracle_filter(oracle, kab, p, 3, 1e-4), cases[p]["name"] + " (min 3, 1e-4)")


def test_kabsch_filter_on_the_other_pair_set(gpu, oracle, kab):
    """bf_siftmgr_set_pair_stage(1, NULL, 0): setters, kernel and getters work on set 1 (here: the cases in reverse slot order, min_matches 8, max_res2 1e-3);
    the lists of set 0 are the same afterwards"""
    lib, check = gpu.capi.lib, gpu.capi.check
    mgr, cases, B = kab["mgr"], kab["cases"], len(kab["cases"])
    _inject_raw(kab)
    mgr.filter_keypoint_matches(B, 0, B + 1, kab["Kinv"])
    before = [(mgr.raw_matches(p), mgr.filt_matches(p)) for p in range(B)]
    check(lib.bf_siftmgr_set_pair_stage(mgr._h, 1, None, 0))
    try:
        order = list(range(B))[::-1]
        _inject_raw(kab, order)
        mgr.filter_keypoint_matches(B, 0, B + 1, kab["Kinv"], min_matches=8, max_res2=1e-3)
        for p, c in enumerate(order):
            _assert_filtered(oracle, mgr.filt_matches(p), _oracle_filter(oracle, kab, c, 8, 1e-3), cases[c]["name"] + " (set 1, min 8, 1e-3)")
    finally:
        check(lib.bf_siftmgr_set_pair_stage(mgr._h, 0, None, 0))
    for p in range(B):
        (rn, ri, rd), (fn, fi, fd, fT, fTi) = before[p]
        n, i, d = mgr.raw_matches(p)
        assert n == rn and np.array_equal(i, ri) and np.array_equal(d.view(np.uint32), rd.view(np.uint32)), p
        n, i, d, T, Ti = mgr.filt_matches(p)
        assert n == fn and np.array_equal(i, fi) and np.array_equal(d.view(np.uint32), fd.view(np.uint32)), p
        assert np.array_equal(T.view(np.uint32), fT.view(np.uint32)) and np.array_equal(Ti.view(np.uint32), fTi.view(np.uint32)), p


# ------------------------------------------------------------------------------------------------ surface area
def test_surface_area_filter_flips_at_the_oracle_area(gpu, oracle):
    cases = fc.area_cases()
    allkeys, fidx, num_images = fc.pack(cases, "fidx")
    Kinv = oracle.inverse44(fc.K)
    mgr = _manager(gpu, allkeys, num_images, fc.MAX_KEYS)
    cur, B = num_images - 1, len(cases)
    eye = np.eye(4, dtype=np.float32)
    dist = (0.01 * np.arange(25)).astype(np.float32)

    def inject(p):
        g = fc.check_indices(fidx[p], num_images, fc.MAX_KEYS)
        mgr.set_filt_matches(p, len(g), g, dist[:len(g)], eye, eye)

    def verdict(p, what):
        n, idx, _, _, _ = mgr.filt_matches(p)
        assert n in (0, len(fidx[p])) and np.array_equal(idx[:len(fidx[p])], fidx[p]), what      # only the count is ever written
        return n > 0

    # the default threshold: one launch over all pairs
    for p in range(B):
        inject(p)
    mgr.set_filt_matches(cur, 0)
    mgr.filter_surface_area(cur, 0, num_images, Kinv, 0.032)
    seen = set()
    for p in range(B):
        exp, areas = oracle.filter_surface_area(allkeys, fidx[p], Kinv, 0.032)
        assert verdict(p, cases[p]["name"]) == exp, (cases[p]["name"], areas)
        seen.add(exp)
    assert seen == {True, False}
    # the pair's own area a and the next float: one single-pair launch each (the threshold is a launch parameter)
    flips = 0
    for p in range(B):
        _, areas = oracle.filter_surface_area(allkeys, fidx[p], Kinv)
        if not np.isfinite(areas).all():
            continue                                   # a NaN area compares false with every threshold: covered by the launch above
        a = np.float32(max(areas))
        for thr, survives in ((a, True), (np.nextafter(a, np.float32(np.inf)), False)):
            exp, _ = oracle.filter_surface_area(allkeys, fidx[p], Kinv, float(thr))
            assert exp == survives, (cases[p]["name"], float(a), float(thr))
            inject(p)
            mgr.filter_surface_area(cur, p, p + 1, Kinv, float(thr))
            assert verdict(p, cases[p]["name"]) == exp, (cases[p]["name"], areas, float(thr))
            flips += 1
    assert flips >= 60


# ------------------------------------------------------------------------------------------------ dense verification
_DENSE = {}


def _dense_inputs():
    if "in" not in _DENSE:
        frames, Kin = fc.dense_inputs()
        _DENSE["in"] = (frames, Kin, fc.dense_transforms(frames))
    return _DENSE["in"]


def _cached(gpu, oracle, W, H, which):
    """a device cache holding frames `which` of the dense inputs at W x H, its intrinsics, and the oracle's frames (asserted equal bit for bit in the arrays the
    verification reads)"""
    import torch
    frames, Kin, _ = _dense_inputs()
    w, h = fc.DENSE_INPUT
    cache = gpu.capi.Cache(w, h, W, H, len(which), Kin)
    of = []
    for slot, i in enumerate(which):
        cache.store_frame(torch.from_numpy(frames[i][0]).cuda(), torch.from_numpy(frames[i][1]).cuda())
        o = oracle.cache_store_frame(frames[i][0], frames[i][1], W, H, Kin)
        g = cache.download_frame(slot)
        for key in ("depth", "campos", "normals"):
            assert np.array_equal(g[key].view(np.uint32), np.ascontiguousarray(o[key]).view(np.uint32)), (W, H, slot, key)
        of.append(o)
    gw, gh, gk = cache.geometry()
    Kc = intrinsics_matrix(*gk)
    assert (gw, gh) == (W, H) and np.array_equal(Kc.view(np.uint32), fc.cache_intrinsics(Kin, W, H).view(np.uint32))
    return cache, Kc, of


def _small_manager(gpu, n):
    mgr = gpu.capi.SiftManager(n + 1, 16)
    for i in range(n):
        mgr.add_image_host(np.zeros((16, 4), np.float32), np.zeros((16, 128), np.uint8))
        mgr.set_valid_image(i, 1)
    mgr.update_gpu_valid_images()
    return mgr


@pytest.mark.parametrize("geom", fc.DENSE_GEOMETRIES, ids=lambda g: "%dx%d" % g)
def test_dense_verify_flips_at_the_oracle_sums(gpu, oracle, geom):
    """The verdict flips exactly at the oracle's err and corr: the device block sum (from LDS up to DV_MAX_PIX pixels, recomputed above) equals the reference's
    bit for bit."""
    W, H = geom
    _, _, transforms = _dense_inputs()
    cache, Kc, of = _cached(gpu, oracle, W, H, (0, 1, 3))
    mgr = _small_manager(gpu, 3)
    verdicts = set()
    for name, T in transforms:
        ok, err, corr = oracle.dense_verify(of[0], of[1], W, H, Kc, T)
        print(geom, name, ok, err, corr)
        verdicts.add(ok)
        for et, ct, expect in fc.dense_flips(err, corr, ok):
            mgr.set_filt_matches(0, 7, T=T, Tinv=oracle.inverse44(T))
            mgr.filter_dense_verify(1, 0, 2, W, H, Kc, cache.frames_gpu(), err_thresh=et, corr_thresh=ct)
            assert mgr.filt_matches(0)[0] == (7 if expect else 0), (geom, name, err, corr, et, ct)
    assert verdicts == {True, False}
    # the second frame has no valid depth: err = 0 / 0, the pair is rejected whatever the thresholds; the pair with no filtered matches is not looked at
    T = transforms[0][1]
    mgr.set_filt_matches(0, 7, T=T, Tinv=oracle.inverse44(T))
    mgr.set_filt_matches(1, 0)
    mgr.filter_dense_verify(2, 0, 3, W, H, Kc, cache.frames_gpu(), err_thresh=10.0, corr_thresh=0.0)
    assert mgr.filt_matches(0)[0] == 0 and mgr.filt_matches(1)[0] == 0
    ok, err, _ = oracle.dense_verify(of[0], of[2], W, H, Kc, T, err_thresh=10.0, corr_thresh=0.0)
    assert not ok and np.isnan(err)
    cache.close()


def test_dense_verify_refuses_a_frame_larger_than_its_block(gpu, oracle):
    """W * ceil(H / 32) > 1024 threads: refused before anything is launched"""
    _, Kin, transforms = _dense_inputs()
    cache, Kc, _ = _cached(gpu, oracle, 80, 60, (0, 1))
    mgr = _small_manager(gpu, 2)
    mgr.set_filt_matches(0, 7, T=transforms[0][1], Tinv=oracle.inverse44(transforms[0][1]))
    with pytest.raises(BFError):
        mgr.filter_dense_verify(1, 0, 2, 80, 480, Kc, cache.frames_gpu())
    assert mgr.filt_matches(0)[0] == 7
    import torch
    traj = torch.eye(4).repeat(2, 1, 1).cuda()
    with pytest.raises(BFError):
        mgr.verify_trajectory(2, traj.data_ptr(), 80, 480, Kc, cache.frames_gpu())
    cache.close()


@pytest.mark.parametrize("geom", ((160, 120), (33, 17)), ids=lambda g: "%dx%d" % g)
def test_verify_trajectory_recompute_path_and_partial_warps(gpu, oracle, geom):
    """VerifyTrajectory over three cached frames against the restatement of tests/test_match_gpu.py (the reference's pair decoding (block / N, block % N) over
    N (N - 1) / 2 blocks, quirk included): ground truth, one pose pushed 0.5 m, the pushed pose on an invalid image.  err_thresh is 0.075, the match filter's
    default, not the optimiser's 0.05: at 33 x 17 a cache pixel spans ten input pixels and the oracle's mean point distance of the true pair (0, 2) is 0.059 m;
    the pushed pose gives 0.58 - 0.62 m at both sizes, so 0.075 separates the two everywhere."""
    import torch
    W, H = geom
    frames, _, _ = _dense_inputs()
    n = 3
    cache, Kc, of = _cached(gpu, oracle, W, H, (0, 1, 2))
    mgr = _small_manager(gpu, n)
    T0inv = np.linalg.inv(frames[0][2].astype(np.float64))
    gt = np.stack([(T0inv @ frames[i][2].astype(np.float64)).astype(np.float32) for i in range(n)])

    def restated(traj, valid):
        ok = 1
        for blk in range(n * (n - 1) // 2):
            i0, i1 = blk // n, blk % n
            if i0 >= i1 or not valid[i0] or not valid[i1]:
                continue
            T = oracle.mul44(oracle.inverse44(traj[i1]), traj[i0])
            ok &= int(oracle.dense_verify(of[i0], of[i1], W, H, Kc, T, err_thresh=0.075, corr_thresh=0.001)[0])
        return ok

    pushed = gt.copy(); pushed[1, 0, 3] += np.float32(0.5)
    seen = []
    for traj, valid in ((gt, (1, 1, 1)), (pushed, (1, 1, 1)), (pushed, (1, 0, 1))):
        for i, v in enumerate(valid):
            mgr.set_valid_image(i, v)
        d = torch.from_numpy(traj).cuda()
        got = mgr.verify_trajectory(n, d.data_ptr(), W, H, Kc, cache.frames_gpu(), err_thresh=0.075, corr_thresh=0.001)
        exp = restated(traj, valid)
        assert got == exp, (geom, valid, got, exp)
        seen.append(exp)
    assert seen == [1, 0, 1], seen
    cache.close()


# ------------------------------------------------------------------------------------------------ residuals
def _residual_setup(gpu, oracle, n_images, counts, seed):
    """a manager of n_images images (the last one is the current frame) with filtered sets of the given sizes; returns it and the expected rows / key pairs"""
    mk = 64
    rng = np.random.default_rng(seed)
    allkeys = np.c_[rng.uniform(5, 630, n_images * mk), rng.uniform(5, 470, n_images * mk), rng.uniform(3, 12, n_images * mk),
                    rng.uniform(0.8, 3.0, n_images * mk)].astype(np.float32)
    mgr = _manager(gpu, allkeys, n_images, mk)
    Kinv = oracle.inverse44(fc.K)
    cur = n_images - 1
    rows, pairs = [], []
    for p, cnt in enumerate(counts):
        idx = np.c_[p * mk + rng.permutation(mk)[:fc.MAX_FILT], cur * mk + rng.permutation(mk)[:fc.MAX_FILT]].astype(np.uint32)
        fc.check_indices(idx, n_images, mk)
        mgr.set_filt_matches(p, cnt, idx, np.zeros(fc.MAX_FILT, np.float32), np.eye(4), np.eye(4))
        for k in range(cnt):
            rows.append(oracle.make_entry(allkeys, idx[k, 0], idx[k, 1], p, cur, Kinv))
            pairs.append((idx[k, 0], idx[k, 1]))
    return mgr, Kinv, cur, np.array(rows, dtype=ENTRYJ_DTYPE), np.array(pairs, np.uint32).reshape(-1, 2)


def _add_frame(mgr, cur, Kinv):
    mgr.filter_frames_async(cur, 0, cur + 1)
    mgr.add_curr_to_residuals(cur, 0, cur + 1, Kinv)
    mgr.sync_frame_result(cur)
    return mgr.num_global_correspondences()


def test_add_curr_to_residuals_mixed_counts_bit_exact(gpu, oracle):
    counts = (25, 0, 1, 25, 1)
    mgr, Kinv, cur, rows, pairs = _residual_setup(gpu, oracle, 6, counts, 77)
    assert _add_frame(mgr, cur, Kinv) == sum(counts) == len(rows)
    corr, ckeys = mgr.download_global_correspondences()
    assert np.array_equal(corr.view(np.uint8), rows.view(np.uint8))            # EntryJ rows, in ascending previous-image order
    assert np.array_equal(ckeys, pairs)                                        # the key side table
    assert np.all(np.diff(corr["imgIdx_i"].astype(np.int64)) >= 0) and (corr["imgIdx_j"] == cur).all()
    # an invalid current frame (no valid previous image is connected to it) adds nothing and leaves the list alone
    for p in range(cur):
        mgr.set_valid_image(p, 0)
    mgr.update_gpu_valid_images()
    assert _add_frame(mgr, cur, Kinv) == len(rows)
    assert mgr.valid_images(cur + 1)[cur] == 0
    corr2, ckeys2 = mgr.download_global_correspondences()
    assert np.array_equal(corr2.view(np.uint8), rows.view(np.uint8)) and np.array_equal(ckeys2, pairs)
    # ... and on a fresh manager: nothing at all
    mgr2, Kinv, cur, _, _ = _residual_setup(gpu, oracle, 6, counts, 78)
    for p in range(cur):
        mgr2.set_valid_image(p, 0)
    mgr2.update_gpu_valid_images()
    assert _add_frame(mgr2, cur, Kinv) == 0


def test_add_curr_to_residuals_stops_at_capacity(gpu, oracle):
    """a 4-image manager holds 25 * 4 * 3 / 2 = 150 entries: 60 per call -> 60, 120, 150 (the third call is cut), 150 (the fourth adds nothing and writes nothing)"""
    counts = (25, 25, 10)
    mgr, Kinv, cur, rows, pairs = _residual_setup(gpu, oracle, 4, counts, 79)
    cap = fc.MAX_FILT * 4 * 3 // 2
    assert cap == 150
    totals = [_add_frame(mgr, cur, Kinv) for _ in range(3)]
    assert totals == [60, 120, 150]
    corr, ckeys = mgr.download_global_correspondences()
    exp_rows, exp_pairs = np.concatenate([rows] * 3)[:cap], np.concatenate([pairs] * 3)[:cap]
    assert np.array_equal(corr.view(np.uint8), exp_rows.view(np.uint8)) and np.array_equal(ckeys, exp_pairs)
    assert _add_frame(mgr, cur, Kinv) == cap
    corr2, ckeys2 = mgr.download_global_correspondences()
    assert np.array_equal(corr2.view(np.uint8), exp_rows.view(np.uint8)) and np.array_equal(ckeys2, exp_pairs)
