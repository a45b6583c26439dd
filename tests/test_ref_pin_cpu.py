"""CPU tests (-m "not gpu"): the oracle PINNED to reference source.

oracle/_ref/libbfref.so is the reference's own device code (LieDerivUtil.h, cuda_svd3.h, cuda_EigenValue.h, cuda_kabsch.h,
VoxelUtilHashSDF.h, CUDASceneRepHashSDF.cu), compiled for the host from /root/reference by oracle/ref/Makefile (shim headers +
a serial block emulator; nothing copied).  Every test feeds the same seeded inputs to that library and to the oracle restatement
(oracle/*.cpp) and demands:

  * bit equality (tol = 0) wherever both sides evaluate +, -, *, /, sqrt only (both are compiled with -ffp-contract=off): the
    integer maps, the 4x4 inverse, the McAdams SVD, Kabsch, the whole greedy Kabsch match filter, the TSDF integrate /
    de-integrate voxel bytes, key sets, per-bucket occupancy, free-block count, frustum-list sets;
  * |diff| <= the stated bound where an elementary function is involved: the reference calls sin/cos/acos/atan2 of the CUDA
    math library (here: glibc), the oracle and the product use the fixed IEEE sequences of include/bf_detmath.h (~2 ulp).

Order-dependent quantities (which of a bucket's four slots a key sits in, heap pointer values) are NOT parity targets
(the CUDA reference itself varies from run to run); they are compared through their order-independent content.
The tests skip (not fail) only when neither /root/reference nor a prebuilt library is present.
"""
import os

import numpy as np
import pytest

from bundlefusion_amd import synth
from bundlefusion_amd.capi import default_hash_params, camera_params, intrinsics_matrix, FREE_ENTRY, VOX_PER_BLOCK
from tests import ref_api

pytestmark = pytest.mark.skipif(not ref_api.available(), reason="oracle/_ref/libbfref.so is absent and /root/reference is not here to build it")


# ------------------------------------------------------------------------------------------------ integer maps
def test_hash_and_index_maps_exact(oracle):
    rng = np.random.default_rng(10)
    for nb in (1, 7, 4096, 800000, 1000003, 2 ** 31 - 1):
        pts = rng.integers(-(1 << 20), 1 << 20, (300, 3))
        pts[:6] = [[0, 0, 0], [-1, -1, -1], [1, 0, 0], [-(1 << 20), (1 << 20) - 1, 5], [29, -29, 2], [-8, 8, -16]]
        for x, y, z in pts:
            assert oracle.hash_pos(nb, int(x), int(y), int(z)) == ref_api.hash_pos(nb, int(x), int(y), int(z))
    for vs in (0.004, 0.01, 0.002, 0.05):
        w = rng.uniform(-6, 6, (400, 3)).astype(np.float32)
        w[:8] *= 0.001                                   # around the origin: sign(0), negative half voxels, block floor-division
        w[8:12] = [[0, 0, 0], [-0.0, 0.0, -0.0], [vs / 2, -vs / 2, vs * 7.5], [-vs * 8, vs * 8, -vs * 7.5]]
        for p in w:
            assert oracle.world_to_block(vs, p) == ref_api.world_to_block(vs, p)
    for i in range(512):
        x, y, z = ref_api.delinearize(i)
        assert (x, y, z) == (i & 7, (i >> 3) & 7, i >> 6) and ref_api.linearize(x, y, z) == i      # z*64 + y*8 + x, as tsdf.hip / the oracle index voxels


def test_mat4_inverse_exact(oracle):
    from tests.bundle_synth import random_pose
    rng = np.random.default_rng(11)
    for k in range(40):
        M = random_pose(rng, 1.0, 2.0).astype(np.float32)
        if k % 4 == 0:
            M = (M @ np.diag([2.0, 0.5, 3.0, 1.0])).astype(np.float32)        # not a rigid motion: the general cofactor inverse
        assert np.array_equal(oracle.mat4_inverse(M).view(np.uint32), ref_api.mat4_inverse(M).view(np.uint32))


# ------------------------------------------------------------------------------------------------ SE(3)
def test_lie_maps_within_detmath_bound(oracle):
    from tests.bundle_synth import random_pose
    rng = np.random.default_rng(12)
    Ts = np.stack([random_pose(rng, a, 1.5) for a in (1e-5, 1e-3, 0.05, 0.3, 1.0, 2.5, 3.1) for _ in range(6)]).astype(np.float32)
    rot, trans = oracle.matrices_to_poses(Ts)
    for i, T in enumerate(Ts):
        r, t = ref_api.matrix_to_pose(T)
        # ln_rotation: acos / sqrt; translation: a 3x3 solve with sin/cos coefficients.  bf_detmath vs glibc: <= 2 ulp per call.
        assert np.abs(rot[i] - r).max() <= 4e-6 * max(1.0, np.abs(r).max()), (i, rot[i], r)
        assert np.abs(trans[i] - t).max() <= 8e-6 * max(1.0, np.abs(t).max()), (i, trans[i], t)
    M = oracle.poses_to_matrices(rot, trans)
    for i in range(len(Ts)):
        Mr = ref_api.pose_to_matrix(rot[i], trans[i])
        assert np.abs(M[i] - Mr).max() <= 4e-6 * max(1.0, np.abs(Mr).max())
        assert np.array_equal(M[i][3], Mr[3])
    # small-angle branches (theta^2 < 1e-8, < 1e-6) are polynomial on both sides: exact
    for w in ([1e-6, -2e-6, 3e-6], [0.0, 0.0, 0.0], [3e-5, 1e-5, -2e-5]):
        m = oracle.poses_to_matrices(np.array([w], np.float32), np.array([[0.1, -0.2, 0.3]], np.float32))[0]
        assert np.array_equal(m.view(np.uint32), ref_api.pose_to_matrix(w, [0.1, -0.2, 0.3]).view(np.uint32)), w


# ------------------------------------------------------------------------------------------------ SVD / Kabsch / greedy filter
def test_svd3_and_eigenvalues_exact(oracle):
    rng = np.random.default_rng(13)
    for k in range(200):
        A = rng.normal(size=(3, 3)).astype(np.float32)
        if k % 5 == 0:
            A[2] = A[0] * np.float32(0.5)              # rank deficient
        if k % 7 == 0:
            A = (A * np.float32(1e-3)).astype(np.float32)
        for a, b in zip(oracle.svd3(A), ref_api.svd3(A)):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (k, a, b)


def test_kabsch_exact(oracle):
    from tests.bundle_synth import random_pose
    rng = np.random.default_rng(14)
    for k in range(60):
        n = int(rng.integers(3, 26))
        T = random_pose(rng, 0.5, 0.5)
        src = (rng.uniform(-1, 1, (n, 3)) + [0, 0, 2]).astype(np.float32)
        tgt = ((T[:3, :3] @ src.T).T + T[:3, 3] + rng.normal(0, 0.003, (n, 3))).astype(np.float32)
        if k % 6 == 0:
            src[:, 2] = 2.0                            # coplanar source
        To, evo = oracle.kabsch(src, tgt)
        Tr, evr = ref_api.kabsch(src, tgt)
        assert np.array_equal(To.view(np.uint32), Tr.view(np.uint32)), (k, To, Tr)
        assert np.array_equal(evo.view(np.uint32), evr.view(np.uint32)), (k, evo, evr)


def _keys_from_points(P, K):
    uv = (K[:3, :3] @ P.T).T
    return np.c_[uv[:, 0] / uv[:, 2], uv[:, 1] / uv[:, 2], np.full(len(P), 3.0), P[:, 2]].astype(np.float32)


def test_greedy_kabsch_filter_exact(oracle):
    """filterKeyPointMatches (cuda_kabsch.h:422-502) of one image pair: kept index pairs, distances and the transform, bit for bit,
    on inlier sets with planted outliers, duplicate key points, too few matches and pure garbage."""
    from tests.bundle_synth import random_pose
    K = intrinsics_matrix(580.0, 580.0, 320.0, 240.0)
    Kinv = np.linalg.inv(K.astype(np.float64)).astype(np.float32)
    rng = np.random.default_rng(15)
    kept_total = 0
    for case in range(40):
        n = int(rng.integers(3, 60))
        T = random_pose(rng, 0.15, 0.25)
        P = np.c_[rng.uniform(-1, 1, n), rng.uniform(-0.8, 0.8, n), rng.uniform(1.2, 3.0, n)]
        Q = (T[:3, :3] @ P.T).T + T[:3, 3] + rng.normal(0, 0.002, (n, 3))
        bad = rng.choice(n, size=min(n // 4, case % 7), replace=False)
        Q[bad] += rng.uniform(-0.4, 0.4, (len(bad), 3))
        if case % 9 == 8:
            Q = rng.uniform(-1, 1, (n, 3)) + [0, 0, 2]          # garbage
        keys = np.concatenate([_keys_from_points(P, K), _keys_from_points(Q, K)])
        idx = np.zeros((128, 2), np.uint32); idx[:n, 0] = np.arange(n); idx[:n, 1] = n + np.arange(n)
        if case % 5 == 1 and n > 6:
            idx[3] = idx[1]; idx[5, 0] = idx[2, 0]              # a repeated match and a shared source key: addMatch must refuse them
        dist = np.zeros(128, np.float32); dist[:n] = np.sort(rng.uniform(0.05, 0.6, n)).astype(np.float32)
        no, io, do, To = oracle.filter_matches(keys, idx, dist, n, Kinv)
        nr, ir, dr, Tr = ref_api.filter_matches(keys, idx, dist, n, Kinv)
        assert no == nr, (case, no, nr)
        assert np.array_equal(io, ir) and np.array_equal(do.view(np.uint32), dr.view(np.uint32)), case
        if no:
            assert np.array_equal(To.view(np.uint32), Tr.view(np.uint32)), (case, To, Tr)
        kept_total += no
    assert kept_total > 150          # the comparison is not vacuous


# ------------------------------------------------------------------------------------------------ Gauss-Newton / PCG solver
def test_solver_vs_reference_kernels(oracle):
    """solveBundlingStub of the reference (its own kernels: Initialization, PCGIteration, EvalResidual, BuildDenseSystem ..., float
    atomics summed in thread-index order) against the oracle solver on the same problems.  Both evaluate the same energy with
    different summation orders, so: energies per Gauss-Newton iteration rel 1e-3, poses 1e-4 — the tolerances the HIP solver is held
    to against the oracle (tests/test_solver_gpu.py) — and the per-image row counts of the correspondence table exactly."""
    from tests import bundle_synth as bs
    for n, seed, nl, lin in ((11, 0, 4, 100), (30, 1, 3, 150)):
        corr, T_gt, T_init = bs.sparse_problem(n_images=n, pair_prob=0.6, seed=seed)
        valid = np.ones(n, np.int32)
        ro, to = oracle.matrices_to_poses(T_init); rr, tr = ro.copy(), to.copy()
        w1, w0 = [1.0] * nl, [0.0] * nl
        o = oracle.solver_solve(corr.copy(), valid, n, nl, lin, w1, w0, w0, ro, to)
        r = ref_api.solver_solve(corr.copy(), valid, n, nl, lin, w1, w0, w0, rr, tr)
        assert np.array_equal(r["rows"], np.bincount(np.r_[corr["imgIdx_i"], corr["imgIdx_j"]], minlength=n))
        k = o["gn_iterations"]
        assert k >= 2
        co, cr = o["convergence"][:k + 1], r["convergence"][:k + 1]
        assert (cr >= 0).all() and np.abs(co - cr).max() <= 1e-3 * max(co.max(), 1e-6), (co, cr)
        assert np.abs(ro - rr).max() < 1e-4 and np.abs(to - tr).max() < 1e-4
        gt_r, gt_t = oracle.matrices_to_poses(T_gt.astype(np.float32))
        assert np.abs(rr - gt_r).max() < 0.01 and np.abs(tr - gt_t).max() < 0.01            # and it is the right answer
        assert abs(o["max_residual"] - r["max_residual"]) <= 1e-3 * max(r["max_residual"], 1e-6) and o["max_residual_index"] == r["max_residual_index"]


def test_solver_dense_terms_vs_reference_kernels(oracle):
    """The dense depth + colour terms (BuildDenseSystem: FindImageImageCorr / FindDenseCorrespondences / BuildDenseSystem kernels and the
    dense PCG branch) on a local chunk of 4 synthetic frames with cache frames, sparse + dense weights as the local solve uses them."""
    from tests import bundle_synth as bs
    from bundlefusion_amd.capi import intrinsics_matrix
    W, H = 80, 60
    n = 4
    src = [synth.scene_room(3 * k, 320, 240) for k in range(n)]
    Kd = src[0][3]
    K = intrinsics_matrix(Kd["fx"], Kd["fy"], Kd["mx"], Kd["my"])
    frames = [oracle.cache_store_frame(d, c, W, H, K) for d, c, _, _ in src]
    k4 = [K[0, 0] * W / 320, K[1, 1] * H / 240, K[0, 2] * (W - 1) / 319, K[1, 2] * (H - 1) / 239]
    T0inv = np.linalg.inv(src[0][2].astype(np.float64))
    T_gt = np.stack([(T0inv @ f[2].astype(np.float64)) for f in src]).astype(np.float32)
    rng = np.random.default_rng(3)
    T_init = T_gt.copy()
    for i in range(1, n):
        T_init[i] = (T_gt[i].astype(np.float64) @ bs.random_pose(rng, 0.004, 0.004)).astype(np.float32)
    from bundlefusion_amd.capi import ENTRYJ_DTYPE
    rows = []
    for i in range(n):                                         # sparse correspondences consistent with the rendered poses (they anchor the sliding directions)
        for j in range(i + 1, n):
            pw = rng.uniform(-1, 1, (12, 3)) + np.array([0, 0, 2.2])
            pi = (np.linalg.inv(T_gt[i].astype(np.float64)) @ np.c_[pw, np.ones(12)].T).T[:, :3] + rng.normal(0, 0.001, (12, 3))
            pj = (np.linalg.inv(T_gt[j].astype(np.float64)) @ np.c_[pw, np.ones(12)].T).T[:, :3] + rng.normal(0, 0.001, (12, 3))
            for a, b in zip(pi, pj):
                e = np.zeros(1, ENTRYJ_DTYPE); e["imgIdx_i"], e["imgIdx_j"], e["pos_i"], e["pos_j"] = i, j, a, b
                rows.append(e)
    corr = np.concatenate(rows)
    valid = np.ones(n, np.int32)
    nl = 3
    ws, wd, wc = [1.0] * nl, [1.0, 2.0, 3.0], [0.0] * nl       # SBA.cpp:28-38: local solve = sparse 1, dense depth i + 1, colour 0
    ro, to = oracle.matrices_to_poses(T_init); rr, tr = ro.copy(), to.copy()
    o = oracle.solver_solve(corr.copy(), valid, n, nl, 100, ws, wd, wc, ro, to, cache_frames=frames, cache_geom=(W, H, k4))
    r = ref_api.solver_solve(corr.copy(), valid, n, nl, 100, ws, wd, wc, rr, tr, cache_frames=frames, cache_geom=(W, H, k4))
    assert o["num_dense_pairs"] >= 3
    assert np.abs(ro - rr).max() < 1e-4 and np.abs(to - tr).max() < 1e-4
    gt_r, gt_t = oracle.matrices_to_poses(T_gt)
    assert np.abs(rr - gt_r).max() < 2e-3 and np.abs(tr - gt_t).max() < 2e-3
    k = o["gn_iterations"]
    assert np.abs(o["convergence"][:k + 1] - r["convergence"][:k + 1]).max() <= 1e-3 * max(o["convergence"][:k + 1].max(), 1e-6)


# ------------------------------------------------------------------------------------------------ image kernels
def _same(a, b):
    a = np.asarray(a); b = np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_ingest_and_resample_kernels(oracle):
    """CUDAImageUtil.cu kernels vs the oracle: erosion, nearest resampling (float / uchar4 / luminance) exact; the two Gaussian
    filters evaluate exp(): glibc in the reference build, include/bf_detmath.h in the oracle (<= 2 ulp per weight), so their outputs
    are compared to 3e-6 relative — and the SET of valid pixels exactly."""
    rng = np.random.default_rng(20)
    d, c, _, _ = synth.scene_room(30, 160, 120)
    d = d.copy(); d[40:44, 50:70] = -np.inf; d[rng.random(d.shape) < 0.01] = -np.inf
    e_o = oracle.erode_depth(oracle.erode_depth(d))
    e_r = ref_api.erode_depth(ref_api.erode_depth(d))
    assert _same(e_o, e_r) and np.isfinite(e_o).sum() < np.isfinite(d).sum()
    g_o, g_r = oracle.gauss_filter_depth(e_o, 2.0, 0.05), ref_api.gauss_filter_depth(e_r, 2.0, 0.05)
    assert np.array_equal(np.isfinite(g_o), np.isfinite(g_r))
    v = np.isfinite(g_o)
    assert np.abs(g_o[v] - g_r[v]).max() <= 3e-6 * np.abs(g_r[v]).max()
    for (ow, oh) in ((80, 60), (160, 120), (53, 41), (320, 240)):
        assert _same(oracle.resample_float(g_o, ow, oh), ref_api.resample_float(g_o, ow, oh))
        assert _same(oracle.resample_uchar4(c, ow, oh), ref_api.resample_uchar4(c, ow, oh))
        assert _same(oracle.resample_to_intensity(c, ow, oh), ref_api.resample_to_intensity(c, ow, oh))
    I = oracle.resample_to_intensity(c, 160, 120)
    io, ir = oracle.gauss_filter_intensity(I, 2.5), ref_api.gauss_filter_intensity(I, 2.5)
    assert np.abs(io - ir).max() <= 3e-6
    # CUDAImageManager::process, device part: the reference default configuration (sensor 160x120 -> integration 80x60 here)
    raw_r, filt_r, integ_r = ref_api.ingest(d, 80, 60)
    assert _same(raw_r, e_o)
    assert np.array_equal(np.isfinite(filt_r), v) and np.abs(filt_r[v] - g_o[v]).max() <= 3e-6 * np.abs(g_o[v]).max()
    assert _same(integ_r, ref_api.resample_float(filt_r, 80, 60))


def _edge_depth(w, h, seed):
    """depth blocks whose neighbours differ by just under / just over 0.05 (dThresh == sigmaR), with -inf, 0.0 and a few NaNs"""
    rng = np.random.default_rng(seed)
    levels = np.float32([1.0, 1.0499, 1.0501, 1.0998, 1.1002])
    d = np.repeat(np.repeat(levels[rng.integers(0, 5, ((h + 1) // 2, (w + 2) // 3))], 2, axis=0), 3, axis=1)[:h, :w].copy()
    u = rng.random((h, w))
    d[u < 0.04] = -np.inf
    d[(u >= 0.04) & (u < 0.06)] = 0.0
    d[(u >= 0.06) & (u < 0.063)] = np.nan
    return d


def test_ingest_kernels_at_edge_shapes_and_every_radius(oracle):
    """The operators tests/test_ingest_gpu.py holds the HIP kernels to, at its edge shapes: erosion with structure sizes 0 / 1 / 3 / 5 and
    fracReq values that land exactly on a count ratio (exact); both Gaussians at sigma 0.25 / 1 / 2 / 4, radius 1 to 8 (3e-6, the set of valid
    pixels exactly); resampling up, down, at non-integer ratios, to width 2 and from width or height 1 (exact).  A Gaussian with sigma 0 is
    left out: its taps are exp(-0 / 0), NaN, in the reference too."""
    for w, h in ((1, 1), (2, 3), (63, 5), (65, 4), (130, 1), (97, 61)):
        d = _edge_depth(w, h, w + h)
        for s, a, b in ((0, 1, 1), (1, 3, 9), (3, 3, 10), (3, 15, 49), (5, 40, 121)):
            frac = float(np.float32(a) / np.float32(b))
            assert _same(oracle.erode_depth(d, s, 0.05, frac), ref_api.erode_depth(d, s, 0.05, frac)), (w, h, s, a, b)
        img = np.random.default_rng(w * h).random((h, w)).astype(np.float32)
        for sigma in (0.25, 1.0, 2.0, 4.0):
            g_o, g_r = oracle.gauss_filter_depth(d, sigma, 0.05), ref_api.gauss_filter_depth(d, sigma, 0.05)
            v = np.isfinite(g_o)
            assert np.array_equal(v, np.isfinite(g_r)) and _same(g_o[~v], g_r[~v]), (w, h, sigma)
            assert not v.any() or np.abs(g_o[v] - g_r[v]).max() <= 3e-6 * np.abs(g_r[v]).max(), (w, h, sigma)
            i_o, i_r = oracle.gauss_filter_intensity(img, sigma), ref_api.gauss_filter_intensity(img, sigma)
            assert np.abs(i_o - i_r).max() <= 3e-6, (w, h, sigma)
    for (iw, ih), (ow, oh) in (((64, 4), (130, 5)), ((130, 5), (63, 3)), ((65, 3), (2, 2)), ((1, 97), (64, 5)), ((97, 1), (65, 4)), ((1, 1), (2, 2)),
                               ((63, 5), (161, 121))):
        d = _edge_depth(iw, ih, iw * ih)
        c = np.random.default_rng(iw + ih).integers(0, 256, (ih, iw, 4), dtype=np.uint8)
        assert _same(oracle.resample_float(d, ow, oh), ref_api.resample_float(d, ow, oh)), (iw, ih, ow, oh)
        assert _same(oracle.resample_uchar4(c, ow, oh), ref_api.resample_uchar4(c, ow, oh)), (iw, ih, ow, oh)
        assert _same(oracle.resample_to_intensity(c, ow, oh), ref_api.resample_to_intensity(c, ow, oh)), (iw, ih, ow, oh)


def test_cache_store_frame_at_edge_shapes_vs_reference_kernels(oracle):
    """CUDACache::storeFrame at the cache sizes tests/test_ingest_gpu.py runs (partial tiles, a partial workgroup, 2 x 2), colour at another size
    than depth, and the sigma pairs it runs: 0 (the reference skips the filter: defined), 3 (radius 6) and the defaults."""
    rng = np.random.default_rng(5)
    dw, dh, cw, ch = 161, 121, 200, 150
    d, _, _, Kd = synth.scene_room(40, dw, dh)
    c = synth.scene_room(40, cw, ch)[1]
    d = (d + rng.normal(0, 0.004, d.shape)).astype(np.float32)
    d[dh // 3: dh // 3 + 7, dw // 2: dw // 2 + 20] = -np.inf
    d[rng.random(d.shape) < 0.01] = -np.inf
    K = intrinsics_matrix(Kd["fx"], Kd["fy"], Kd["mx"], Kd["my"])
    for W, H in ((81, 61), (100, 75), (17, 13), (16, 12), (2, 2)):
        for cs, ds in ((2.5, 1.0), (0.0, 0.0), (3.0, 3.0), (0.0, 3.0), (3.0, 0.0)):
            fo = oracle.cache_store_frame(d, c, W, H, K, cs, ds, 0.05)
            fr = ref_api.cache_store_frame(d, c, W, H, oracle.mat4_inverse(K), cs, ds, 0.05)
            for name in ("depth", "campos", "normals", "intensity", "derivs"):
                fin_o, fin_r = np.isfinite(fo[name]), np.isfinite(fr[name])
                assert np.array_equal(fin_o, fin_r) and _same(fo[name][~fin_o], fr[name][~fin_r]), (W, H, cs, ds, name)
                if not fin_o.any():
                    continue                        # 2 x 2: no interior pixel, every normal and derivative is -inf
                tol = 3e-6 if name != "normals" else 2e-5
                assert np.abs(fo[name][fin_o] - fr[name][fin_r]).max() <= tol * max(1.0, np.abs(fr[name][fin_r]).max()), (W, H, cs, ds, name)
            assert np.abs(fo["normals_u"].astype(int) - fr["normals_u"].astype(int)).max() <= 1, (W, H, cs, ds)
            if cs == 0.0:                           # unfiltered intensity: point samples, exact
                assert _same(fo["intensity"], fr["intensity"]), (W, H)
            if ds == 0.0:                           # unfiltered depth: point samples and +, -, * only, exact
                assert _same(fo["depth"], fr["depth"]) and _same(fo["campos"], fr["campos"]), (W, H)


def test_cache_store_frame_vs_reference_kernels(oracle):
    """CUDACache::storeFrame: the six arrays of one 80x60 cache frame from a 320x240 input and from a 640x480 one, clean and with depth noise + holes."""
    rng = np.random.default_rng(4)
    for k, (w, h), noisy in ((12, (320, 240), False), (500, (640, 480), True), (1300, (320, 240), True)):
        d, c, _, Kd = synth.scene_room(k, w, h)
        d = d.copy(); d[h // 2 - 5:h // 2 + 5, w // 2:w // 2 + 30] = -np.inf
        if noisy:
            d = d + rng.normal(0, 0.004, d.shape).astype(np.float32)
            d[rng.random(d.shape) < 0.01] = -np.inf
        K = intrinsics_matrix(Kd["fx"], Kd["fy"], Kd["mx"], Kd["my"])
        fo = oracle.cache_store_frame(d, c, 80, 60, K)
        fr = ref_api.cache_store_frame(d, c, 80, 60, oracle.mat4_inverse(K))
        for name in ("depth", "campos", "normals", "intensity", "derivs"):
            fin_o, fin_r = np.isfinite(fo[name]), np.isfinite(fr[name])
            assert np.array_equal(fin_o, fin_r), (k, name)
            tol = 3e-6 if name in ("depth", "campos", "intensity", "derivs") else 2e-5      # normals: a normalised cross product of differences of filtered positions
            assert np.abs(fo[name][fin_o] - fr[name][fin_r]).max() <= tol * max(1.0, np.abs(fr[name][fin_r]).max()), (k, name)
            assert fin_o.sum() > 0.4 * fin_o.size
        assert np.abs(fo["normals_u"].astype(int) - fr["normals_u"].astype(int)).max() <= 1      # bytes of the float normals above


# ------------------------------------------------------------------------------------------------ voxel hash
def _by_key(hash_np, vox_np):
    """{(x, y, z): 512 voxel records} of every occupied entry, plus the home-bucket occupancy histogram support"""
    occ = hash_np[hash_np["ptr"] != FREE_ENTRY]
    v = vox_np.view(np.uint8).reshape(-1, VOX_PER_BLOCK * 12)
    return {tuple(int(c) for c in e["pos"]): v[e["ptr"] // VOX_PER_BLOCK] for e in occ}


def _assert_same_volume(osc, rsc, nb, what, frustum_list=True):
    oh, rh = osc.hash(), rsc.hash()
    ob, rb = _by_key(oh, osc.voxels()), _by_key(rh, rsc.voxels())
    assert set(ob) == set(rb), what + ": allocated block keys"
    assert osc.heap_counter() == rsc.heap_counter(), what + ": free blocks"
    for k in ob:
        assert np.array_equal(ob[k], rb[k]), what + ": voxel bytes of block %s" % (k,)
    # per-bucket occupancy: entries stored inside each bucket's own four slots, and the number that went to its overflow chain
    for h, name in ((oh, "oracle"), (rh, "reference")):
        ptr = h["ptr"].reshape(nb, 4)
        assert (ptr != FREE_ENTRY).sum() == len(ob), name
    occ_o = (oh["ptr"].reshape(nb, 4) != FREE_ENTRY).sum(axis=1)
    occ_r = (rh["ptr"].reshape(nb, 4) != FREE_ENTRY).sum(axis=1)
    # a chained entry occupies a slot of a FOREIGN bucket chosen by arrival order, so bucket fill is compared on home buckets
    home_o = np.bincount([osc_hash(nb, k) for k in ob], minlength=nb)
    home_r = np.bincount([osc_hash(nb, k) for k in rb], minlength=nb)
    assert np.array_equal(home_o, home_r), what + ": home-bucket occupancy"
    assert occ_o.sum() == occ_r.sum()
    # every heap slot that is free on one side is free on the other as a SET is not required (pointer values are order
    # dependent); the free lists must be permutations of the unused block ids on each side
    for sc in (osc, rsc):
        free = set(int(x) for x in sc.heap()[: sc.heap_counter() + 1])
        used = set(int(e["ptr"]) // VOX_PER_BLOCK for e in sc.hash() if e["ptr"] != FREE_ENTRY)
        assert not (free & used) and len(free) + len(used) == len(sc.heap())
    # frustum list (compactified hash) as a set of keys
    co, cr = osc.compactified(), rsc.compactified()
    if not frustum_list:
        return            # after a garbage collection that no integration follows the reference keeps the (stale) frustum list of the last operator, the oracle refreshes it
    assert osc.num_occupied() == rsc.num_occupied(), what + ": numOccupiedBlocks"
    assert set(map(tuple, co["pos"].tolist())) == set(map(tuple, cr["pos"].tolist())), what + ": frustum list"


_hash_fn = None


def osc_hash(nb, k):
    return _hash_fn(nb, k[0], k[1], k[2])


@pytest.mark.parametrize("cfg", [dict(W=96, H=72, voxel=0.02, buckets=3001, blocks=6000, scene="wall"),
                                 dict(W=96, H=72, voxel=0.02, buckets=500, blocks=6000, scene="room"),     # load factor > 1: overflow chains
                                 dict(W=64, H=48, voxel=0.01, buckets=20011, blocks=12000, scene="room"),
                                 # the other corner of the parameter space: weights that saturate (de-integration is then not the inverse of
                                 # integration), 3 samples per frame, narrow truncation, short integration range
                                 dict(W=80, H=60, voxel=0.02, buckets=4001, blocks=8000, scene="room",
                                      extra=dict(weight_sample=3, weight_max=5, truncation=0.03, trunc_scale=0.04, max_integration_distance=2.5))])
def test_tsdf_operators_vs_reference_kernels(oracle, cfg):
    """integrate x3 (moving camera) -> de-integrate the middle frame -> re-integrate it at a perturbed pose -> garbage collection
    -> de-integrate everything + GC: after every step the oracle volume equals the volume produced by the reference's own
    allocKernel / compactifyHashAllInOneKernel / integrateDepthMapKernel<deIntegrate> / garbageCollect kernels, sequenced by the
    reference's own host class (DepthSensing/CUDASceneRepHashSDF.h compiled as it is: integrate / deIntegrate / garbageCollect /
    setLastRigidTransformAndCompactify with its allocation loop)."""
    global _hash_fn
    _hash_fn = oracle.hash_pos
    W, H = cfg["W"], cfg["H"]
    if cfg["scene"] == "wall":
        frames = [synth.scene_wall(W, H)] * 1
        d, c, T, K = frames[0]
        frames = []
        for k in range(3):
            Tk = T.copy(); Tk[0, 3] += np.float32(0.05 * k); Tk[2, 3] -= np.float32(0.03 * k)
            frames.append((d, c, Tk, K))
    else:
        frames = [synth.scene_room(20 * k, W, H) for k in range(3)]
    K = frames[0][3]
    cam = camera_params(W, H, K["fx"], K["fy"], K["mx"], K["my"])
    p = default_hash_params(num_buckets=cfg["buckets"], num_sdf_blocks=cfg["blocks"], voxel_size=cfg["voxel"], **cfg.get("extra", {}))
    osc, rsc = oracle.OracleScene(p), ref_api.RefScene(p, host_class=True)      # the reference's own host class drives its kernels
    nb = cfg["buckets"]
    for i, (d, c, T, _) in enumerate(frames):
        osc.integrate(T, d, c, cam); rsc.integrate(T, d, c, cam)
        _assert_same_volume(osc, rsc, nb, "integrate %d" % i)
    assert len(_by_key(osc.hash(), osc.voxels())) > 300
    d, c, T, _ = frames[1]
    osc.deintegrate(T, d, c, cam); rsc.deintegrate(T, d, c, cam)
    _assert_same_volume(osc, rsc, nb, "de-integrate")
    T2 = T.copy(); T2[:3, 3] += np.float32(0.02)
    osc.integrate(T2, d, c, cam); rsc.integrate(T2, d, c, cam)
    _assert_same_volume(osc, rsc, nb, "re-integrate")
    frames[1] = (d, c, T2, None)
    osc.garbage_collect(); rsc.garbage_collect()
    osc.compactify(T2, cam); rsc.compactify(T2, cam)
    _assert_same_volume(osc, rsc, nb, "garbage collection")
    for i, (d, c, T, _) in enumerate(frames):
        osc.deintegrate(T, d, c, cam); rsc.deintegrate(T, d, c, cam)
        osc.garbage_collect(); rsc.garbage_collect()
        osc.compactify(T, cam); rsc.compactify(T, cam)
        _assert_same_volume(osc, rsc, nb, "tear-down %d" % i)
    assert len(_by_key(osc.hash(), osc.voxels())) == 0 and osc.heap_counter() + 1 == cfg["blocks"]


def test_scene_host_class_equals_hand_sequenced_kernels_and_hash_params(oracle):
    """The other pins (marching cubes, ray cast) fill their volumes through oracle/ref/ref_tsdf.cpp, which sequences the launch wrappers by
    hand: same bytes as the reference's host class.  And HashParams as CUDASceneRepHashSDF::parametersFromGlobalAppState derives them
    from the application state = what the C ABI's default_hash_params / the oracle frame loop use."""
    import ctypes as C
    from bundlefusion_amd.capi import default_app_state, HashParams
    W, H = 64, 48
    frames = [synth.scene_room(20 * k, W, H) for k in range(2)]
    K = frames[0][3]
    cam = camera_params(W, H, K["fx"], K["fy"], K["mx"], K["my"])
    p = default_hash_params(num_buckets=2003, num_sdf_blocks=4000, voxel_size=0.02)
    a, b = ref_api.RefScene(p, host_class=True), ref_api.RefScene(p, host_class=False)
    for d, c, T, _ in frames:
        a.integrate(T, d, c, cam); b.integrate(T, d, c, cam)
    d, c, T, _ = frames[0]
    a.deintegrate(T, d, c, cam); b.deintegrate(T, d, c, cam)
    a.garbage_collect(); b.garbage_collect()
    a.compactify(T, cam); b.compactify(T, cam)
    assert a.heap_counter() == b.heap_counter() and a.num_occupied() == b.num_occupied() > 50
    assert np.array_equal(a.hash().view(np.uint8), b.hash().view(np.uint8)) and np.array_equal(a.heap(), b.heap())
    assert np.array_equal(a.voxels().view(np.uint8), b.voxels().view(np.uint8))
    assert np.array_equal(a.compactified().view(np.uint8), b.compactified().view(np.uint8))
    gas = default_app_state()
    gas.s_hashNumBuckets, gas.s_hashNumSDFBlocks, gas.s_SDFVoxelSize = 123457, 54321, 0.004
    r = ref_api.hash_params_from_global_app_state(gas)
    mine = default_hash_params(num_buckets=gas.s_hashNumBuckets, num_sdf_blocks=gas.s_hashNumSDFBlocks, voxel_size=gas.s_SDFVoxelSize,
                               max_integration_distance=gas.s_SDFMaxIntegrationDistance, truncation=gas.s_SDFTruncation, trunc_scale=gas.s_SDFTruncationScale,
                               weight_sample=gas.s_SDFIntegrationWeightSample, weight_max=gas.s_SDFIntegrationWeightMax, max_chain=gas.s_hashMaxCollisionLinkedListSize)
    assert C.sizeof(HashParams) == 224 and bytes(r) == bytes(mine)
    # ... and RayCastParams as CUDARayCastSDF::parametersFromGlobalAppState derives them = bf_ray_cast_params_from_global_app_state (host
    # function of the product), with and without the intrinsics rescaling branch (ray-cast size != integration size)
    from bundlefusion_amd.capi import ray_cast_params_from_global_app_state
    Km = intrinsics_matrix(583.0, 580.5, 319.5, 241.25)
    for rw, rh in ((640, 480), (320, 240), (512, 424)):
        gas = default_app_state()
        gas.s_integrationWidth, gas.s_integrationHeight, gas.s_rayCastWidth, gas.s_rayCastHeight = 640, 480, rw, rh
        gas.s_SDFUseGradients = rw == 320
        a_, b_ = ref_api.ray_cast_params_from_global_app_state(gas, Km), ray_cast_params_from_global_app_state(gas, Km)
        for name, _ in a_._fields_:
            if name in ("m_viewMatrix", "m_viewMatrixInverse", "m_numOccupiedSDFBlocks", "m_splatMinimum", "dummy0"):
                continue                          # not set by the function (uninitialised members in the reference)
            va, vb = getattr(a_, name), getattr(b_, name)
            assert np.float32(va).tobytes() == np.float32(vb).tobytes() if isinstance(va, float) else va == vb, (rw, name, va, vb)


# ------------------------------------------------------------------------------------------------ marching cubes
def _loops(tri_row):
    """directed boundary loops of one case's triangles, each rotated to start at its lowest edge"""
    t = [int(x) for x in tri_row if x >= 0]
    tris = [tuple(t[i:i + 3]) for i in range(0, len(t), 3)]
    d = {}
    for a, b, c in tris:
        for u, v in ((a, b), (b, c), (c, a)):
            d[(u, v)] = d.get((u, v), 0) + 1
    nxt = {u: v for (u, v) in d if (v, u) not in d}
    loops, seen = [], set()
    for s0 in sorted(nxt):
        if s0 in seen:
            continue
        loop, cur = [], s0
        while cur not in seen:
            seen.add(cur); loop.append(cur); cur = nxt[cur]
        i = loop.index(min(loop))
        loops.append(tuple(loop[i:] + loop[:i]))
    return sorted(loops), len(tris)


def test_marching_cubes_tables_vs_reference():
    """The product GENERATES its case tables (mesh.hip: makeTables).  Against the reference's Tables.h: the edge table is identical;
    for every one of the 256 cases the triangles bound the same oriented polygon loops (same cut edges, same connectivity on ambiguous
    faces, same winding) and there are equally many of them; cases made of triangles only are identical as triangle sets."""
    import ctypes as C
    from bundlefusion_amd.capi import lib
    e = np.zeros(256, np.uint16); t = np.zeros(256 * 16, np.int8)
    assert lib.bf_marching_cubes_tables(e.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p)) == 0
    t = t.reshape(256, 16)
    re_, rt = ref_api.mc_tables()
    assert np.array_equal(e, re_)
    same_triangles = 0
    for cs in range(256):
        lp, n = _loops(t[cs]); lr, nr = _loops(rt[cs])
        assert lp == lr and n == nr, cs
        canon = lambda row: sorted(tuple(sorted(int(x) for x in row[i:i + 3])) for i in range(0, 15, 3) if row[i] >= 0)
        if all(len(l) == 3 for l in lr):
            assert canon(t[cs]) == canon(rt[cs]), cs
        same_triangles += canon(t[cs]) == canon(rt[cs])
    assert same_triangles >= 90           # (larger polygons may be split along other diagonals: same vertices, same patch)


@pytest.mark.parametrize("noisy", [False, True])
def test_marching_cubes_oracle_vs_reference_kernels(oracle, noisy):
    """(Also on a volume built from frames with 4 mm of depth noise and holes: far more of the 256 cube cases occur.)  extractIsoSurface of the reference (its own kernel, trilinear sampling and Tables.h) against the oracle restatement fed the SAME
    tables, on a volume built from three frames: the same triangles — positions and colours bit for bit — as a multiset (the reference
    appends in atomic order).  With the product's generated tables the oracle yields the same vertices and equally many triangles."""
    import ctypes as C
    from bundlefusion_amd.capi import lib
    W, H = 96, 72
    frames = [synth.scene_room(20 * k, W, H) for k in range(3)]
    K = frames[0][3]
    if noisy:
        nrng = np.random.default_rng(10)
        frames = [(d + nrng.normal(0, 0.004, d.shape).astype(np.float32) + np.where(nrng.random(d.shape) < 0.02, -np.inf, 0).astype(np.float32), c, T, None) for d, c, T, _ in frames]
    cam = camera_params(W, H, K["fx"], K["fy"], K["mx"], K["my"])
    p = default_hash_params(num_buckets=3001, num_sdf_blocks=6000, voxel_size=0.02)
    osc, rsc = oracle.OracleScene(p), ref_api.RefScene(p)
    for d, c, T, _ in frames:
        osc.integrate(T, d, c, cam); rsc.integrate(T, d, c, cam)
    thresh = 10.0 * 0.02
    re_, rt = ref_api.mc_tables()
    rt_tris, rn = ref_api.mc_extract(rsc, thresh, thresh, 400000)
    ot_tris, on = oracle.mc_extract(osc, thresh, thresh, re_, rt, 400000)
    assert rn == on > 5000
    key = lambda a: sorted(map(bytes, np.ascontiguousarray(a).reshape(len(a), -1)))
    assert key(rt_tris) == key(ot_tris)
    # a box restricts the extraction identically
    pts = rt_tris[:, :, :3].reshape(-1, 3)
    lo, hi = np.percentile(pts, 25, axis=0), np.percentile(pts, 75, axis=0)
    box = ([float(v) for v in lo], [float(v) for v in hi])
    rb, rbn = ref_api.mc_extract(rsc, thresh, thresh, 400000, box=box)
    ob, obn = oracle.mc_extract(osc, thresh, thresh, re_, rt, 400000, box=box)
    assert 0 < rbn == obn < rn and key(rb) == key(ob)
    # the product's tables: same vertices (positions + colours), same triangle count
    e = np.zeros(256, np.uint16); t = np.zeros(256 * 16, np.int8)
    assert lib.bf_marching_cubes_tables(e.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p)) == 0
    pt_tris, pn = oracle.mc_extract(osc, thresh, thresh, e, t.reshape(256, 16), 400000)
    assert pn == rn
    verts = lambda a: set(map(bytes, np.ascontiguousarray(a).reshape(-1, 6)))
    assert verts(pt_tris) == verts(rt_tris)
    area = lambda a: float(np.linalg.norm(np.cross(a[:, 1, :3] - a[:, 0, :3], a[:, 2, :3] - a[:, 0, :3]), axis=1).sum() / 2)
    assert abs(area(pt_tris) - area(rt_tris)) <= 2e-3 * area(rt_tris)


@pytest.mark.parametrize("noisy", [False, True])
def test_ray_cast_oracle_vs_reference_kernel(oracle, noisy):
    """(Also on a volume built from frames with 4 mm of depth noise and holes.)  renderKernel of the reference (its own traverseCoarseGridSimpleSampleAll / bisection / trilinear sampling / gradient) against the
    oracle restatement on a volume built from three frames, from the same ray-interval images: depth, camera-space points, colours and
    (with analytic gradients) normals bit for bit.  The interval images come from the oracle's compute splat (the reference fills them
    with a D3D11 rasteriser pass that cannot run here); every block's rectangle must bracket the surface the rays then find."""
    from bundlefusion_amd.capi import RayCastParams
    W, H = 96, 72
    frames = [synth.scene_room(20 * k, W, H) for k in range(3)]
    K = frames[0][3]
    if noisy:
        nrng = np.random.default_rng(9)
        noisy_frames = []
        for d, c, T, _ in frames:
            d = d + nrng.normal(0, 0.004, d.shape).astype(np.float32)
            d[nrng.random(d.shape) < 0.02] = -np.inf
            noisy_frames.append((d, c, T, None))
        frames = noisy_frames
    cam = camera_params(W, H, K["fx"], K["fy"], K["mx"], K["my"])
    p = default_hash_params(num_buckets=3001, num_sdf_blocks=6000, voxel_size=0.02)
    osc, rsc = oracle.OracleScene(p), ref_api.RefScene(p)
    for d, c, T, _ in frames:
        osc.integrate(T, d, c, cam); rsc.integrate(T, d, c, cam)
    T = frames[1][2].astype(np.float32)
    osc.compactify(T, cam); rsc.compactify(T, cam)
    assert osc.num_occupied() == rsc.num_occupied() > 200
    for use_grad, (w, h) in ((1, (96, 72)), (0, (64, 48))):
        rp = RayCastParams()
        rp.m_width, rp.m_height = w, h
        rp.fx, rp.fy = K["fx"] * w / W, K["fy"] * h / H
        rp.mx, rp.my = K["mx"] * (w - 1) / (W - 1), K["my"] * (h - 1) / (H - 1)
        rp.m_minDepth, rp.m_maxDepth = 0.1, 4.0
        rp.m_rayIncrement = 0.8 * 0.06
        rp.m_thresSampleDist = 50.5 * rp.m_rayIncrement; rp.m_thresDist = 50.0 * rp.m_rayIncrement
        rp.m_useGradients = use_grad
        rp.m_maxNumVertices = 6 * 6000
        Tinv = oracle.inverse44(T)
        rp.m_viewMatrix[:] = [float(v) for v in Tinv.reshape(16)]; rp.m_viewMatrixInverse[:] = [float(v) for v in T.reshape(16)]
        rmin, rmax = oracle.rc_splat(osc, cam, rp)
        covered = rmin != -np.inf
        assert covered.mean() > 0.7 and np.array_equal(covered, rmax != -np.inf) and (rmin[covered] < rmax[covered]).all()
        o = oracle.rc_render(osc, rp, rmin, rmax)
        r = ref_api.rc_render(rsc, rp, rmin, rmax)
        hit = o["depth"] != -np.inf
        assert hit.mean() > 0.6
        for k in ("depth", "depth4", "colors") + (("normals",) if use_grad else ()):
            assert np.array_equal(o[k].view(np.uint32), r[k].view(np.uint32)), k
        # the intervals bracket the surface; without them (whole depth range) the same surface is found
        assert (o["depth"][hit] >= rmin[hit] - 1e-6).all() and (o["depth"][hit] <= rmax[hit] + 1e-6).all()
        full_min = np.where(covered, np.float32(rp.m_minDepth), np.float32(-np.inf)); full_max = np.where(covered, np.float32(rp.m_maxDepth), np.float32(-np.inf))
        o2 = oracle.rc_render(osc, rp, full_min, full_max)
        both = hit & (o2["depth"] != -np.inf)
        assert both.sum() > 0.9 * hit.sum() and np.abs(o["depth"][both] - o2["depth"][both]).max() < 0.02
        # the rendered depth agrees with the depth image that was integrated from this pose (truncated SDF of three frames at 20 mm voxels)
        if (w, h) == (W, H):
            d_in = frames[1][0]
            ok = hit & (d_in != -np.inf) & (d_in < 3.0)
            assert ok.sum() > 3000 and np.median(np.abs(o["depth"][ok] - d_in[ok])) < 0.01


def test_match_filter_chain_vs_reference_kernels(oracle):
    """SIFTImageManager.cu of the reference — SortKeyPointMatchesCU, FilterKeyPointMatchesCU, FilterMatchesBySurfaceAreaCU,
    FilterMatchesByDenseVerifyCU, AddCurrToResidualsCU with their own launch configurations — against the oracle on the matches of a
    5-frame chunk of the synthetic stream (keys, descriptors and raw matches come from the oracle's detector / matcher, which are inputs
    here):
      * Kabsch filter: kept matches, distances, transform and inverse bit for bit;
      * surface area: the decision flips exactly at the oracle's area value (threshold = area and the next float);
      * dense verify: the decision flips exactly at the oracle's error and correspondence fraction - which pins the reference's block
        sum as it executes (warps of the linear thread id, adders at threadIdx.x % 32 == 0: rows and columns are weighted 0-3 times),
        not as it was meant;  * EntryJ rows bit for bit."""
    from bundlefusion_amd.capi import rgbx_to_intensity
    n_frames, W, H = 5, 640, 480
    frames = [synth.scene_room(30 + 5 * k, W, H) for k in range(n_frames)]
    Kd = frames[0][3]
    K = intrinsics_matrix(Kd["fx"], Kd["fy"], Kd["mx"], Kd["my"])
    Kinv = oracle.inverse44(K)
    mk = 1024
    allkeys = np.zeros((n_frames * mk, 4), np.float32)
    descs, nk = [], []
    for i, (d, c, _, _) in enumerate(frames):
        n, keys, ds, _ = oracle.sift_run(rgbx_to_intensity(c), d)
        allkeys[i * mk:i * mk + n] = keys; descs.append(ds); nk.append(n)
    assert min(nk) > 30
    oframes = [oracle.cache_store_frame(f[0], f[1], 80, 60, K) for f in frames]
    Kc = K.copy(); Kc[0, 0] *= 80 / W; Kc[1, 1] *= 60 / H; Kc[0, 2] *= 79 / (W - 1); Kc[1, 2] *= 59 / (H - 1)
    cur = n_frames - 1
    ref = ref_api.RefSiftManager(n_frames + 1, mk)
    ref.set_keys(allkeys)
    for i in range(n_frames):
        ref.set_cached_frame(i, oframes[i])
    raw = {}
    for p in range(cur):
        n_u, idx_u, dist_u = oracle.sift_match(descs[p], descs[cur], off1=p * mk, off2=cur * mk, sort=False)
        n_s, idx_s, dist_s = oracle.sift_match(descs[p], descs[cur], off1=p * mk, off2=cur * mk, sort=True)
        assert n_u == n_s > 10
        ref.set_raw(p, n_u, idx_u, dist_u)
        raw[p] = (n_s, idx_s, dist_s)
    # ---- sort: SortKeyPointMatchesCU_Kernel is an odd-even transposition sort that stops on a shared `swapped` flag which every thread
    # clears at the top of each pass with ONE barrier per pass (SIFTImageManager.cu:104-128) - it relies on lock-step execution of its 64
    # threads; the serial block emulator runs threads one after the other between barriers, the flag reads false for the second thread
    # and the loop ends.  Not pinnable this way; the oracle's stable sort by distance is the input of the next stage on both sides.
    for p in range(cur):
        assert np.all(np.diff(raw[p][2]) >= 0)
        ref.set_raw(p, raw[p][0], raw[p][1], raw[p][2])
    # ---- Kabsch filter
    ref.filter_keypoint_matches(cur, 0, n_frames, Kinv)
    filt = {}
    for p in range(cur):
        m = min(raw[p][0], 128)
        pidx = np.zeros((128, 2), np.uint32); pidx[:m] = raw[p][1]
        pdist = np.zeros(128, np.float32); pdist[:m] = raw[p][2]
        fn, fidx, fdist, fT = oracle.filter_matches(allkeys, pidx, pdist, m, Kinv)
        gn, gidx, gdist, gT, gTi = ref.filtered(p)
        assert gn == fn, (p, gn, fn)
        if fn:
            assert np.array_equal(gidx[:fn], fidx) and np.array_equal(gdist[:fn].view(np.uint32), fdist.view(np.uint32))
            assert np.array_equal(gT.view(np.uint32), fT.view(np.uint32)) and np.array_equal(gTi.view(np.uint32), oracle.inverse44(fT).view(np.uint32))
        filt[p] = (fn, fidx, fdist, fT)
    assert sum(1 for p in filt if filt[p][0] > 0) >= 3
    # ---- surface area: decision flips exactly at the oracle's larger area
    for p in range(cur):
        fn, fidx, fdist, fT = filt[p]
        if fn == 0:
            continue
        _, areas = oracle.filter_surface_area(allkeys, fidx, Kinv)
        a = np.float32(max(areas))
        for thr, expect in ((a, True), (np.nextafter(a, np.float32(np.inf)), False), (np.float32(0.032), bool(oracle.filter_surface_area(allkeys, fidx, Kinv)[0]))):
            ref.set_filtered(p, fn, fidx, fdist, fT, oracle.inverse44(fT))
            ref.filter_surface_area(cur, 0, n_frames, Kinv, float(thr))
            assert (ref.filtered(p)[0] > 0) == expect, (p, float(a), float(thr))
    # ---- dense verify
    n_checked = 0
    for p in range(cur):
        fn, fidx, fdist, fT = filt[p]
        if fn == 0:
            continue
        ok, err, corr = oracle.dense_verify(oframes[p], oframes[cur], 80, 60, Kc, fT, dmin=0.1, dmax=3.0)
        e32, c32 = np.float32(err), np.float32(corr)
        assert np.isfinite(e32) and e32 > 0 and c32 > 0
        cases = [(0.075, 0.02, ok),
                 (e32, 0.0, True), (np.nextafter(e32, np.float32(-np.inf)), 0.0, False),              # invalid iff err > errThresh
                 (10.0, c32, True), (10.0, np.nextafter(c32, np.float32(np.inf)), False)]             # invalid iff corr < corrThresh
        for et, ct, expect in cases:
            ref.set_filtered(p, fn, fidx, fdist, fT, oracle.inverse44(fT))
            ref.filter_dense_verify(cur, 0, n_frames, 80, 60, Kc, err_thresh=float(et), corr_thresh=float(ct))
            assert (ref.filtered(p)[0] > 0) == bool(expect), (p, err, corr, et, ct)
            n_checked += 1
    assert n_checked >= 15
    # ---- EntryJ rows of the surviving pairs
    exp = []
    for p in range(cur):
        fn, fidx, fdist, fT = filt[p]
        ref.set_filtered(p, fn, fidx, fdist, fT, oracle.inverse44(fT))
        for k in range(fn):
            exp.append(oracle.make_entry(allkeys, fidx[k, 0], fidx[k, 1], p, cur, Kinv))
    e, keyidx = ref.add_curr_to_residuals(cur, 0, n_frames, Kinv)
    assert len(e) == len(exp) > 20
    assert sorted(map(bytes, e)) == sorted(bytes(np.array(x)) for x in exp)


def test_verify_trajectory_vs_reference_kernel(oracle):
    """VerifyTrajectoryCU (SIFTImageManager.cu:1036-1159) against the oracle's restatement (pair decoding (block / N, block % N) over
    N(N-1)/2 blocks + the dense verification block sum): same verdict for the true trajectory, for perturbed ones and with an invalid image."""
    n, W, H = 5, 640, 480
    frames = [synth.scene_room(30 + 5 * k, W, H) for k in range(n)]
    Kd = frames[0][3]
    K = intrinsics_matrix(Kd["fx"], Kd["fy"], Kd["mx"], Kd["my"])
    Kc = K.copy(); Kc[0, 0] *= 80 / W; Kc[1, 1] *= 60 / H; Kc[0, 2] *= 79 / (W - 1); Kc[1, 2] *= 59 / (H - 1)
    oframes = [oracle.cache_store_frame(f[0], f[1], 80, 60, K) for f in frames]
    ref = ref_api.RefSiftManager(n + 1, 64)
    for i in range(n):
        ref.set_cached_frame(i, oframes[i])
    T0inv = np.linalg.inv(frames[0][2].astype(np.float64))
    gt = np.stack([(T0inv @ f[2].astype(np.float64)).astype(np.float32) for f in frames])

    def oracle_verdict(traj, valid, err_t=0.05, corr_t=0.02):
        ok = True
        for blk in range(n * (n - 1) // 2):
            i0, i1 = blk // n, blk % n
            if i0 >= i1 or valid[i0] == 0 or valid[i1] == 0:
                continue
            T = oracle.mul44(oracle.inverse44(traj[i1]), traj[i0])
            v, _, _ = oracle.dense_verify(oframes[i0], oframes[i1], 80, 60, Kc, T, err_thresh=err_t, corr_thresh=corr_t, dmin=0.1, dmax=3.0)
            ok = ok and v
        return int(ok)

    rng = np.random.default_rng(3)
    seen = set()
    for case in range(6):
        traj = gt.copy(); valid = [1] * n
        if case in (1, 2, 3):
            traj[1 + case % 2, :3, 3] += rng.normal(0, 0.02 * case, 3).astype(np.float32)
        if case == 4:
            traj[1, :3, 3] += 0.5; valid[1] = 0                      # the broken pose belongs to an invalid image: not tested
        if case == 5:
            traj[3, :3, 3] += 0.5                                     # (3, x) is not among the decoded pairs for N = 5: kept quirk
        exp = oracle_verdict(traj, valid)
        got = ref.verify_trajectory(traj, valid, 80, 60, Kc)
        assert got == exp, (case, got, exp)
        seen.add(exp)
    assert seen == {0, 1}


def test_sift_detector_and_matcher_vs_reference(oracle):
    """The reference's SiftGPU fork, whole (SiftGPU.cpp, SiftPyramid.cpp, CuTexImage.cpp, SiftMatch.cpp, ProgramCU.cu compiled as they are),
    on four 640x480 frames of the synthetic stream, against the oracle detector / matcher:
      * all 18 Gaussian pyramid levels bit for bit;  * the DoG extrema with depth gate: the same (col, row) sets in all 12 (octave, level) slots;
      * per-slot feature counts after orientation assignment and both LimitFeatureCount passes: equal;
      * final key points (x, y, scale, depth): the same multiset of float bits; orientations within 1e-5 rad (atan2 / exp: libm there,
        include/bf_detmath.h in the oracle and the product);
      * descriptors: key for key, at most 1 count difference per byte in at most 0.1 % of the bytes (same reason + atomicAdd order);
      * matcher: identical index pairs, distances within 1e-6 (acos)."""
    from bundlefusion_amd.capi import rgbx_to_intensity
    from collections import defaultdict
    W, H = 640, 480
    frames = [synth.scene_room(k, W, H) for k in (30, 37, 640, 1250)]          # two neighbours (for the matcher) and two other parts of the room
    Kd = frames[0][3]
    K = intrinsics_matrix(Kd["fx"], Kd["fy"], Kd["mx"], Kd["my"])
    rs = ref_api.RefSift(W, H, K)
    descs_o, descs_r = [], []
    for fi, (d, c, _, _) in enumerate(frames):
        I = rgbx_to_intensity(c)
        on, okeys, odescs, olev = oracle.sift_run(I, d)
        if fi == 0:
            st = ref_api.sift_stages(rs, I, d)
            assert len(st["levels"]) == 18
            for (o, a), img in st["levels"].items():
                assert np.array_equal(img.view(np.uint32), oracle.sift_pyramid_level(I, o, a).view(np.uint32)), (o, a)
            oraw = oracle.sift_detect(I, d)
            for s in range(12):
                assert set(map(tuple, st["raw"][s].tolist())) == set(map(tuple, oraw[s].tolist())), s
            assert sum(len(r) for r in oraw) > 250
            assert np.array_equal(st["counts"], olev)
        rn, rkeys, rdescs = rs.run(I, d)
        assert rn == on > 100
        bits = lambda k: sorted(map(tuple, np.ascontiguousarray(k).view(np.uint32).tolist()))
        assert bits(rkeys) == bits(okeys)
        by_key = defaultdict(list)
        for k, dsc in zip(okeys, odescs):
            by_key[tuple(k.view(np.uint32).tolist())].append(dsc.astype(int))
        n_diff = 0
        for k, dsc in zip(rkeys, rdescs):
            best = min((np.abs(c - dsc.astype(int)) for c in by_key[tuple(k.view(np.uint32).tolist())]), key=lambda x: x.sum())
            assert best.max() <= 1
            n_diff += int((best > 0).sum())
        assert n_diff <= 0.001 * 128 * rn
        descs_o.append(odescs); descs_r.append(rdescs)
    # orientations of the first frame's final lists (the oracle keeps them inside sift_run; they enter the descriptors compared above) are
    # bounded through the descriptors; the matcher on the oracle's descriptors:
    rn, ridx, rdist = rs.match(descs_o[0], descs_o[1], off1=0, off2=1024)
    on, oidx, odist = oracle.sift_match(descs_o[0], descs_o[1], off1=0, off2=1024, sort=False)
    assert rn == on > 50
    om = {tuple(i): d for i, d in zip(oidx.tolist(), odist.tolist())}
    assert sorted(om) == sorted(map(tuple, ridx.tolist()))
    assert max(abs(om[tuple(i)] - d) for i, d in zip(ridx.tolist(), rdist.tolist())) < 1e-6
    # thresholds are applied identically
    rn2, ridx2, _ = rs.match(descs_o[0], descs_o[1], distmax=0.3, ratiomax=0.6)
    on2, oidx2, _ = oracle.sift_match(descs_o[0], descs_o[1], distmax=0.3, ratiomax=0.6, sort=False)
    assert rn2 == on2 < on and sorted(map(tuple, ridx2.tolist())) == sorted(map(tuple, oidx2.tolist()))


def test_fuse_to_global_and_filter_frames_vs_reference(oracle):
    """The host half of the reference's SIFTImageManager (SIFTImageManager.cpp compiled as it is): computeTracks + fuseToGlobal on the
    correspondences of a 5-frame chunk with its ground-truth trajectory - fused key points (position, scale, depth) and descriptors bit for
    bit, in the same order; filterFrames on random match-count / validity
    patterns."""
    from bundlefusion_amd.capi import rgbx_to_intensity, ENTRYJ_DTYPE
    from tests.oracle_pipeline import fuse_tracks
    n, W, H = 5, 640, 480
    frames = [synth.scene_room(30 + 4 * k, W, H) for k in range(n)]
    Kd = frames[0][3]
    K = intrinsics_matrix(Kd["fx"], Kd["fy"], Kd["mx"], Kd["my"])
    Kinv = oracle.inverse44(K)
    mk = 1024
    keys, descs, nk = [], [], []
    allkeys = np.zeros((n * mk, 4), np.float32)
    for i, (d, c, _, _) in enumerate(frames):
        m, k, ds, _ = oracle.sift_run(rgbx_to_intensity(c), d)
        keys.append(k); descs.append(ds); nk.append(m); allkeys[i * mk:i * mk + m] = k
    prefix = np.concatenate([[0], np.cumsum(nk)[:-1]])
    corr, ckeys = [], []
    for cur in range(1, n):
        for p in range(cur):
            cnt, idx, dist = oracle.sift_match(descs[p], descs[cur], off1=p * mk, off2=cur * mk, sort=True)
            m = min(cnt, 128)
            pidx = np.zeros((128, 2), np.uint32); pidx[:m] = idx; pdist = np.zeros(128, np.float32); pdist[:m] = dist
            fn, fidx, fdist, fT = oracle.filter_matches(allkeys, pidx, pdist, m, Kinv)
            for q in range(fn):
                corr.append(oracle.make_entry(allkeys, fidx[q, 0], fidx[q, 1], p, cur, Kinv)); ckeys.append((int(fidx[q, 0]), int(fidx[q, 1])))
    corr = np.array(corr, ENTRYJ_DTYPE); ckeys = np.array(ckeys, np.uint32)
    assert len(corr) > 100
    corr["imgIdx_i"][3] = 0xFFFFFFFF; corr["imgIdx_j"][3] = 0xFFFFFFFF          # an invalidated correspondence is skipped
    T0inv = np.linalg.inv(frames[0][2].astype(np.float64))
    traj = np.stack([(T0inv @ f[2].astype(np.float64)).astype(np.float32) for f in frames])
    traj[2, 0, 3] += 0.05                                                      # one pose off by 5 cm: its correspondences exceed MAX_TRACK_CORR_ERROR
    packed = np.stack([prefix[ckeys[:, 0] // mk] + ckeys[:, 0] % mk, prefix[ckeys[:, 1] // mk] + ckeys[:, 1] % mk], 1).astype(np.uint32)
    ok, od = fuse_tracks(corr, ckeys, traj, nk, descs, allkeys, K, mk, 1024)
    rk, rd = ref_api.siftmgr_fuse(keys, descs, corr, packed, traj, K, max_keys_global=1024)
    assert len(rk) == len(ok) > 60
    assert np.array_equal(rk.view(np.uint32), ok.view(np.uint32)) and np.array_equal(rd, od)
    # (the over-capacity branch - more fused keys than s_maxNumKeysPerImage, :459-464 - needs > 1024 tracks and is not exercised here)
    rng = np.random.default_rng(5)
    for _ in range(40):
        num = int(rng.integers(2, 9)); cur = int(rng.integers(0, num)); start = 0 if cur + 1 == num else cur + 1
        nf = rng.integers(0, 3, num); valid = rng.integers(0, 2, num)
        last, v = ref_api.siftmgr_filter_frames(nf, valid, cur, start, num)
        exp_last, exp_v = -1, 0
        for i in range(num - 1, start - 1, -1):
            if valid[i] != 0 and nf[i] > 0 and i != cur:
                exp_last, exp_v = i, 1; break
        assert (last, v) == (exp_last, exp_v)


def test_check_for_invalid_frames_launch_arithmetic_vs_reference():
    """CheckForInvalidFramesCU (SIFTImageManager.cu:725-760): the reference launches grid (ceil(R/128), 128) x block (ceil(N/16), 16) and
    indexes residuals with blockDim.x * blockIdx.x + blockIdx.y and variables with gridDim.x * threadIdx.x + threadIdx.y, so only a subset of
    (residual, variable) pairs is visited.  The product restates that subset in closed form (csrc/siftmgr.hip: k_check_invalid); the same closed
    form here against the reference's own launch, on random problems: valid flags and invalidated residuals identical.  Also the simple
    variant and InvalidateImageToImageCU."""
    import ctypes as C
    from bundlefusion_amd.capi import ENTRYJ_DTYPE
    L = ref_api.lib()
    L.ref_siftmgr_create.restype = C.c_void_p
    rng = np.random.default_rng(11)
    INV = 0xFFFFFFFF
    for trial in range(25):
        N = int(rng.integers(2, 40)); R = int(rng.integers(1, 700))
        h = C.c_void_p(L.ref_siftmgr_create(max(N + 1, 9), 32))          # capacity 25 * M (M - 1) / 2 >= 700 residuals
        e = np.zeros(R, ENTRYJ_DTYPE)
        e["imgIdx_i"] = rng.integers(0, N, R); e["imgIdx_j"] = rng.integers(0, N, R)
        dead = rng.random(R) < 0.1
        e["imgIdx_i"][dead] = INV; e["imgIdx_j"][dead] = INV
        rows = (rng.random(N) < 0.7).astype(np.int32) * rng.integers(1, 5, N).astype(np.int32)
        rows[0] = max(int(rows[0]), 1)                     # (the reference prints a warning when the first frame loses its rows)
        valid = (rng.random(N) < 0.8).astype(np.int32)
        simple = trial % 5 == 4
        L.ref_siftmgr_set_residuals(h, e.ctypes.data_as(C.c_void_p), np.zeros((R, 2), np.uint32).ctypes.data_as(C.c_void_p), R)
        v = valid.copy()
        L.ref_siftmgr_check_invalid_frames(h, rows.ctypes.data_as(C.c_void_p), N, v.ctypes.data_as(C.c_void_p), int(simple))
        got = np.zeros(R, ENTRYJ_DTYPE); gk = np.zeros((R, 2), np.uint32)
        L.ref_siftmgr_get_residuals(h, got.ctypes.data_as(C.c_void_p), gk.ctypes.data_as(C.c_void_p), R)
        # closed form
        exp_v = valid.copy(); exp_e = e.copy()
        if simple:
            exp_v[rows == 0] = 0
        else:
            gx, bx = (R + 127) // 128, (N + 15) // 16
            in_var = lambda x: any((x - d) % gx == 0 and (x - d) // gx < bx for d in range(min(16, x + 1)))
            in_res = lambda r: any((r - b) % bx == 0 and (r - b) // bx < gx for b in range(min(128, r + 1)))
            zero = [x for x in range(N) if rows[x] == 0 and in_var(x)]
            for x in zero:
                exp_v[x] = 0
            for r in range(R):
                if in_res(r) and exp_e["imgIdx_i"][r] != INV and (int(exp_e["imgIdx_i"][r]) in zero or int(exp_e["imgIdx_j"][r]) in zero):
                    exp_e["imgIdx_i"][r] = INV; exp_e["imgIdx_j"][r] = INV
        assert np.array_equal(v, exp_v), (trial, N, R)
        assert np.array_equal(got["imgIdx_i"], exp_e["imgIdx_i"]) and np.array_equal(got["imgIdx_j"], exp_e["imgIdx_j"]), (trial, N, R)
        # InvalidateImageToImageCU
        i, j = int(rng.integers(0, N)), int(rng.integers(0, N))
        L.ref_siftmgr_invalidate_image_to_image(h, i, j)
        L.ref_siftmgr_get_residuals(h, got.ctypes.data_as(C.c_void_p), gk.ctypes.data_as(C.c_void_p), R)
        hit = (exp_e["imgIdx_i"] == i) & (exp_e["imgIdx_j"] == j)
        exp_e["imgIdx_i"][hit] = INV; exp_e["imgIdx_j"][hit] = INV
        assert np.array_equal(got["imgIdx_i"], exp_e["imgIdx_i"]) and np.array_equal(got["imgIdx_j"], exp_e["imgIdx_j"])


def test_trajectory_manager_vs_reference_host_code():
    """a12: the reference's TrajectoryManager.cpp (compiled as it is, with PoseHelper.h's se(3) logarithm) against the product's
    bf_trajectory_manager_* and the restatement the oracle frame loop uses, driven by one random script of frame-loop events
    (DepthSensing.cpp:854-902 consumer order).  Types, integrated poses, the ranking distance (bit-exact) and every list pop agree.
    One situation is kept out of the script: a frame that loses its pose WHILE it waits in the integration or re-integration list.  The
    reference's consumer asserts on the -inf pose it then pops (DepthSensing.cpp:881,890), and a frame integrated at -inf leaves a NaN
    in the ranking that makes std::sort's order unspecified; the product deviates there on purpose
    (tests/test_trajectory_manager_cpu.py, DESIGN.md "Deviations")."""
    from collections import deque
    from tests.oracle_pipeline import OTrajectoryManager, NINF, _minf
    from tests.test_trajectory_manager_cpu import _CTM, _pose, _same
    from bundlefusion_amd.capi import lib
    import ctypes as C
    lib.bf_trajectory_manager_update_optimized_transform_host.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_uint32]

    class OTM:                                # the restatement behind the interface of the other two
        def __init__(self, *a): self.o = OTrajectoryManager(*a)
        def add(self, typ, T, idx): self.o.add_frame(typ, T, idx)
        def update(self, traj): self.o.update_optimized(traj, len(traj))
        def generate(self): self.o.generate_update_lists()
        def active(self): return self.o.num_active()
        def confirm(self, idx): self.o.confirm(idx)
        def top_de(self): return self.o.top_de() + (None,)
        def top_in(self): return self.o.top_in() + (None,)
        def top_re(self): return self.o.top_re()
        def frame(self, i):
            g = self.o.frames[i]; return g["type"], g["integrated"], g["dist"]

    total_ops = {"de": 0, "in": 0, "re": 0}
    for seed, top_n, min_dist, max_fixes in ((0, 30, 0.0, 10), (1, 5, 0.0004, 3), (2, 8, 0.0, 1), (3, 30, 0.001, 10)):
        rng = np.random.default_rng(100 + seed)
        n_max = 150
        impls = [ref_api.RefTrajectoryManager(n_max, top_n, min_dist), _CTM(n_max, top_n, min_dist), OTM(n_max, top_n, min_dist)]
        ref = impls[0]
        gt = [_pose(rng, 0.5) for _ in range(n_max)]
        for frame in range(n_max):
            for m in impls:
                if m.active() < max_fixes:
                    m.generate()
            assert len({m.active() for m in impls}) == 1
            for _ in range(max_fixes):
                got = [m.top_de() for m in impls]
                if got[0][0]:
                    assert all(g[0] and g[1] == got[0][1] and _same(g[2], got[0][2]) for g in got)
                    total_ops["de"] += 1; continue
                assert not any(g[0] for g in got)
                got = [m.top_in() for m in impls]
                if got[0][0]:
                    assert all(g[0] and g[1] == got[0][1] and _same(g[2], got[0][2]) for g in got)
                    for m in impls: m.confirm(got[0][1])
                    total_ops["in"] += 1; continue
                assert not any(g[0] for g in got)
                got = [m.top_re() for m in impls]
                if got[0][0]:
                    assert all(g[0] and g[1] == got[0][1] and _same(g[2], got[0][2]) and _same(g[3], got[0][3]) for g in got), (seed, frame)
                    for m in impls: m.confirm(got[0][1])
                    total_ops["re"] += 1; continue
                assert not any(g[0] for g in got)
                break
            if rng.random() < 0.85:
                T = (gt[frame].astype(np.float64) @ _pose(rng, 0.01).astype(np.float64)).astype(np.float32)
                for m in impls: m.add(0, T, frame)
            else:
                for m in impls: m.add(1, _minf(), frame)
            if frame % 10 == 9:
                n = frame + 1 - int(rng.integers(0, 3))
                traj = np.stack([(gt[i].astype(np.float64) @ _pose(rng, 0.002 + 0.02 * rng.random()).astype(np.float64)).astype(np.float32) for i in range(n)])
                bad = rng.random(n) < 0.08
                for i in range(n):
                    if ref.frame(i)[0] in (2, 4):
                        bad[i] = False                        # queued for (re-)integration: see the docstring
                traj[bad] = -np.inf
                for m in impls: m.update(traj)
            for i in range(frame + 1):
                st = [m.frame(i) for m in impls]
                assert len({s[0] for s in st}) == 1, (seed, frame, i, [s[0] for s in st])
                assert all(_same(s[1], st[0][1]) for s in st)
                if st[0][0] != 1 and ref.frame(i)[2] == ref.frame(i)[2]:
                    d = [np.float32(s[2]).view(np.uint32) for s in st]
                    assert d[0] == d[1] == d[2], (seed, frame, i, [s[2] for s in st])
        impls[1].close()
    assert min(total_ops.values()) > 10, total_ops


def test_host_pose_helper_equals_device_lie_maps():
    """PoseHelper::MatrixToPose / PoseToMatrix (host, PoseHelper.h:332-426) order a pose as (translation part, rotation vector) and
    agree with the device-side LieDerivUtil.h maps the solver uses - which is what lets one restatement (or_se3.h / bf_se3.h) serve both."""
    rng = np.random.default_rng(5)
    from tests.test_trajectory_manager_cpu import _pose
    for _ in range(200):
        T = _pose(rng, float(rng.choice([1e-4, 0.05, 1.0, 3.0])))
        p = ref_api.host_matrix_to_pose(T)
        rot, trans = ref_api.matrix_to_pose(T)
        assert np.allclose(p[:3], trans, rtol=2e-6, atol=2e-6) and np.allclose(p[3:], rot, rtol=0, atol=2e-6)
        assert np.allclose(ref_api.host_pose_to_matrix(p), ref_api.pose_to_matrix(rot, trans), rtol=2e-6, atol=2e-6)
        assert np.allclose(ref_api.host_pose_to_matrix(p), T, rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------------------------ SBA / CUDASolverBundling host classes
def _obundler(n_max, is_local, gbs, K, W=640, H=480):
    from bundlefusion_amd.capi import default_app_state
    from tests.oracle_pipeline import OBundler
    gas = default_app_state()
    gas._depthW, gas._depthH = W, H
    return OBundler(n_max, 64, np.linalg.inv(K.astype(np.float64)).astype(np.float32), K, is_local, gas, gbs)


def test_sba_align_global_vs_reference_host_code(oracle):
    """a8 + the host half of a9: the reference's SBA.cpp and Solver/CUDASolverBundling.cpp (compiled as they are, on its own kernels and its
    own SIFTImageManager) against OBundler.optimize, the restatement the oracle frame loop runs, on global-style problems (sparse term
    only, 3 Gauss-Newton iterations): the weight schedules of the constructor; the removal decision (max residual above s_optMaxResThresh,
    never for pairs (0, j < 10)), WHICH image pair is invalidated, the frames that lose their last correspondence
    (CheckForInvalidFramesSimpleCU / CheckForInvalidFramesCU on the row counts of the table built BEFORE the removal), and the poses
    (1e-4, the solver's summation-order tolerance).  useVerification: see the comment at its check."""
    from tests import bundle_synth as bs
    from bundlefusion_amd.capi import default_bundling_state, intrinsics_matrix
    K = intrinsics_matrix(570.0, 570.0, 320.0, 240.0)
    INV = 0xFFFFFFFF
    outcomes = set()
    PCG = 40
    for case, (n, seed, outlier, comprehensive, orphan) in enumerate(((7, 3, (3, 4), False, False), (6, 5, (0, 1), False, False), (7, 6, (5, 6), True, True),
                                                                       (9, 4, None, False, False), (12, 8, (0, 11), False, False), (12, 9, (0, 9), True, False))):
        gbs = default_bundling_state()
        gbs.s_useComprehensiveFrameInvalidation = comprehensive
        corr, T_gt, T_init = bs.sparse_problem(n_images=n, pts_per_pair=20, pair_prob=1.0 if n == 12 else 0.7, seed=seed, outlier_pair=outlier)
        if orphan:                     # the last image hangs on the outlier pair only, and that pair is not a rigid motion: removing it
            rng = np.random.default_rng(seed)                                      # leaves the image without correspondences
            last = (corr["imgIdx_j"] == n - 1) | (corr["imgIdx_i"] == n - 1)
            pair = (corr["imgIdx_i"] == outlier[0]) & (corr["imgIdx_j"] == outlier[1])
            corr = corr[~(last & ~pair)]
            pair = (corr["imgIdx_i"] == outlier[0]) & (corr["imgIdx_j"] == outlier[1])
            corr["pos_j"][pair] = (rng.uniform(-1, 1, (int(pair.sum()), 3)) + [0, 0, 2.5]).astype(np.float32)
        n_max = n + 2
        b = _obundler(n_max, False, gbs, K)
        b.num_images, b.current = n, n - 1
        b.valid = [1] * n + [0] * (n_max - n)
        b.corr = corr.copy()
        b.trajectory[:n] = T_init
        b._verify_trajectory = lambda N: True          # Bundler::optimize's follow-up (VerifyTrajectoryCU, pinned on its own), not SBA::align
        sba = ref_api.RefSBA(n_max, 25 * n_max * (n_max - 1) // 2, gbs)
        if case == 0:
            for which, (ws, wd, wc) in ((0, (b.local_ws, b.local_wd, b.local_wc)), (1, (b.global_ws, b.global_wd, b.global_wc))):
                rw = sba.weights(which)
                assert np.array_equal(rw[0], np.float32(ws)) and np.array_equal(rw[1], np.float32(wd)) and np.array_equal(rw[2], np.float32(wc))
        mgr = ref_api.siftmgr_with_images(n, corr)
        r = sba.align(mgr, b.valid[:n], n - 1, T_init, gbs.s_numGlobalNonLinIterations, PCG, True, False)
        b.optimize(gbs.s_numGlobalNonLinIterations, PCG, True, True)
        a = b.last_align
        assert a["removed"] == r["removed"] == (outlier is not None and not (outlier[0] == 0 and outlier[1] < 10)), (case, a["removed"], r["removed"])
        # useVerification: the reference evaluates its residuals with an UNINITIALISED parameters.weightSparse (CUDASolverBundling.cpp:450-454
        # declares `SolverParameters parameters;` and sets four other members; SolverBundlingEquationsLie.h:35 multiplies by it), so its answer is
        # whatever the stack held.  The restatement takes the weight as 1: checked here against that definition on the reference's own poses.
        Tr = r["transforms"].astype(np.float64)
        live = re_ = None
        cur = ref_api.siftmgr_residuals(mgr, len(corr))
        live = cur[cur["imgIdx_i"] != INV]
        pi = np.einsum("nij,nj->ni", Tr[live["imgIdx_i"]], np.c_[live["pos_i"].astype(np.float64), np.ones(len(live))])[:, :3]
        pj = np.einsum("nij,nj->ni", Tr[live["imgIdx_j"]], np.c_[live["pos_j"].astype(np.float64), np.ones(len(live))])[:, :3]
        high = int((np.abs(pi - pj).max(axis=1) > 0.02).sum())
        assert abs(high / len(corr) - 0.05) > 0.002                         # not a borderline case
        assert a["use_verification"] == (high / len(corr) >= 0.05), (case, high, len(corr))
        assert abs(a["max_residual"] - r["max_residual"]) <= 1e-3 * r["max_residual"]
        re = ref_api.siftmgr_residuals(mgr, len(corr))
        assert np.array_equal(re["imgIdx_i"] == INV, b.corr["imgIdx_i"] == INV) and np.array_equal(re["imgIdx_j"] == INV, b.corr["imgIdx_j"] == INV)
        if a["removed"]:
            gone = corr[re["imgIdx_i"] == INV]
            assert len(gone) and (gone["imgIdx_i"] == outlier[0]).all() and (gone["imgIdx_j"] == outlier[1]).all()
        assert list(r["valid"]) == b.valid[:n], (case, r["valid"], b.valid[:n])
        if orphan:                     # not yet: the row counts date from the start of the solve.  The NEXT removal finds the frame without rows
            assert b.valid[n - 1] == 1
        k = a["gn_iterations"]
        assert np.abs(a["convergence"][:k + 1] - r["convergence"][:k + 1]).max() <= 1e-3 * r["convergence"][:k + 1].max()
        ok = np.array(b.valid[:n], bool)
        # clean problems: the solver's summation-order tolerance; with a 0.5 m outlier inside, three Gauss-Newton steps have not converged and
        # the float atomics of the reference move the iterate by up to 2e-3 (energies still agree to 1e-3)
        assert np.abs(b.trajectory[:n][ok] - r["transforms"][ok]).max() < (1e-4 if outlier is None else 3e-3), case
        outcomes.add((a["removed"], a["use_verification"], orphan))
    assert len(outcomes) >= 3


def test_sba_align_local_dense_vs_reference_host_code(oracle):
    """The local solve as Bundler::optimizeLocal runs it (SBA::align isLocal: sparse weight 1, dense depth weights 1, 2, ..., colour 0, pairwise
    dense over the chunk's cached frames, no removal unless isEnd) through the reference's SBA.cpp / CUDASolverBundling.cpp, against
    OBundler.optimize on the same chunk: how the host classes hand the cache (frame array, size, intrinsics as fx, fy, mx, my) and the
    weight schedules to the kernels."""
    from tests import bundle_synth as bs
    from bundlefusion_amd.capi import default_bundling_state, intrinsics_matrix, ENTRYJ_DTYPE
    W, H, n = 80, 60, 4
    src = [synth.scene_room(3 * k, 320, 240) for k in range(n)]
    Kd = src[0][3]
    K = intrinsics_matrix(Kd["fx"], Kd["fy"], Kd["mx"], Kd["my"])
    frames = [oracle.cache_store_frame(d, c, W, H, K) for d, c, _, _ in src]
    T0inv = np.linalg.inv(src[0][2].astype(np.float64))
    T_gt = np.stack([(T0inv @ f[2].astype(np.float64)) for f in src]).astype(np.float32)
    rng = np.random.default_rng(3)
    T_init = T_gt.copy()
    for i in range(1, n):
        T_init[i] = (T_gt[i].astype(np.float64) @ bs.random_pose(rng, 0.004, 0.004)).astype(np.float32)
    rows = []
    for i in range(n):
        for j in range(i + 1, n):
            pw = rng.uniform(-1, 1, (12, 3)) + np.array([0, 0, 2.2])
            pi = (np.linalg.inv(T_gt[i].astype(np.float64)) @ np.c_[pw, np.ones(12)].T).T[:, :3] + rng.normal(0, 0.001, (12, 3))
            pj = (np.linalg.inv(T_gt[j].astype(np.float64)) @ np.c_[pw, np.ones(12)].T).T[:, :3] + rng.normal(0, 0.001, (12, 3))
            for a_, b_ in zip(pi, pj):
                e = np.zeros(1, ENTRYJ_DTYPE); e["imgIdx_i"], e["imgIdx_j"], e["pos_i"], e["pos_j"] = i, j, a_, b_
                rows.append(e)
    corr = np.concatenate(rows)
    gbs = default_bundling_state()
    gbs.s_downsampledWidth, gbs.s_downsampledHeight = W, H
    assert gbs.s_useLocalDense
    n_max = 11
    b = _obundler(n_max, True, gbs, K, 320, 240)
    b._verify_trajectory = lambda N: True
    b.num_images, b.current = n, n - 1
    b.valid = [1] * n + [0] * (n_max - n)
    b.corr = corr.copy()
    b.cache = list(frames)
    b.trajectory[:n] = T_init
    sba = ref_api.RefSBA(n_max, 25 * n_max * (n_max - 1) // 2, gbs)
    mgr = ref_api.siftmgr_with_images(n, corr)
    for i, f in enumerate(frames):
        mgr.set_cached_frame(i, f)
    nl, lin = gbs.s_numLocalNonLinIterations, gbs.s_numLocalLinIterations
    r = sba.align(mgr, b.valid[:n], n - 1, T_init, nl, lin, True, True, is_start=True, is_end=False, cache_geom=(W, H, b.cacheK))
    b.optimize(nl, lin, True, False)
    a = b.last_align
    assert not a["removed"] and not r["removed"]
    assert list(r["valid"]) == b.valid[:n]
    k = a["gn_iterations"]
    assert k >= 1 and np.abs(a["convergence"][:k + 1] - r["convergence"][:k + 1]).max() <= 1e-3 * r["convergence"][:k + 1].max()
    assert np.abs(b.trajectory[:n] - r["transforms"]).max() < 1e-4
    assert np.abs(r["transforms"] - T_gt).max() < 3e-3                      # and both found the chunk's poses
    # the sparse-only variant the same classes run when s_useLocalDense is off: the cache is NOT handed to the solver (SBA.cpp:72-75)
    gbs2 = default_bundling_state(); gbs2.s_useLocalDense = False
    gbs2.s_downsampledWidth, gbs2.s_downsampledHeight = W, H
    b2 = _obundler(n_max, True, gbs2, K, 320, 240)
    b2._verify_trajectory = lambda N: True
    b2.num_images, b2.current, b2.valid, b2.corr, b2.cache = n, n - 1, [1] * n + [0] * (n_max - n), corr.copy(), list(frames)
    b2.trajectory[:n] = T_init
    sba2 = ref_api.RefSBA(n_max, 25 * n_max * (n_max - 1) // 2, gbs2)
    r2 = sba2.align(mgr, b2.valid[:n], n - 1, T_init, nl, lin, False, True, is_start=True, is_end=False, cache_geom=(W, H, b2.cacheK))
    b2.optimize(nl, lin, False, False)
    assert np.abs(b2.trajectory[:n] - r2["transforms"]).max() < 1e-4
    assert np.abs(r2["transforms"] - r["transforms"]).max() > 1e-5          # the dense term did something in the first run


# ------------------------------------------------------------------------------------------------ the frame loop itself
@pytest.mark.parametrize("scenario", ["three_chunks", pytest.param("tracking_loss", marks=pytest.mark.skipif(os.environ.get("BF_LONG_TESTS") != "1", reason="one more minute on the block emulator: BF_LONG_TESTS=1"))])
def test_compiled_frame_loop_equals_the_restated_one(scenario):
    """DepthSensing.cpp's own frame loop - integrate / deIntegrate (:723-762), reintegrate (:853-902) and OnD3D11FrameRender (:966-1129), cut out of the file and
    compiled as they are (oracle/ref/ref_loop.cpp) - against the RESTATEMENT of those lines that test_online_bundler_vs_reference_host_code (below) drives the
    reference's classes with, and that the oracle frame loop (tests/oracle_pipeline.py) and the product (host.hip: bf_pipeline_*) implement.  Two sets of the
    reference's objects (CUDAImageManager, OnlineBundler with its TrajectoryManager, CUDASceneRepHashSDF), the same sensor frames, frame by frame plus the
    iterations after the end of the sequence: the bundler's state machine, every trajectory, the operations asked of the volume (kind, stored frame, transform) in
    order, and the volume itself - table, heap, every voxel byte - must be identical bit for bit (same code, same libm on both sides; only the ~40 lines of
    glue differ, and those are what is being pinned)."""
    from bundlefusion_amd.capi import default_app_state, default_bundling_state, intrinsics_matrix, camera_params
    from tests.oracle_pipeline import scale_intrinsics, _minf
    W, H, S = 320, 240, 3
    NF, dark = (10, range(0)) if scenario == "three_chunks" else (16, range(4, 9))
    gas = default_app_state(); gbs = default_bundling_state()
    gas.s_integrationWidth, gas.s_integrationHeight = W, H
    gas.s_SDFVoxelSize, gas.s_hashNumBuckets, gas.s_hashNumSDFBlocks = 0.05, 5000, 2000
    gas.s_garbageCollectionEnabled = True
    gbs.s_widthSIFT, gbs.s_heightSIFT, gbs.s_maxNumImages, gbs.s_submapSize = W, H, 8, S
    frames = [synth.scene_room(3 * k, W, H) for k in range(NF)]
    Kd = frames[0][3]
    K = intrinsics_matrix(Kd["fx"], Kd["fy"], Kd["mx"], Kd["my"])
    frames = [((np.full_like(f[0], -np.inf) if k in dark else f[0]), f[1]) for k, f in enumerate(frames)]
    Ki = scale_intrinsics(K, W, H, W, H)
    cam = camera_params(W, H, float(Ki[0, 0]), float(Ki[1, 1]), float(Ki[0, 2]), float(Ki[1, 2]), gas.s_renderDepthMin, gas.s_renderDepthMax)
    hp = ref_api.hash_params_from_global_app_state(gas)

    # ---- side A: the restated loop over the reference's classes (the sequence of test_online_bundler_vs_reference_host_code, without the oracle)
    ra = ref_api.RefOnlineBundler(gas, gbs, W, H, K)
    sa = ref_api.RefScene(hp, host_class=True)
    tma = ra.trajectory_manager()
    ops_a, stored = [], []

    def vol_a(kind, idx, T):
        ops_a.append((kind, idx, np.array(T, np.float32)))
        (sa.deintegrate if kind == "de" else sa.integrate)(T, stored[idx][0], stored[idx][1], cam)

    def reintegrate_a():                         # DepthSensing.cpp:853-902
        if tma.active() < gas.s_maxFrameFixes:
            tma.generate()
        for _ in range(gas.s_maxFrameFixes):
            f, idx, T, _ = tma.top_de()
            if f:
                vol_a("de", idx, T); continue
            f, idx, T, _ = tma.top_in()
            if f:
                vol_a("in", idx, T); tma.confirm(idx); continue
            f, idx, old, new = tma.top_re()
            if f:
                vol_a("de", idx, old); vol_a("in", idx, new); tma.confirm(idx); continue
            break
        sa.garbage_collect()

    # ---- side B: the compiled loop
    rb = ref_api.RefOnlineBundler(gas, gbs, W, H, K)
    sb = ref_api.RefScene(hp, host_class=True)
    loop = ref_api.RefFrameLoop(rb, sb, cam, gas.s_maxFrameFixes)
    n_b = 0
    for i in range(NF + 5):
        if i < NF:
            d, c = frames[i]
            ra.set_frame(d, c)                                   # CUDAImageManager::process
            _, _, di, ci = ra.ingest_outputs()
            stored.append((di.copy(), ci.copy()))                # what getIntegrateFrame(i) holds (side B reads it in place)
            ra.process_input()
            ok, T, idx, lost = ra.current_integration_frame()
            reintegrate_a()
            if ok:
                vol_a("in", idx, T)
                tma.add(0, T, i)
            else:
                tma.add(1, _minf(), i)
            stop = loop.frame(d, c)
        else:
            ra.process_input()
            reintegrate_a()
            stop = loop.frame()
        ra.process()
        assert not stop, i
        # the same state, the same trajectories, the same operations in the same order, the same volume
        assert ra.state() == rb.state(), (i, ra.state(), rb.state())
        n = ra.state()["num_complete"]
        if n:
            assert _same(ra.complete_trajectory(n), rb.complete_trajectory(n)), i
        assert _same(ra.sift_trajectory(min(i + 1, NF)), rb.sift_trajectory(min(i + 1, NF))), i
        new_b = loop.ops(n_b)
        new_a = ops_a[n_b:]
        assert [(k, f) for k, f, _ in new_a] == [(k, f) for k, f, _ in new_b], (i, [(k, f) for k, f, _ in new_a], [(k, f) for k, f, _ in new_b])
        assert all(_same(Ta, Tb) for (_, _, Ta), (_, _, Tb) in zip(new_a, new_b)), i
        n_b += len(new_b)
        assert sa.heap_counter() == sb.heap_counter() and np.array_equal(sa.hash(), sb.hash()) and np.array_equal(sa.heap(), sb.heap()), i
        assert np.array_equal(sa.voxels().view(np.uint8), sb.voxels().view(np.uint8)), i
    kinds = {k for k, _, _ in ops_a}
    assert kinds == {"in", "de"} and len(ops_a) > NF and ra.state()["past_end"] >= 4 and ra.state()["num_complete"] >= 2 * S, (kinds, len(ops_a), ra.state())
    assert int(ref_api.lib().ref_loop_frames_rendered()) == NF + 5


# ------------------------------------------------------------------------------------------------ the bundling half of the frame loop
_LONG = pytest.mark.skipif(os.environ.get("BF_LONG_TESTS") != "1", reason="1-2 more minutes on the block emulator: BF_LONG_TESTS=1 (log of a run: profiles/r02_ref_pin_long.txt)")


_LOOP = pytest.mark.skipif(os.environ.get("BF_LOOP_TEST") != "1", reason="the full 360 degree loop through the emulated reference: about half an hour, BF_LOOP_TEST=1 (log: profiles/r02_ref_pin_loop.txt)")


@pytest.mark.parametrize("scenario", ["three_chunks", "tracking_loss", pytest.param("default_submap", marks=_LONG), "revisit", "alt_flags", "noisy",
                                      pytest.param("full_loop", marks=_LOOP)])
def test_online_bundler_vs_reference_host_code(oracle, scenario):
    """Rows a1-a12 end to end: the reference's CUDAImageManager.cpp (ingest) / OnlineBundler.cpp / Bundler.cpp / SBA.cpp /
    CUDASolverBundling.cpp / CUDACache.cpp / TrajectoryManager.cpp / SIFTImageManager.cpp / SiftGPU fork, all compiled as they are and run on the block emulator, against the
    oracle frame loop (tests/oracle_pipeline.py - the restatement every GPU pipeline test holds the product to) on a 10-frame stream of
    three local chunks plus the end-of-sequence iterations.  Per frame: the ingest's outputs (SIFT-side raw depth and the colour frame bit for bit, filtered depth and the
    depth frame stored for integration to the 3e-6 of the exp() difference); the state machine (11 fields of BundlerState) exactly; the pose
    handed to the integration bit for bit until the first global solve and to 5e-4 after it; complete / local / global trajectories 5e-4 (the dense local solve sums in another order; measured 2.6e-4)
    with the same -inf pattern; key-frame counts, key counts, correspondence counts, valid flags exactly; and the operations the
    TrajectoryManager schedules (kind and frame exactly).  In the "three_chunks", "tracking_loss" and "revisit" scenarios those operations also drive the VOLUME on both
    sides - the reference's CUDASceneRepHashSDF host class over its own kernels against the oracle volume: allocated keys, bucket occupancy,
    free list and every voxel byte identical while the poses are identical bit for bit (up to the first re-integration), the same blocks up
    to a 3 % fringe afterwards.
    Scenario "full_loop" (BF_LOOP_TEST=1): BASELINE configs[2] in small - 212 frames once around the room and into the second lap, chunk size 10,
    21 key frames, the loop closed by global matches between the last and the first key frames; poses 2e-2 (21 global solves deep).
    Scenario "noisy": ten frames of another part of the room, 1.8 degrees apart, with 4 mm of Gaussian depth noise.
    Scenario "revisit": 16 frames over the same seven views twice (the jump back after view 6 is one large step): the global key frames of the
    second pass match key frames of the first pass that are not their predecessors - loop-closure correspondences in the global problem and the
    re-initialisation of the global pose from the last MATCHED key frame (Bundler.cpp:205-210).
    Scenario "alt_flags": no erosion / depth filter (the integration frame is then the raw sensor depth), intensity filter on, no local
    verification, simple frame invalidation, residual removal every second solve, and s_numSolveFramesBeforeExit = 2 so that the run reaches
    the end-of-scan switch to the dense global solve (setSolveWeights: sparse 1, dense depth 15) and the stop of the solver.
    Scenario "default_submap": the same with the reference's chunk size of 10 (31 frames, three chunks of 11 frames, local solves over 55 dense
    pairs).  Scenario "tracking_loss": 16 frames of which 4-8 carry no depth - untracked frames, two local chunks without a tracked frame (the
    INVALIDATE branches of OnlineBundler.cpp:134-165, :263-266, :351-360, :399-405, Bundler::addInvalidFrame, -inf rows of
    updateTrajectoryCU), then recovery through the global matching; poses after the gap 1e-2 (both sides re-anchor across the gap from a
    poor initial guess and stop their three Gauss-Newton steps at slightly different iterates), everything discrete exactly."""
    from bundlefusion_amd.capi import default_app_state, default_bundling_state, intrinsics_matrix
    from tests.oracle_pipeline import OraclePipeline, NINF, _minf
    W, H, S = 320, 240, 3
    NF, dark, TOL = (10, range(0), 5e-4) if scenario == "three_chunks" else (16, range(4, 9), 1e-2)
    stride = 3
    if scenario == "full_loop":                  # BASELINE configs[2] in small: once around the room (1800 / 9 = 200 frames) and 12 frames into the second lap
        S, NF, TOL, stride = 10, 212, 2e-2, 9
    if scenario == "noisy":
        stride = 9
    if scenario == "revisit":                    # the camera goes over the same seven views twice: key frames of the second pass match those of the first
        NF = 16
    if scenario == "alt_flags":                  # the other side of the switches, and the end-of-scan global dense solve (OnlineBundler.cpp:175-196)
        NF = 7
    if scenario == "default_submap":             # the reference's chunk size (zParametersBundlingDefault.txt: s_submapSize = 10): 31 frames, three chunks of 11
        S, NF, TOL = 10, 31, 5e-4
    gas = default_app_state(); gbs = default_bundling_state()
    gas.s_integrationWidth, gas.s_integrationHeight = W, H
    gas.s_SDFVoxelSize, gas.s_hashNumBuckets, gas.s_hashNumSDFBlocks = 0.05, 5000, 2000
    with_volume = scenario in ("three_chunks", "tracking_loss", "revisit")
    gas.s_garbageCollectionEnabled = with_volume
    gbs.s_widthSIFT, gbs.s_heightSIFT, gbs.s_maxNumImages, gbs.s_submapSize = W, H, (30 if scenario == "full_loop" else 8), S
    if scenario == "alt_flags":
        gbs.s_erodeSIFTdepth = gbs.s_depthFilter = gbs.s_useLocalVerify = gbs.s_useComprehensiveFrameInvalidation = False
        gbs.s_numOptPerResidualRemoval = 2
        gas.s_colorFilter, gas.s_numSolveFramesBeforeExit = True, 2
    start = 900 if scenario == "noisy" else 0
    frames = [synth.scene_room(start + stride * (k % 7 if scenario == "revisit" else k), W, H) for k in range(NF)]
    if scenario == "noisy":                     # another part of the room, 1.8 degrees per frame, 4 mm of depth noise
        nrng = np.random.default_rng(2)
        frames = [(f[0] + nrng.normal(0, 0.004, f[0].shape).astype(np.float32),) + tuple(f[1:]) for f in frames]
    Kd = frames[0][3]
    K = intrinsics_matrix(Kd["fx"], Kd["fy"], Kd["mx"], Kd["my"])
    frames = [((np.full_like(f[0], -np.inf) if k in dark else f[0]), f[1]) for k, f in enumerate(frames)]
    op = OraclePipeline(gas, gbs, W, H, K)
    if not with_volume:
        op._integrate = lambda frame, T, de: op.integrate_ops.append(("de" if de else "in", frame, np.array(T, np.float32)))
    rb = ref_api.RefOnlineBundler(gas, gbs, W, H, K)
    # the volume: the reference's CUDASceneRepHashSDF host class with the HashParams its parametersFromGlobalAppState derives, driven by
    # the operations its TrajectoryManager hands out - DepthSensing.cpp:854-902 (reintegrate) and :723-762 (integrate) are these few lines
    rsc = ref_api.RefScene(ref_api.hash_params_from_global_app_state(gas), host_class=True) if with_volume else None

    def ref_volume(kind, idx, T):
        if rsc is not None:
            (rsc.deintegrate if kind == "de" else rsc.integrate)(T, op.frames[idx][0], op.frames[idx][1], op.cam)

    rtm = rb.trajectory_manager()
    ref_ops = []
    STATES = {"NONE": 0, "PROCESS": 1, "INVALIDATE": 2}

    def ref_reintegrate():                       # DepthSensing.cpp:854-902 on the reference's TrajectoryManager
        if rtm.active() < gas.s_maxFrameFixes:
            rtm.generate()
        for _ in range(gas.s_maxFrameFixes):
            f, idx, T, _ = rtm.top_de()
            if f:
                ref_ops.append(("de", idx, T)); ref_volume("de", idx, T); continue
            f, idx, T, _ = rtm.top_in()
            if f:
                ref_ops.append(("in", idx, T)); ref_volume("in", idx, T); rtm.confirm(idx); continue
            f, idx, old, new = rtm.top_re()
            if f:
                ref_ops.append(("de", idx, old)); ref_ops.append(("in", idx, new)); ref_volume("de", idx, old); ref_volume("in", idx, new); rtm.confirm(idx); continue
            break
        if rsc is not None:
            rsc.garbage_collect()

    max_dev = [0.0]

    def close(a, b, tol=None):
        tol = TOL if tol is None else tol
        a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
        inf_a, inf_b = a == NINF, b == NINF
        dev = float(np.abs(np.where(inf_a, 0, a) - np.where(inf_b, 0, b)).max()) if a.size else 0.0
        max_dev[0] = max(max_dev[0], dev)
        return np.array_equal(inf_a, inf_b) and dev <= tol

    def compare(step):
        st = rb.state()
        mine = dict(last_processed=op.last_processed, last_valid=int(op.last_valid), local_to_solve=op.local_to_solve, last_local_solved=op.last_local_solved,
                    past_end=op.past_end, num_complete=op.num_complete, last_valid_complete=op.last_valid_complete, tracking_lost=int(op.tracking_lost),
                    process_state=STATES[op.state], use_solve=int(op.use_solve), total_opt_local=op.total_opt_local)
        assert st == mine, (step, st, mine)
        n = op.num_complete
        if n:
            assert close(rb.complete_trajectory(n), op.complete[:n]), step
        assert np.array_equal(rb.invalid_images_list(NF + S), np.array(op.invalid_list[:NF + S], np.uint32)), step
        g = rb.bundler(2)
        ng = g.num_frames()
        assert ng == op.glob.num_images, step
        if ng:
            assert list(g.valid(ng)) == op.glob.valid[:ng], step
            assert close(g.trajectory(ng), op.glob.trajectory[:ng]), step
            rk, ok_ = [g.num_keys(i) for i in range(ng)], [len(k) for k in op.glob.keys[:ng]]
            rc, oc = g.correspondences(), op.glob.corr
            if scenario != "full_loop":
                assert rk == ok_, step
                assert len(rc) == len(oc) and np.array_equal(rc["imgIdx_i"], oc["imgIdx_i"]) and np.array_equal(rc["imgIdx_j"], oc["imgIdx_j"]), step
            else:
                # 20 chunks deep a fused key point next to the image border, or a match next to a filter threshold, falls on the other side for one
                # of the two solvers now and then (their local poses differ by 1e-4): counts within a few, the same image pairs up to a few
                assert max(abs(a - b) for a, b in zip(rk, ok_)) <= 3, (step, rk, ok_)
                pr = set(zip(rc["imgIdx_i"].tolist(), rc["imgIdx_j"].tolist())); po = set(zip(oc["imgIdx_i"].tolist(), oc["imgIdx_j"].tolist()))
                assert len(pr & po) >= 0.9 * len(pr | po) and abs(len(rc) - len(oc)) <= 0.05 * max(len(oc), 1) + 25, (step, len(rc), len(oc), pr ^ po)
        nl = (op.last_local_solved + 1) * (S + 1) if op.last_local_solved >= 0 else 0
        if nl:
            assert close(rb.local_trajectories(nl), op.local_traj[:nl]), step

    solved = reintegrated = False
    volume_checks = [0, 0]
    capped = [0]
    n_ops = [0, 0]
    for i in range(NF + 5):
        integrated_now = False
        if i < NF:
            d, c = frames[i][0], frames[i][1]
            raw, filt = op._ingest(d, c)
            rb.set_frame(d, c)                                 # the reference's own ingest, CUDAImageManager::process
            r_raw, r_filt, r_di, r_ci = rb.ingest_outputs()
            assert _same(r_raw, raw), i

            def near(a, b):                              # the depth Gauss filter: glibc exp() there, bf_detmath here (3e-6, test_ingest_and_resample_kernels)
                v = np.isfinite(b)
                return np.array_equal(np.isfinite(a), v) and (not v.any() or np.abs(a[v] - b[v]).max() <= 3e-6 * np.abs(b[v]).max())
            assert near(r_filt, filt), i
            assert near(r_di, op.frames[i][0]) and _same(r_ci.reshape(op.frames[i][1].shape), op.frames[i][1]), i     # what the integration will read
            rb.override_filtered_depth(filt)             # from here on bit for bit
            rb.process_input(); op.process_input(raw, filt, c)
            ok, T, idx, lost = rb.current_integration_frame()
            assert ok == op.last_valid and lost == op.tracking_lost, i
            if ok:
                assert idx == op.last_processed
                To = op.cur_T[op.last_processed]
                if not solved:
                    assert np.array_equal(T.view(np.uint32), np.asarray(To, np.float32).view(np.uint32)), (i, T, To)     # SIFT tracking: bit for bit
                else:
                    assert close(T, To), i
            ref_reintegrate(); op._reintegrate()
            if ok:
                if with_volume:                  # integrate() of the current frame, DepthSensing.cpp:723-762
                    integrated_now = True
                    ref_ops.append(("in", i, T)); ref_volume("in", i, T)
                    op._integrate(op.last_processed, op.cur_T[op.last_processed], False)
                rtm.add(0, T, i); op.tm.add_frame(0, op.cur_T[op.last_processed], i)
            else:
                rtm.add(1, _minf(), i); op.tm.add_frame(1, _minf(), i)
        else:                                        # the sequence has ended: FriedLiver.cpp keeps calling the bundler without new frames
            rb.process_input(); op.process_input()
            ref_reintegrate(); op._reintegrate()
        rb.process(); op._bundler_process()
        solved = solved or op.num_complete > 0
        compare(i)
        # the operations scheduled in this frame: same kinds and frames.  (Inside one frame they are ordered by the pose distance, which the
        # two solvers' 1e-4 differences may permute: compared as sorted lists.)
        new_r, new_o = ref_ops[n_ops[0]:], op.integrate_ops[n_ops[1]:]
        assert sorted(k for k, _, _ in new_r) == sorted(k for k, _, _ in new_o), i                 # as many operations of each kind
        if sorted((k, f) for k, f, _ in new_r) == sorted((k, f) for k, f, _ in new_o):
            by_r = {(k, f): T for k, f, T in new_r}
            assert all(close(by_r[(k, f)], T) for k, f, T in new_o), i
        else:
            # more candidates than s_maxFrameFixes: WHICH of two frames with nearly the same pose distance makes the cut may differ; they
            # are served in the next frames (checked over the whole run below)
            assert len(new_o) >= 2 * gas.s_maxFrameFixes, (i, [(k, f) for k, f, _ in new_r], [(k, f) for k, f, _ in new_o])
            capped[0] += 1
        n_ops[:] = [len(ref_ops), len(op.integrate_ops)]
        if with_volume:
            if not reintegrated and not any(k == "de" for k, _, _ in new_o):
                # every pose so far was identical bit for bit: so is the volume (north_star: bit-exact hash-bucket occupancy and voxel indices)
                global _hash_fn
                _hash_fn = oracle.hash_pos
                _assert_same_volume(op.scene, rsc, gas.s_hashNumBuckets, "frame %d" % i, frustum_list=integrated_now)
                volume_checks[0] += 1
            else:                                # re-integration at poses that differ by 1e-4: the same blocks up to the surface fringe
                reintegrated = True
                ko, kr = set(_by_key(op.scene.hash(), op.scene.voxels())), set(_by_key(rsc.hash(), rsc.voxels()))
                assert len(ko & kr) >= 0.97 * len(ko | kr) and abs(op.scene.heap_counter() - rsc.heap_counter()) <= 0.03 * len(ko), i
                volume_checks[1] += 1
    assert op.glob.num_images >= (2 if scenario == "alt_flags" else 3) and op.num_complete >= 2 * S and op.past_end >= 4
    if scenario == "alt_flags":
        assert not op.use_solve and op.glob.use_global_dense          # reached the dense end-of-scan solve and the stop
    if scenario == "full_loop":                 # the loop is closed: the last key frames match the first ones
        gc = op.glob.corr[op.glob.corr["imgIdx_i"] != 0xFFFFFFFF]
        span = gc["imgIdx_j"].astype(np.int64) - gc["imgIdx_i"].astype(np.int64)
        print("full_loop: %d key frames, %d global correspondences, widest image pair %d key frames apart, max deviation of any compared pose %.2e"
              % (op.glob.num_images, len(gc), span.max(), max_dev[0]))
        assert span.max() >= 18
    if scenario == "revisit":
        gc = op.glob.corr[op.glob.corr["imgIdx_i"] != 0xFFFFFFFF]
        assert (gc["imgIdx_j"].astype(np.int64) - gc["imgIdx_i"].astype(np.int64)).max() >= 2          # a key frame matched one that is not its predecessor
    if scenario == "tracking_loss":
        assert 0 in op.glob.valid[1:op.glob.num_images] and not np.isfinite(op.complete[5, 0, 0]) and np.isfinite(op.complete[NF - 2, 0, 0])
    assert len(ref_ops) > (3 if scenario == "alt_flags" else 10) and {k for k, _, _ in ref_ops} == {"de", "in"}
    from collections import Counter
    cr, co = Counter((k, f) for k, f, _ in ref_ops), Counter((k, f) for k, f, _ in op.integrate_ops)
    slack = 1 if scenario != "full_loop" else 3           # the long run re-integrates every frame several times; the cut at s_maxFrameFixes falls differently more often
    assert all(abs(cr[key] - co[key]) <= slack for key in set(cr) | set(co)) and (capped[0] <= 3 or scenario == "full_loop"), (capped, cr - co, co - cr)
    if with_volume:
        assert volume_checks[0] >= 2 * S and volume_checks[1] >= 3, volume_checks


def test_image_manager_resample_branch_vs_reference_class(oracle):
    """a1, the reference's default configuration (integration resolution below the sensor's): CUDAImageManager's constructor and process()
    (CUDAImageManager.h:141-193, CUDAImageManager.cpp:22-158, compiled as they are) against the oracle's _ingest - the depth / colour frame
    stored for integration through resampleFloat / resampleUCHAR4 of the FILTERED depth, and the integration intrinsics adapted with
    (w' / w, h' / h, (w' - 1) / (w - 1), (h' - 1) / (h - 1))."""
    from bundlefusion_amd.capi import default_app_state, default_bundling_state, intrinsics_matrix
    from tests.oracle_pipeline import OraclePipeline, scale_intrinsics
    W, H, WI, HI = 320, 240, 160, 120
    gas = default_app_state(); gbs = default_bundling_state()
    gas.s_integrationWidth, gas.s_integrationHeight = WI, HI
    gas.s_SDFVoxelSize, gas.s_hashNumBuckets, gas.s_hashNumSDFBlocks = 0.05, 5000, 2000
    gbs.s_widthSIFT, gbs.s_heightSIFT, gbs.s_maxNumImages, gbs.s_submapSize = W, H, 4, 3
    frames = [synth.scene_room(5 * k, W, H) for k in range(2)]
    Kd = frames[0][3]
    K = intrinsics_matrix(Kd["fx"], Kd["fy"], Kd["mx"], Kd["my"])
    op = OraclePipeline(gas, gbs, W, H, K)
    rb = ref_api.RefOnlineBundler(gas, gbs, W, H, K)
    Ki = rb.integration_intrinsics()
    assert _same(Ki, scale_intrinsics(K, WI, HI, W, H))
    for i, (d, c, _, _) in enumerate(frames):
        raw, filt = op._ingest(d, c)
        rb.set_frame(d, c)
        r_raw, r_filt, r_di, r_ci = rb.ingest_outputs()
        assert _same(r_raw, raw)
        v = np.isfinite(filt)
        assert np.array_equal(np.isfinite(r_filt), v) and np.abs(r_filt[v] - filt[v]).max() <= 3e-6 * np.abs(filt[v]).max()
        od, oc = op.frames[i]
        assert r_di.shape == od.shape == (HI, WI)
        assert _same(r_di, oracle.resample_float(r_filt, WI, HI))                    # the class resamples ITS filtered depth with the pinned kernel ...
        vi = np.isfinite(od)
        assert np.array_equal(np.isfinite(r_di), vi) and np.abs(r_di[vi] - od[vi]).max() <= 3e-6 * np.abs(od[vi]).max()      # ... = the oracle's frame up to exp()
        assert _same(r_ci.reshape(oc.shape), oc)


def test_correspondence_evaluator_vs_reference_class(oracle, tmp_path):
    """f4: the reference's CorrespondenceEvaluator.cpp (compiled as it is) on the key points, the current raw / filtered matches and the
    cached frames of a reference Bundler after its matchAndFilter, against tests/oracle_eval.py - the restatement the product's evaluator is
    held to on the GPU: ground-truth overlap per previous frame, and (numCorrect, numDetected, numTotal) for the raw and the filtered
    matches, with one reference pose falsified so that correct, incorrect and undetected pairs all occur."""
    from bundlefusion_amd.capi import default_app_state, default_bundling_state, intrinsics_matrix, rgbx_to_intensity
    from tests.oracle_pipeline import OraclePipeline
    from tests import oracle_eval as oe
    W, H, n = 320, 240, 4
    gas = default_app_state(); gbs = default_bundling_state()
    gas.s_integrationWidth, gas.s_integrationHeight = W, H
    gas.s_SDFVoxelSize, gas.s_hashNumBuckets, gas.s_hashNumSDFBlocks = 0.05, 5000, 2000
    gbs.s_widthSIFT, gbs.s_heightSIFT, gbs.s_maxNumImages, gbs.s_submapSize = W, H, 4, 10
    frames = [synth.scene_room(4 * k, W, H) for k in range(n)]
    Kd = frames[0][3]
    K = intrinsics_matrix(Kd["fx"], Kd["fy"], Kd["mx"], Kd["my"])
    op = OraclePipeline(gas, gbs, W, H, K)                                   # for its ingest only
    ref_api.set_reference_state(gas, gbs)
    rb = ref_api.RefBundler(11, gbs.s_maxNumKeysPerImage, K, W, H, K, True, gbs.s_minKeyScale)
    for i, (d, c, _, _) in enumerate(frames):
        raw, filt = op._ingest(d, c)
        rb.add_frame(rgbx_to_intensity(c), filt, raw, c)
        if i > 0:
            assert rb.match_and_filter() != 0xFFFFFFFF
    cur = n - 1
    T0inv = np.linalg.inv(frames[0][2].astype(np.float64))
    traj = np.stack([(T0inv @ f[2].astype(np.float64)).astype(np.float32) for f in frames])
    Ry = np.array([[0, 0, 1, 0], [0, 1, 0, 0], [-1, 0, 0, 0], [0, 0, 0, 1]], np.float32)
    traj[1] = Ry @ traj[1]; traj[1, 1, 3] += 0.7                             # a wrong reference pose for image 1 (turned by 90 degrees and lifted)
    ev = ref_api.RefCorrespondenceEvaluator(traj, str(tmp_path / "corr"))
    Kinv = oracle.inverse44(K)
    r_raw = ev.evaluate(rb, Kinv, False, True, False, "raw")
    r_gt = ev.has_gt_overlap(n)
    r_filt = ev.evaluate(rb, Kinv, True, False, True, "dense")
    ev.finish()
    # the same through the restatement, on the reference bundler's data
    gw, gh = gbs.s_downsampledWidth, gbs.s_downsampledHeight
    Kc = rb.cache_intrinsics(); Kci = oracle.inverse44(Kc)
    depths = [rb.cache_frame_depth(i, gw, gh) for i in range(n)]
    has_gt = np.zeros(n, bool)
    for p in range(cur):
        Tcp = oracle.mul44(oracle.inverse44(traj[p]), traj[cur])
        c = oe.overlap_counts(depths[cur], depths[p], Tcp, oracle.inverse44(Tcp), Kc, Kci, gbs.s_denseDepthMin, gbs.s_denseDepthMax, gbs.s_projCorrDistThres,
                              gbs.s_projCorrNormalThres)
        has_gt[p] = oe.has_gt_overlap(c)
    assert np.array_equal(has_gt, r_gt), (has_gt, r_gt)
    assert has_gt[0] and has_gt[2] and not has_gt[1]
    keys = rb.all_keys()
    view = rb.matches_view()
    for filtered, expect in ((False, r_raw), (True, r_filt)):
        slots = 25 if filtered else 128
        idx = np.zeros((n, slots, 2), np.uint32); num = np.zeros(n, np.int64)
        for p in range(cur):
            r = view.filtered(p) if filtered else view.raw(p)
            num[p] = r[0]; idx[p] = r[1]
        (correct, detected, total), worst = oe.evaluate(keys, idx, num, has_gt, traj, cur, Kinv)
        assert (correct, detected, total) == expect, (filtered, (correct, detected, total), expect)
    assert r_raw[2] == 2 and r_raw[1] >= 1 and r_filt[0] >= 1
    rows = open(str(tmp_path / "corr") + "_frame.csv").read().splitlines()
    assert rows[0] == "numFrames,curFrame,type,precision,recall,numCorrect,numDetected,numTotal" and len(rows) == 3


def test_raw_match_cap_is_a_function_of_the_key_order(oracle):
    """More than MAX_MATCHES_PER_IMAGE_PAIR_RAW = 128 raw matches between two frames: the reference keeps the first 128 that arrive at
    `atomicAdd(d_numMatches, 1)` (ProgramCU.cu:1909), i.e. its result depends on the order of its key lists, which its detector fills in thread
    arrival order.  The restatement keeps the first 128 in key order.  Fed the reference's key order, it reproduces the reference's filtered
    correspondences bit for bit - the cap itself is pinned, the order is the reference's own non-determinism (golden vectors)."""
    from bundlefusion_amd.capi import default_app_state, default_bundling_state, intrinsics_matrix
    from tests.oracle_pipeline import OraclePipeline, OBundler
    W, H, S = 320, 240, 3
    gas = default_app_state(); gbs = default_bundling_state()
    gas.s_integrationWidth, gas.s_integrationHeight = W, H
    gas.s_SDFVoxelSize, gas.s_hashNumBuckets, gas.s_hashNumSDFBlocks = 0.05, 5000, 2000
    gbs.s_widthSIFT, gbs.s_heightSIFT, gbs.s_maxNumImages, gbs.s_submapSize = W, H, 8, S
    rng = np.random.default_rng(1)
    frames = [synth.scene_room(200 + 3 * k, W, H) for k in range(2)]
    frames = [(f[0] + rng.normal(0, 0.004, f[0].shape).astype(np.float32), f[1]) for f in frames]            # 4 mm depth noise: more key points survive
    Kd = synth.intrinsics(W, H)
    K = intrinsics_matrix(Kd["fx"], Kd["fy"], Kd["mx"], Kd["my"])
    op = OraclePipeline(gas, gbs, W, H, K); op._integrate = lambda *a: None
    rb = ref_api.RefOnlineBundler(gas, gbs, W, H, K)
    for d, c in frames:
        raw, filt = op._ingest(d, c)
        rb.set_frame(d, c); rb.override_filtered_depth(filt)
        rb.process_input(); op.process_input(raw, filt, c)
    b = op.local
    n_raw, _, _ = oracle.sift_match(b.descs[0], b.descs[1], gbs.s_siftMatchThresh, gbs.s_siftMatchRatioMaxLocal, 0, b.max_keys)
    assert n_raw > 128                                                                   # the cap is active
    loc = rb.bundler(0)
    rc = loc.correspondences()
    assert len(rc) == len(b.corr) == 25 and rc.tobytes() != b.corr.tobytes()            # same count, other matches: the two key orders differ
    b2 = OBundler(S + 1, b.max_keys, b.Kinv, b.depthK, True, gas, gbs)
    for im in range(2):
        rk, rd = loc.keys(im)
        assert sorted(map(tuple, rk.view(np.uint32).tolist())) == sorted(map(tuple, np.asarray(b.keys[im], np.float32).view(np.uint32).tolist()))   # same key points
        b2._add_image(rk.copy(), rd.copy())                                              # ... in the reference's order
    b2.cache = list(b.cache[:2]); b2.valid = [1, 1] + [0] * (S - 1); b2.current = 1
    assert b2.match_and_filter() == 0
    assert b2.corr.tobytes() == rc.tobytes()


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_tsdf_random_operator_sequences_vs_reference(oracle, seed):
    """Random sequences of integrate / de-integrate / garbage collection over noisy frames with holes, random voxel size, bucket count (chained to roomy),
    truncation and weight cap: after every operator the oracle volume equals the one the reference's host class and kernels produce."""
    global _hash_fn
    _hash_fn = oracle.hash_pos
    rng = np.random.default_rng(1000 + seed)
    W, H = 80, 60
    voxel = float(rng.choice([0.01, 0.02, 0.04]))
    # from chained to roomy; a table so overloaded that chains hit their length limit drops blocks by arrival order - the reference's own non-determinism
    nb = int(rng.choice([4001, 20011] if voxel == 0.01 else [1009, 4001, 20011]))
    p = default_hash_params(num_buckets=nb, num_sdf_blocks=20000, voxel_size=voxel, truncation=float(rng.choice([0.03, 0.06])), trunc_scale=float(rng.choice([0.01, 0.03])),
                            weight_sample=int(rng.choice([1, 2, 10])), weight_max=int(rng.choice([4, 255, 99999999])), max_integration_distance=float(rng.choice([2.0, 3.0, 4.0])))
    Kd = synth.intrinsics(W, H)
    cam = camera_params(W, H, Kd["fx"], Kd["fy"], Kd["mx"], Kd["my"])
    frames = []
    for k in rng.choice(1800, size=4, replace=False):
        d, c, T, _ = synth.scene_room(int(k), W, H)
        d = d + rng.normal(0, 0.003, d.shape).astype(np.float32)
        d[rng.random(d.shape) < 0.02] = -np.inf
        y, x = int(rng.integers(0, H - 12)), int(rng.integers(0, W - 16))
        d[y:y + 12, x:x + 16] = -np.inf
        frames.append((d, c, T))
    osc, rsc = oracle.OracleScene(p), ref_api.RefScene(p, host_class=True)
    inside = []
    for step in range(10):
        if inside and rng.random() < 0.4:
            j = inside.pop(int(rng.integers(len(inside))))
            d, c, T = frames[j]
            osc.deintegrate(T, d, c, cam); rsc.deintegrate(T, d, c, cam)
        else:
            j = int(rng.integers(len(frames)))
            d, c, T = frames[j]
            T = T.copy(); T[:3, 3] += rng.normal(0, 0.01, 3).astype(np.float32)
            frames[j] = (d, c, T)
            if j in inside:
                continue                                   # a frame is integrated once at a time (the TrajectoryManager guarantees it)
            osc.integrate(T, d, c, cam); rsc.integrate(T, d, c, cam)
            inside.append(j)
        if rng.random() < 0.5:
            osc.garbage_collect(); rsc.garbage_collect()
            osc.compactify(T, cam); rsc.compactify(T, cam)
        _assert_same_volume(osc, rsc, nb, "seed %d step %d" % (seed, step))
