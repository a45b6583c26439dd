"""GPU tests (-m gpu): the bundling solver (csrc/solver.hip) against tests/solver_ref64.py, a float64 restatement of the
reference's equations that does not rest on the oracle.

Bound per entry of A, b = -J^T F and M^-1:  |gpu - ref| <= K * sqrt(n) * 2^-24 * S  (+ the borderline allowance of the dense
term), with n the number of terms summed into the entry and S the sum of their magnitudes (tests/solver_ref64.py).  K = 32.
Every system test prints its worst ratio |gpu - ref| / bar, and asserts that the bar is tighter than one term:
  * sparse: on every translation diagonal entry (where each correspondence adds exactly w), bar < w;
  * dense: on every variable diagonal entry, bar < 16 mean single-pixel contributions (16 S / n).  One pixel is not enough
    there: a diagonal entry sums up to ~20000 pixel terms, and sqrt(n) * n * 2^-24 * K outgrows one term; 16 pixels are a
    quarter of the 64 that one wave of k_dense_build feeds through the matrix core at a time.
Entries whose bar is 0 (no term reaches them) must be exactly 0 on the GPU.
Step tests: the GPU step equals the float64 PCG run on the GPU's own system for the GPU's iteration count to STEP_REL of the
step's size (float32 CG round-off), and its linear residual on the float64 system is at most twice the float64 PCG's, or below
RES_FLOOR.  SE(3) conversions: bounds in float32 ulps of max(1, |value|): exp 8 (plus, for the translation just above the
1e-3 branch point, the float32 cancellation of the closed forms: 4 ulp |trans| / theta), log 16 away from pi, exp(log T) 64
near pi.
"""
import numpy as np
import pytest

from bundlefusion_amd.capi import ENTRYJ_DTYPE, default_solver_config, intrinsics_matrix
from tests import bundle_synth as bs
from tests import solver_ref64 as R

pytestmark = pytest.mark.gpu

K = 32
EPS = 2.0 ** -24
ULP = 2.0 ** -23
STEP_REL = 1e-3
RES_FLOOR = 1e-4


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _poses32(T):
    rt = [R.log_se3(t) for t in np.asarray(T, np.float64)]
    return np.array([r for r, _ in rt], np.float32), np.array([t for _, t in rt], np.float32)


def _solve(gpu, corr, rot, tr, n, ws, wd, wc, cache=None, n_lin=1, pairwise=True, record=False, find_max=False):
    solver = gpu.capi.Solver(max(n, 2), max(len(corr), 1), default_solver_config(record_convergence=record))
    grot, gtr = _dev(rot.copy()), _dev(tr.copy())
    gcorr = _dev(corr.view(np.uint8)) if len(corr) else None
    solver.solve(gcorr, len(corr), _dev(np.ones(n, np.int32)), n, 1, n_lin, cache, [ws], [wd], [wc], grot, gtr,
                 use_pairwise=pairwise, find_max_residual=find_max)
    return solver, grot.cpu().numpy(), gtr.cpu().numpy()


def _ratio(got, ref, S, n, allow=0.0):
    bar = K * np.sqrt(np.maximum(n, 1)) * EPS * S + allow
    z = bar == 0
    assert not np.asarray(got)[z].any(), "an entry no term reaches is not 0"
    err = np.abs(np.asarray(got, np.float64) - ref)
    return (float((err[~z] / bar[~z]).max()) if (~z).any() else 0.0), bar


def _check_system(label, solver, n, sys, minv, pcnt, allow=None, dense=False):
    gA, gb, gP = solver.debug_system(n)
    v = slice(6, None)
    aA = allow.SA if allow is not None else 0.0
    ab = allow.Sb if allow is not None else 0.0
    rA, _ = _ratio(gA[v, v], sys.A[v, v], sys.SA[v, v], sys.nA[v, v], aA[v, v] if allow is not None else 0.0)
    rb, _ = _ratio(gb[v], sys.b[v], sys.Sb[v], sys.nb[v], ab[v] if allow is not None else 0.0)
    barP = K * np.sqrt(np.maximum(pcnt, 1)) * EPS * minv
    one = minv == 1.0
    assert np.array_equal(gP[one], minv[one].astype(np.float32)), "M^-1 of an image without correspondences is not 1"
    rP = float((np.abs(gP[~one] - minv[~one]) / barP[~one]).max()) if (~one).any() else 0.0
    diag = np.diag(K * np.sqrt(np.maximum(sys.nA[v, v], 1)) * EPS * sys.SA[v, v])       # the float32 part of the bar
    if dense:
        d = np.diag(sys.nA[v, v]) > 0
        teeth = float((diag[d] / (np.diag(sys.SA[v, v])[d] / np.diag(sys.nA[v, v])[d])).max()) if d.any() else 0.0
    else:
        tdiag = np.array([6 * i + a for i in range(1, n) for a in range(3)]) - 6
        d = np.diag(sys.nA[v, v])[tdiag] > 0
        teeth = float((diag[tdiag][d] / np.diag(sys.minA[v, v])[tdiag][d]).max()) if d.any() else 0.0
    print("%s: worst |gpu - ref| / bar: A %.3f  b %.3f  M^-1 %.3f   (bar / single term %.2e)" % (label, rA, rb, rP, teeth))
    assert rA <= 1 and rb <= 1 and rP <= 1, label
    assert teeth < (16 if dense else 1), "%s: the bar is not tighter than the terms it must see (%.3g)" % (label, teeth)
    return gA, gb, gP


# ------------------------------------------------------------------------------------------------------- sparse systems
def _pair_corr(T_gt, pairs, rng, noise=0.002):
    rows = []
    for (i, j), cnt in pairs:
        pw = rng.uniform(-1, 1, (cnt, 3)) + np.array([0, 0, 2.5])
        ph = np.c_[pw, np.ones(cnt)].T
        pi = (np.linalg.inv(T_gt[i]) @ ph).T[:, :3] + rng.normal(0, noise, (cnt, 3))
        pj = (np.linalg.inv(T_gt[j]) @ ph).T[:, :3] + rng.normal(0, noise, (cnt, 3))
        rows += [(i, j, a, b) for a, b in zip(pi, pj)]
    corr = np.zeros(len(rows), dtype=ENTRYJ_DTYPE)
    for k, (i, j, a, b) in enumerate(rows):
        corr[k] = (i, j, a.astype(np.float32), b.astype(np.float32))
    return corr


def _sparse_check(gpu, label, corr, T_init, n, ws):
    rot, tr = _poses32(T_init)
    T = R.poses_to_matrices(rot, tr)
    solver, _, _ = _solve(gpu, corr, rot, tr, n, ws, 0.0, 0.0, record=True)
    s = R.sparse_system(corr, T, n, ws)
    minv, _, cnt = R.sparse_preconditioner(corr, T, n)
    _check_system(label, solver, n, s, minv, cnt)
    e, eS = R.energy(corr, T, n, ws)
    ge = solver.convergence()[0]
    re = abs(ge - e) / (K * np.sqrt(max(R.valid_corr(corr, n).sum(), 1)) * EPS * eS)
    print("%s: energy gpu %.9g ref %.9g  ratio %.3f" % (label, ge, e, re))
    assert re <= 1
    return solver, rot, tr


@pytest.mark.parametrize("n", [2, 3, 33, 120])
def test_sparse_system_complete_graph(gpu, n):
    """Every image pair shares correspondences: at N = 120 every block row has 119 neighbours (> 96)."""
    corr, _, T_init = bs.sparse_problem(n_images=n, pair_prob=1.0, pts_per_pair=20 if n <= 33 else 3, seed=100 + n)
    _sparse_check(gpu, "complete graph N=%d" % n, corr, T_init, n, 1.0)


@pytest.mark.parametrize("ws", [1.0, 0.5])
def test_sparse_system_slot_lengths_empty_image_invalid_entries(gpu, ws):
    """Directed pairs with 1, 63, 64, 65 and 130 correspondences (k_slots walks a slot's list 64 lanes at a time), half of them
    with the roles swapped, an image with no correspondence, invalid entries interleaved and the input order permuted; the
    sparse weight scales A and b but not the preconditioner.  Also the energy and the largest residual."""
    rng = np.random.default_rng(7)
    n = 8
    T_gt = np.stack([np.eye(4)] + [bs.random_pose(rng, 0.3, 0.5) for _ in range(n - 1)])
    corr = _pair_corr(T_gt, [((0, 1), 20), ((1, 2), 1), ((2, 3), 63), ((3, 4), 64), ((4, 5), 65), ((5, 6), 130), ((1, 6), 9)], rng)
    flip = rng.uniform(size=len(corr)) < 0.5
    c2 = corr.copy()
    c2["imgIdx_i"][flip], c2["imgIdx_j"][flip] = corr["imgIdx_j"][flip], corr["imgIdx_i"][flip]
    c2["pos_i"][flip], c2["pos_j"][flip] = corr["pos_j"][flip], corr["pos_i"][flip]
    c2["pos_j"][5] += 0.3                                          # one clear outlier: a unique largest residual
    bad = np.zeros(60, dtype=ENTRYJ_DTYPE)
    bad["imgIdx_i"] = bad["imgIdx_j"] = 0xFFFFFFFF
    bad["pos_i"] = rng.normal(size=(60, 3)); bad["pos_j"] = rng.normal(size=(60, 3))
    allc = np.concatenate([c2, bad])[rng.permutation(len(c2) + 60)]
    T_init = T_gt.copy()
    for i in range(1, n):
        T_init[i] = bs.random_pose(rng, 0.03, 0.05) @ T_gt[i]
    rot, tr = _poses32(T_init)
    solver, _, _ = _sparse_check(gpu, "slot lengths w=%g" % ws, allc, T_init, n, ws)
    gA, gb, gP = solver.debug_system(n)
    assert not gA[42:48].any() and not gA[:, 42:48].any() and not gb[42:48].any() and (gP[42:48] == 1.0).all()     # image 7
    solver, grot, gtr = _solve(gpu, allc, rot, tr, n, ws, 0.0, 0.0, find_max=True)
    mres, midx = solver.max_residual()
    v, k, second, mag = R.max_residual(allc, R.poses_to_matrices(grot, gtr), n, ws)
    bar = K * EPS * mag
    print("slot lengths w=%g: max residual gpu %.9g (#%d) ref %.9g (#%d), runner-up %.4g, ratio %.3f" % (ws, mres, midx, v, k, second, abs(mres - v) / bar))
    assert abs(mres - v) <= bar
    assert v - second > 2 * bar and midx == k


# ------------------------------------------------------------------------------------------------------- dense systems
def _dense_setup(gpu, n_frames, cw, ch, perturb=(0.004, 0.01), stride=6):
    frames, Kd, T_gt, T_init = bs.dense_chunk(n_frames=n_frames, stride=stride, perturb=perturb)
    Kin = intrinsics_matrix(Kd["fx"], Kd["fy"], Kd["mx"], Kd["my"])
    cache = gpu.capi.Cache(160, 120, cw, ch, n_frames, Kin)
    for d, c in frames:
        cache.store_frame(_dev(d), _dev(c))
    w, h, k = cache.geometry()
    host = [cache.download_frame(i) for i in range(n_frames)]
    return cache, host, (w, h, tuple(float(x) for x in k)), T_gt, T_init


def _dense_check(gpu, label, cache, host, geom, T_init, wd, wc, pairwise=True, corr=None, ws=0.0):
    n = len(host)
    corr = np.zeros(0, dtype=ENTRYJ_DTYPE) if corr is None else corr
    rot, tr = _poses32(T_init)
    T = R.poses_to_matrices(rot, tr)
    solver, _, _ = _solve(gpu, corr, rot, tr, n, ws, wd, wc, cache=cache, pairwise=pairwise)
    v, allow, info = R.dense_system(host, T, geom, wd, wc, use_pairwise=pairwise)
    acc = sum(r["accepted"] for r in info); bord = sum(r["border"] for r in info)
    for r in info:          # the pair-level decisions must sit further from their thresholds than the borderline pixels reach
        assert not r["angle_border"], r
        if "overlap" in r:
            assert abs(r["overlap"] - 10.5) > r["overlap_border"] + 0.5, r
        if "count" in r and r["count"] > 0:
            assert abs(r["count"] - 799.5) > r["count_border"] + 0.5, r
    print("%s: %d pairs, weights %s, %d accepted pixels, %d borderline" % (label, len(info), ["%.3f" % r["pw"] for r in info], acc, bord))
    assert bord <= 0.005 * max(acc, 1)
    s = R.sparse_system(corr, T, n, ws)
    s += v
    minv, _, cnt = R.sparse_preconditioner(corr, T, n)
    gA, gb, gP = _check_system(label, solver, n, s, minv, cnt, allow=allow, dense=True)
    return gA, gb, info


@pytest.mark.parametrize("cw, ch", [(80, 60), (96, 80), (40, 30), (81, 61)])
def test_dense_system_at_cache_geometries(gpu, cw, ch):
    """4800 pixels (a partial last 256-pixel pass of k_dense_build), 7680 = 30 x 256, 1200 (pairs below 800 pixels: blocks exactly
    0: frames further apart there, so that some pairs fall below) and odd 81 x 61; depth only, colour only, both; pairs that include
    image 0."""
    cache, host, geom, _, T_init = _dense_setup(gpu, 4, cw, ch, stride=18 if cw == 40 else 6)
    below = False
    for wd, wc in ((1.0, 0.0), (0.0, 0.1), (1.0, 0.1)):
        gA, _, info = _dense_check(gpu, "dense %dx%d wd=%g wc=%g" % (cw, ch, wd, wc), cache, host, geom, T_init, wd, wc)
        for r in info:
            if r["pw"] == 0.0:
                i, j = r["i"], r["j"]
                assert not gA[6 * i:6 * i + 6, 6 * j:6 * j + 6].any()
                below |= 0 < r.get("count", 0) < 800
    if (cw, ch) == (40, 30):
        assert below, "no pair below 800 accepted pixels at 40 x 30"


def test_dense_system_angle_test_and_frame_to_frame(gpu):
    """A pose turned 0.7 rad (beyond the 30 degree test) leaves its pairs' blocks exactly 0; use_pairwise off keeps (i, i+1) only."""
    cache, host, geom, T_gt, T_init = _dense_setup(gpu, 4, 80, 60)
    ax = np.array([1.0, -1.0, 0.0]) / np.sqrt(2.0)                  # perpendicular to (1,1,1): the test's probe direction turns fully
    T_rot = T_init.copy()
    T_rot[3] = R.exp_se3(0.7 * ax, np.zeros(3)).astype(np.float32) @ T_init[3]
    gA, _, info = _dense_check(gpu, "dense angle test", cache, host, geom, T_rot, 1.0, 0.1)
    far = [r for r in info if 3 in (r["i"], r["j"])]
    assert far and all(not r["angle"] < 0.52 for r in far)
    for r in far:
        assert not gA[6 * r["i"]:6 * r["i"] + 6, 6 * r["j"]:6 * r["j"] + 6].any()
    _, _, info = _dense_check(gpu, "dense frame-to-frame", cache, host, geom, T_init, 1.0, 0.1, pairwise=False)
    assert sorted((r["i"], r["j"]) for r in info) == [(0, 1), (1, 2), (2, 3)]


def test_sparse_plus_dense_local_chunk_system(gpu):
    """The local chunk's first Gauss-Newton iteration: 5 frames, sparse weight 1, dense depth weight 1, sparse-only preconditioner."""
    n = 5
    cache, host, geom, T_gt, T_init = _dense_setup(gpu, n, 80, 60, perturb=(0.006, 0.015))
    corr = _pair_corr(T_gt.astype(np.float64), [((i, j), 15) for i in range(n) for j in range(i + 1, n)], np.random.default_rng(4), noise=0.003)
    _dense_check(gpu, "local chunk sparse + dense", cache, host, geom, T_init, 1.0, 0.0, corr=corr, ws=1.0)


# ------------------------------------------------------------------------------------------------------- the step
def _step_case(gpu, monkeypatch, n, groups=None, empty_last=False):
    if groups is not None:
        monkeypatch.setenv("BF_PCG_GROUPS", groups)
    complete = n >= 120
    corr, _, T_init = bs.sparse_problem(n_images=n, pair_prob=1.0 if complete else min(1.0, 8.0 / n), pts_per_pair=3 if complete else 20, seed=200 + n)
    if empty_last:
        corr = corr[(corr["imgIdx_i"] != n - 1) & (corr["imgIdx_j"] != n - 1)]
    rot, tr = _poses32(T_init)
    solver, grot, gtr = _solve(gpu, corr, rot, tr, n, 1.0, 0.0, 0.0, n_lin=150)
    monkeypatch.delenv("BF_PCG_GROUPS", raising=False)
    _, its = solver.iteration_counts()
    it = its[0]
    gA, gb, gP = solver.debug_system(n)
    T0, T1 = R.poses_to_matrices(rot, tr), R.poses_to_matrices(grot, gtr)
    dg = np.zeros((n, 6))
    for i in range(n):
        r_, t_ = R.log_se3(T1[i] @ np.linalg.inv(T0[i]))
        dg[i, :3], dg[i, 3:] = t_, r_
    x_own, _ = R.pcg(gA, gb, gP, it, early_out=False)
    step_err = np.abs(dg.reshape(-1)[6:] - x_own[6:]).max() / np.abs(x_own).max()
    s = R.sparse_system(corr, T0, n, 1.0)
    minv, _, _ = R.sparse_preconditioner(corr, T0, n)
    x_ref, _ = R.pcg(s.A, s.b, minv, it, early_out=False)
    res_ref = R.linear_residual(s.A, s.b, minv, x_ref)
    res_gpu = R.linear_residual(s.A, s.b, minv, dg.reshape(-1))
    print("step N=%d%s: %d PCG iterations, |d_gpu - d64(own system)| / |d| = %.2e (bound %.0e), linear residual gpu %.2e float64 %.2e"
          % (n, " groups=" + groups if groups is not None else "", it, step_err, STEP_REL, res_gpu, res_ref))
    if empty_last:
        drift = max(np.abs(grot[-1] - rot[-1]).max() / max(1.0, np.abs(rot[-1]).max()), np.abs(gtr[-1] - tr[-1]).max() / max(1.0, np.abs(tr[-1]).max())) / ULP
        print("step N=%d: image without correspondences moved by %.1f ulp (exp/log round trip)" % (n, drift))
        assert not dg[-1].any() or np.abs(dg[-1]).max() < 1e-5
        assert drift <= 8
    assert step_err <= STEP_REL
    assert res_gpu <= 2 * res_ref or res_gpu < RES_FLOOR


@pytest.mark.parametrize("n", [2, 32, 33, 120])
def test_step_matches_float64_pcg(gpu, monkeypatch, n):
    """N = 2 and 32: one workgroup; 33: the grid-barrier kernel (image 32 has no correspondence: zero step); 120: a complete
    graph whose off-diagonal blocks exceed the per-workgroup LDS budget."""
    _step_case(gpu, monkeypatch, n, empty_last=(n == 33))


def test_step_matches_float64_pcg_single_workgroup_kernel(gpu, monkeypatch):
    _step_case(gpu, monkeypatch, 33, groups="0", empty_last=True)


# ------------------------------------------------------------------------------------------------------- SE(3) conversions
def _angles():
    c = 1 / np.sqrt(2.0)
    out = [b * (1 + s * 1e-3) for b in (1e-5, 1e-4, 1e-3) for s in (-1, 1)]
    out += [float(np.arccos(float(np.float32(cc)) + k * 2.0 ** -24)) for cc in (c, -c) for k in (-3, -1, 1, 3)]
    return out


def test_se3_conversions_at_branch_boundaries(gpu):
    import torch
    rng = np.random.default_rng(31)
    angles = _angles() + [np.pi - 1e-3, np.pi - 1e-6, np.pi]
    rots, trans = [], []
    for th in angles:
        for _ in range(4):
            ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
            rots.append(ax * th); trans.append(rng.normal(size=3))
    rot32, tr32 = np.array(rots, np.float32), np.array(trans, np.float32)
    n = len(rot32)
    valid = _dev(np.ones(n, np.int32))
    T = torch.zeros(n, 4, 4, device="cuda")
    gpu.capi.convert_poses_to_matrices(_dev(rot32), _dev(tr32), T, valid)
    Tg = T.cpu().numpy()
    Tr = R.poses_to_matrices(rot32, tr32)
    # the translation V(rot) trans: above theta = 1e-3 the closed forms 1 - sin(t)/t and 1 - cos(t) cancel in float32 (the
    # reference's own branch points, LieDerivUtil.h); their error, ~ulp / theta^2 relative, enters with |rot x trans| ~ theta |trans|
    th = np.repeat(angles, 4)
    cancel = np.zeros_like(Tr)
    cancel[:, :3, 3] = (4 * ULP * np.linalg.norm(tr32, axis=1) / np.maximum(th, 1e-3) * (th > 1e-3))[:, None]
    e_exp = ((np.abs(Tg - Tr) - cancel * np.maximum(1.0, np.abs(Tr))) / np.maximum(1.0, np.abs(Tr))).max() / ULP
    e_cancel = (np.abs(Tg - Tr)[:, :3, 3] / np.maximum(1.0, np.abs(Tr[:, :3, 3]))).max() / ULP
    # matrices -> poses away from pi against the float64 log of the same float32 matrix
    T32 = Tr.astype(np.float32)
    gr, gt = torch.zeros(n, 3, device="cuda"), torch.zeros(n, 3, device="cuda")
    gpu.capi.convert_matrices_to_poses(_dev(T32), gr, gt, valid)
    gr, gt = gr.cpu().numpy(), gt.cpu().numpy()
    away = th < np.pi - 1e-2
    e_log = 0.0
    for k in np.nonzero(away)[0]:
        r_, t_ = R.log_se3(T32[k].astype(np.float64))
        e_log = max(e_log, (np.abs(gr[k] - r_) / np.maximum(1.0, np.abs(r_))).max() / ULP, (np.abs(gt[k] - t_) / np.maximum(1.0, np.abs(t_))).max() / ULP)
    # near pi: the log is ill-conditioned; its exp must give the matrix back and the angle must stay within pi
    near = np.nonzero(~away)[0]
    e_rt = max((np.abs(R.exp_se3(gr[k], gt[k]) - T32[k]) / np.maximum(1.0, np.abs(T32[k]))).max() / ULP for k in near)
    th_max = max(np.linalg.norm(gr[k].astype(np.float64)) for k in near)
    print("SE(3): exp %.1f ulp beyond the cancellation allowance (translation error before it: %.1f ulp), log %.1f ulp (away from pi), "
          "exp(log T) near pi %.1f ulp, max angle pi + %.2e" % (e_exp, e_cancel, e_log, e_rt, th_max - np.pi))
    assert e_exp <= 8 and e_log <= 16 and e_rt <= 64
    assert th_max <= np.pi * (1 + 4 * ULP)


# ------------------------------------------------------------------------------------------------------- slot capacity
def test_directed_slots_beyond_capacity_are_reported(gpu):
    """100 identical frames at identity overlap pairwise: 9900 directed dense slots against a capacity of min(N^2, 2C + 4N) = 402
    (one correspondence).  The row offsets are clamped to the capacity (no read past the slot arrays) and the 9498 slots that did
    not fit are reported."""
    from bundlefusion_amd import synth
    n = 100
    d, c, _, Kd = synth.scene_room(0, 160, 120)
    cache = gpu.capi.Cache(160, 120, 80, 60, n, intrinsics_matrix(Kd["fx"], Kd["fy"], Kd["mx"], Kd["my"]))
    dd, cc = _dev(d), _dev(c)
    for _ in range(n):
        cache.store_frame(dd, cc)
    corr = np.zeros(1, dtype=ENTRYJ_DTYPE)
    corr[0] = (0, 1, np.array([0.1, 0.2, 1.5], np.float32), np.array([0.1, 0.2, 1.5], np.float32))
    z = np.zeros((n, 3), np.float32)
    solver, grot, gtr = _solve(gpu, corr, z, z, n, 1.0, 1.0, 0.0, cache=cache, n_lin=5)
    over = solver.slot_overflow()
    print("slot overflow: %d directed slots dropped" % over)
    assert over == n * (n - 1) - (2 * 1 + 4 * n)
    assert np.isfinite(grot).all() and np.isfinite(gtr).all()
    solver2, _, _ = _solve(gpu, corr, z[:4], z[:4], 4, 1.0, 0.0, 0.0)
    assert solver2.slot_overflow() == 0
