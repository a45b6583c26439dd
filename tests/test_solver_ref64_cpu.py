"""CPU self-checks (-m "not gpu") of tests/solver_ref64.py, the float64 restatement the solver's GPU tests are held to:
its Jacobians are the derivatives of its residuals, its normal matrix has the symmetry of J^T J, its dense term agrees with
the oracle's float32 dump entry by entry within the float32 bound, and its PCG converges to the direct solution."""
import numpy as np
import pytest

from bundlefusion_amd.capi import ENTRYJ_DTYPE, intrinsics_matrix
from tests import bundle_synth as bs
from tests import solver_ref64 as R

K_BOUND = 32                      # the GPU tests' bound: |x - ref| <= K * sqrt(n) * 2^-24 * S
EPS = 2.0 ** -24


def _perturbed(T, img, delta):
    T = T.copy()
    T[img] = R.exp_se3(delta[3:], delta[:3]) @ T[img]
    return T


def test_sparse_jacobians_match_central_differences():
    corr, _, T_init = bs.sparse_problem(n_images=5, pair_prob=1.0, pts_per_pair=4, seed=3)
    corr = np.concatenate([corr, corr[::3].copy()])
    corr["imgIdx_i"][-4:], corr["imgIdx_j"][-4:] = corr["imgIdx_j"][-4:].copy(), corr["imgIdx_i"][-4:].copy()     # both roles
    corr["pos_i"][-4:], corr["pos_j"][-4:] = corr["pos_j"][-4:].copy(), corr["pos_i"][-4:].copy()
    n, T = 5, T_init.astype(np.float64)
    q = R.sparse_rows(corr, T, n)
    h = 1e-6
    for img in range(n):
        for c in range(6):
            d = np.zeros(6); d[c] = h
            fd = (R.sparse_rows(corr, _perturbed(T, img, d), n)["r"] - R.sparse_rows(corr, _perturbed(T, img, -d), n)["r"]) / (2 * h)
            an = np.where((q["i"] == img)[:, None], q["Ji"][:, :, c], 0.0) + np.where((q["j"] == img)[:, None], q["Jj"][:, :, c], 0.0)
            assert np.abs(fd - an).max() < 1e-6, (img, c, np.abs(fd - an).max())


def _oracle_frames(oracle, n_frames, cw=80, ch=60, perturb=(0.004, 0.01)):
    frames, K, T_gt, T_init = bs.dense_chunk(n_frames=n_frames, perturb=perturb)
    Kin = intrinsics_matrix(K["fx"], K["fy"], K["mx"], K["my"])
    cache = [oracle.cache_store_frame(d, c, cw, ch, Kin) for d, c in frames]
    k4 = [float(np.float32(v)) for v in (K["fx"] * cw / 160, K["fy"] * ch / 120, K["mx"] * (cw - 1) / 159, K["my"] * (ch - 1) / 119)]
    return cache, (cw, ch, k4), T_gt, T_init


def test_dense_jacobians_match_central_differences(oracle):
    cache, geom, _, T_init = _oracle_frames(oracle, 3)
    T = T_init.astype(np.float64)
    p = dict(R.DEFAULTS)
    W, H, K = geom
    tr = np.linalg.inv(T[1]) @ T[2]
    cnt, _ = R.weight_count(cache[1], cache[2], tr, geom, p, 1e-4)
    rows, nacc, _ = R.dense_pair_rows(cache[1], cache[2], T[1], T[2], geom, p, 1.0, 1.0, R.pair_weight(cnt), 1e-4)
    assert nacc > 500
    depth, color = rows
    m = np.nonzero(depth["accept"])[0][::37]
    mc = np.nonzero(color["accept"])[0][::37]
    assert len(m) > 10 and len(mc) > 5
    fx, fy, cx, cy = K

    def cst(Ti, Tj, cs):
        t = np.linalg.inv(Ti) @ Tj
        return cs @ t[:3, :3].T + t[:3, 3]

    h = 1e-6
    for which, Xkey in ((1, "Xi"), (2, "Xj")):
        for c in range(6):
            d = np.zeros(6); d[c] = h
            Tp, Tm = _perturbed(T, which, d), _perturbed(T, which, -d)
            # depth: r = (ct - cst) . nt with the target point and normal held (the reference's point-to-plane linearisation)
            rp = ((depth["ct"][m] - cst(Tp[1], Tp[2], depth["cs"][m])) * depth["nt"][m]).sum(1)
            rm = ((depth["ct"][m] - cst(Tm[1], Tm[2], depth["cs"][m])) * depth["nt"][m]).sum(1)
            assert np.abs((rp - rm) / (2 * h) - depth[Xkey][m, c]).max() < 1e-5 * (1 + np.abs(depth[Xkey][m, c]).max())
            # colour: r = dI . pi(cst) with the intensity gradient held
            def proj(Tx, idx):
                q = cst(Tx[1], Tx[2], color["cs"][idx])
                return np.stack([q[:, 0] * fx / q[:, 2], q[:, 1] * fy / q[:, 2]], 1)
            fd = ((color["dI"][mc] * (proj(Tp, mc) - proj(Tm, mc))).sum(1)) / (2 * h)
            assert np.abs(fd - color[Xkey][mc, c]).max() < 1e-5 * (1 + np.abs(color[Xkey][mc, c]).max())


def test_normal_matrix_is_symmetric_with_transposed_directed_blocks(oracle):
    cache, geom, _, T_init = _oracle_frames(oracle, 4)
    corr, _, _ = bs.sparse_problem(n_images=4, pair_prob=1.0, pts_per_pair=5, seed=7)
    T = T_init.astype(np.float64)
    s = R.sparse_system(corr, T, 4, 1.0)
    v, _, _ = R.dense_system(cache, T, geom, 1.0, 0.1)
    s += v
    A = s.A
    assert np.array_equal(A, A.T)
    for i in range(4):
        for j in range(4):
            assert np.array_equal(A[6 * i:6 * i + 6, 6 * j:6 * j + 6], A[6 * j:6 * j + 6, 6 * i:6 * i + 6].T)
    assert np.linalg.eigvalsh(A[6:, 6:]).min() > 0


@pytest.mark.parametrize("wd, wc", [(1.0, 0.0), (0.0, 0.1), (1.0, 0.1)])
def test_dense_system_agrees_with_the_oracle_dump(oracle, wd, wc):
    """The oracle (the reference's float32 algorithm) and the float64 restatement, entry by entry within the GPU tests' bound."""
    cache, geom, _, T_init = _oracle_frames(oracle, 4)
    n = 4
    rot, tr = oracle.matrices_to_poses(T_init)
    T = R.poses_to_matrices(rot, tr)
    res = oracle.solver_solve(np.zeros(0, dtype=ENTRYJ_DTYPE), np.ones(n, np.int32), n, 1, 1, [0.0], [wd], [wc], rot.copy(), tr.copy(),
                              cache_frames=cache, cache_geom=geom, dump_dense=True)
    v, allow, info = R.dense_system(cache, T, geom, wd, wc)
    assert res["num_dense_pairs"] == sum(1 for r in info if r.get("overlap", 0) > 10) == 6
    acc = sum(r["accepted"] for r in info); bord = sum(r["border"] for r in info)
    assert acc > 5000 and bord < 0.005 * acc, (acc, bord)
    barA = K_BOUND * np.sqrt(np.maximum(v.nA, 1)) * EPS * v.SA + allow.SA
    barb = K_BOUND * np.sqrt(np.maximum(v.nb, 1)) * EPS * v.Sb + allow.Sb
    errA = np.abs(res["JtJ"].astype(np.float64) - v.A)
    errb = np.abs(res["Jtr"].astype(np.float64) + v.b)          # the dump holds J^T r, the system b = -J^T r
    zA, zb = barA == 0, barb == 0
    assert not res["JtJ"][zA].any() and not res["Jtr"][zb].any()
    ratio = max((errA[~zA] / barA[~zA]).max(), (errb[~zb] / barb[~zb]).max())
    print("oracle vs float64 dense system (wd %g, wc %g): worst |diff| / bar = %.3f" % (wd, wc, ratio))
    assert ratio <= 1.0


def test_pcg_converges_to_the_direct_solution():
    corr, _, T_init = bs.sparse_problem(n_images=7, pair_prob=0.6, seed=11)
    n = 7
    T = T_init.astype(np.float64)
    s = R.sparse_system(corr, T, n, 1.0)
    minv, _, _ = R.sparse_preconditioner(corr, T, n)
    direct = np.linalg.solve(s.A[6:, 6:], s.b[6:])
    # the recurrence's FLOAT_EPSILON guards on pAp and r.z are absolute: they stop it at pAp <= 1e-6.  Scaling A and b by
    # 1e20 and M^-1 by 1e-20 leaves every iterate unchanged and moves the guards below float64 round-off.
    x, it = R.pcg(1e20 * s.A, 1e20 * s.b, 1e-20 * minv, 400, early_out=False)
    assert not x[:6].any()
    assert np.abs(x[6:] - direct).max() < 1e-9 * np.abs(direct).max()
    assert R.linear_residual(s.A, s.b, minv, x) < 1e-10
    x_guarded, _ = R.pcg(s.A, s.b, minv, 400)              # unscaled, the guards end it early, near the solution
    assert R.linear_residual(s.A, s.b, minv, x_guarded) < 1e-2


def test_se3_exp_log_round_trip():
    rng = np.random.default_rng(2)
    for th in (0.0, 1e-9, 1e-5, 1e-3, 0.5, np.pi / 4, 3 * np.pi / 4, np.pi - 1e-3, np.pi - 1e-7):
        ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
        rot, trans = ax * th, rng.normal(size=3)
        T = R.exp_se3(rot, trans)
        assert np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() < 1e-14
        r2, t2 = R.log_se3(T)
        assert np.abs(R.exp_se3(r2, t2) - T).max() < 1e-9, th
        if th < np.pi - 1e-2:
            assert np.abs(r2 - rot).max() < 1e-12 and np.abs(t2 - trans).max() < 1e-11, th
