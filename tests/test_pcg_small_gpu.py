"""GPU tests (-m gpu): the single-workgroup small-problem PCG (k_pcg_small: 6 N <= 256, CG vectors in registers, every wave carrying the whole state, one
barrier per iteration) against the 256-thread cooperative kernel it replaces there (BF_PCG_WIDE=0).

The claim is bit identity, so there is no tolerance in this file: every case is one problem solved twice, BF_PCG_WIDE=1 and =0, and the rotations, the
translations, iteration_counts(), convergence() and max_residual() are compared with np.array_equal / ==.

The library takes one workgroup by itself for N <= 32; N = 33 .. 42 still have 6 N <= 256 and reach the kernel with BF_PCG_GROUPS=1, which the cases at those
sizes set for both solves (N = 43 then takes the 256-thread kernel either way: the switch itself).
"""
import numpy as np
import pytest

from bundlefusion_amd.capi import ENTRYJ_DTYPE, default_solver_config, intrinsics_matrix
from tests import bundle_synth as bs

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _solve(gpu, oracle, monkeypatch, wide, corr, T_init, n_nonlin, n_lin, valid=None, groups=None, cache=None, wd=None, wc=None):
    monkeypatch.setenv("BF_PCG_WIDE", wide)
    if groups is None:
        monkeypatch.delenv("BF_PCG_GROUPS", raising=False)
    else:
        monkeypatch.setenv("BF_PCG_GROUPS", groups)
    n = len(T_init)
    rot0, tr0 = oracle.matrices_to_poses(T_init)
    valid = np.ones(n, np.int32) if valid is None else valid
    solver = gpu.capi.Solver(max(n, 2), max(len(corr), 1), default_solver_config(record_convergence=True))      # the hooks are read when a solver is created
    monkeypatch.delenv("BF_PCG_WIDE", raising=False)
    monkeypatch.delenv("BF_PCG_GROUPS", raising=False)
    grot, gtr = _dev(rot0.copy()), _dev(tr0.copy())
    gcorr = _dev(corr.view(np.uint8)) if len(corr) else None
    wd = [0.0] * n_nonlin if wd is None else wd
    wc = [0.0] * n_nonlin if wc is None else wc
    solver.solve(gcorr, len(corr), _dev(valid), n, n_nonlin, n_lin, cache, [1.0] * n_nonlin, wd, wc, grot, gtr, find_max_residual=True)
    gn, pcg = solver.iteration_counts()
    return grot.cpu().numpy(), gtr.cpu().numpy(), (gn, list(pcg)), np.array(solver.convergence(), np.float32), np.array(solver.max_residual())


def _same(a, b, what=""):
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), "rotations differ " + what
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), "translations differ " + what
    assert a[2] == b[2], "iteration counts differ %s: %s / %s" % (what, a[2], b[2])
    assert np.array_equal(a[3].view(np.uint32), b[3].view(np.uint32)), "energies differ " + what
    assert np.array_equal(a[4], b[4]), "largest residual differs " + what


def _both(gpu, oracle, monkeypatch, corr, T_init, n_nonlin=3, n_lin=150, **kw):
    wide = _solve(gpu, oracle, monkeypatch, "1", corr, T_init, n_nonlin, n_lin, **kw)
    narrow = _solve(gpu, oracle, monkeypatch, "0", corr, T_init, n_nonlin, n_lin, **kw)
    _same(wide, narrow)
    assert np.isfinite(wide[0]).all() and np.isfinite(wide[1]).all()
    return wide


def _keep_pairs(corr, pairs):
    key = set(pairs)
    return corr[np.array([(int(e["imgIdx_i"]), int(e["imgIdx_j"])) in key for e in corr], bool)]


@pytest.mark.parametrize("n", [2, 11, 12, 22, 23, 33, 34, 42, 43])
def test_register_occupancy_and_its_boundaries(gpu, oracle, monkeypatch, n):
    """Register j of a lane holds element 6 + 64 j + lane: N = 11 fills part of register 0, 12 puts the first element into register 1, 22 / 23 are the same
    step into register 2, 33 / 34 into register 3, 42 is the last size of the form and 43 the first of the other kernel."""
    corr, _, T_init = bs.sparse_problem(n_images=n, pair_prob=min(1.0, 8.0 / n), seed=300 + n)
    out = _both(gpu, oracle, monkeypatch, corr, T_init, groups="1" if n > 32 else None)
    assert out[2][0] >= 1 and all(k >= 1 for k in out[2][1])


def test_rows_of_0_1_8_and_9_slots(gpu, oracle, monkeypatch):
    """Eight lanes take one off-diagonal block each, eight blocks per trip of the slot loop.  Frame 1 is matched only to frame 0 (one slot, whose column is the
    fixed frame: the zeros at the head of p), frame 2 to nothing (no slot, a zero diagonal block, preconditioner 1), frame 3 to eight frames (one full trip),
    frame 4 to nine (a second trip with one block)."""
    n = 12
    corr, _, T_init = bs.sparse_problem(n_images=n, pair_prob=1.0, pts_per_pair=12, seed=41)
    pairs = [(0, 1)] + [(3, j) for j in range(4, 12)] + [(0, 4)] + [(4, j) for j in range(5, 12)]
    corr = _keep_pairs(corr, pairs)
    deg = np.zeros(n, int)
    for i, j in pairs:
        deg[i] += 1; deg[j] += 1
    assert deg[1] == 1 and deg[2] == 0 and deg[3] == 8 and deg[4] == 9
    _both(gpu, oracle, monkeypatch, corr, T_init)


def test_rows_of_41_slots(gpu, oracle, monkeypatch):
    """The complete graph at N = 42: every row has 41 slots, six trips of the slot loop, the last with one block; 41 rows over 16 waves are three trips of the
    row loop, the last with nine rows."""
    corr, _, T_init = bs.sparse_problem(n_images=42, pair_prob=1.0, pts_per_pair=4, seed=42)
    _both(gpu, oracle, monkeypatch, corr, T_init, groups="1")


def test_one_linear_iteration(gpu, oracle, monkeypatch):
    corr, _, T_init = bs.sparse_problem(n_images=11, seed=43)
    out = _both(gpu, oracle, monkeypatch, corr, T_init, n_nonlin=2, n_lin=1)
    assert out[2][1] == [1] * out[2][0]


def test_start_at_the_optimum_ends_the_loop_early(gpu, oracle, monkeypatch):
    """T_init = T_gt and no noise: the right-hand side is round-off, |pAp| < 5e-7 (or alpha = 0) ends the loop long before its 150 iterations."""
    corr, T_gt, T_init = bs.sparse_problem(n_images=11, noise=0.0, perturb=(0.0, 0.0), seed=44)
    assert np.array_equal(T_init, T_gt)
    out = _both(gpu, oracle, monkeypatch, corr, T_init)
    assert all(k < 150 for k in out[2][1]), out[2]


def test_later_gauss_newton_iterations_find_the_solve_done(gpu, oracle, monkeypatch):
    """A start 1 mm / 1 mrad from the optimum with 0.1 mm noise: the first update is far below the 5 mm / 5 mrad bar, so the first iteration sets FL_DONE and
    the two later launches return at once - one Gauss-Newton iteration is counted, by both kernels."""
    corr, _, T_init = bs.sparse_problem(n_images=22, pair_prob=0.4, noise=0.0001, perturb=(0.001, 0.001), seed=45)
    out = _both(gpu, oracle, monkeypatch, corr, T_init, n_nonlin=3)
    assert out[2][0] == 1 and len(out[2][1]) == 1, out[2]


def test_invalid_frames_and_invalid_correspondences(gpu, oracle, monkeypatch):
    """Frames with valid = 0 stay in the system and leave the convergence test; correspondences with invalid indices (every fourth, scattered) leave the system."""
    n = 30
    corr, _, T_init = bs.sparse_problem(n_images=n, seed=9)
    corr["imgIdx_i"][::4] = 0xFFFFFFFF
    corr["imgIdx_j"][::4] = 0xFFFFFFFF
    corr = corr[np.random.default_rng(0).permutation(len(corr))]
    valid = np.ones(n, np.int32); valid[[3, 7, 29]] = 0
    _both(gpu, oracle, monkeypatch, corr, T_init, valid=valid)
    _both(gpu, oracle, monkeypatch, corr, T_init)


def test_the_same_solve_twice_gives_the_same_bits(gpu, oracle, monkeypatch):
    corr, _, T_init = bs.sparse_problem(n_images=32, pair_prob=0.3, seed=46)
    a = _solve(gpu, oracle, monkeypatch, "1", corr, T_init, 3, 150)
    b = _solve(gpu, oracle, monkeypatch, "1", corr, T_init, 3, 150)
    _same(a, b, "between two runs")


@pytest.mark.parametrize("cw, ch", [(36, 27), (40, 30)])
def test_local_chunk_with_the_dense_term(gpu, oracle, monkeypatch, cw, ch):
    """The local-chunk configuration (2 Gauss-Newton x <= 100 PCG iterations, sparse weight 1, dense depth weight i + 1): the matrix comes from k_dense_build.
    36 x 27 is the smallest cache the solver accepts (width / subsample factor 4 must exceed 8); its 972 pixels leave few pairs above the 800-pixel floor, so
    40 x 30 runs beside it."""
    n = 5
    frames, K, T_gt, T_init = bs.dense_chunk(n_frames=n, width=160, height=120, perturb=(0.006, 0.015))
    cache = gpu.capi.Cache(160, 120, cw, ch, n, intrinsics_matrix(K["fx"], K["fy"], K["mx"], K["my"]))
    for d, c in frames:
        cache.store_frame(_dev(d), _dev(c))
    rng = np.random.default_rng(4)
    rows = []
    for i in range(n):
        for j in range(i + 1, n):
            for p in rng.uniform(-0.8, 0.8, (15, 3)) + np.array([0, 0, 1.5]):
                ph = np.r_[p, 1.0]
                rows.append((i, j, (np.linalg.inv(T_gt[i].astype(np.float64)) @ ph)[:3] + rng.normal(0, 0.003, 3),
                             (np.linalg.inv(T_gt[j].astype(np.float64)) @ ph)[:3] + rng.normal(0, 0.003, 3)))
    corr = np.zeros(len(rows), dtype=ENTRYJ_DTYPE)
    for k, (i, j, a, b) in enumerate(rows):
        corr[k] = (i, j, a.astype(np.float32), b.astype(np.float32))
    _both(gpu, oracle, monkeypatch, corr, T_init, n_nonlin=2, n_lin=100, cache=cache, wd=[1.0, 2.0], wc=[0.0, 0.0])
