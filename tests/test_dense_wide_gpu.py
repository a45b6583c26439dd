"""GPU tests (-m gpu): the wide form of the solver's dense term (k_dense_wide: one workgroup per accumulation chain, the pair's weight counted in the same
launch) against the two kernels it replaces (k_dense_weight + k_dense_build, BF_DENSE_WIDE=0).

The claim is bit identity, so there is no tolerance in this file: every case is one problem solved twice, BF_DENSE_WIDE=0 and the default, and
debug_dense_system() (JtJ, Jtr, the pair count) and the returned rotations and translations are compared as raw 32-bit words - a flipped sign of zero fails.

The cached frames are a tilted textured plane seen from poses around the first frame's, rendered here, so that every cache size is possible.  Every case that is
meant to exercise the build asserts, on the BF_DENSE_WIDE=0 output, that a pair has a non-zero block (hence a non-zero weight).
"""
import functools

import numpy as np
import pytest

from bundlefusion_amd import synth
from bundlefusion_amd.capi import ENTRYJ_DTYPE, default_solver_config, intrinsics_matrix
from tests import bundle_synth as bs

pytestmark = pytest.mark.gpu

IN_W, IN_H = 160, 120
PLANE_P0 = np.array([0.0, 0.0, 1.6])
PLANE_N = np.array([0.25, 0.15, -1.0]) / np.linalg.norm([0.25, 0.15, -1.0])


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _render(T):
    """depth f32 [H, W] and colour u8 [H, W, 4] of the plane seen through camera-to-world T"""
    K = synth.intrinsics(IN_W, IN_H)
    xs, ys = np.meshgrid(np.arange(IN_W, dtype=np.float64), np.arange(IN_H, dtype=np.float64))
    dc = np.stack([(xs - K["mx"]) / K["fx"], (ys - K["my"]) / K["fy"], np.ones_like(xs)], axis=-1)
    d = dc @ T[:3, :3].T
    o = T[:3, 3]
    t = (PLANE_N @ (PLANE_P0 - o)) / (d @ PLANE_N)
    p = o + d * t[..., None]
    a, b = p[..., 0], p[..., 1]
    img = 0.5 + 0.22 * np.sin(9.0 * a + 1.0) * np.cos(7.0 * b) + 0.2 * np.sin(23.0 * a - 17.0 * b) + 0.07 * np.cos(41.0 * b + 13.0 * a)
    colour = np.zeros((IN_H, IN_W, 4), np.uint8)
    for ch, gain in enumerate((1.0, 0.9, 0.8)):
        colour[..., ch] = np.clip(np.floor(img * gain * 256.0), 0, 255).astype(np.uint8)
    colour[..., 3] = 255
    return t.astype(np.float32), colour


@functools.lru_cache(maxsize=None)
def _scene(n, rot, trans, seed, far_frame=False, holes=False):
    """n frames: poses (frame 0 the identity), a perturbed start, the rendered frames.  far_frame: the last frame looks at the plane from 0.75 m to the side (a
    pair of little overlap).  holes: patches without depth in every frame (their rim has no normals)."""
    rng = np.random.default_rng(seed)
    T_gt = [np.eye(4)] + [bs.random_pose(rng, rot, trans) for _ in range(n - 1)]
    if far_frame:
        T_gt[-1] = np.eye(4); T_gt[-1][0, 3] = 0.75
    T_init = [T_gt[0]] + [bs.random_pose(rng, 0.004, 0.004) @ T for T in T_gt[1:]]
    frames = []
    for k, T in enumerate(T_gt):
        depth, colour = _render(T)
        if holes:
            depth[20 + 5 * k: 50 + 5 * k, 30: 60] = -np.inf
            depth[80: 95, 100 - 4 * k: 140 - 4 * k] = -np.inf
        frames.append((depth, colour))
    return np.stack(T_gt).astype(np.float32), np.stack(T_init).astype(np.float32), frames


def _cache(gpu, frames, cw, ch):
    K = synth.intrinsics(IN_W, IN_H)
    cache = gpu.capi.Cache(IN_W, IN_H, cw, ch, len(frames), intrinsics_matrix(K["fx"], K["fy"], K["mx"], K["my"]))
    for d, c in frames:
        cache.store_frame(_dev(d), _dev(c))
    return cache


def _solve(gpu, oracle, monkeypatch, wide, cache, T_init, wd, wc, n_lin=10, use_pairwise=True, cfg=None, corr=None, max_residuals=1):
    if wide is None:
        monkeypatch.delenv("BF_DENSE_WIDE", raising=False)          # the default is the wide form
    else:
        monkeypatch.setenv("BF_DENSE_WIDE", wide)
    n = len(T_init)
    corr = np.zeros(0, dtype=ENTRYJ_DTYPE) if corr is None else corr
    solver = gpu.capi.Solver(n, max(len(corr), max_residuals), cfg or default_solver_config())           # the switch is read when a solver is created
    monkeypatch.delenv("BF_DENSE_WIDE", raising=False)
    rot0, tr0 = oracle.matrices_to_poses(T_init)
    grot, gtr = _dev(rot0.copy()), _dev(tr0.copy())
    gcorr = _dev(corr.view(np.uint8)) if len(corr) else None
    solver.solve(gcorr, len(corr), _dev(np.ones(n, np.int32)), n, len(wd), n_lin, cache, [1.0] * len(wd), wd, wc, grot, gtr, use_pairwise=use_pairwise)
    JtJ, Jtr, npairs = solver.debug_dense_system(n)
    return JtJ, Jtr, npairs, grot.cpu().numpy(), gtr.cpu().numpy()


def _block(JtJ, i, j):
    return JtJ[6 * i: 6 * i + 6, 6 * j: 6 * j + 6]


def _both(gpu, oracle, monkeypatch, cache, T_init, wd, wc, build=True, **kw):
    ref = _solve(gpu, oracle, monkeypatch, "0", cache, T_init, wd, wc, **kw)
    new = _solve(gpu, oracle, monkeypatch, None, cache, T_init, wd, wc, **kw)
    if build:        # the reference path did real work: a pair has a non-zero block (its jj part at the least: frame 0's columns are zero), hence a non-zero weight
        assert ref[2] > 0 and ref[0].any() and ref[1].any(), "no pair above the gate: the case checks nothing"
    for k, what in enumerate(("JtJ", "Jtr")):
        assert np.array_equal(ref[k].view(np.uint32), new[k].view(np.uint32)), "%s differs in %d words" % (what, (ref[k].view(np.uint32) != new[k].view(np.uint32)).sum())
    assert ref[2] == new[2], "pair counts differ: %d / %d" % (ref[2], new[2])
    assert np.array_equal(ref[3].view(np.uint32), new[3].view(np.uint32)), "rotations differ"
    assert np.array_equal(ref[4].view(np.uint32), new[4].view(np.uint32)), "translations differ"
    assert np.isfinite(new[3]).all() and np.isfinite(new[4]).all()
    return ref


WEIGHTS = {"depth": ([1.0], [0.0]), "colour": ([0.0], [0.1]), "both": ([1.0], [0.1])}


@pytest.mark.parametrize("weights", ["depth", "colour", "both"])
@pytest.mark.parametrize("cw, ch", [(40, 30), (80, 60)])
def test_cache_sizes_and_pass_order(gpu, oracle, monkeypatch, cw, ch, weights):
    """40 x 30: five trips, the last with 176 pixels, one round of the wide form.  80 x 60: 18.75 trips, three rounds, the last with three trips.  Depth rows
    only, colour rows only, and both (the depth pass of a trip runs before its colour pass)."""
    _, T_init, frames = _scene(4, 0.012, 0.012, 1)
    wd, wc = WEIGHTS[weights]
    _both(gpu, oracle, monkeypatch, _cache(gpu, frames, cw, ch), T_init, wd, wc)


def test_cache_20x15_every_weight_is_zero(gpu, oracle, monkeypatch):
    """300 pixels cannot reach the 800-correspondence gate: every listed pair takes the zero-block path."""
    _, T_init, frames = _scene(4, 0.012, 0.012, 1)
    cfg = default_solver_config()
    cfg.denseOverlapCheckSubsampleFactor = 2               # the overlap pre-filter needs more than 8 samples per row
    ref = _both(gpu, oracle, monkeypatch, _cache(gpu, frames, 20, 15), T_init, [1.0], [0.1], build=False, cfg=cfg)
    assert ref[2] > 0 and not ref[0].any() and not ref[1].any()


@pytest.mark.parametrize("n", [2, 3])
def test_two_and_three_frames(gpu, oracle, monkeypatch, n):
    """N = 2: the one pair has i = 0, the fixed frame, so the derivI columns stay zero.  N = 3 adds the pair (1, 2) with both."""
    _, T_init, frames = _scene(n, 0.012, 0.012, 2)
    ref = _both(gpu, oracle, monkeypatch, _cache(gpu, frames, 40, 30), T_init, [1.0], [0.1])
    assert not _block(ref[0], 0, 0).any() and _block(ref[0], 1, 1).any()


@pytest.mark.parametrize("pairwise", [True, False])
def test_eleven_frames(gpu, oracle, monkeypatch, pairwise):
    """The local chunk's size at the workload's cache size: up to 55 pairs, or the 10 pairs of consecutive frames."""
    _, T_init, frames = _scene(11, 0.02, 0.02, 3)
    ref = _both(gpu, oracle, monkeypatch, _cache(gpu, frames, 80, 60), T_init, [1.0], [0.1], use_pairwise=pairwise)
    assert ref[2] == 10 if not pairwise else ref[2] > 10


def test_a_pair_below_the_gate_beside_pairs_above_it(gpu, oracle, monkeypatch):
    """The last frame stands 0.75 m to the side: its pairs pass the overlap pre-filter with too few correspondences, and get zero blocks between the others'."""
    n = 4
    _, T_init, frames = _scene(n, 0.008, 0.008, 4, far_frame=True)
    ref = _both(gpu, oracle, monkeypatch, _cache(gpu, frames, 40, 30), T_init, [1.0], [0.1])
    assert ref[2] == 6, ref[2]
    assert _block(ref[0], 1, 2).any() and not any(_block(ref[0], i, 3).any() for i in range(3)) and not _block(ref[0], 3, 3).any()


def test_invalid_regions(gpu, oracle, monkeypatch):
    """Holes without depth (and no normals on their rim) in every frame, a dense depth range that ends inside the plane, and poses 3 degrees apart, whose
    projections leave the image on one side."""
    _, T_init, frames = _scene(4, 0.03, 0.03, 5, holes=True)
    cfg = default_solver_config()
    cfg.denseDepthMin, cfg.denseDepthMax = 1.45, 1.8
    _both(gpu, oracle, monkeypatch, _cache(gpu, frames, 80, 60), T_init, [1.0], [0.1], cfg=cfg)


def test_two_gauss_newton_iterations(gpu, oracle, monkeypatch):
    """The second iteration's system is built from the first's poses: the dump is the second's, the poses are after both."""
    _, T_init, frames = _scene(5, 0.012, 0.012, 6)
    _both(gpu, oracle, monkeypatch, _cache(gpu, frames, 40, 30), T_init, [1.0, 2.0], [0.1, 0.1], n_lin=20)


def test_more_than_1024_pairs(gpu, oracle, monkeypatch):
    """48 frames that all see each other: 1128 pairs, more than the 1024 a launch has workgroup groups for, so some workgroups take a second chain."""
    _, T_init, frames = _scene(48, 0.006, 0.006, 7)
    ref = _both(gpu, oracle, monkeypatch, _cache(gpu, frames, 40, 30), T_init, [1.0], [0.0], n_lin=2)
    assert ref[2] > 1024, ref[2]


def test_more_pairs_than_the_wide_form_holds(gpu, oracle, monkeypatch):
    """66 frames that all see each other in a solver with room for them: 2145 possible pairs, more than the 2048 the wide form keeps parts and tickets for, so the
    default takes the two kernels as well - the switch itself."""
    _, T_init, frames = _scene(66, 0.005, 0.005, 8)
    ref = _both(gpu, oracle, monkeypatch, _cache(gpu, frames, 40, 30), T_init, [1.0], [0.0], n_lin=2, max_residuals=2000)
    assert ref[2] > 2048, ref[2]
