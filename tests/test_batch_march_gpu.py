"""GPU parity tests (-m gpu) of the ray march that finds the blocks an operator allocates (csrc/tsdf.hip: marchTile, waveSetInsert, waveSetFlush and their three
sinks - the per-operator allocation, the collect pass of the divided march, the batch's claims), at the smallest shapes at which its pieces can go wrong: partial
tiles, dead pixels, rays along an axis, the neighbour pre-filter firing always / never, more distinct blocks per tile than the wave's key set buffers, a full batch
whose operator masks reach the result, batches back to back, a sharded volume.

Every case holds table, heap, allocated-block list and voxels to the CPU oracle (exact contract, tol = 0); where a batch is used, also to the same operators issued
one at a time.  The march only decides WHICH blocks exist: one lost or extra key shows as a different table."""
import numpy as np
import pytest

from bundlefusion_amd import synth
from bundlefusion_amd.capi import default_hash_params, camera_params, FREE_ENTRY, VOX_PER_BLOCK, SCENE_BATCH_MAX

from tests.test_tsdf_gpu import assert_same_state, _to_dev
from tests.test_tsdf_batch_gpu import _apply_serial_gpu, _apply_oracle, _apply_batch, _volume, _perturbed

pytestmark = pytest.mark.gpu

MINF = np.float32(-np.inf)
ROT180Y = np.array([[-1, 0, 0, 0], [0, 1, 0, 0], [0, 0, -1, 0], [0, 0, 0, 1]], np.float32)


def _color(H, W, seed=0):
    c = np.random.default_rng(seed).integers(0, 256, size=(H, W, 4), dtype=np.uint8)
    c[..., 3] = 255
    return c


def _pose(tx=0.0, ty=0.0, tz=0.0, R=None):
    T = np.eye(4, dtype=np.float32) if R is None else R.copy()
    T[:3, 3] = [tx, ty, tz]
    return T


def _apply_collected(gs, ops, dev, cam, bufs):
    """The operators one at a time, each allocation through the collect pass of the divided march (one band = the whole image), ingest and placement."""
    keys, slots, cnt = bufs
    for kind, i, T0, T1 in ops:
        if kind != "de":
            gs.alloc_collect(T0 if kind == "in" else T1, dev[i][0], cam, 0, 1, keys, slots, cnt)
            gs.alloc_sync()
            gs.alloc_ingest(keys, cnt)
            gs.alloc_place()
            gs.alloc_sync()
        _apply_serial_gpu(gs, [(kind, i, T0, T1)], dev, cam)


def _hold_to_oracle(gpu, oracle, p, cam, frames, batches, collect=True, gc=True):
    """frames: [(depth, colour)], batches: [[(kind, frame, T0, T1)]].  The batch, the operators one by one and (collect) the operators behind a collect / ingest /
    place allocation, each against the oracle after every batch; returns the oracle scene for the caller's own assertions about the scenario."""
    import torch
    gb, ga = gpu.capi.SceneRepHashSDF(p), gpu.capi.SceneRepHashSDF(p)
    ge = gpu.capi.SceneRepHashSDF(p) if collect else None
    for g in (gb, ga, ge):
        if g is not None:
            g.set_arith("exact")
    if collect:
        ge.set_external_alloc(True)
        bufs = (torch.zeros(1 << 15, dtype=torch.int64, device="cuda"), torch.zeros(1 << 15, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"))
    osc = oracle.OracleScene(p)
    dev = [_to_dev(d, c) for d, c in frames]
    for r, ops in enumerate(batches):
        assert len(ops) <= SCENE_BATCH_MAX
        _apply_batch(gb, ops, dev, cam)
        _apply_serial_gpu(ga, ops, dev, cam)
        _apply_oracle(osc, ops, frames, cam)
        assert_same_state(gb, osc, "batch %d, as a batch:" % r)
        assert_same_state(ga, osc, "batch %d, one by one:" % r)
        assert _volume(gb) == _volume(ga), "batch %d: the batch against the operators one at a time" % r
        if collect:
            _apply_collected(ge, ops, dev, cam, bufs)
            assert_same_state(ge, osc, "batch %d, collected allocation:" % r)
        if gc:
            for g in (gb, ga, ge):
                if g is not None:
                    g.garbage_collect()
            osc.garbage_collect()
            assert_same_state(gb, osc, "batch %d + GC:" % r)
    return osc


def _mixed_ops(n, poses):
    """integrate every frame, then move the first, take the last out, put it back elsewhere"""
    first = [("in", i, poses[i], None) for i in range(n)]
    moved = _pose(0.03, -0.02, 0.05)
    second = [("re", 0, poses[0], moved @ poses[0]), ("de", n - 1, poses[n - 1], None), ("in", n - 1, _pose(-0.04, 0.01, 0.0) @ poses[n - 1], None)]
    return [first, second]


# ---------------------------------------------------------------------------------------
# 1. image shapes: partial tiles at the right and bottom edges (lanes dead from the start), one image of whole tiles
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(8, 8), (20, 12), (9, 17), (64, 48)])
def test_image_shapes_with_partial_tiles(gpu, oracle, W, H):
    K = synth.intrinsics(W, H)
    cam = camera_params(W, H, K["fx"], K["fy"], K["mx"], K["my"])
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    frames = [((1.2 + 0.02 * xs + 0.013 * ys).astype(np.float32), _color(H, W, 1)), ((2.1 - 0.015 * xs + 0.01 * ys).astype(np.float32), _color(H, W, 2))]
    poses = [_pose(), _pose(0.1, 0.05, -0.2)]
    p = default_hash_params(num_buckets=20000, num_sdf_blocks=6000, voxel_size=0.02)
    osc = _hold_to_oracle(gpu, oracle, p, cam, frames, _mixed_ops(2, poses))
    assert osc.num_allocated() > 0 and osc.num_dropped() == 0


# ---------------------------------------------------------------------------------------
# 2. dead pixels: -inf, 0, at and beyond maxIntegrationDistance, valid - mixed inside tiles, and tiles that are invalid as a whole
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(20, 12), (64, 48)])
def test_dead_pixels_and_dead_tiles(gpu, oracle, W, H):
    K = synth.intrinsics(W, H)
    cam = camera_params(W, H, K["fx"], K["fy"], K["mx"], K["my"])
    p = default_hash_params(num_buckets=20000, num_sdf_blocks=6000, voxel_size=0.02, max_integration_distance=3.0)
    rng = np.random.default_rng(7)
    kinds = np.array([MINF, 0.0, 3.0, 3.5, 1.4, 1.9, 2.6], np.float32)          # 3.0 == maxIntegrationDistance: dead; 2.6: its band is clipped at the distance
    frames = []
    for s in range(2):
        d = kinds[rng.integers(0, len(kinds), size=(H, W))]
        d[0:8, 0:8] = MINF                                                         # whole tiles: -inf, 0, at the distance
        if W > 16:
            d[0:8, 8:16] = 0.0
        if W > 24:
            d[0:8, 16:24] = 3.0
            d[8:16, 0:8] = 1.5 + 0.001 * np.arange(8, dtype=np.float32)            # and one that is valid as a whole
        frames.append((d.astype(np.float32), _color(H, W, s)))
    poses = [_pose(), _pose(-0.2, 0.1, 0.3)]
    osc = _hold_to_oracle(gpu, oracle, p, cam, frames, _mixed_ops(2, poses))
    assert osc.num_allocated() > 0


# ---------------------------------------------------------------------------------------
# 3. rays along an axis: the +inf paths of tMax / tDelta
# ---------------------------------------------------------------------------------------
def test_axis_aligned_rays(gpu, oracle):
    """The principal point on a pixel centre and poses whose rotations hold only 0 and +-1: the centre column's rays have direction x == 0 exactly, the centre row's
    y == 0, the centre pixel both.  Voxel size, truncation and the translation are powers of two and short sums of them, so the second pose also puts the start of
    the centre ray exactly ON the block boundary it marches away from: boundary - rayMin == 0 on z with a direction that is not 0 (camera looking down -z,
    rayMin.z = 1.90625 - 0.9375 = 0.96875 = 2 * 0.5 - 0.03125, the lower face of block 2), and on x and y together with direction 0."""
    W = H = 9
    cam = camera_params(W, H, 10.0, 10.0, 4.0, 4.0)
    p = default_hash_params(num_buckets=20000, num_sdf_blocks=6000, voxel_size=0.0625, truncation=0.0625, trunc_scale=0.0)
    assert np.float32(1.90625) - (np.float32(1.0) - np.float32(0.0625)) == np.float32(2 * 0.5 - 0.03125)
    frames = [(np.full((H, W), 1.0, np.float32), _color(H, W, 3)), (np.full((H, W), 1.0, np.float32), _color(H, W, 4))]
    poses = [_pose(), _pose(0.46875, 0.46875, 1.90625, ROT180Y)]
    batches = [[("in", 0, poses[0], None), ("in", 1, poses[1], None)], [("re", 1, poses[1], _pose(0.46875, -0.53125, 1.40625, ROT180Y)), ("de", 0, poses[0], None)]]
    osc = _hold_to_oracle(gpu, oracle, p, cam, frames, batches)
    assert osc.num_allocated() > 0 and osc.num_dropped() == 0


# ---------------------------------------------------------------------------------------
# 4. the neighbour pre-filter: always (a fronto-parallel plane) and never (a per-pixel checkerboard with jumps larger than a block)
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("surface", ["plane", "checkerboard"])
def test_neighbour_filter_always_and_never(gpu, oracle, surface):
    W, H = 64, 48
    K = synth.intrinsics(W, H)
    cam = camera_params(W, H, K["fx"] * 8, K["fy"] * 8, K["mx"], K["my"])      # a narrow view: a block is many pixels wide, neighbours share it nearly every step
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    if surface == "plane":
        d = np.full((H, W), 1.5, np.float32)
    else:
        d = np.where((xs + ys) % 2 == 0, np.float32(1.0), np.float32(2.5)).astype(np.float32)      # 1.5 m apart: nine blocks of 0.16 m
    frames = [(d, _color(H, W, 5)), (np.roll(d, 1, axis=1).copy(), _color(H, W, 6))]
    poses = [_pose(), _pose(0.05, 0.0, 0.1)]
    p = default_hash_params(num_buckets=20000, num_sdf_blocks=6000, voxel_size=0.02)
    osc = _hold_to_oracle(gpu, oracle, p, cam, frames, _mixed_ops(2, poses))
    assert osc.num_allocated() > 0 and osc.num_dropped() == 0


# ---------------------------------------------------------------------------------------
# 5. more distinct blocks per tile than the wave's set buffers: flushes inside the loop, the cleared set used again
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("spread", ["disjoint", "overlapping"])
def test_many_keys_per_tile(gpu, oracle, spread):
    """One 8x8 tile, 4 mm voxels (a block is 3.2 cm), a truncation band of 0.6 m: every ray crosses ~20 blocks.  disjoint: the pixels are 20 cm apart at the surface,
    so all 64 lanes bring a new block in every step - 64 keys after the first step (the flush threshold exactly: not flushed), 128 after the second (the list full to
    its last entry, flushed, the set cleared and filled again, ~10 times).  overlapping: pixels 2.5 cm apart, neighbours share some blocks and not others, the
    count passes the threshold at irregular steps."""
    W = H = 8
    f = 7.3 if spread == "disjoint" else 60.0
    cam = camera_params(W, H, f, f, 3.5, 3.5)
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    frames = [((1.5 + 0.003 * xs - 0.002 * ys).astype(np.float32), _color(H, W, 8)), ((1.3 + 0.004 * ys).astype(np.float32), _color(H, W, 9))]
    poses = [_pose(), _pose(0.02, 0.01, 0.0)]
    p = default_hash_params(num_buckets=50000, num_sdf_blocks=12000, voxel_size=0.004, truncation=0.3, trunc_scale=0.0)
    osc = _hold_to_oracle(gpu, oracle, p, cam, frames, [[("in", 0, poses[0], None), ("in", 1, poses[1], None)], [("de", 0, poses[0], None)]])
    assert osc.num_dropped() == 0
    assert osc.num_allocated() > (600 if spread == "disjoint" else 64), "the tile was supposed to meet more blocks than one fill of the wave's set"


# ---------------------------------------------------------------------------------------
# 6. a full batch whose operator masks reach the result
# ---------------------------------------------------------------------------------------
def test_full_batch_with_too_small_a_heap(gpu, oracle):
    """BF_SCENE_BATCH_MAX operators - integrations, de-integrations (texels only: no march), re-integrations - of overlapping views, so several operators claim the
    same key; the heap holds fewer blocks than the batch needs, so the placement replays operator by operator and WHICH operators needed a key decides who gets the
    last blocks."""
    W, H = 64, 48
    frames5 = [synth.scene_room(k * 6, W, H) for k in range(8)]
    K = frames5[0][3]
    cam = camera_params(W, H, K["fx"], K["fy"], K["mx"], K["my"])
    frames = [(f[0], f[1]) for f in frames5]
    T = [f[2] for f in frames5]
    rng = np.random.default_rng(3)
    first = [("in", i, T[i], None) for i in range(6)]
    T2 = [_perturbed(T[i], rng, 0.05, 0.02) for i in range(8)]
    full = ([("re", i, T[i], T2[i]) for i in range(4)] + [("de", 4, T[4], None), ("de", 5, T[5], None)] + [("in", 6, T[6], None), ("in", 7, T[7], None)]
            + [("in", 4, T2[4], None), ("re", 0, T2[0], T[0]), ("de", 6, T[6], None), ("in", 5, T2[5], None)])
    assert len(full) == SCENE_BATCH_MAX
    p = default_hash_params(num_buckets=20000, num_sdf_blocks=500, voxel_size=0.02)
    osc = _hold_to_oracle(gpu, oracle, p, cam, frames, [first, full], collect=False)
    assert osc.num_dropped() > 0, "the heap was supposed to run out inside the batch"
    roomy = default_hash_params(num_buckets=20000, num_sdf_blocks=6000, voxel_size=0.02)
    osc = _hold_to_oracle(gpu, oracle, roomy, cam, frames, [first, full], collect=False)
    assert osc.num_dropped() == 0 and osc.num_allocated() > 500


# ---------------------------------------------------------------------------------------
# 7. batches back to back: a key set that was not left clean shows in the next batch
# ---------------------------------------------------------------------------------------
def test_two_batches_and_a_collection_without_host_synchronisation(gpu, oracle):
    W, H = 64, 48
    fr = [synth.scene_room(k * 8, W, H) for k in range(6)]
    K = fr[0][3]
    cam = camera_params(W, H, K["fx"], K["fy"], K["mx"], K["my"])
    frames = [(f[0], f[1]) for f in fr]
    T = [f[2] for f in fr]
    rng = np.random.default_rng(9)
    b1 = [("in", i, T[i], None) for i in range(4)]
    T2 = [_perturbed(T[i], rng, 0.1, 0.05) for i in range(4)]
    b2 = [("re", i, T[i], T2[i]) for i in range(4)] + [("in", 4, T[4], None), ("in", 5, T[5], None)]
    p = default_hash_params(num_buckets=20000, num_sdf_blocks=6000, voxel_size=0.02)
    gs, osc = gpu.capi.SceneRepHashSDF(p), oracle.OracleScene(p)
    gs.set_arith("exact"); gs.set_overlap(True)
    dev = [_to_dev(d, c) for d, c in frames]
    _apply_batch(gs, b1, dev, cam)              # nothing below reads the device until all three are queued
    _apply_batch(gs, b2, dev, cam)
    gs.garbage_collect()
    _apply_batch(gs, [("de", 4, T[4], None), ("in", 4, T2[0], None)], dev, cam)
    _apply_oracle(osc, b1, frames, cam); _apply_oracle(osc, b2, frames, cam)
    osc.garbage_collect()
    _apply_oracle(osc, [("de", 4, T[4], None), ("in", 4, T2[0], None)], frames, cam)
    assert_same_state(gs, osc, "two batches, a collection, a third batch:")
    assert osc.num_dropped() == 0


# ---------------------------------------------------------------------------------------
# 8. a sharded volume: keys outside the owned bucket range are claimed and dropped
# ---------------------------------------------------------------------------------------
def test_batch_on_a_sharded_volume(gpu, oracle):
    W, H = 64, 48
    fr = [synth.scene_room(k * 8, W, H) for k in range(5)]
    K = fr[0][3]
    cam = camera_params(W, H, K["fx"], K["fy"], K["mx"], K["my"])
    frames = [(f[0], f[1]) for f in fr]
    T = [f[2] for f in fr]
    b1 = [("in", i, T[i], None) for i in range(5)]
    b2 = [("re", 1, T[1], _pose(0.04, 0.0, 0.02) @ T[1]), ("de", 0, T[0], None), ("in", 0, _pose(0.0, 0.03, 0.0) @ T[0], None)]
    p = default_hash_params(num_buckets=20000, num_sdf_blocks=6000, voxel_size=0.02)
    osc = oracle.OracleScene(p)
    dev = [_to_dev(d, c) for d, c in frames]
    _apply_oracle(osc, b1, frames, cam); _apply_oracle(osc, b2, frames, cam)

    def blocks(hash_, vox):
        occ = hash_[hash_["ptr"] != FREE_ENTRY]
        return {tuple(int(v) for v in e["pos"]): vox[int(e["ptr"]):int(e["ptr"]) + VOX_PER_BLOCK].tobytes() for e in occ}
    whole = blocks(osc.hash(), osc.voxels())
    G, union = 2, {}
    for r in range(G):
        gb, ga = gpu.capi.SceneRepHashSDF(p), gpu.capi.SceneRepHashSDF(p)
        for g, apply in ((gb, _apply_batch), (ga, _apply_serial_gpu)):
            g.set_arith("exact"); g.set_shard(r, G)
            apply(g, b1, dev, cam); apply(g, b2, dev, cam)
        assert _volume(gb) == _volume(ga), "shard %d: the batch against the operators one at a time" % r
        gh, _, _, gvox = gb.download()
        mine = blocks(gh, gvox)
        assert mine and all(oracle.hash_pos(p.m_hashNumBuckets, *k) * G // p.m_hashNumBuckets == r for k in mine)
        assert not (mine.keys() & union.keys())
        union.update(mine)
        dbg = gb.debug_hash()
        assert dbg["duplicate_keys"] == 0 and dbg["leaked"] == 0 and dbg["free_and_allocated"] == 0 and dbg["dropped"] == 0
    assert union.keys() == whole.keys() and len(whole) > 100
    assert all(union[k] == whole[k] for k in whole), "the shards' voxels against the oracle's"
