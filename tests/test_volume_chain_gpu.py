"""GPU parity tests (-m gpu) of the launches between two batched voxel updates (csrc/tsdf.hip: k_gc_identify's early-out scan, the hand-offs inside k_gc_delete and
k_compact_scatter; csrc/tsdf_batch.h: the batch's march) against the CPU oracle under the exact contract: table, heap, allocated-block list and every voxel byte.

The garbage collection deletes the blocks of the last pose's frustum list whose weights ALL truncate to zero.  The scan leaves a block at the first 64-voxel slice
that holds another weight, so the planted cases put the only such weight where a scan that stops early - or reads a slice short - would miss it.
"""
import numpy as np
import pytest

from bundlefusion_amd import synth
from bundlefusion_amd.capi import default_hash_params, camera_params, FREE_ENTRY, VOX_PER_BLOCK, _h2d

from tests.test_tsdf_gpu import assert_same_state, _to_dev

pytestmark = pytest.mark.gpu

W, H = 160, 120
# name -> {voxel: weight} of the planted block (every other weight 0)
PLANTS = {
    "all_zero": {},
    "voxel_0": {0: 1.0},
    "voxel_511": {511: 2.0},
    "voxels_63_64": {63: 1.0, 64: 1.0},
    "voxel_448": {448: 3.0},
    "half_only": {5: 0.5, 200: 0.5, 511: 0.5},      # (uint) 0.5 == 0
}
DELETED = {"all_zero", "half_only"}


def _gc_frames():
    """four frames along the room stream and one from a clearly different view LAST: part of what the first four allocated lies outside the last pose's frustum"""
    frames = [synth.scene_room(12 * k, W, H) for k in range(4)] + [synth.scene_room(48 * 4, W, H)]
    K = frames[0][3]
    return frames, camera_params(W, H, K["fx"], K["fy"], K["mx"], K["my"])


def _allocated(osc):
    h = osc.hash()
    return {tuple(int(v) for v in e["pos"]): int(e["ptr"]) for e in h[h["ptr"] != FREE_ENTRY]}


def _plant(osc, d_vox):
    """Overwrites the weights of chosen blocks in the oracle and, byte for byte, on the device.  Returns ({case: key}, keys the collection has to delete)."""
    alloc = _allocated(osc)
    lst = osc.compactified()
    inside = sorted((int(e["ptr"]), tuple(int(v) for v in e["pos"])) for e in lst)
    outside = sorted((p, k) for k, p in alloc.items() if k not in {k2 for _, k2 in inside})
    assert len(inside) >= 100 and len(outside) >= 20, "the scenario needs blocks inside and outside the last pose's frustum (%d, %d)" % (len(inside), len(outside))
    vox = osc.voxels()
    chosen = {}
    seen = [(p, k) for p, k in inside if (vox["weight"][p:p + VOX_PER_BLOCK] >= 1.0).any()]      # blocks the collection would keep as they are
    assert len(seen) >= len(PLANTS)
    step = len(seen) // len(PLANTS)
    todo = [(name, seen[i * step], PLANTS[name]) for i, name in enumerate(PLANTS)]
    todo.append(("outside_all_zero", outside[len(outside) // 2], {}))
    for name, (ptr, key), weights in todo:
        blk = vox[ptr:ptr + VOX_PER_BLOCK]
        blk["weight"] = 0.0
        for v, w in weights.items():
            blk["weight"][v] = w
        _h2d(d_vox + ptr * 12, blk)
        chosen[name] = key
    expect = {k for p, k in inside if (vox["weight"][p:p + VOX_PER_BLOCK].astype(np.int64) == 0).all()}      # (weights are >= 0 and small: the cast truncates like (uint))
    return chosen, expect


@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("batched", [True, False])
def test_planted_garbage_collection_cases_vs_oracle(gpu, oracle, batched, overlap):
    """behind a batch the collection filters the batch's union list by the last operator's mask; behind single operators it walks the last operator's own list"""
    import torch
    frames, cam = _gc_frames()
    p = default_hash_params(num_buckets=50000, num_sdf_blocks=40000, voxel_size=0.02)
    gs = gpu.capi.SceneRepHashSDF(p)
    gs.set_arith("exact")
    if overlap:
        gs.set_overlap(True)
    d_vox = gs.hash_data().d_SDFBlocks           # (asked for before the first operator: the accessor would rebuild the list a batch leaves behind)
    osc = oracle.OracleScene(p)
    dev = [_to_dev(f[0], f[1]) for f in frames]
    if batched:
        gs.run_batch([("in", f[2], None, d[0], d[1]) for f, d in zip(frames, dev)], cam)
    else:
        for f, d in zip(frames, dev):
            gs.integrate(f[2], d[0], d[1], cam)
    for f in frames:
        osc.integrate(f[2], f[0], f[1], cam)
    assert osc.num_dropped() == 0
    torch.cuda.synchronize()
    before = _allocated(osc)
    chosen, expect = _plant(osc, d_vox)
    # the oracle alone first: every case is there, and it deletes exactly the expected blocks
    assert len(set(chosen.values())) == len(PLANTS) + 1
    assert {chosen[n] for n in DELETED} <= expect and not ({chosen[n] for n in chosen if n not in DELETED} & expect)
    assert len(expect) > len(DELETED), "the collection was supposed to delete blocks of its own too"
    osc.garbage_collect()
    assert set(before) - set(_allocated(osc)) == expect
    gs.garbage_collect()
    assert_same_state(gs, osc, "planted GC (%s, overlap %s):" % ("batch" if batched else "single operators", overlap))


def _noise_frames(w, h, n, seed):
    """per-pixel random depth in 0.5 .. 2.9 m: every 8x8 tile meets far more distinct blocks than a wave's or a workgroup's key set holds"""
    rng = np.random.default_rng(seed)
    _, _, _, K = synth.scene_room(0, w, h)
    out = []
    for k in range(n):
        _, color, T, _ = synth.scene_room(6 * k, w, h)
        depth = rng.uniform(0.5, 2.9, size=(h, w)).astype(np.float32)
        out.append((depth, color, T, K))
    return out, camera_params(w, h, K["fx"], K["fy"], K["mx"], K["my"])


@pytest.mark.parametrize("w,h", [(72, 40), (160, 120)])
def test_march_shapes_with_overflowing_key_sets_vs_oracle(gpu, oracle, w, h):
    """run_batch([in, in, re, in]) on images that are no multiple of 16 or 32 pixels, every tile through the flush path of the march's key sets"""
    frames, cam = _noise_frames(w, h, 3, 7)
    p = default_hash_params(num_buckets=50000, num_sdf_blocks=40000, voxel_size=0.02)
    gs = gpu.capi.SceneRepHashSDF(p)
    gs.set_arith("exact"); gs.set_overlap(True)
    osc = oracle.OracleScene(p)
    dev = [_to_dev(f[0], f[1]) for f in frames]
    T2 = frames[0][2].copy(); T2[:3, 3] += np.float32(0.05)
    ops = [("in", 0, frames[0][2], None), ("in", 1, frames[1][2], None), ("re", 0, frames[0][2], T2), ("in", 2, frames[2][2], None)]
    gs.run_batch([(kind, T0, T1, dev[i][0], dev[i][1]) for kind, i, T0, T1 in ops], cam)
    for kind, i, T0, T1 in ops:
        if kind == "re":
            osc.deintegrate(T0, frames[i][0], frames[i][1], cam)
        osc.integrate(T1 if kind == "re" else T0, frames[i][0], frames[i][1], cam)
    assert osc.num_dropped() == 0 and osc.num_allocated() > 1000, "the scenario is not the one the test describes"
    assert_same_state(gs, osc, "noise batch %dx%d:" % (w, h))
    gs.garbage_collect(); osc.garbage_collect()
    assert_same_state(gs, osc, "noise batch %dx%d + GC:" % (w, h))
    assert gs.debug_hash()["dropped"] == 0


def test_twenty_batches_with_collections_and_no_host_synchronisation(gpu, oracle):
    """batch, collection, batch, collection ... queued back to back with overlap on: the next batch's placement follows the collection on the device alone"""
    frames = [synth.scene_room(9 * k, W, H) for k in range(8)]
    K = frames[0][3]
    cam = camera_params(W, H, K["fx"], K["fy"], K["mx"], K["my"])
    p = default_hash_params(num_buckets=50000, num_sdf_blocks=40000, voxel_size=0.02)
    gs = gpu.capi.SceneRepHashSDF(p)
    gs.set_arith("exact"); gs.set_overlap(True)
    osc = oracle.OracleScene(p)
    dev = [_to_dev(f[0], f[1]) for f in frames]
    rng = np.random.default_rng(3)
    poses = {}
    script = []
    for r in range(20):
        ops = []
        i = r % len(frames)
        if i in poses:                     # the frame comes round again: out (its blocks empty: the collection behind this batch frees them), back in later
            ops.append(("de", i, poses.pop(i), None))
        else:
            poses[i] = frames[i][2].copy(); ops.append(("in", i, poses[i], None))
        for j in [int(v) for v in rng.permutation(sorted(poses))[:2] if int(v) != i]:
            T2 = poses[j].copy(); T2[:3, 3] += (rng.normal(size=3) * 0.05).astype(np.float32)
            ops.append(("re", j, poses[j], T2)); poses[j] = T2
        script.append(ops)
    for ops in script:                     # the device side first, nothing in between that waits for it
        gs.run_batch([(kind, T0, T1, dev[i][0], dev[i][1]) for kind, i, T0, T1 in ops], cam)
        gs.garbage_collect()
    deleted = 0
    for ops in script:
        for kind, i, T0, T1 in ops:
            if kind != "in":
                osc.deintegrate(T0, frames[i][0], frames[i][1], cam)
            if kind != "de":
                osc.integrate(T1 if kind == "re" else T0, frames[i][0], frames[i][1], cam)
        n = osc.num_allocated(); osc.garbage_collect(); deleted += n - osc.num_allocated()
    assert deleted > 0 and osc.num_dropped() == 0, "the scenario is not the one the test describes"
    assert_same_state(gs, osc, "20 batches + collections:")
