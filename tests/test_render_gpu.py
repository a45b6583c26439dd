"""GPU tests (-m gpu) of the frame renderer (csrc/render.hip, include/bf_render.h) against its numpy restatement tests/render_ref.py: the float target as
bits, the RGBA8 picture as bytes, tolerance 0 - on planted G-buffers, behind the ray caster, and as a command of the frame loop's volume queue, where a
render must leave the reconstruction exactly as it would have been without it."""
import ctypes as C

import numpy as np
import pytest

from bundlefusion_amd import synth
from bundlefusion_amd.capi import (camera_params, default_app_state, default_bundling_state, default_hash_params, default_render_state, intrinsics_matrix,
                                   ray_cast_intrinsics_inv, ray_cast_params_from_global_app_state, sensor_desc)
from tests import render_ref as rr
from tests.test_render_cpu import RUNS, planted_depth_hsv

pytestmark = pytest.mark.gpu


def _state(overrides):
    st = default_render_state()
    for k, v in (overrides or {}).items():
        if hasattr(v, "__len__"):
            getattr(st, k)[:] = [float(x) for x in v]
        else:
            setattr(st, k, float(v))
    return st


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _shade_and_compare(gpu, fr, depth, colors, Kinv, overrides, mat, lost, off=0.012, lin=0.001):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(depth)).cuda(); c = torch.from_numpy(np.ascontiguousarray(colors)).cuda()
    fr.shade(d, c, Kinv, _state(overrides), mat, lost, off, lin)
    rgba = fr.download_rgba8(); target = fr.download_target()
    et, er, info = rr.shade(depth, colors, Kinv, overrides, mat, lost, off, lin)
    assert np.array_equal(_bits(target), _bits(et)), (depth.shape, mat, lost, int((_bits(target) != _bits(et)).sum()))
    assert np.array_equal(rgba, er)
    return info


@pytest.mark.parametrize("size", [(67, 9), (1, 1), (2, 2), (64, 4), (65, 5), (128, 8)])
def test_shade_planted_gbuffers_bit_exact(gpu, size):
    """1. Planted G-buffers (tests/render_ref.py::planted_gbuffer; 67 x 9 crosses the 64-wide tile edge and leaves a partial tile both ways): both shader
    branches, the overlay, the default lights, a brighter light and a light along a normal."""
    w, h = size
    Kinv = rr.planted_kinv()
    depth, colors = rr.planted_gbuffer(w, h)
    fr = gpu.capi.FrameRenderer(w, h)
    for overrides, mat, lost in RUNS:
        info = _shade_and_compare(gpu, fr, depth, colors, Kinv, overrides, mat, lost)
    if size == (67, 9):
        assert info["drawn"].mean() >= 0.5
        # renderTopDown's thresholds are arguments of their own
        _shade_and_compare(gpu, fr, depth, colors, Kinv, None, False, False, 0.02, 0.01)


def test_input_modes_bit_exact(gpu):
    """2. Mode 4 on planted depths (tests/test_render_cpu.py::planted_depth_hsv) and mode 3 on random RGBX bytes, 67 x 9."""
    import torch
    w, h = 67, 9
    d, dmin, dmax = planted_depth_hsv(w, h)
    fr = gpu.capi.FrameRenderer(w, h)
    fr.depth_hsv(torch.from_numpy(d).cuda(), dmin, dmax)
    rgba = fr.download_rgba8(); target = fr.download_target()
    et, er, info = rr.depth_hsv(d, dmin, dmax)
    assert np.array_equal(_bits(target), _bits(et)) and np.array_equal(rgba, er)
    assert info["gate"].any() and (~info["gate"]).any() and (er[info["gate"]][:, 3] == 255).all() and (er[~info["gate"]] == 0).all()
    # a degenerate range: min == max divides 0 by 0 where the gate passes
    d2 = d.copy(); d2.reshape(-1)[:4] = 1.5
    fr.depth_hsv(torch.from_numpy(d2).cuda(), 1.5, 1.5)
    rgba = fr.download_rgba8(); target = fr.download_target()
    et, er, _ = rr.depth_hsv(d2, 1.5, 1.5)
    assert np.array_equal(_bits(target), _bits(et)) and np.array_equal(rgba, er)
    img = np.random.default_rng(2).integers(0, 256, (h, w, 4), dtype=np.uint8)
    fr.rgbx(torch.from_numpy(img).cuda())
    assert np.array_equal(fr.download_rgba8(), rr.rgbx(img))


def _gas_small():
    gas = default_app_state()
    gas.s_integrationWidth, gas.s_integrationHeight, gas.s_rayCastWidth, gas.s_rayCastHeight = 160, 120, 160, 120
    gas.s_hashNumSDFBlocks = 20000
    return gas


def test_shade_behind_the_ray_caster(gpu):
    """3. The scene of test_ray_cast_bit_exact_small_volume (160 x 120, 2 cm, three frames): ray cast, shade, compare with the restatement applied to the
    downloaded depth / colours; a second render on the same renderer at another pose does not depend on the first."""
    import torch
    W, H = 160, 120
    frames = [synth.scene_room(k, W, H) for k in (0, 20, 40)]
    K = frames[0][3]
    cam = camera_params(W, H, K["fx"], K["fy"], K["mx"], K["my"])
    gs = gpu.capi.SceneRepHashSDF(default_hash_params(num_buckets=20011, num_sdf_blocks=20000, voxel_size=0.02))
    for d, c, T, _ in frames:
        gs.integrate(T, torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda(), cam)
    rp = ray_cast_params_from_global_app_state(_gas_small(), intrinsics_matrix(K["fx"], K["fy"], K["mx"], K["my"]))
    rc = gpu.capi.RayCastSDF(rp)
    Kinv = ray_cast_intrinsics_inv(rc.params())
    assert Kinv[0, 0] == np.float32(1.0) / np.float32(K["fx"]) and Kinv[1, 2] == -np.float32(K["my"]) / np.float32(K["fy"])
    fr = gpu.capi.FrameRenderer(W, H)
    T1 = frames[1][2].astype(np.float32)
    T2 = (frames[0][2].astype(np.float64) @ np.array([[1, 0, 0, 0.05], [0, 1, 0, -0.03], [0, 0, 1, 0.1], [0, 0, 0, 1.0]])).astype(np.float32)

    def render(renderer, T, mat, lost):
        gs.compactify(T, cam)
        rc.render(gs, cam, T)
        g = rc.download()
        d = gpu.capi.RayCastData(); gpu.capi.check(gpu.capi.lib.bf_ray_cast_get_data(rc._h, C.byref(d)))
        renderer.shade(d.d_depth, d.d_colors, Kinv, None, mat, lost)
        rgba = renderer.download_rgba8(); target = renderer.download_target()
        et, er, info = rr.shade(g["depth"], g["colors"], Kinv, None, mat, lost)
        assert np.array_equal(_bits(target), _bits(et)) and np.array_equal(rgba, er)
        return rgba, target, info

    first = {}
    for mat, lost in ((False, False), (True, False), (False, True)):
        rgba, target, info = render(fr, T1, mat, lost)
        first[(mat, lost)] = rgba
        assert info["drawn"].mean() > 0.5
    assert not np.array_equal(first[(False, False)], first[(True, False)])
    # another pose on the same renderer, and on a fresh one: the same picture, no stale pixels
    a, ta, ia = render(fr, T2, False, False)
    b, tb, _ = render(gpu.capi.FrameRenderer(W, H), T2, False, False)
    assert np.array_equal(a, b) and np.array_equal(_bits(ta), _bits(tb)) and not np.array_equal(a, first[(False, False)])
    assert (ia["drawn"] != (first[(False, False)][..., 3] == 255)).any()              # pixels drawn before and not now (or the reverse) exist


# --------------------------------------------------------------------------- the frame loop
PW, PH = 640, 480
_frames = {}


def _stream(n):
    if n not in _frames:
        _frames[n] = synth.render_frames(range(n))
    return _frames[n]


def _run_pipeline(gpu, n, render, gc=True, timings=False):
    import torch
    frames = _stream(n)
    Kd = frames[0][3]
    K = intrinsics_matrix(Kd["fx"], Kd["fy"], Kd["mx"], Kd["my"])
    gas, gbs = default_app_state(), default_bundling_state()
    gas.s_integrationWidth, gas.s_integrationHeight = PW, PH
    gas.s_SDFVoxelSize, gas.s_hashNumBuckets, gas.s_hashNumSDFBlocks = 0.02, 50000, 20000
    gas.s_garbageCollectionEnabled = 1 if gc else 0
    gbs.s_maxNumImages = 8
    gp = gpu.capi.Pipeline(gas, gbs, sensor_desc(PW, PH, K))
    if timings:
        gp.enable_timings(True)
    st = default_render_state()
    st.s_topVideoCameraPose[:] = [20.0, 0.1, -0.05, -0.6]
    st.s_topVideoMinMax[:] = [0.3, 6.0]
    gp.set_render_state(st)
    pics = 0
    for k, (d, c, T, _) in enumerate(frames):
        assert gp.process_frame(torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda())
        if render:
            pic = gp.render(1)
            assert pic.shape == (gas.s_rayCastHeight, gas.s_rayCastWidth, 4)
            pics += int(pic.any())
            if k % 5 == 4:
                top = gp.render_top_down()
                assert top.shape == pic.shape
    gp.synchronize()
    if render:
        assert pics >= n - 4          # all but the first calls, whose frames have not reached the volume yet, show something
    return gp, gas, K, Kd


def _volume_state(gp):
    sc = gp.scene()
    return dict(traj=gp.integrated_trajectory().copy(), opt=gp.optimized_trajectory().copy(), dbg=sc.debug_hash(), heap_free=sc.heap_free_count(),
                blocks=sc.num_allocated_blocks(), counters=gp.counters())


def _final_picture_matches_stand_alone(gpu, gp, gas, K, Kd):
    """the pipeline's picture of the last frame == compactify + bf_ray_cast_render + bf_frame_renderer_shade of the final volume at that pose"""
    pic = gp.render(1)
    colored = gp.render(2)
    T = gp.integrated_trajectory()[-1].astype(np.float32)
    assert np.isfinite(T).all() and pic.any()
    cam = camera_params(PW, PH, Kd["fx"], Kd["fy"], Kd["mx"], Kd["my"], gas.s_renderDepthMin, gas.s_renderDepthMax)
    sc = gp.scene()
    rc = gpu.capi.RayCastSDF(ray_cast_params_from_global_app_state(gas, K))
    sc.compactify(T, cam)
    rc.render(sc, cam, T)
    g = rc.download()
    d = gpu.capi.RayCastData(); gpu.capi.check(gpu.capi.lib.bf_ray_cast_get_data(rc._h, C.byref(d)))
    Kinv = ray_cast_intrinsics_inv(rc.params())
    fr = gpu.capi.FrameRenderer(gas.s_rayCastWidth, gas.s_rayCastHeight)
    for mat, got in ((False, pic), (True, colored)):
        fr.shade(d.d_depth, d.d_colors, Kinv, None, mat, False)
        assert np.array_equal(fr.download_rgba8(), got)
        assert np.array_equal(got, rr.shade(g["depth"], g["colors"], Kinv, None, mat, False)[1])
    assert (pic[..., 3] == 255).mean() > 0.3
    # the input modes show the last frame handed to the volume
    dl, cl = gp.integrate_frame_cpu(len(gp.integrated_trajectory()) - 1)
    assert np.array_equal(gp.render(3), rr.rgbx(cl))
    assert np.array_equal(gp.render(4), rr.depth_hsv(dl, gas.s_sensorDepthMin, gas.s_sensorDepthMax)[1])


def test_pipeline_render_leaves_the_reconstruction_alone(gpu):
    """4. 25 frames (two chunk boundaries), the smallest configuration of tests/test_pipeline_gpu.py, the suite's schedule: one run renders mode 1 after every frame
    and the top-down picture every fifth, the other renders nothing.  Trajectories, bf_scene_debug_hash, heap free count and allocated-block count are identical;
    the last frame's picture is the stand-alone one."""
    n = 25
    plain, _, _, _ = _run_pipeline(gpu, n, render=False)
    a = _volume_state(plain)
    plain.close()
    gp, gas, K, Kd = _run_pipeline(gpu, n, render=True)
    b = _volume_state(gp)
    assert np.array_equal(a["traj"].view(np.uint32), b["traj"].view(np.uint32)) and np.array_equal(a["opt"].view(np.uint32), b["opt"].view(np.uint32))
    assert a["dbg"] == b["dbg"] and a["heap_free"] == b["heap_free"] and a["blocks"] == b["blocks"] and a["counters"] == b["counters"]
    assert b["counters"]["deintegrate"] > 0 and b["dbg"]["duplicate_keys"] == 0
    _final_picture_matches_stand_alone(gpu, gp, gas, K, Kd)


@pytest.mark.parametrize("gc,timings", [(False, False), (True, True), (False, True)])
def test_pipeline_render_without_collection_and_under_timings(gpu, gc, timings):
    """4, repeated with garbage collection off (the frame boundary is a flush command) and with timings on (commands are handled on the calling thread): the same
    volume as the run that renders nothing, and the final picture is the stand-alone one."""
    n = 25
    plain, _, _, _ = _run_pipeline(gpu, n, render=False, gc=gc, timings=timings)
    a = _volume_state(plain)
    plain.close()
    gp, gas, K, Kd = _run_pipeline(gpu, n, render=True, gc=gc, timings=timings)
    b = _volume_state(gp)
    assert np.array_equal(a["traj"].view(np.uint32), b["traj"].view(np.uint32))
    assert a["dbg"] == b["dbg"] and a["heap_free"] == b["heap_free"] and a["blocks"] == b["blocks"] and a["counters"] == b["counters"]
    _final_picture_matches_stand_alone(gpu, gp, gas, K, Kd)
