"""CPU tests (-m "not gpu") of the depth registration's host side and of its yardstick, tests/calibrator_ref.py (the definition of DESIGN.md
"Depth registration" in numpy): the ABI and the two parameters, synth.scene_room_at, and the restatement itself - an exact no-op under the identity
calibration, and within the quad stage's own admission bound of a ground truth rendered from the colour camera."""
import ctypes as C
import importlib.util
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from bundlefusion_amd import synth
from tests import calibrator_cases as cc
from tests import calibrator_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- 1. ABI and parameters
def test_library_exports_the_calibrator_abi(built):
    lib = C.CDLL(os.path.join(ROOT, "bundlefusion_amd", "lib", "libbf_hip.so"))
    names = ["bf_image_calibrator_create", "bf_image_calibrator_destroy", "bf_image_calibrator_set_stream", "bf_image_calibrator_process",
             "bf_image_manager_set_camera_calibration", "bf_image_manager_get_camera_calibration"]
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    for header, mine in (("bf_hip.h", names[:4]), ("bf_pipeline.h", names[4:])):
        txt = open(os.path.join(ROOT, "include", header)).read()
        assert all("BF_API int %s(" % n in txt for n in mine), header


def test_remapping_thresholds_are_parameters(built, tmp_path):
    from bundlefusion_amd.capi import GlobalAppState, default_app_state, lib
    g = default_app_state()
    assert g.s_remappingDepthDiscontinuityThresOffset == np.float32(0.012) and g.s_remappingDepthDiscontinuityThresLin == np.float32(0.01)      # zParametersDefault.txt:92-93
    assert g.s_bUseCameraCalibration == 0
    # appended: the layout in front of them is the one before
    assert GlobalAppState.s_remappingDepthDiscontinuityThresOffset.offset == GlobalAppState.s_SDFUseGradients.offset + 4
    assert C.sizeof(GlobalAppState) == GlobalAppState.s_remappingDepthDiscontinuityThresLin.offset + 4
    f = tmp_path / "app.txt"
    f.write_text(textwrap.dedent('''
        s_bUseCameraCalibration = true;
        s_remappingDepthDiscontinuityThresOffset = 0.02f; // discontinuity offset in meter
        s_remappingDepthDiscontinuityThresLin	 = 0.005f;
    '''))
    r = GlobalAppState(); missing = C.c_uint32()
    assert lib.bf_global_app_state_read(str(f).encode(), C.byref(r), C.byref(missing)) == 0
    assert r.s_bUseCameraCalibration == 1
    assert r.s_remappingDepthDiscontinuityThresOffset == np.float32(0.02) and r.s_remappingDepthDiscontinuityThresLin == np.float32(0.005)
    assert missing.value > 0                                  # the file sets three of the fields only
    r.s_bUseCameraCalibration = 0
    r.s_remappingDepthDiscontinuityThresOffset, r.s_remappingDepthDiscontinuityThresLin = 0.012, 0.01
    assert bytes(r) == bytes(g)                               # everything else is the default


def test_sensor_desc_carries_the_rig(built):
    from bundlefusion_amd.capi import sensor_desc
    Kd, Kc, E = cc.mat(synth.intrinsics(160, 120)), cc.mat(cc.colour_intrinsics(160, 120)), cc.extrinsics()
    s = sensor_desc(160, 120, Kd, color_K=Kc, depth_extrinsics=E)
    assert np.array_equal(np.array(s.depthIntrinsics[:], np.float32), Kd.reshape(16)) and np.array_equal(np.array(s.colorIntrinsics[:], np.float32), Kc.reshape(16))
    assert np.array_equal(np.array(s.depthExtrinsics[:], np.float32), E.reshape(16)) and np.array_equal(np.array(s.colorExtrinsics[:], np.float32), np.eye(4, dtype=np.float32).reshape(16))
    t = sensor_desc(160, 120, Kd)                             # as before: coinciding cameras
    assert bytes(t.depthIntrinsics) == bytes(t.colorIntrinsics) and bytes(t.depthExtrinsics) == bytes(t.colorExtrinsics)


def test_class_layer_calibrator_compiles_and_links(built, tmp_path):
    """CUDAImageCalibrator of include/bundlefusion/bundlefusion.hpp with plain g++; without a created device process() fails loudly and touches no GPU"""
    src = tmp_path / "cal.cpp"
    src.write_text(textwrap.dedent('''
        #include "bundlefusion/bundlefusion.hpp"
        using namespace bundlefusion;
        int main() {
            GlobalAppState& g = GlobalAppState::get();
            if (g.s_bUseCameraCalibration || g.s_remappingDepthDiscontinuityThresOffset != 0.012f || g.s_remappingDepthDiscontinuityThresLin != 0.01f) return 2;
            CUDAImageCalibrator c;
            mat4f I = mat4f::identity();
            try { c.process(nullptr, I, I, I); return 3; } catch (const std::runtime_error& e) { std::printf("%s\\n", e.what()); }
            void (CUDAImageCalibrator::*create)(unsigned int, unsigned int) = &CUDAImageCalibrator::OnD3D11CreateDevice; (void)create;
            bool (CUDAImageManager::*uses)() const = &CUDAImageManager::usesCameraCalibration; (void)uses;
            c.OnD3D11DestroyDevice();
            return 0;
        }
    '''))
    libdir = os.path.join(ROOT, "bundlefusion_amd", "lib")
    exe = tmp_path / "cal"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-L", libdir, "-lbf_hip", "-Wl,-rpath," + libdir, "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "before OnD3D11CreateDevice" in out.stdout, (out.returncode, out.stdout, out.stderr)


def test_make_sens_writes_the_rig_into_the_header(built, tmp_path):
    from bundlefusion_amd import sensordata as sdm
    spec = importlib.util.spec_from_file_location("make_sens", os.path.join(ROOT, "tools", "make_sens.py"))
    ms = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ms)
    E = ms.depth_offset_matrix(0.025, 0.005, -0.01, 0.5, 1.0, 0.8)
    assert np.allclose(E[:3, :3] @ E[:3, :3].T, np.eye(3), atol=1e-6) and np.array_equal(E[:3, 3], np.array([0.025, 0.005, -0.01], np.float32)) and E[0, 1] < 0 < E[1, 0]
    out = tmp_path / "rig.sens"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_sens.py"), str(out), "--frames", "2", "--width", "64", "--height", "48",
                        "--depth-offset", "0.025", "0.005", "-0.01", "0.5", "1.0", "0.8", "--colour-focal-scale", "1.08"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    sd = sdm.SensorData(out, use_pillow=False)
    d = sd.sensor_desc()
    Kd = synth.intrinsics(64, 48)
    assert np.array_equal(np.array(d.depthExtrinsics[:], np.float32).reshape(4, 4), E)
    assert d.depthIntrinsics[0] == np.float32(Kd["fx"]) and d.colorIntrinsics[0] == np.float32(Kd["fx"] * 1.08) and d.colorIntrinsics[5] == np.float32(Kd["fy"] * 1.08)
    # depth is the displaced camera's, colour and pose the colour camera's
    T = synth.trajectory_pose(1)
    want = synth.scene_room_at(T.astype(np.float64) @ E.astype(np.float64), Kd, 64, 48)[0]
    assert np.array_equal(sdm.depth_to_u16(want, 1000.0), sdm.depth_to_u16(sd.depth(1), 1000.0))
    Kc = dict(Kd, fx=Kd["fx"] * 1.08, fy=Kd["fy"] * 1.08)
    assert np.array_equal(sd.color_rgbx(1)[..., :3].reshape(48, 64, 3), synth.scene_room_at(T, Kc, 64, 48)[1][..., :3])
    sd.close()


# ---------------------------------------------------------------------------------------------- 2. scene_room_at
@pytest.mark.parametrize("k", [0, 7, 333])
def test_scene_room_at_is_scene_room(k):
    a = synth.scene_room(k, 160, 120)
    b = synth.scene_room_at(synth.trajectory_pose(k), synth.intrinsics(160, 120), 160, 120)
    for x, y in zip(a[:3], b[:3]):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert a[3] == b[3]
    if k == 0:                                                # the defaults are the 640x480 camera
        c = synth.scene_room_at(synth.trajectory_pose(k), synth.intrinsics())
        d = synth.scene_room(k)
        assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(c[:3], d[:3])) and c[3] == d[3]


# ---------------------------------------------------------------------------------------------- 3. the restatement under the identity calibration
@pytest.mark.parametrize("noise", [False, True])
def test_restatement_identity_is_a_no_op_where_the_quad_survives(noise):
    w, h = 160, 120
    depth = synth.scene_room(200, w, h)[0]                    # a frame with clutter close to the camera: many dropped quads
    if noise:
        depth = synth.add_depth_noise(depth)
    K = synth.intrinsics(w, h)
    out = ref.register(depth, cc.mat(K), cc.mat_inv(K), np.eye(4, dtype=np.float32), cc.THRESH_OFFSET, cc.THRESH_LIN)
    q = ref.quad_survives(depth, cc.THRESH_OFFSET, cc.THRESH_LIN)
    assert 0.5 < q.mean() < 1.0 and not q[:, -1].any() and not q[-1, :].any()          # both outcomes occur; the last column / row has corners outside the image
    assert np.array_equal(out[q].view(np.uint32), depth[q].view(np.uint32))
    assert np.all(out[~q] == -np.inf)


def test_restatement_quad_stage_edge_values():
    d = np.full((4, 4), 1.0, np.float32)
    assert ref.quad_survives(d, 0.012, 0.01)[:3, :3].all()
    for bad in (0.1, 0.0, -1.0, -np.inf, np.inf, np.nan):     # <= 0.1, -inf, not finite: all four quads that touch the pixel go
        e = d.copy(); e[1, 1] = bad
        q = ref.quad_survives(e, 0.012, 0.01)
        assert not q[:2, :2].any() and q[2, 2] and q[0, 2] and q[2, 0]
    e = d.copy(); e[1, 1] = np.float32(1.0) + np.float32(0.03)        # spread 0.03 > 0.012 + 0.01 * 1.015
    assert not ref.quad_survives(e, 0.012, 0.01)[:2, :2].any()
    e[1, 1] = np.float32(1.0) + np.float32(0.02)                      # 0.02 < 0.012 + 0.01 * 1.01
    assert ref.quad_survives(e, 0.012, 0.01)[:3, :3].all()


# ---------------------------------------------------------------------------------------------- 4. the restatement against ground truth
def _dilate(m, r):
    h, w = m.shape
    p = np.zeros((h + 2 * r, w + 2 * r), bool)
    p[r:r + h, r:r + w] = m
    out = np.zeros_like(m)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out |= p[dy:dy + h, dx:dx + w]
    return out


@pytest.mark.parametrize("k", [100, 200])
def test_restatement_against_ground_truth(k):
    """Depth rendered from the displaced depth camera (T E, depth intrinsics), registered by the restatement, against the scene rendered from the colour
    camera (T, colour intrinsics).  Every registered pixel farther than 2 px (Chebyshev) from a ground-truth jump lies within threshOffset + threshLin * gt
    of the ground truth: that bound is the one under which the quad stage admits a quad, so an admitted quad cannot span more.  A jump: two 4-neighbours of
    the ground truth that differ by more than threshOffset + threshLin * their mean, or of which exactly one is invalid (an infinite difference: the image
    border and the 4 m range limit end the mesh the way a silhouette does).  k = 100 is a frame of walls, k = 200 has a clutter box 0.48 m in front of the
    camera (16 px of parallax); in both the 2 px rule excludes less than 10 % of the compared pixels.
    Measured here (320x240; python -m pytest tests/test_calibrator_cpu.py -k ground_truth -s; profiles/calibrator_registration.md):
        k = 100: median |error| 0.000001 m, 97.28 % of the ground-truth-valid pixels registered, 4.78 % excluded
        k = 200: median |error| 0.000004 m, 96.21 % registered, 5.49 % excluded"""
    w, h = 320, 240
    depth, _, gt, _ = cc.rig_frame(k, w, h)
    Kc, KdInv, E = cc.rig_matrices(w, h)
    reg = ref.register(depth, Kc, KdInv, E, cc.THRESH_OFFSET, cc.THRESH_LIN)
    gv = np.isfinite(gt)
    g = np.where(gv, gt, 0).astype(np.float64)
    jump = np.zeros_like(gv)
    for a, b in ((np.s_[:, :-1], np.s_[:, 1:]), (np.s_[:-1, :], np.s_[1:, :])):
        big = (gv[a] != gv[b]) | (gv[a] & gv[b] & (np.abs(g[a] - g[b]) > cc.THRESH_OFFSET + cc.THRESH_LIN * 0.5 * (g[a] + g[b])))
        jump[a] |= big
        jump[b] |= big
    near = _dilate(jump, 2)
    both = np.isfinite(reg) & gv
    err = np.abs(np.where(both, reg, 0).astype(np.float64) - g)
    median, covered, excluded = float(np.median(err[both])), both.sum() / gv.sum(), (both & near).sum() / both.sum()
    print("\nregistration vs ground truth, %dx%d k=%d: median |error| %.6f m, registered %.2f %% of the ground-truth-valid pixels, excluded by the 2 px rule %.2f %%"
          % (w, h, k, median, 100 * covered, 100 * excluded))
    assert np.all(reg[np.isfinite(reg)] > 0.1)
    assert excluded <= 0.10
    check = both & ~near
    assert check.sum() > 0.5 * w * h
    bad = check & (err > cc.THRESH_OFFSET + cc.THRESH_LIN * g)
    assert not bad.any(), "%d pixels off by up to %.4f m" % (bad.sum(), err[bad].max())
