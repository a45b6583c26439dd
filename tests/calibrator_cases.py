"""Inputs shared by tests/test_calibrator_cpu.py and tests/test_calibrator_gpu.py: a sensor rig whose depth camera is displaced from its colour camera,
and scene S2 (bundlefusion_amd.synth) seen through either.

The rig: E (depth camera -> colour camera) = 25 / 5 / -10 mm and 1.5 degrees about the oblique axis (1, 2, 0.5); colour camera = the synthetic
pinhole with the focal lengths x `focal_scale` (1.08) and the principal point moved by (+3.5, -2.25) px at 640x480 (scaled with the width).
With colour camera-to-world T, the depth camera's is T E.
"""
import functools

import numpy as np

from bundlefusion_amd import synth

THRESH_OFFSET, THRESH_LIN = 0.012, 0.01          # zParametersDefault.txt:92-93


def extrinsics(t_mm=(25.0, 5.0, -10.0), angle_deg=1.5, axis=(1.0, 2.0, 0.5)):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    th = np.deg2rad(angle_deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)          # Rodrigues
    E = np.eye(4)
    E[:3, :3] = R
    E[:3, 3] = np.asarray(t_mm, np.float64) / 1000.0
    return E.astype(np.float32)


def colour_intrinsics(width, height, focal_scale=1.08):
    K = synth.intrinsics(width, height)
    s = width / 640.0
    return dict(fx=K["fx"] * focal_scale, fy=K["fy"] * focal_scale, mx=K["mx"] + 3.5 * s, my=K["my"] - 2.25 * s)


def mat(K):
    m = np.eye(4, dtype=np.float32)
    m[0, 0], m[1, 1], m[0, 2], m[1, 2] = K["fx"], K["fy"], K["mx"], K["my"]
    return m


def mat_inv(K):
    """the pinhole's inverse, rounded once to binary32 (tests of the standalone operator; the frame loop's own inverse comes from the image manager)"""
    m = np.eye(4, dtype=np.float64)
    m[0, 0], m[1, 1], m[0, 2], m[1, 2] = 1.0 / K["fx"], 1.0 / K["fy"], -K["mx"] / K["fx"], -K["my"] / K["fy"]
    return m.astype(np.float32)


@functools.lru_cache(maxsize=None)
def rig_frame(k, width, height, focal_scale=1.08):
    """(depth from the displaced depth camera, colour from the colour camera, ground-truth depth in the colour camera, T) of S2 frame k; read-only arrays"""
    E = extrinsics()
    T = synth.trajectory_pose(k).astype(np.float64)
    Kd, Kc = synth.intrinsics(width, height), colour_intrinsics(width, height, focal_scale)
    depth = synth.scene_room_at(T @ E.astype(np.float64), Kd, width, height)[0]
    gt, colour, T32, _ = synth.scene_room_at(T, Kc, width, height)
    for a in (depth, colour, gt, T32):
        a.setflags(write=False)
    return depth, colour, gt, T32


def rig_matrices(width, height, focal_scale=1.08):
    """(colour intrinsics, inverse depth intrinsics, extrinsics) as the operator takes them"""
    return mat(colour_intrinsics(width, height, focal_scale)), mat_inv(synth.intrinsics(width, height)), extrinsics()
