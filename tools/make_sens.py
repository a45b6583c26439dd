"""Write the synthetic S2 stream as a .sens file (the "config 2 stand-in" of SURVEY.md 8d: depth as u16 with depthShift 1000,
colour RGB8 raw or JPEG, ground-truth camera-to-world per frame).  Host only.

usage: python tools/make_sens.py out.sens [--frames 200] [--width 640 --height 480] [--jpeg 90] [--bob 0.0]
                                [--depth-offset tx ty tz rx ry rz] [--colour-focal-scale s]
--depth-offset: a rig whose depth camera is displaced from its colour camera - translation in metres, rotation in degrees about x, y, z (R = Rz Ry Rx).
The stored poses and the colour images are the colour camera's, depth is rendered from the displaced camera, and the header carries the offset as the
depth extrinsics (depth camera -> colour camera).  --colour-focal-scale: the colour camera's focal lengths relative to the depth camera's; the header carries
both intrinsics.  Such a file is what s_bUseCameraCalibration (tools/run_sens.py --camera-calibration) is for.
"""
import argparse
import io
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from bundlefusion_amd import synth
from bundlefusion_amd import sensordata as sdm
from bundlefusion_amd.capi import intrinsics_matrix


def depth_offset_matrix(tx, ty, tz, rx, ry, rz):
    ax, ay, az = np.deg2rad([rx, ry, rz])
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    E = np.eye(4)
    E[:3, :3] = Rz @ Ry @ Rx
    E[:3, 3] = [tx, ty, tz]
    return E.astype(np.float32)


def _rig_frame(job):
    """(depth from the displaced camera, colour from the colour camera, colour camera-to-world) of frame k: one job of the render pool"""
    k, W, H, bob, E, Kc = job
    T = synth.trajectory_pose(k, bob=bob)
    depth = synth.scene_room_at(T.astype(np.float64) @ E.astype(np.float64), synth.intrinsics(W, H), W, H)[0]
    color = synth.scene_room_at(T, Kc, W, H)[1]
    return depth, color, T, synth.intrinsics(W, H)


def render_rig_frames(indices, W, H, bob, E, Kc):
    import multiprocessing as mp
    jobs = [(k, W, H, bob, E, Kc) for k in indices]
    with mp.get_context("spawn").Pool(max(1, min(16, os.cpu_count() or 1, len(jobs)))) as pool:
        return pool.map(_rig_frame, jobs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--first", type=int, default=0)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--bob", type=float, default=0.0)
    ap.add_argument("--jpeg", type=int, default=0, help="JPEG quality for the colour frames (0: raw RGB8)")
    ap.add_argument("--raw-depth", action="store_true", help="store depth uncompressed instead of zlib")
    ap.add_argument("--depth-offset", type=float, nargs=6, default=None, metavar=("TX", "TY", "TZ", "RX", "RY", "RZ"),
                    help="depth camera -> colour camera: translation in metres, rotation in degrees about x, y, z")
    ap.add_argument("--colour-focal-scale", type=float, default=1.0, help="focal lengths of the colour camera relative to the depth camera's")
    a = ap.parse_args()
    W, H = a.width, a.height
    rig = a.depth_offset is not None or a.colour_focal_scale != 1.0
    E = depth_offset_matrix(*a.depth_offset) if a.depth_offset is not None else np.eye(4, dtype=np.float32)
    Kc = dict(synth.intrinsics(W, H))
    Kc["fx"] *= a.colour_focal_scale; Kc["fy"] *= a.colour_focal_scale
    writer = None
    for c0 in range(0, a.frames, 256):
        idx = [a.first + k for k in range(c0, min(a.frames, c0 + 256))]
        for depth, color, T, Kd in (render_rig_frames(idx, W, H, a.bob, E, Kc) if rig else synth.render_frames(idx, W, H, bob=a.bob)):
            if writer is None:
                K = intrinsics_matrix(Kd["fx"], Kd["fy"], Kd["mx"], Kd["my"])
                writer = sdm.SensorDataWriter(a.out, (W, H), (W, H), K, color_intrinsic=intrinsics_matrix(Kc["fx"], Kc["fy"], Kc["mx"], Kc["my"]) if rig else None,
                                              depth_extrinsic=E if rig else None, depth_shift=1000.0, sensor_name="synthetic S2 room",
                                              depth_compression=sdm.DEPTH_RAW_USHORT if a.raw_depth else sdm.DEPTH_ZLIB_USHORT,
                                              color_compression=sdm.COLOR_JPEG if a.jpeg else sdm.COLOR_RAW)
            rgb = np.ascontiguousarray(color.reshape(H, W, 4)[..., :3])
            if a.jpeg:
                from PIL import Image
                buf = io.BytesIO()
                Image.fromarray(rgb).save(buf, format="JPEG", quality=a.jpeg)
                cbytes = buf.getvalue()
            else:
                cbytes = rgb.tobytes()
            writer.add_frame(T, sdm.depth_to_u16(depth.reshape(H, W), 1000.0), cbytes)
    writer.close()
    print("wrote %s: %d frames %dx%d, %.1f MB" % (a.out, a.frames, W, H, os.path.getsize(a.out) / 1e6))


if __name__ == "__main__":
    main()
