"""Play a recorded .sens file through the headless BundleFusion frame loop (s_sensorIdx = 8 in the reference) and evaluate the
optimised trajectory against the poses stored in the file (SensorDataReader::evaluateTrajectory).

usage: python tools/run_sens.py sequence.sens [--voxel 0.01] [--app zParametersDefault.txt] [--bundling zParametersBundlingDefault.txt]
                                [--ingest host|device] [--decode-threads N] [--camera-calibration] [--mesh scan.ply] [--mesh-host scan_host.ply]
--mesh: the scan's mesh after the end of the sequence, extracted and welded on the device (bf_pipeline_save_mesh); --mesh-host: the same file by the host route
(bf_marching_cubes_extract + bf_marching_cubes_save_mesh).  Both print the vertex, face and triangle counts and the seconds spent.
--mesh-min-faces N / --mesh-largest / --mesh-normals: clean the mesh before it is written - connected pieces below N faces and unused vertices dropped, only the
largest piece kept, per-vertex normals added to the PLY - on the device with --mesh (bf_pipeline_save_mesh_clean), on one core with --mesh-host
(bf_mesh_clean_host); both print the cleaning's stats.
--mesh-simplify-cell METRES: simplify the cleaned mesh before it is written, one vertex per grid cell of that size (bf_pipeline_save_mesh_simplified with --mesh,
bf_mesh_simplify_host with --mesh-host); both print the simplification's stats and its time.
--mesh-recolour [--mesh-recolour-stride N] [--mesh-recolour-best]: take the cleaned mesh's vertex colours from the stored frames on the stride (default
s_submapSize: the key frames) under the optimised trajectory, before the simplification if there is one (bf_pipeline_save_mesh_recoloured with --mesh,
bf_mesh_recolour_host with --mesh-host); both print the recolouring's stats and its time.
--mesh-texture (with --mesh): write the mesh with a texture atlas from the same frames, a PNG next to the PLY (bf_pipeline_save_mesh_textured; after the
recolouring and the simplification if those are asked for); prints the texture's stats and times and compares with bf_mesh_texture_host on one core.
--mesh-evaluate-against other.ply: measure the mesh (cleaned, simplified as the other options say) against a PLY on disk in both directions on the device
(bf_pipeline_measure_mesh) and print mean, RMS, median, 90th percentile, max, the share within one voxel and the share beyond --mesh-evaluate-max (default
0.1 m); --mesh-evaluate-spacing sets the surface sampling, --mesh-evaluate-surface samples the scan's surface too, --mesh-error-ply err.ply writes the mesh
coloured by its distance; --mesh-evaluate measures against synth.room_mesh(), which is the truth for a recording of the synthetic room only.
--point-cloud FILE [--point-cloud-stride N --point-cloud-cell M]: the stored frames on the stride (default s_submapSize: the key frames) under the optimised
trajectory as a coloured, oriented point cloud, one point per cell of M metres (default 0.005), thinned on the device (bf_pipeline_save_point_cloud);
--point-cloud-host FILE: the same file by the host route on one core.  Both print frame and point counts and the seconds spent.
--camera-calibration: s_bUseCameraCalibration = true - register every frame's depth to the colour camera with the extrinsics and intrinsics of the file's
header (a file whose depth extrinsics are the identity has nothing to register; the line below says whether it is active).
--ingest host (default): frames are decoded on the host and handed over as host buffers (the PCIe path of bf_pipeline_process_frame).
--ingest device: sensordata.SensPlayer - N threads (default 4, at most 12) read, inflate and entropy-decode ahead, the u16 depth and the RGB8 / JPEG
coefficients go up the bus and are converted / reconstructed on the device (bf_pipeline_process_frame_raw_decoded).  Same results, bit for bit.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import bundlefusion_amd as bf
from bundlefusion_amd import sensordata as sdm
from tools import mesh_out, point_cloud_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sens")
    ap.add_argument("--app", default=None, help="zParametersDefault.txt (defaults: the shipped values)")
    ap.add_argument("--bundling", default=None, help="zParametersBundlingDefault.txt")
    ap.add_argument("--voxel", type=float, default=None)
    ap.add_argument("--buckets", type=int, default=None)
    ap.add_argument("--blocks", type=int, default=None)
    ap.add_argument("--frames", type=int, default=0, help="play only the first N frames")
    ap.add_argument("--tail", type=int, default=5, help="end-of-sequence iterations")
    ap.add_argument("--ingest", choices=("host", "device"), default="host", help="where frames are converted to float depth / RGBX")
    ap.add_argument("--decode-threads", type=int, default=4, help="decode-ahead threads of --ingest device (1 .. 12)")
    ap.add_argument("--decoder", choices=("auto", "builtin"), default="auto", help="--ingest host: auto decodes JPEG / PNG with Pillow where it is installed, builtin with the library's decoder")
    ap.add_argument("--camera-calibration", action="store_true", help="s_bUseCameraCalibration = true (a parameter file given with --app may set it as well)")
    ap.add_argument("--save", default=None, help="write a copy of the file with the optimised trajectory (SensorDataReader::saveToFile)")
    ap.add_argument("--record", default=None, metavar="FILE", help="s_recordData: record every accepted frame and save FILE with the optimised trajectory (bf_pipeline_save_recording)")
    ap.add_argument("--record-threads", type=int, default=4, help="encode threads of --record (1 .. 12)")
    mesh_out.add_arguments(ap)
    point_cloud_out.add_arguments(ap)
    a = ap.parse_args()
    sd = sdm.SensorData(a.sens, use_pillow=a.ingest == "host" and a.decoder == "auto")        # (the player's workers decode with the library's own decoder)
    n = len(sd) if a.frames <= 0 else min(a.frames, len(sd))
    desc = sd.sensor_desc()
    gas = bf.capi.default_app_state(a.app)
    gbs = bf.capi.default_bundling_state(a.bundling)
    gas.s_sensorIdx = 8
    if a.app is None:                       # integrate at the sensor resolution unless a parameter file says otherwise
        gas.s_integrationWidth, gas.s_integrationHeight = desc.depthWidth, desc.depthHeight
    if a.voxel: gas.s_SDFVoxelSize = a.voxel
    if a.buckets: gas.s_hashNumBuckets = a.buckets
    if a.blocks: gas.s_hashNumSDFBlocks = a.blocks
    if a.camera_calibration: gas.s_bUseCameraCalibration = 1
    if n > gbs.s_maxNumImages * gbs.s_submapSize:          # SensorDataReader.cpp:65-67
        raise SystemExit("sens file #frames = %d, please change param file to accommodate" % n)
    p = bf.capi.Pipeline(gas, gbs, desc)
    if a.record:
        rs = bf.capi.default_record_state(a.app) if a.app else bf.capi.default_record_state()
        rs.s_recordData, rs.s_recordCompression = 1, 1
        p.set_record_state(rs, a.record_threads)
    print("camera calibration: %s" % ("registering depth to the colour camera" if p.camera_calibration() else
                                      "asked for, but the depth extrinsics are the identity: off" if gas.s_bUseCameraCalibration else "off"))
    t0 = time.time()
    keep = []                                               # the last few host frames stay alive while their upload may be in flight
    if a.ingest == "device":
        with sdm.SensPlayer(p, sd, a.decode_threads) as player:
            for k in range(n):
                if not player.next():
                    raise RuntimeError("frame not accepted")
    else:
        for k in range(n):
            depth = sd.depth(k)                                 # metres, -inf invalid
            color = sd.color_rgbx(k)
            if not p.process_frame(depth, color):
                raise RuntimeError("frame not accepted")
            keep = (keep + [(depth, color)])[-4:]
    for _ in range(a.tail):
        p.process_end_of_sequence()
    p.synchronize()
    dt = time.time() - t0
    print("%s: %d frames  wall %.3f s -> %.1f frames/s (decode + PCIe included; ingest %s%s)" % (
        sd.sensor_name, n, dt, n / dt, a.ingest, ", %d decode threads" % a.decode_threads if a.ingest == "device" else ""))
    print("counters", p.counters())
    traj = p.optimized_trajectory()
    valid = np.isfinite(traj[:, 0, 0])
    rmse, used = sd.evaluate_trajectory(traj)
    print("optimised trajectory: %d/%d valid; ate rmse = %.4f m over %d poses" % (valid.sum(), len(traj), rmse, used))
    sc = p.scene()
    print("allocated blocks", sc.num_allocated_blocks(), "heap free", sc.heap_free_count())
    if a.save:
        sd.save_with_trajectory(a.save, traj)
        print("wrote", a.save)
    if a.record:
        t1 = time.time()
        name, frames = p.save_recording(a.record)
        print("recorded %d frames to %s (%.3f s to drain and save)" % (frames, name, time.time() - t1))
    mesh_out.write(p, a)
    point_cloud_out.write(p, a)


if __name__ == "__main__":
    main()
