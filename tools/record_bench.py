#!/usr/bin/env python3
"""What recording costs the frame loop (profiles/record_in_loop.md): the synthetic 640x480 stream at bench.py's operating point - `--preroll` frames
untimed (re-integration queue saturated), `--warmup` more, then `--steps` timed frames, device-resident input, 4 mm voxels, the library's default schedule.

  off     the loop with no record state
  recN    bf_pipeline_set_record_state with N encode threads; the time to drain and save afterwards is reported beside the rate
  host    per frame: device-to-host copy of depth and colour + what RGBDSensor::recordFrame did on the calling thread before the recorder existed
          (RGBX -> RGB, bf_encode_jpeg_rgb at quality 90, the depth rule, bf_sensor_data_writer_add_frame with zlib level 8) - milliseconds per frame

usage: python tools/record_bench.py [--variants off,rec1,rec4,rec8,host] [--rounds 3] [--steps 100] [--frames-cache FILE.npz]
The variants run alternately, `--rounds` times, each in a fresh pipeline; one JSON line per measurement.  --frames-cache: keep the rendered frames in a file, so
that another process (BF_LIB_PATH: another build of the library, `--variants off`) measures the same stream without rendering it again.
"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

W, H = 640, 480


def frames_of(n, cache):
    from bundlefusion_amd import synth
    if cache and os.path.exists(cache):
        z = np.load(cache)
        if len(z["depth"]) >= n:
            return z["depth"][:n], z["colour"][:n]
    fr = synth.render_frames(range(n), W, H, workers=16)
    depth = np.stack([np.asarray(f[0], np.float32).reshape(H, W) for f in fr])
    colour = np.stack([np.asarray(f[1], np.uint8).reshape(H, W, 4) for f in fr])
    if cache:
        np.savez(cache, depth=depth, colour=colour)
    return depth, colour


def pipeline(a):
    import bundlefusion_amd as bf
    from bundlefusion_amd import synth
    Kd = synth.intrinsics(W, H)
    gas = bf.capi.default_app_state(); gbs = bf.capi.default_bundling_state()
    gas.s_integrationWidth, gas.s_integrationHeight = W, H
    gas.s_SDFVoxelSize, gas.s_hashNumBuckets, gas.s_hashNumSDFBlocks = a.voxel, a.buckets, a.blocks
    gbs.s_maxNumImages = max(8, (a.preroll + a.warmup + a.steps) // 10 + 4)
    return bf.capi.Pipeline(gas, gbs, bf.capi.sensor_desc(W, H, bf.capi.intrinsics_matrix(Kd["fx"], Kd["fy"], Kd["mx"], Kd["my"])))


def loop(a, dev, threads, tmp):
    """-> (frames/s over the timed steps, seconds to drain and save or None, frames saved or None)"""
    import torch
    import bundlefusion_amd as bf
    p = pipeline(a)
    if threads:
        rs = bf.capi.default_record_state()
        rs.s_recordData = 1
        p.set_record_state(rs, threads, os.path.join(tmp, "bf_"))
    pre = a.preroll + a.warmup
    for k in range(pre):
        assert p.process_frame(*dev[k])
    p.synchronize(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(pre, pre + a.steps):
        assert p.process_frame(*dev[k])
    p.synchronize()
    dt = time.perf_counter() - t0
    save = saved = None
    if threads:
        t1 = time.perf_counter()
        _, saved = p.save_recording(os.path.join(tmp, "rec.sens"), overwrite=True)
        save = time.perf_counter() - t1
    p.close()
    return a.steps / dt, save, saved


def host_route(a, dev, tmp, n=20):
    """milliseconds per frame: (device-to-host copies, the encode on the calling thread)"""
    import torch
    from bundlefusion_amd import sensordata as sdm
    from bundlefusion_amd import synth
    from bundlefusion_amd.capi import intrinsics_matrix
    Kd = synth.intrinsics(W, H)
    w = sdm.SensorDataWriter(os.path.join(tmp, "host.sens"), (W, H), (W, H), intrinsics_matrix(Kd["fx"], Kd["fy"], Kd["mx"], Kd["my"]), color_compression=sdm.COLOR_JPEG)
    tc = te = 0.0
    for k in range(a.preroll, a.preroll + n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d = dev[k][0].cpu().numpy(); c = dev[k][1].cpu().numpy()
        t1 = time.perf_counter()
        jpeg = sdm.encode_jpeg_rgb(np.ascontiguousarray(c[:, :, :3]), 90)
        w.add_frame(np.eye(4, dtype=np.float32), sdm.record_depth_rule(d, 1000.0), jpeg)
        t2 = time.perf_counter()
        tc += t1 - t0; te += t2 - t1
    w.close()
    return 1e3 * tc / n, 1e3 * te / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", default="off,rec1,rec4,rec8,host")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--preroll", type=int, default=200)
    ap.add_argument("--voxel", type=float, default=0.004)
    ap.add_argument("--buckets", type=int, default=1000000)
    ap.add_argument("--blocks", type=int, default=600000)
    ap.add_argument("--frames-cache", default=None)
    ap.add_argument("--label", default="this build")
    a = ap.parse_args()
    import torch
    import bundlefusion_amd as bf
    depth, colour = frames_of(a.preroll + a.warmup + a.steps, a.frames_cache)
    dev = [(torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda()) for d, c in zip(depth, colour)]
    bf.capi.bind_host_threads_to_device(0)
    x = torch.ones((2048, 2048), device="cuda")              # untimed: bring the GPU out of its idle power state
    tw = time.perf_counter()
    while time.perf_counter() - tw < 3.0:
        (x @ x).sum().item()
    with tempfile.TemporaryDirectory() as tmp:
        for r in range(a.rounds):
            for v in a.variants.split(","):
                if v == "host":
                    copy_ms, encode_ms = host_route(a, dev, tmp)
                    print(json.dumps(dict(label=a.label, variant=v, round=r, copy_ms_per_frame=round(copy_ms, 3), encode_ms_per_frame=round(encode_ms, 3))), flush=True)
                else:
                    fps, save, saved = loop(a, dev, 0 if v == "off" else int(v[3:]), tmp)
                    rec = dict(label=a.label, variant=v, round=r, frames_per_s=round(fps, 1))
                    if save is not None:
                        rec.update(drain_and_save_s=round(save, 3), frames_saved=int(saved))
                    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
