"""The frame renderer's C and C++ surface: libbf_hip.so exports every symbol include/bf_render.h declares, the wrappers of include/bundlefusion/bundlefusion.hpp
(GlobalRenderState, FrameRenderer) build with plain g++ and link, and - on a GPU - examples/headless_driver --video writes the reference's PNG sequences."""
import ctypes as C
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "bundlefusion_amd", "lib")


def test_library_exports_every_symbol_of_bf_render_h(built):
    """the rule of tests/test_host_cpu.py::test_library_exports_every_declared_symbol applied to bf_render.h"""
    txt = open(os.path.join(ROOT, "include", "bf_render.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    names = sorted(set(re.findall(r"BF_API\s+[\w\s\*]+?\b(bf_\w+)\s*\(", txt)))
    assert len(names) >= 16 and "bf_pipeline_render_top_down" in names and "bf_frame_renderer_shade" in names
    lib = C.CDLL(os.path.join(LIBDIR, "libbf_hip.so"))
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing


_WRAPPER_CPP = r'''
#include "bundlefusion/bundlefusion.hpp"
using namespace bundlefusion;
int main(int argc, char** argv) {
    GlobalRenderState& rs = GlobalRenderState::get();
    if (rs.s_materialShininess != 16.0f || rs.s_RenderMode != 1 || rs.s_lightDirection[2] != 2.0f) return 2;
    rs.readMembers(argv[1]);
    if (rs.s_RenderMode != 2 || rs.s_lightDirection[0] != 1.0f || std::string(rs.s_generateVideoDir) != "pictures/") return 3;
    std::printf("state ok\n");
    try {
        FrameRenderer fr(8, 4);
        if (fr.getWidth() != 8 || fr.getHeight() != 4 || !fr.GetColors() || !fr.getImageGPU()) return 4;
        fr.saveToFile(std::string(argv[2]));
        std::printf("renderer ok\n");
    } catch (const std::exception& e) { std::printf("error: %s\n", e.what()); return 1; }
    return 0;
}
'''


def test_cpp_render_wrappers_compile_and_link(built, tmp_path):
    """GlobalRenderState and FrameRenderer of bundlefusion.hpp build with plain g++ (no HIP headers) and resolve against libbf_hip.so; without a GPU the first
    device call fails loudly."""
    src = tmp_path / "wrap.cpp"; src.write_text(_WRAPPER_CPP)
    params = tmp_path / "p.txt"; params.write_text('s_RenderMode = 2;\ns_lightDirection = 1.0f 0.0f 0.0f;\ns_generateVideoDir = "pictures/";\n')
    exe = tmp_path / "wrap"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-L", LIBDIR, "-lbf_hip", "-Wl,-rpath," + LIBDIR, "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([str(exe), str(params), str(tmp_path / "a.png")], capture_output=True, text=True, timeout=120)
    assert "state ok" in out.stdout
    import torch
    if torch.cuda.is_available():
        assert out.returncode == 0 and "renderer ok" in out.stdout and (tmp_path / "a.png").read_bytes()[:8] == b"\x89PNG\r\n\x1a\n"
    else:
        assert out.returncode == 1 and "error: bundlefusion:" in out.stdout


def _png(path):
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    o, idat, size = 8, b"", None
    while o < len(raw):
        n, typ = struct.unpack(">I4s", raw[o:o + 8])
        data = raw[o + 8:o + 8 + n]
        assert struct.unpack(">I", raw[o + 8 + n:o + 12 + n])[0] == (zlib.crc32(typ + data) & 0xFFFFFFFF)
        if typ == b"IHDR":
            size = struct.unpack(">II", data[:8])
        if typ == b"IDAT":
            idat += data
        o += 12 + n
    w, h = size
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, w * 4 + 1)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(h, w, 4)


@pytest.mark.gpu
def test_headless_driver_writes_the_video_sequences(gpu, tmp_path):
    """examples/headless_driver --video DIR playing a .sens file of 12 synthetic frames (one chunk boundary; its dummy sensor shows a featureless wall, on which the
    first chunk is invalid by design): the folders of renderToFile and renderTopDown, six-digit frame numbers, and pictures that show the room."""
    from bundlefusion_amd import sensordata as sdm, synth
    W, H, n = 640, 480, 12
    frames = synth.render_frames(range(n))
    Kd = frames[0][3]
    K4 = np.eye(4, dtype=np.float32); K4[0, 0], K4[1, 1], K4[0, 2], K4[1, 2] = Kd["fx"], Kd["fy"], Kd["mx"], Kd["my"]
    sens = tmp_path / "stream.sens"
    with sdm.SensorDataWriter(sens, (W, H), (W, H), K4, depth_shift=1000.0, color_compression=sdm.COLOR_JPEG) as wr:
        for d, c, T, _ in frames:
            wr.add_frame(T, sdm.depth_to_u16(d, 1000.0), sdm.encode_jpeg_rgb(np.ascontiguousarray(c[:, :, :3]), 92))
    exe = tmp_path / "headless_driver"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "headless_driver.cpp"),
                        "-L", LIBDIR, "-lbf_hip", "-Wl,-rpath," + LIBDIR, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    app = tmp_path / "app.txt"
    app.write_text('s_sensorIdx = 8;\ns_binaryDumpSensorFile = "%s";\ns_integrationWidth = 320;\ns_integrationHeight = 240;\ns_SDFVoxelSize = 0.02f;\n'
                   's_hashNumBuckets = 50000;\ns_hashNumSDFBlocks = 20000;\ns_topVideoCameraPose = 0.0f 0.0f 0.0f 0.0f;\ns_topVideoMinMax = 0.3f 6.0f;\n' % sens)
    bun = tmp_path / "bundling.txt"
    bun.write_text("s_maxNumImages = 8;\n")
    video = tmp_path / "video"
    out = subprocess.run([str(exe), str(app), str(bun), "--video", str(video)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:]
    subs = ("self_reconstruction", "self_reconstruction_color", "reconstruction", "reconstruction_color", "input_color", "input_depth")
    counts = {s: sorted(os.listdir(video / s)) for s in subs}
    assert all(v == ["%06d.png" % k for k in range(n)] for v in counts.values()), counts
    for k in (0, n - 1):                                                  # before and behind the chunk boundary
        shaded = _png(video / "self_reconstruction" / ("%06d.png" % k))
        colored = _png(video / "self_reconstruction_color" / ("%06d.png" % k))
        assert shaded.shape == colored.shape == (240, 320, 4)
        assert (shaded[..., 3] == 255).mean() > 0.5 and (colored[..., 3] == 255).mean() > 0.5 and not np.array_equal(shaded, colored)
        top = _png(video / "reconstruction" / ("%06d.png" % k))
        assert (top[..., 3] == 255).mean() > 0.3
    col = _png(video / "input_color" / "000000.png")
    assert col.shape == (240, 320, 4) and (col[..., 3] == 255).all() and len(np.unique(col.reshape(-1, 4), axis=0)) > 10
    dep = _png(video / "input_depth" / "000000.png")
    assert (dep[..., 3] == 255).mean() > 0.5 and len(np.unique(dep.reshape(-1, 4), axis=0)) > 10
