// Stand-alone check of the recorder's threaded back end (bf_sens_recorder with pipeline == NULL), meant to be built under -fsanitize=thread and run
// on the CPU - never on a GPU machine:
//
//   g++ -std=c++17 -O1 -g -fsanitize=thread -ffp-contract=off -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude \
//       tools/record_backend_check.cpp bundlefusion_amd/csrc/sensordata.cpp bundlefusion_amd/csrc/imagecodec.cpp bundlefusion_amd/csrc/common.cpp \
//       -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib -lz -lpthread -o record_backend_check && ./record_backend_check
//
// It drives 37 frames (colour 40x24, depth 24x16) through 12 workers and 7 slots, finishes with 30 transforms (one all -inf), does the same with 1 worker
// and 2 slots and on the calling thread through bf_sensor_data_writer_add_frame, and compares the three files byte for byte; then a recorder that is
// destroyed with frames in flight.  The HIP runtime is linked for the symbols only: without a pipeline the recorder calls none of it, and the device
// entries the recorder's device front end needs are stubs here.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "bf_record.h"

extern "C" {
int bf_image_convert_depth_to_u16(uint16_t*, const float*, float, uint32_t, void*) { return BF_ERR_NO_DEVICE; }
int bf_jpeg_forward_device(const uint8_t*, uint32_t, uint32_t, int32_t, int16_t*, void*) { return BF_ERR_NO_DEVICE; }
int bf_pipeline_process_frame_raw_decoded(bf_pipeline*, const uint16_t*, float, const void*, const bf_jpeg_info*, int*) { return BF_ERR_NO_DEVICE; }
}
namespace bf { bool jpeg_on_device(const bf_jpeg_info&) { return false; } }

namespace {

const uint32_t CW = 40, CH = 24, DW = 24, DH = 16, FRAMES = 37, TRANSFORMS = 30;

#define CHECK(expr) do { const int _rc = (expr); if (_rc != BF_OK) { std::fprintf(stderr, "%s failed (%d): %s\n", #expr, _rc, bf_last_error()); std::exit(1); } } while (0)

uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

void makeFrame(uint32_t i, std::vector<uint8_t>& rgbx, std::vector<float>& depth) {
    uint32_t s = 12345u + i * 977u;
    rgbx.resize((size_t)CW * CH * 4); depth.resize((size_t)DW * DH);
    for (uint32_t y = 0; y < CH; ++y)
        for (uint32_t x = 0; x < CW; ++x) {
            uint8_t* p = &rgbx[((size_t)y * CW + x) * 4];
            p[0] = (uint8_t)(127 + 100 * std::sin((x + i) / 7.0 + y / 11.0)); p[1] = (uint8_t)(lcg(s) & 255u); p[2] = (uint8_t)((x * 5 + y * 3 + i) & 255u); p[3] = (uint8_t)(lcg(s) & 255u);
        }
    for (size_t k = 0; k < depth.size(); ++k) depth[k] = 0.3f + (float)(lcg(s) % 6000u) / 1000.0f;
    depth[i % depth.size()] = -std::numeric_limits<float>::infinity();
    depth[(i * 7 + 3) % depth.size()] = std::numeric_limits<float>::quiet_NaN();
    depth[(i * 13 + 5) % depth.size()] = 70.0f;
}

bf_sensor_data_info header() {
    bf_sensor_data_info info;
    std::memset(&info, 0, sizeof info);
    info.versionNumber = 4;
    std::snprintf(info.sensorName, sizeof info.sensorName, "%s", "RGBDSensor");
    for (int k = 0; k < 16; ++k) info.colorIntrinsic[k] = info.colorExtrinsic[k] = info.depthIntrinsic[k] = info.depthExtrinsic[k] = (k % 5 == 0) ? 1.0f : 0.0f;
    info.colorCompressionType = BF_SENS_COLOR_JPEG; info.depthCompressionType = BF_SENS_DEPTH_ZLIB_USHORT;
    info.colorWidth = CW; info.colorHeight = CH; info.depthWidth = DW; info.depthHeight = DH;
    info.depthShift = 1000.0f;
    return info;
}

std::vector<float> trajectory() {
    std::vector<float> T((size_t)TRANSFORMS * 16, 0.0f);
    for (uint32_t i = 0; i < TRANSFORMS; ++i) {
        float* m = &T[(size_t)i * 16];
        m[0] = m[5] = m[10] = m[15] = 1.0f; m[3] = 0.02f * i; m[7] = -0.01f * i;
        if (i == 7) for (int k = 0; k < 16; ++k) m[k] = -std::numeric_limits<float>::infinity();
    }
    return T;
}

std::vector<uint8_t> slurp(const std::string& path) {
    std::vector<uint8_t> out;
    if (FILE* f = std::fopen(path.c_str(), "rb")) { uint8_t buf[65536]; size_t n; while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n); std::fclose(f); }
    return out;
}

std::vector<uint8_t> recorded(const std::string& dir, uint32_t threads, uint32_t slots) {
    const bf_sensor_data_info info = header();
    const std::string tmp = dir + "/rec.tmp.sens", out = dir + "/rec.sens";
    bf_sens_recorder* rec = nullptr;
    CHECK(bf_sens_recorder_create(nullptr, &info, tmp.c_str(), threads, slots, &rec));
    std::vector<uint8_t> rgbx; std::vector<float> depth;
    for (uint32_t i = 0; i < FRAMES; ++i) { makeFrame(i, rgbx, depth); CHECK(bf_sens_recorder_record_host(rec, rgbx.data(), depth.data())); }
    const std::vector<float> T = trajectory();
    char name[1024]; uint64_t n = 0;
    CHECK(bf_sens_recorder_finish(rec, out.c_str(), T.data(), TRANSFORMS, 1, name, sizeof name, &n));
    if (n != TRANSFORMS || out != name) { std::fprintf(stderr, "finish wrote %llu frames to %s\n", (unsigned long long)n, name); std::exit(1); }
    CHECK(bf_sens_recorder_destroy(rec));
    std::vector<uint8_t> bytes = slurp(out);
    std::remove(out.c_str());
    return bytes;
}

std::vector<uint8_t> hostRoute(const std::string& dir) {
    const bf_sensor_data_info info = header();
    const std::string tmp = dir + "/host.tmp.sens", out = dir + "/host.sens";
    bf_sensor_data_writer* w = nullptr;
    CHECK(bf_sensor_data_writer_create(tmp.c_str(), &info, &w));
    std::vector<uint8_t> rgbx, rgb, jpeg; std::vector<float> depth; std::vector<uint16_t> u16;
    const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    for (uint32_t i = 0; i < FRAMES; ++i) {
        makeFrame(i, rgbx, depth);
        rgb.resize((size_t)CW * CH * 3); u16.resize(depth.size());
        for (size_t k = 0; k < (size_t)CW * CH; ++k) { rgb[3 * k] = rgbx[4 * k]; rgb[3 * k + 1] = rgbx[4 * k + 1]; rgb[3 * k + 2] = rgbx[4 * k + 2]; }
        for (size_t k = 0; k < depth.size(); ++k) { const float v = depth[k] * 1000.0f; u16[k] = (v > 0.0f && v < 65535.5f) ? (uint16_t)(v + 0.5f) : (uint16_t)0; }
        uint64_t n = 0;
        CHECK(bf_encode_jpeg_rgb(rgb.data(), CW, CH, 90, nullptr, 0, &n));
        jpeg.resize(n);
        CHECK(bf_encode_jpeg_rgb(rgb.data(), CW, CH, 90, jpeg.data(), jpeg.size(), &n));
        CHECK(bf_sensor_data_writer_add_frame(w, I, 0, 0, jpeg.data(), n, u16.data()));
    }
    CHECK(bf_sensor_data_writer_close(w));
    bf_sensor_data* sd = nullptr;
    CHECK(bf_sensor_data_open(tmp.c_str(), &sd));
    const std::vector<float> T = trajectory();
    CHECK(bf_sensor_data_save_recorded(sd, out.c_str(), T.data(), TRANSFORMS));
    CHECK(bf_sensor_data_close(sd));
    std::vector<uint8_t> bytes = slurp(out);
    std::remove(tmp.c_str()); std::remove(out.c_str());
    return bytes;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string dir = argc > 1 ? argv[1] : ".";
    const std::vector<uint8_t> a = recorded(dir, 12, 7), b = recorded(dir, 1, 2), c = hostRoute(dir);
    if (a.empty() || a != b || a != c) { std::fprintf(stderr, "the files differ: %zu / %zu / %zu bytes\n", a.size(), b.size(), c.size()); return 1; }
    {   // destroyed with frames in flight: the workers are joined, the temporary file goes
        const bf_sensor_data_info info = header();
        const std::string tmp = dir + "/abandoned.tmp.sens";
        bf_sens_recorder* rec = nullptr;
        CHECK(bf_sens_recorder_create(nullptr, &info, tmp.c_str(), 12, 7, &rec));
        std::vector<uint8_t> rgbx; std::vector<float> depth;
        for (uint32_t i = 0; i < 20; ++i) { makeFrame(i, rgbx, depth); CHECK(bf_sens_recorder_record_host(rec, rgbx.data(), depth.data())); }
        CHECK(bf_sens_recorder_destroy(rec));
        if (FILE* f = std::fopen(tmp.c_str(), "rb")) { std::fclose(f); std::fprintf(stderr, "the temporary file survived\n"); return 1; }
    }
    std::printf("record back end: %zu bytes, identical for (12, 7), (1, 2) and the calling thread\n", a.size());
    return 0;
}
