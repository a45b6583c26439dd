// Recorded sequences: the ".sens" container (ml::SensorData version 4) as used by SensorDataReader.cpp:40-128.
// Host-only, except that the decode-ahead player at the end hands its frames to a pipeline's device ingest.
// The byte layout is documented in include/bf_sensordata.h; frames are indexed at open time and read on demand.
#include <zlib.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <mutex>
#include <new>
#include <stdexcept>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../include/bf_record.h"
#include "../../include/bf_sensordata.h"
#include "bf_resources.h"

using namespace bf;

struct bf_sensor_data {
    FILE* f = nullptr;
    std::string path;
    bf_sensor_data_info info;
    struct Frame { float T[16]; uint64_t tsColor, tsDepth, colorSize, depthSize; int64_t colorOffset, depthOffset; };
    std::vector<Frame> frames;
    bf_sens_color_decoder decoder = nullptr;
    void* decoderUser = nullptr;
    std::vector<uint8_t> scratch;
};

struct bf_sensor_data_writer {
    FILE* f = nullptr;
    bf_sensor_data_info info;
    int64_t numFramesOffset = 0;
    uint64_t numFrames = 0;
    std::vector<uint8_t> scratch;
};

namespace {

const uint32_t SENS_VERSION = 4;                 // M_SENS_VERSION_NUMBER of the SensorData revision BundleFusion was written against
const uint64_t IMU_FRAME_BYTES = 5 * 3 * 8 + 8;  // rotationRate, acceleration, magneticField, attitude, gravity (vec3d) + timeStamp

template <class T> bool rd(FILE* f, T* v, size_t n = 1) { return fread(v, sizeof(T), n, f) == n; }
template <class T> bool wr(FILE* f, const T* v, size_t n = 1) { return fwrite(v, sizeof(T), n, f) == n; }

int64_t fileSize(FILE* f) {
    const int64_t cur = ftello(f);
    fseeko(f, 0, SEEK_END);
    const int64_t end = ftello(f);
    fseeko(f, cur, SEEK_SET);
    return end;
}

// no C++ exception leaves the C ABI: allocation failures on absurd (but formally valid) inputs become status codes
template <class F> int guarded(F f) {
    try { return f(); }
    catch (const std::bad_alloc&) { set_error("out of host memory"); return BF_ERR_CAPACITY; }
    catch (const std::exception& e) { set_error("%s", e.what()); return BF_ERR_STATE; }
}

int readBytes(FILE* f, int64_t offset, uint64_t size, uint8_t* out) {
    if (fseeko(f, offset, SEEK_SET) != 0 || fread(out, 1, size, f) != size) { set_error("sens: short read at offset %lld", (long long)offset); return BF_ERR_STATE; }
    return BF_OK;
}
int readBytes(bf_sensor_data* sd, int64_t offset, uint64_t size, uint8_t* out) { return readBytes(sd->f, offset, size, out); }

// SensorData::decompressDepthAlloc through file handle `f` (the reader's own, or a player thread's) with `scratch` for the compressed bytes
int readDepthRaw(bf_sensor_data* sd, FILE* f, std::vector<uint8_t>& scratch, uint64_t frame, uint16_t* out) {
    const bf_sensor_data::Frame& fr = sd->frames[frame];
    const uint64_t bytes = (uint64_t)sd->info.depthWidth * sd->info.depthHeight * 2;
    if (sd->info.depthCompressionType == BF_SENS_DEPTH_RAW_USHORT) {
        if (fr.depthSize != bytes) { set_error("sens: frame %llu: raw depth has %llu bytes, expected %llu", (unsigned long long)frame, (unsigned long long)fr.depthSize, (unsigned long long)bytes); return BF_ERR_STATE; }
        return readBytes(f, fr.depthOffset, bytes, reinterpret_cast<uint8_t*>(out));
    }
    if (sd->info.depthCompressionType == BF_SENS_DEPTH_ZLIB_USHORT) {
        scratch.resize(fr.depthSize);
        const int rc = readBytes(f, fr.depthOffset, fr.depthSize, scratch.data());
        if (rc) return rc;
        uLongf dstLen = (uLongf)bytes;
        const int z = uncompress(reinterpret_cast<Bytef*>(out), &dstLen, scratch.data(), (uLong)fr.depthSize);
        if (z != Z_OK || dstLen != bytes) { set_error("sens: frame %llu: zlib depth does not inflate to %llu bytes (zlib %d)", (unsigned long long)frame, (unsigned long long)bytes, z); return BF_ERR_STATE; }
        return BF_OK;
    }
    set_error("sens: depth compression type %d is not supported (raw and zlib u16 are)", sd->info.depthCompressionType);   // "unknown depth compression type"
    return BF_ERR_INVALID_ARG;
}

}  // namespace

extern "C" {

int bf_sensor_data_open(const char* filename, bf_sensor_data** out) {
    return guarded([&]() -> int {
    BF_REQUIRE(filename && out, "null argument");
    FILE* f = fopen(filename, "rb");
    if (!f) { set_error("could not open file %s", filename); return BF_ERR_INVALID_ARG; }          // "could not open file" (SensorData::loadFromFile)
    struct Closer { void operator()(bf_sensor_data* p) const { bf_sensor_data_close(p); } };
    std::unique_ptr<bf_sensor_data, Closer> guard(new bf_sensor_data);          // an exception below (bad_alloc) must not leak sd / its FILE*
    bf_sensor_data* sd = guard.get();
    sd->f = f;
    sd->path = filename;
    bf_sensor_data_info& h = sd->info;
    memset(&h, 0, sizeof h);
    const int64_t total = fileSize(f);
    bool ok = rd(f, &h.versionNumber);
    if (ok && h.versionNumber != SENS_VERSION) {
        set_error("sens: version %u, expected %u", h.versionNumber, SENS_VERSION);                   // "Invalid file format" / version mismatch
        return BF_ERR_INVALID_ARG;
    }
    uint64_t strLen = 0;
    ok = ok && rd(f, &strLen) && strLen <= (uint64_t)total;
    if (ok) {
        std::string name(strLen, '\0');
        ok = strLen == 0 || rd(f, &name[0], strLen);
        snprintf(h.sensorName, sizeof h.sensorName, "%s", name.c_str());
    }
    ok = ok && rd(f, h.colorIntrinsic, 16) && rd(f, h.colorExtrinsic, 16) && rd(f, h.depthIntrinsic, 16) && rd(f, h.depthExtrinsic, 16) &&
         rd(f, &h.colorCompressionType) && rd(f, &h.depthCompressionType) && rd(f, &h.colorWidth) && rd(f, &h.colorHeight) &&
         rd(f, &h.depthWidth) && rd(f, &h.depthHeight) && rd(f, &h.depthShift) && rd(f, &h.numFrames);
    // a frame record is at least 64 + 4 * 8 = 96 bytes (pose, two time stamps, two sizes): bound numFrames by what the rest of the
    // file can hold before frames.resize() (112 B of bookkeeping per frame) — a small forged header cannot ask for 100x the file size
    const int64_t afterHeader = ftello(f);
    if (!ok || afterHeader < 0 || h.numFrames > (uint64_t)(total - afterHeader) / 96u) { set_error("sens: truncated or invalid header in %s", filename); return BF_ERR_INVALID_ARG; }
    const uint32_t MAXDIM = 1u << 15;                                      // image buffers are sized from these fields
    if (h.depthWidth > MAXDIM || h.depthHeight > MAXDIM || h.colorWidth > MAXDIM || h.colorHeight > MAXDIM || !(h.depthShift > 0.0f) || !std::isfinite(h.depthShift)) {
        set_error("sens: implausible header in %s (depth %ux%u, colour %ux%u, depthShift %g)", filename, h.depthWidth, h.depthHeight, h.colorWidth, h.colorHeight, (double)h.depthShift);
        return BF_ERR_INVALID_ARG;
    }
    sd->frames.resize(h.numFrames);
    for (uint64_t i = 0; i < h.numFrames; ++i) {
        bf_sensor_data::Frame& fr = sd->frames[i];
        ok = rd(f, fr.T, 16) && rd(f, &fr.tsColor) && rd(f, &fr.tsDepth) && rd(f, &fr.colorSize) && rd(f, &fr.depthSize);
        if (ok) {
            fr.colorOffset = ftello(f);
            fr.depthOffset = fr.colorOffset + (int64_t)fr.colorSize;
            ok = fr.colorSize <= (uint64_t)total && fr.depthSize <= (uint64_t)total && fr.depthOffset + (int64_t)fr.depthSize <= total &&
                 fseeko(f, fr.depthOffset + (int64_t)fr.depthSize, SEEK_SET) == 0;
        }
        if (!ok) { set_error("sens: truncated at frame %llu of %llu in %s", (unsigned long long)i, (unsigned long long)h.numFrames, filename); return BF_ERR_INVALID_ARG; }
    }
    uint64_t numIMU = 0;
    if (rd(f, &numIMU)) {                                                   // the IMU block is optional; no multiplication that could wrap
        const int64_t pos = ftello(f);
        if (pos >= 0 && pos <= total && numIMU <= (uint64_t)(total - pos) / IMU_FRAME_BYTES) h.numIMUFrames = numIMU;
    }
    *out = guard.release();
    return BF_OK;
    });
}

int bf_sensor_data_close(bf_sensor_data* sd) {
    if (!sd) return BF_OK;
    if (sd->f) fclose(sd->f);
    delete sd;
    return BF_OK;
}

int bf_sensor_data_get_info(bf_sensor_data* sd, bf_sensor_data_info* out) { BF_REQUIRE(sd && out, "null argument"); *out = sd->info; return BF_OK; }

int bf_sensor_data_get_sensor_desc(bf_sensor_data* sd, bf_rgbd_sensor_desc* out) {                // SensorDataReader.cpp:57-63
    BF_REQUIRE(sd && out, "null argument");
    const bf_sensor_data_info& h = sd->info;
    memset(out, 0, sizeof *out);
    out->depthWidth = h.depthWidth; out->depthHeight = h.depthHeight;
    out->colorWidth = h.colorWidth > 1u ? h.colorWidth : 1u; out->colorHeight = h.colorHeight > 1u ? h.colorHeight : 1u;   // std::max(.., 1u) :57
    // initializeDepth/ColorIntrinsics(fx, fy, mx, my) build a 4x4 from the four scalars (RGBDSensor.cpp:142-147, 161-166); extrinsics are taken whole
    const float* src[2] = {h.depthIntrinsic, h.colorIntrinsic};
    float* dst[2] = {out->depthIntrinsics, out->colorIntrinsics};
    for (int k = 0; k < 2; ++k) {
        float* K = dst[k];
        for (int i = 0; i < 16; ++i) K[i] = 0.0f;
        K[0] = src[k][0]; K[5] = src[k][5]; K[2] = src[k][2]; K[6] = src[k][6]; K[10] = 1.0f; K[15] = 1.0f;
    }
    memcpy(out->depthExtrinsics, h.depthExtrinsic, 64);
    memcpy(out->colorExtrinsics, h.colorExtrinsic, 64);
    return BF_OK;
}

int bf_sensor_data_set_color_decoder(bf_sensor_data* sd, bf_sens_color_decoder fn, void* user) {
    BF_REQUIRE(sd, "null argument");
    sd->decoder = fn; sd->decoderUser = user;
    return BF_OK;
}

int bf_sensor_data_get_frame_pose(bf_sensor_data* sd, uint64_t frame, float T[16], uint64_t* tsColor, uint64_t* tsDepth) {
    BF_REQUIRE(sd && frame < sd->frames.size(), "frame index out of range");
    if (T) memcpy(T, sd->frames[frame].T, 64);
    if (tsColor) *tsColor = sd->frames[frame].tsColor;
    if (tsDepth) *tsDepth = sd->frames[frame].tsDepth;
    return BF_OK;
}

int bf_sensor_data_get_frame_sizes(bf_sensor_data* sd, uint64_t frame, uint64_t* colorSize, uint64_t* depthSize) {
    BF_REQUIRE(sd && frame < sd->frames.size(), "frame index out of range");
    if (colorSize) *colorSize = sd->frames[frame].colorSize;
    if (depthSize) *depthSize = sd->frames[frame].depthSize;
    return BF_OK;
}

int bf_sensor_data_read_depth_raw(bf_sensor_data* sd, uint64_t frame, uint16_t* out) {             // SensorData::decompressDepthAlloc
    return guarded([&]() -> int {
    BF_REQUIRE(sd && out && frame < sd->frames.size(), "bad argument");
    return readDepthRaw(sd, sd->f, sd->scratch, frame, out);
    });
}

int bf_sensor_data_read_depth(bf_sensor_data* sd, uint64_t frame, float* out) {                    // SensorDataReader::processDepth :98-103
    return guarded([&]() -> int {
    BF_REQUIRE(sd && out && frame < sd->frames.size(), "bad argument");
    const size_t n = (size_t)sd->info.depthWidth * sd->info.depthHeight;
    std::vector<uint16_t> raw(n);
    const int rc = bf_sensor_data_read_depth_raw(sd, frame, raw.data());
    if (rc) return rc;
    const float shift = sd->info.depthShift;
    for (size_t i = 0; i < n; ++i) out[i] = raw[i] == 0 ? -std::numeric_limits<float>::infinity() : (float)raw[i] / shift;
    return BF_OK;
    });
}

int bf_sensor_data_read_color_compressed(bf_sensor_data* sd, uint64_t frame, uint8_t* out, uint64_t capacity, uint64_t* size) {
    BF_REQUIRE(sd && size && frame < sd->frames.size(), "bad argument");
    const bf_sensor_data::Frame& fr = sd->frames[frame];
    *size = fr.colorSize;
    if (!out) return BF_OK;                                                       // size query
    BF_REQUIRE(capacity >= fr.colorSize, "buffer too small");
    return readBytes(sd, fr.colorOffset, fr.colorSize, out);
}

int bf_sensor_data_read_color_rgbx(bf_sensor_data* sd, uint64_t frame, uint8_t* out) {            // decompressColorAlloc + :107-111
    return guarded([&]() -> int {
    BF_REQUIRE(sd && out && frame < sd->frames.size(), "bad argument");
    const bf_sensor_data::Frame& fr = sd->frames[frame];
    const size_t n = (size_t)sd->info.colorWidth * sd->info.colorHeight;
    if (fr.colorSize == 0) { memset(out, 0, std::max<size_t>(n, 1) * 4); return BF_OK; }            // m_bHasColorData == false
    std::vector<uint8_t> rgb(n * 3);
    if (sd->info.colorCompressionType == BF_SENS_COLOR_RAW) {
        if (fr.colorSize != n * 3) { set_error("sens: frame %llu: raw colour has %llu bytes, expected %llu", (unsigned long long)frame, (unsigned long long)fr.colorSize, (unsigned long long)(n * 3)); return BF_ERR_STATE; }
        const int rc = readBytes(sd, fr.colorOffset, fr.colorSize, rgb.data());
        if (rc) return rc;
    } else if (sd->info.colorCompressionType == BF_SENS_COLOR_PNG || sd->info.colorCompressionType == BF_SENS_COLOR_JPEG) {
        sd->scratch.resize(fr.colorSize);
        const int rc = readBytes(sd, fr.colorOffset, fr.colorSize, sd->scratch.data());
        if (rc) return rc;
        if (sd->decoder) {
            if (sd->decoder(sd->decoderUser, sd->scratch.data(), fr.colorSize, sd->info.colorCompressionType, sd->info.colorWidth, sd->info.colorHeight, rgb.data()) != 0) {
                set_error("sens: frame %llu: the colour decoder failed", (unsigned long long)frame);
                return BF_ERR_STATE;
            }
        } else {
            const int drc = bf_decode_color_rgb(sd->scratch.data(), fr.colorSize, sd->info.colorCompressionType, sd->info.colorWidth, sd->info.colorHeight, rgb.data());
            if (drc) return drc;                                                   // message set by the decoder
        }
    } else {
        set_error("sens: colour compression type %d is not supported", sd->info.colorCompressionType);                 // "unknown compression type"
        return BF_ERR_INVALID_ARG;
    }
    for (size_t i = 0; i < n; ++i) { out[4 * i] = rgb[3 * i]; out[4 * i + 1] = rgb[3 * i + 1]; out[4 * i + 2] = rgb[3 * i + 2]; out[4 * i + 3] = 255; }   // vec4uc(vec3uc): w = 255
    return BF_OK;
    });
}

// ------------------------------------------------------------------------------------------------ writer
int bf_sensor_data_writer_create(const char* filename, const bf_sensor_data_info* info, bf_sensor_data_writer** out) {
    BF_REQUIRE(filename && info && out, "null argument");
    BF_REQUIRE(info->depthCompressionType == BF_SENS_DEPTH_RAW_USHORT || info->depthCompressionType == BF_SENS_DEPTH_ZLIB_USHORT, "depth compression must be raw or zlib u16");
    BF_REQUIRE(info->depthWidth > 0 && info->depthHeight > 0 && info->depthShift > 0.0f, "bad depth geometry");
    FILE* f = fopen(filename, "wb");
    if (!f) { set_error("could not open file %s for writing", filename); return BF_ERR_INVALID_ARG; }
    bf_sensor_data_writer* w = new bf_sensor_data_writer;
    w->f = f; w->info = *info;
    const bf_sensor_data_info& h = w->info;
    const uint32_t version = SENS_VERSION;
    const uint64_t strLen = strnlen(h.sensorName, sizeof h.sensorName);
    const uint64_t zero = 0;
    bool ok = wr(f, &version) && wr(f, &strLen) && (strLen == 0 || wr(f, h.sensorName, strLen)) && wr(f, h.colorIntrinsic, 16) && wr(f, h.colorExtrinsic, 16) &&
              wr(f, h.depthIntrinsic, 16) && wr(f, h.depthExtrinsic, 16) && wr(f, &h.colorCompressionType) && wr(f, &h.depthCompressionType) &&
              wr(f, &h.colorWidth) && wr(f, &h.colorHeight) && wr(f, &h.depthWidth) && wr(f, &h.depthHeight) && wr(f, &h.depthShift);
    w->numFramesOffset = ftello(f);
    ok = ok && wr(f, &zero);
    if (!ok) { set_error("sens: write failed (%s)", filename); fclose(f); delete w; return BF_ERR_STATE; }
    *out = w;
    return BF_OK;
}

int bf_sensor_data_writer_add_frame(bf_sensor_data_writer* w, const float T[16], uint64_t tsColor, uint64_t tsDepth, const uint8_t* colorBytes,
                                    uint64_t colorSize, const uint16_t* depth) {
    return guarded([&]() -> int {
    BF_REQUIRE(w && T && depth && (colorBytes || colorSize == 0), "null argument");
    const uint64_t rawBytes = (uint64_t)w->info.depthWidth * w->info.depthHeight * 2;
    const uint8_t* depthBytes = reinterpret_cast<const uint8_t*>(depth);
    uint64_t depthSize = rawBytes;
    if (w->info.depthCompressionType == BF_SENS_DEPTH_ZLIB_USHORT) {
        uLongf bound = compressBound((uLong)rawBytes);
        w->scratch.resize(bound);
        if (compress2(w->scratch.data(), &bound, depthBytes, (uLong)rawBytes, 8) != Z_OK) { set_error("sens: zlib compression failed"); return BF_ERR_STATE; }
        depthBytes = w->scratch.data(); depthSize = bound;
    }
    FILE* f = w->f;
    const bool ok = wr(f, T, 16) && wr(f, &tsColor) && wr(f, &tsDepth) && wr(f, &colorSize) && wr(f, &depthSize) &&
                    (colorSize == 0 || wr(f, colorBytes, colorSize)) && wr(f, depthBytes, depthSize);
    if (!ok) { set_error("sens: write failed at frame %llu", (unsigned long long)w->numFrames); return BF_ERR_STATE; }
    w->numFrames++;
    return BF_OK;
    });
}

int bf_sensor_data_writer_add_frame_compressed(bf_sensor_data_writer* w, const float T[16], uint64_t tsColor, uint64_t tsDepth, const uint8_t* colorBytes,
                                               uint64_t colorSize, const uint8_t* depthBytes, uint64_t depthSize) {
    BF_REQUIRE(w && T && depthBytes && (colorBytes || colorSize == 0), "null argument");
    if (w->info.depthCompressionType == BF_SENS_DEPTH_RAW_USHORT) BF_REQUIRE(depthSize == (uint64_t)w->info.depthWidth * w->info.depthHeight * 2, "raw depth has the wrong size");
    FILE* f = w->f;
    const bool ok = wr(f, T, 16) && wr(f, &tsColor) && wr(f, &tsDepth) && wr(f, &colorSize) && wr(f, &depthSize) &&
                    (colorSize == 0 || wr(f, colorBytes, colorSize)) && (depthSize == 0 || wr(f, depthBytes, depthSize));
    if (!ok) { set_error("sens: write failed at frame %llu", (unsigned long long)w->numFrames); return BF_ERR_STATE; }
    w->numFrames++;
    return BF_OK;
}

int bf_sensor_data_writer_close(bf_sensor_data_writer* w) {
    if (!w) return BF_OK;
    const uint64_t zero = 0;
    bool ok = wr(w->f, &zero);                                                    // no IMU frames
    ok = ok && fseeko(w->f, w->numFramesOffset, SEEK_SET) == 0 && wr(w->f, &w->numFrames);
    ok = (fclose(w->f) == 0) && ok;
    delete w;
    if (!ok) { set_error("sens: finishing the file failed"); return BF_ERR_STATE; }
    return BF_OK;
}

// ------------------------------------------------------------------------------------------------ trajectory I/O and evaluation
static int saveCopy(bf_sensor_data* sd, const char* filename, const float* trajectory, uint64_t numTransforms, bool dropRest) {
    FILE* f = fopen(filename, "wb");
    if (!f) { set_error("could not open file %s for writing", filename); return BF_ERR_INVALID_ARG; }
    const bf_sensor_data_info& h = sd->info;
    const uint32_t version = SENS_VERSION;
    const uint64_t strLen = strnlen(h.sensorName, sizeof h.sensorName), zero = 0;
    const uint64_t numFrames = dropRest ? std::min<uint64_t>(numTransforms, sd->frames.size()) : sd->frames.size();
    bool ok = wr(f, &version) && wr(f, &strLen) && (strLen == 0 || wr(f, h.sensorName, strLen)) && wr(f, h.colorIntrinsic, 16) && wr(f, h.colorExtrinsic, 16) &&
              wr(f, h.depthIntrinsic, 16) && wr(f, h.depthExtrinsic, 16) && wr(f, &h.colorCompressionType) && wr(f, &h.depthCompressionType) &&
              wr(f, &h.colorWidth) && wr(f, &h.colorHeight) && wr(f, &h.depthWidth) && wr(f, &h.depthHeight) && wr(f, &h.depthShift) && wr(f, &numFrames);
    float invalid[16];
    for (float& v : invalid) v = -std::numeric_limits<float>::infinity();
    std::vector<uint8_t> buf;
    for (uint64_t i = 0; ok && i < numFrames; ++i) {
        const bf_sensor_data::Frame& fr = sd->frames[i];
        const float* T = i < numTransforms ? trajectory + 16 * i : invalid;
        buf.resize(fr.colorSize + fr.depthSize);
        if (readBytes(sd, fr.colorOffset, fr.colorSize + fr.depthSize, buf.data()) != BF_OK) { fclose(f); return BF_ERR_STATE; }
        ok = wr(f, T, 16) && wr(f, &fr.tsColor) && wr(f, &fr.tsDepth) && wr(f, &fr.colorSize) && wr(f, &fr.depthSize) && (buf.empty() || wr(f, buf.data(), buf.size()));
    }
    ok = ok && wr(f, &zero);                                                      // IMU frames are not carried over
    ok = (fclose(f) == 0) && ok;
    if (!ok) { set_error("sens: writing %s failed", filename); return BF_ERR_STATE; }
    return BF_OK;
}

int bf_sensor_data_save_with_trajectory(bf_sensor_data* sd, const char* filename, const float* trajectory, uint64_t numTransforms) {
    return guarded([&]() -> int {
    BF_REQUIRE(sd && filename && (trajectory || numTransforms == 0), "null argument");
    return saveCopy(sd, filename, trajectory, numTransforms, false);
    });
}

int bf_sensor_data_save_recorded(bf_sensor_data* sd, const char* filename, const float* trajectory, uint64_t numTransforms) {
    return guarded([&]() -> int {
    BF_REQUIRE(sd && filename && trajectory && numTransforms > 0, "null argument");
    if (numTransforms > sd->frames.size()) { set_error("something went wrong; found more transforms than frames"); return BF_ERR_INVALID_ARG; }   // RGBDSensor.cpp:365
    return saveCopy(sd, filename, trajectory, numTransforms, true);
    });
}

}  // extern "C"

namespace {

// symmetric 3x3 eigen-decomposition by cyclic Jacobi rotations (double precision): A = V diag(w) V^T
void jacobiEigen3(double A[3][3], double V[3][3], double w[3]) {
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 64; ++sweep) {
        const double off = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[1][2]);
        if (off < 1e-300) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                if (fabs(A[p][q]) < 1e-300) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 3; ++k) { const double a = A[k][p], b = A[k][q]; A[k][p] = c * a - s * b; A[k][q] = s * a + c * b; }
                for (int k = 0; k < 3; ++k) { const double a = A[p][k], b = A[q][k]; A[p][k] = c * a - s * b; A[q][k] = s * a + c * b; }
                for (int k = 0; k < 3; ++k) { const double a = V[k][p], b = V[k][q]; V[k][p] = c * a - s * b; V[k][q] = s * a + c * b; }
            }
    }
    for (int i = 0; i < 3; ++i) w[i] = A[i][i];
}

// rigid alignment R p + t ~ r (Kabsch): R = argmax tr(R H), H = sum (p - pc)(r - rc)^T, via the polar factor of H^T
void kabschAlign(const std::vector<std::array<double, 3>>& p, const std::vector<std::array<double, 3>>& r, double R[3][3], double t[3]) {
    const size_t n = p.size();
    double pc[3] = {0, 0, 0}, rc[3] = {0, 0, 0};
    for (size_t i = 0; i < n; ++i) for (int k = 0; k < 3; ++k) { pc[k] += p[i][k]; rc[k] += r[i][k]; }
    for (int k = 0; k < 3; ++k) { pc[k] /= (double)n; rc[k] /= (double)n; }
    double H[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (size_t i = 0; i < n; ++i) for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) H[a][b] += (p[i][a] - pc[a]) * (r[i][b] - rc[b]);
    // H = U S V^T  =>  R = V D U^T with D = diag(1, 1, det(V U^T)).  V, S^2 from the eigen-decomposition of H^T H; U = H V S^-1.
    double HtH[3][3], V[3][3], w[3];
    for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) { HtH[a][b] = 0; for (int k = 0; k < 3; ++k) HtH[a][b] += H[k][a] * H[k][b]; }
    jacobiEigen3(HtH, V, w);
    int order[3] = {0, 1, 2};
    std::sort(order, order + 3, [&](int a, int b) { return w[a] > w[b]; });
    double Vs[3][3], U[3][3], sv[3];
    for (int j = 0; j < 3; ++j) { sv[j] = sqrt(std::max(w[order[j]], 0.0)); for (int k = 0; k < 3; ++k) Vs[k][j] = V[k][order[j]]; }
    for (int j = 0; j < 3; ++j) for (int k = 0; k < 3; ++k) { double v = 0; for (int m = 0; m < 3; ++m) v += H[k][m] * Vs[m][j]; U[k][j] = v; }
    // orthonormalise U's columns (Gram-Schmidt); a vanishing singular value (planar / collinear positions) is completed by a cross product
    auto norm = [](double* v) { const double l = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); if (l > 0) { v[0] /= l; v[1] /= l; v[2] /= l; } return l; };
    double u0[3] = {U[0][0], U[1][0], U[2][0]}, u1[3] = {U[0][1], U[1][1], U[2][1]}, u2[3];
    if (norm(u0) == 0.0) { u0[0] = 1; u0[1] = 0; u0[2] = 0; }
    { const double d = u0[0] * u1[0] + u0[1] * u1[1] + u0[2] * u1[2]; for (int k = 0; k < 3; ++k) u1[k] -= d * u0[k]; }
    if (norm(u1) < 1e-12 || sv[1] <= 1e-12 * std::max(sv[0], 1e-300)) {          // rank 1: any unit vector orthogonal to u0
        const int m = fabs(u0[0]) < fabs(u0[1]) ? (fabs(u0[0]) < fabs(u0[2]) ? 0 : 2) : (fabs(u0[1]) < fabs(u0[2]) ? 1 : 2);
        double e[3] = {0, 0, 0}; e[m] = 1;
        u1[0] = u0[1] * e[2] - u0[2] * e[1]; u1[1] = u0[2] * e[0] - u0[0] * e[2]; u1[2] = u0[0] * e[1] - u0[1] * e[0];
        norm(u1);                                                                   // collinear positions: any rotation about the line is optimal
    }
    u2[0] = u0[1] * u1[2] - u0[2] * u1[1]; u2[1] = u0[2] * u1[0] - u0[0] * u1[2]; u2[2] = u0[0] * u1[1] - u0[1] * u1[0];
    double v0[3] = {Vs[0][0], Vs[1][0], Vs[2][0]}, v1[3] = {Vs[0][1], Vs[1][1], Vs[2][1]}, v2[3];
    v2[0] = v0[1] * v1[2] - v0[2] * v1[1]; v2[1] = v0[2] * v1[0] - v0[0] * v1[2]; v2[2] = v0[0] * v1[1] - v0[1] * v1[0];
    // u2 = u0 x u1 and v2 = v0 x v1 make both bases right-handed, so R = sum v_j u_j^T is a proper rotation; this equals the usual
    // V diag(1, 1, det(V U^T)) U^T (the direction of the smallest singular value is the one that flips when H contains a reflection)
    const double* uu[3] = {u0, u1, u2};
    const double* vv[3] = {v0, v1, v2};
    for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) { R[a][b] = 0; for (int j = 0; j < 3; ++j) R[a][b] += vv[j][a] * uu[j][b]; }
    for (int a = 0; a < 3; ++a) { t[a] = rc[a]; for (int b = 0; b < 3; ++b) t[a] -= R[a][b] * pc[b]; }
}

}  // namespace

extern "C" {

static void validPositions(const float* traj, const float* ref, uint32_t n, std::vector<std::array<double, 3>>& pts, std::vector<std::array<double, 3>>& refPts,
                           std::vector<uint32_t>* indices) {
    const float NINF = -std::numeric_limits<float>::infinity();
    auto tr = [](const float* T, uint32_t i, int k) { return (double)T[16 * (size_t)i + 4 * k + 3]; };
    for (uint32_t i = 0; i < n; ++i)
        if (traj[16 * (size_t)i] != NINF && ref[16 * (size_t)i] != NINF) {
            pts.push_back({tr(traj, i, 0), tr(traj, i, 1), tr(traj, i, 2)});
            refPts.push_back({tr(ref, i, 0), tr(ref, i, 1), tr(ref, i, 2)});
            if (indices) indices->push_back(i);
        }
}

int bf_evaluate_ate_rmse(const float* traj, const float* ref, uint32_t numTransforms, float* rmse, uint32_t* numEvaluated) {     // PoseHelper.h:35-79
    return guarded([&]() -> int {
    BF_REQUIRE((traj && ref) || numTransforms == 0, "null argument");
    BF_REQUIRE(rmse && numEvaluated, "null argument");
    const float NINF = -std::numeric_limits<float>::infinity();
    auto tr = [](const float* T, uint32_t i, int k) { return (double)T[16 * (size_t)i + 4 * k + 3]; };
    if (numTransforms < 3) {
        *rmse = NINF; *numEvaluated = numTransforms;
        if (numTransforms == 2) {
            const double l = sqrt(tr(ref, 0, 0) * tr(ref, 0, 0) + tr(ref, 0, 1) * tr(ref, 0, 1) + tr(ref, 0, 2) * tr(ref, 0, 2));
            if (!(l > 0.0001)) {
                double d = 0;
                for (int k = 0; k < 3; ++k) d += (tr(traj, 1, k) - tr(ref, 1, k)) * (tr(traj, 1, k) - tr(ref, 1, k));
                *rmse = (float)sqrt(d);
            }
        }
        return BF_OK;
    }
    std::vector<std::array<double, 3>> pts, refPts;
    validPositions(traj, ref, numTransforms, pts, refPts, nullptr);
    if (pts.empty()) { *rmse = NINF; *numEvaluated = 0; return BF_OK; }                    // "ERROR no points to evaluate"
    double R[3][3], t[3];
    kabschAlign(pts, refPts, R, t);
    double err = 0;
    for (size_t i = 0; i < pts.size(); ++i)
        for (int a = 0; a < 3; ++a) {
            double v = t[a] - refPts[i][a];
            for (int b = 0; b < 3; ++b) v += R[a][b] * pts[i][b];
            err += v * v;
        }
    *rmse = (float)sqrt(err / (double)pts.size());
    *numEvaluated = (uint32_t)pts.size();
    return BF_OK;
    });
}

int bf_trajectory_alignment(const float* traj, const float* ref, uint32_t numTransforms, float align[16]) {                       // PoseHelper.h:81-108
    return guarded([&]() -> int {
    BF_REQUIRE(align && ((traj && ref) || numTransforms == 0), "null argument");
    for (int i = 0; i < 16; ++i) align[i] = -std::numeric_limits<float>::infinity();          // ret.setZero(-inf): "cannot evaluate"
    if (numTransforms < 3) return BF_OK;
    std::vector<std::array<double, 3>> pts, refPts;
    validPositions(traj, ref, numTransforms, pts, refPts, nullptr);
    if (pts.empty()) return BF_OK;
    double R[3][3], t[3];
    kabschAlign(pts, refPts, R, t);
    for (int a = 0; a < 3; ++a) { for (int b = 0; b < 3; ++b) align[4 * a + b] = (float)R[a][b]; align[4 * a + 3] = (float)t[a]; }
    align[12] = align[13] = align[14] = 0.0f; align[15] = 1.0f;
    return BF_OK;
    });
}

int bf_evaluate_err2_per_image(const float* traj, const float* ref, uint32_t numTransforms, uint32_t* imageIndices, float* err2, uint32_t* count) {   // :110-146
    return guarded([&]() -> int {
    BF_REQUIRE(imageIndices && err2 && count && ((traj && ref) || numTransforms == 0), "null argument");
    *count = 0;
    auto tr = [](const float* T, uint32_t i, int k) { return (double)T[16 * (size_t)i + 4 * k + 3]; };
    if (numTransforms < 3) {
        if (numTransforms == 2) {
            const double l = sqrt(tr(ref, 0, 0) * tr(ref, 0, 0) + tr(ref, 0, 1) * tr(ref, 0, 1) + tr(ref, 0, 2) * tr(ref, 0, 2));
            if (!(l > 0.0001)) {
                double d = 0;
                for (int k = 0; k < 3; ++k) d += (tr(traj, 1, k) - tr(ref, 1, k)) * (tr(traj, 1, k) - tr(ref, 1, k));
                imageIndices[0] = 0; err2[0] = (float)sqrt(d); *count = 1;                     // the reference stores the distance (not squared) here
            }
        }
        return BF_OK;
    }
    std::vector<std::array<double, 3>> pts, refPts;
    std::vector<uint32_t> idx;
    validPositions(traj, ref, numTransforms, pts, refPts, &idx);
    if (pts.empty()) return BF_OK;
    double R[3][3], t[3];
    kabschAlign(pts, refPts, R, t);
    for (size_t i = 0; i < pts.size(); ++i) {
        double e = 0;
        for (int a = 0; a < 3; ++a) {
            double v = t[a] - refPts[i][a];
            for (int b = 0; b < 3; ++b) v += R[a][b] * pts[i][b];
            e += v * v;
        }
        imageIndices[i] = idx[i]; err2[i] = (float)e;
    }
    *count = (uint32_t)pts.size();
    return BF_OK;
    });
}

int bf_sensor_data_evaluate_trajectory(bf_sensor_data* sd, const float* trajectory, uint64_t numTransforms, float* rmse, uint32_t* numEvaluated) {   // :167-189
    return guarded([&]() -> int {
    BF_REQUIRE(sd && trajectory && rmse && numEvaluated, "null argument");
    const size_t nRef = sd->frames.size();
    BF_REQUIRE(nRef > 0, "no frames");
    // offset = referenceTrajectory.front().getInverse(); reference[i] = offset * reference[i]  (row-major 4x4, general inverse of a rigid pose)
    const float* F = sd->frames[0].T;
    double Rinv[3][3], tinv[3];
    for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) Rinv[a][b] = F[4 * b + a];
    for (int a = 0; a < 3; ++a) { tinv[a] = 0; for (int b = 0; b < 3; ++b) tinv[a] -= Rinv[a][b] * F[4 * b + 3]; }
    std::vector<float> ref(16 * nRef);
    const float NINF = -std::numeric_limits<float>::infinity();
    for (size_t i = 0; i < nRef; ++i) {
        const float* T = sd->frames[i].T;
        float* o = ref.data() + 16 * i;
        if (T[0] == NINF) { for (int k = 0; k < 16; ++k) o[k] = NINF; continue; }
        for (int a = 0; a < 3; ++a) {
            for (int b = 0; b < 4; ++b) { double v = b == 3 ? tinv[a] : 0.0; for (int k = 0; k < 3; ++k) v += Rinv[a][k] * T[4 * k + b]; o[4 * a + b] = (float)v; }
        }
        o[12] = o[13] = o[14] = 0.0f; o[15] = 1.0f;
    }
    const uint32_t n = (uint32_t)std::min<uint64_t>(numTransforms, nRef);
    return bf_evaluate_ate_rmse(trajectory, ref.data(), n, rmse, numEvaluated);
    });
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ decode-ahead player
// Frame k lives in slot k % numSlots.  A worker claims the next unclaimed frame as soon as that frame's slot has been handed on, reads and decodes it
// through its own file handle, and marks the slot ready; bf_sens_player_next waits for the slot of the next frame in order.  Which thread decodes a
// frame has no influence on the bytes in its slot.
struct bf_sens_player {
    bf_pipeline* pipe = nullptr;
    bf_sensor_data* sd = nullptr;
    struct Slot {
        uint16_t* depth = nullptr; uint8_t* colour = nullptr;
        int state = 0;                        // 0 free, 1 being decoded, 2 ready
        uint64_t frame = 0;
        int rc = BF_OK; std::string err;
        bool coefficients = false; bf_jpeg_info jpeg; uint64_t colourBytes = 0;
    };
    std::vector<Slot> slots;
    size_t colourCapacity = 0;
    bool pinned = false;
    bf::Resources res;                        // the slots' buffers when pinned (malloc otherwise)
    std::mutex m;
    std::condition_variable cvWork, cvReady;
    uint64_t nextClaim = 0, nextOut = 0, numFrames = 0;
    bool stop = false;
    std::vector<std::thread> threads;
};

namespace {

void playerDecode(bf_sens_player* pl, FILE* f, std::vector<uint8_t>& scratch, bf_sens_player::Slot& s) {
    bf_sensor_data* sd = pl->sd;
    const bf_sensor_data_info& h = sd->info;
    const bf_sensor_data::Frame& fr = sd->frames[s.frame];
    const size_t nc = (size_t)h.colorWidth * h.colorHeight;
    s.coefficients = false; s.colourBytes = nc * 3;
    s.rc = guarded([&]() -> int {
        int rc = readDepthRaw(sd, f, scratch, s.frame, s.depth);
        if (rc) return rc;
        if (fr.colorSize == 0) { set_error("sens: frame %llu has no colour data: the device ingest needs colour (use the host ingest for this file)", (unsigned long long)s.frame); return BF_ERR_NOT_ON_DEVICE; }
        const int32_t ct = h.colorCompressionType;
        if (ct == BF_SENS_COLOR_RAW) {
            if (fr.colorSize != nc * 3) { set_error("sens: frame %llu: raw colour has %llu bytes, expected %llu", (unsigned long long)s.frame, (unsigned long long)fr.colorSize, (unsigned long long)(nc * 3)); return BF_ERR_STATE; }
            return readBytes(f, fr.colorOffset, fr.colorSize, s.colour);
        }
        if (ct != BF_SENS_COLOR_PNG && ct != BF_SENS_COLOR_JPEG) { set_error("sens: colour compression type %d is not supported", ct); return BF_ERR_INVALID_ARG; }
        scratch.resize(fr.colorSize);
        rc = readBytes(f, fr.colorOffset, fr.colorSize, scratch.data());
        if (rc) return rc;
        if (sd->decoder) {
            if (sd->decoder(sd->decoderUser, scratch.data(), fr.colorSize, ct, h.colorWidth, h.colorHeight, s.colour) != 0) { set_error("sens: frame %llu: the colour decoder failed", (unsigned long long)s.frame); return BF_ERR_STATE; }
            return BF_OK;
        }
        if (ct == BF_SENS_COLOR_JPEG) {
            rc = bf_jpeg_parse(scratch.data(), fr.colorSize, h.colorWidth, h.colorHeight, &s.jpeg);
            if (rc) return rc;
            if (jpeg_on_device(s.jpeg) && (size_t)s.jpeg.numBlocks * 128 <= pl->colourCapacity) {
                rc = bf_jpeg_entropy_decode(scratch.data(), fr.colorSize, &s.jpeg, reinterpret_cast<int16_t*>(s.colour), (uint64_t)s.jpeg.numBlocks * 64);
                if (rc == BF_OK) { s.coefficients = true; s.colourBytes = (uint64_t)s.jpeg.numBlocks * 128; return BF_OK; }
                if (rc != BF_ERR_NOT_ON_DEVICE) return rc;
            }
        }
        return bf_decode_color_rgb(scratch.data(), fr.colorSize, ct, h.colorWidth, h.colorHeight, s.colour);
    });
    if (s.rc) s.err = bf_last_error();
}

void playerWorker(bf_sens_player* pl) {
    FILE* f = fopen(pl->sd->path.c_str(), "rb");          // a handle of its own: the reader's is not shared between threads
    std::vector<uint8_t> scratch;
    for (;;) {
        bf_sens_player::Slot* s = nullptr;
        {
            std::unique_lock<std::mutex> lk(pl->m);
            pl->cvWork.wait(lk, [&] { return pl->stop || (pl->nextClaim < pl->numFrames && pl->slots[pl->nextClaim % pl->slots.size()].state == 0); });
            if (pl->stop) break;
            s = &pl->slots[pl->nextClaim % pl->slots.size()];
            s->state = 1; s->frame = pl->nextClaim++;
        }
        if (f) playerDecode(pl, f, scratch, *s);
        else { s->rc = BF_ERR_STATE; s->err = "could not open file " + pl->sd->path; }
        {
            std::lock_guard<std::mutex> lk(pl->m);
            s->state = 2;
        }
        pl->cvReady.notify_all();
    }
    if (f) fclose(f);
}

// the slot of the next frame in order, decoded; null at the end of the file
bf_sens_player::Slot* playerWait(bf_sens_player* pl) {
    std::unique_lock<std::mutex> lk(pl->m);
    if (pl->nextOut >= pl->numFrames) return nullptr;
    bf_sens_player::Slot& s = pl->slots[pl->nextOut % pl->slots.size()];
    pl->cvReady.wait(lk, [&] { return s.state == 2 && s.frame == pl->nextOut; });
    return &s;
}

void playerRelease(bf_sens_player* pl, bf_sens_player::Slot* s) {
    {
        std::lock_guard<std::mutex> lk(pl->m);
        s->state = 0; pl->nextOut++;
    }
    pl->cvWork.notify_all();
}

}  // namespace

extern "C" {

int bf_sens_player_destroy(bf_sens_player* pl) {
    if (!pl) return BF_OK;
    {
        std::lock_guard<std::mutex> lk(pl->m);
        pl->stop = true;
    }
    pl->cvWork.notify_all();
    for (std::thread& t : pl->threads) t.join();
    if (!pl->pinned) for (bf_sens_player::Slot& s : pl->slots) { free(s.depth); free(s.colour); }
    delete pl;
    return BF_OK;
}

int bf_sens_player_create(bf_pipeline* pipeline, bf_sensor_data* sd, uint32_t numThreads, bf_sens_player** out) {
    return guarded([&]() -> int {
    BF_REQUIRE(sd && out, "null argument");
    BF_REQUIRE(numThreads <= 12, "at most 12 decode threads");
    if (numThreads == 0) numThreads = 4;
    const bf_sensor_data_info& h = sd->info;
    BF_REQUIRE(h.depthWidth > 0 && h.depthHeight > 0 && h.colorWidth > 0 && h.colorHeight > 0, "the file has no depth or no colour images");
    bf_sens_player* pl = new bf_sens_player;
    bf::CreateGuard<bf_sens_player> guard(pl, bf_sens_player_destroy);
    pl->pipe = pipeline; pl->sd = sd; pl->numFrames = sd->frames.size(); pl->pinned = pipeline != nullptr;
    // the coefficients of any layout the device takes: three components at no more than full resolution, padded to whole 16 x 16 MCUs, 2 bytes each
    const size_t padW = ((size_t)h.colorWidth + 15) / 16 * 16, padH = ((size_t)h.colorHeight + 15) / 16 * 16;
    pl->colourCapacity = std::max((size_t)h.colorWidth * h.colorHeight * 3, padW * padH * 6);
    const size_t depthBytes = (size_t)h.depthWidth * h.depthHeight * 2;
    pl->slots.resize(numThreads + 2);
    for (bf_sens_player::Slot& s : pl->slots) {
        if (pl->pinned) {
            BF_TRY(pl->res.pinned(&s.depth, depthBytes));
            BF_TRY(pl->res.pinned(&s.colour, pl->colourCapacity));
        } else {
            s.depth = (uint16_t*)malloc(depthBytes); s.colour = (uint8_t*)malloc(pl->colourCapacity);
            if (!s.depth || !s.colour) throw std::bad_alloc();
        }
    }
    for (uint32_t t = 0; t < numThreads; ++t) pl->threads.emplace_back(playerWorker, pl);
    *out = guard.dismiss();
    return BF_OK;
    });
}

int bf_sens_player_peek(bf_sens_player* pl, bf_sens_frame* out, int* gotFrame) {
    BF_REQUIRE(pl && out && gotFrame, "null argument");
    *gotFrame = 0;
    bf_sens_player::Slot* s = playerWait(pl);
    if (!s) return BF_OK;
    if (s->rc) { set_error("%s", s->err.c_str()); return s->rc; }
    memset(out, 0, sizeof *out);
    out->frame = s->frame; out->depthU16 = s->depth; out->colour = s->colour; out->colourBytes = s->colourBytes; out->jpegCoefficients = s->coefficients ? 1 : 0;
    if (s->coefficients) out->jpeg = s->jpeg;
    *gotFrame = 1;
    return BF_OK;
}

int bf_sens_player_next(bf_sens_player* pl, int* gotFrame) {
    BF_REQUIRE(pl && gotFrame, "null argument");
    *gotFrame = 0;
    bf_sens_player::Slot* s = playerWait(pl);
    if (!s) return BF_OK;
    int rc = s->rc, got = 1;
    if (rc) set_error("%s", s->err.c_str());
    else if (pl->pipe) rc = bf_pipeline_process_frame_raw_decoded(pl->pipe, s->depth, pl->sd->info.depthShift, s->colour, s->coefficients ? &s->jpeg : nullptr, &got);
    playerRelease(pl, s);                    // a failed frame is passed over: the caller decides whether to go on
    if (rc) return rc;
    *gotFrame = got;
    return BF_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ recorder (bf_record.h): the player's mirror image
// Frame k lives in slot k % numSlots.  The record call fills the slot's front half (coefficients + u16 depth: on the calling thread, or with two kernels and a
// copy whose event the slot carries) and marks it FILLED; a worker claims the next FILLED frame in order, waits for the slot's copy event if it has one,
// entropy-codes and deflates into the slot's blobs and marks it ENCODED.  The thread that finishes frame nextAppend appends it, and whatever is already
// waiting behind it, to the temporary file - one appender at a time, so the file is in frame order whatever the threads' timing.
struct bf_sens_recorder {
    bool pinned = false; int device = 0;
    bf_sensor_data_info info;
    std::string tmp;
    bf_sensor_data_writer* writer = nullptr;              // open while frames of the current recording exist; touched by the appender only (and by finish after the drain)
    size_t coefCount = 0, depthCount = 0;
    enum { FREE = 0, FILLING = 1, FILLED = 2, ENCODING = 3, ENCODED = 4 };
    struct Slot {
        int16_t* coef = nullptr; uint16_t* depth = nullptr;          // host
        int16_t* d_coef = nullptr; uint16_t* d_depth = nullptr;      // device twin (pinned recorders)
        hipEvent_t packed = nullptr, copied = nullptr;
        bool onDevice = false;                            // this frame's front half arrives by the copy: wait for `copied`
        int state = FREE; uint64_t frame = 0;
        std::vector<uint8_t> jpeg, z; uint64_t jpegSize = 0, zSize = 0;
    };
    std::vector<Slot> slots;
    hipStream_t copyStream = nullptr;
    bf::Resources res;                                    // copyStream and the slots' buffers and events when pinned (malloc otherwise)
    std::mutex m;
    std::condition_variable cvWork, cvFree;
    uint64_t nextRecord = 0, nextClaim = 0, nextAppend = 0;          // frames handed in / claimed by a worker / appended (or given up after an error)
    bool appending = false, stop = false;
    int rc = BF_OK; std::string err;                      // the first failure of a worker
    std::vector<std::thread> threads;
};

namespace {

const int RECORD_JPEG_QUALITY = 90;

void recFail(bf_sens_recorder* r, int rc) {               // with r->m held
    if (r->rc == BF_OK) { r->rc = rc; r->err = bf_last_error(); }
}

int recEncode(bf_sens_recorder* r, bf_sens_recorder::Slot& s) {
    return guarded([&]() -> int {
        if (s.onDevice && hipEventSynchronize(s.copied) != hipSuccess) { set_error("recorder: the copy of frame %llu failed (%s)", (unsigned long long)s.frame, hipGetErrorString(hipGetLastError())); return BF_ERR_HIP; }
        const bf_sensor_data_info& h = r->info;
        uint64_t n = 0;
        BF_TRY(bf_jpeg_entropy_encode(h.colorWidth, h.colorHeight, RECORD_JPEG_QUALITY, s.coef, nullptr, 0, &n));
        if (s.jpeg.size() < n) s.jpeg.resize(n);
        BF_TRY(bf_jpeg_entropy_encode(h.colorWidth, h.colorHeight, RECORD_JPEG_QUALITY, s.coef, s.jpeg.data(), s.jpeg.size(), &n));
        s.jpegSize = n;
        const uint64_t rawBytes = (uint64_t)r->depthCount * 2;
        if (h.depthCompressionType == BF_SENS_DEPTH_ZLIB_USHORT) {
            uLongf bound = compressBound((uLong)rawBytes);
            if (s.z.size() < bound) s.z.resize(bound);
            if (compress2(s.z.data(), &bound, reinterpret_cast<const Bytef*>(s.depth), (uLong)rawBytes, 8) != Z_OK) { set_error("sens: zlib compression failed"); return BF_ERR_STATE; }
            s.zSize = bound;
        } else {
            if (s.z.size() < rawBytes) s.z.resize(rawBytes);
            memcpy(s.z.data(), s.depth, rawBytes);
            s.zSize = rawBytes;
        }
        return BF_OK;
    });
}

void recWorker(bf_sens_recorder* r) {
    if (r->pinned) (void)hipSetDevice(r->device);
    static const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    for (;;) {
        bf_sens_recorder::Slot* s = nullptr;
        {
            std::unique_lock<std::mutex> lk(r->m);
            r->cvWork.wait(lk, [&] { return r->stop || (r->nextClaim < r->nextRecord && r->slots[r->nextClaim % r->slots.size()].state == bf_sens_recorder::FILLED); });
            if (r->stop) break;
            s = &r->slots[r->nextClaim % r->slots.size()];
            s->state = bf_sens_recorder::ENCODING; r->nextClaim++;
        }
        const int rc = recEncode(r, *s);
        std::unique_lock<std::mutex> lk(r->m);
        if (rc) recFail(r, rc);
        s->state = bf_sens_recorder::ENCODED;
        if (r->appending) continue;                       // the appender finds this frame when it gets there
        r->appending = true;
        for (;;) {
            bf_sens_recorder::Slot& a = r->slots[r->nextAppend % r->slots.size()];
            if (!(r->nextAppend < r->nextClaim && a.state == bf_sens_recorder::ENCODED && a.frame == r->nextAppend)) break;
            const bool write = r->rc == BF_OK;            // after a failure the frames behind it are given up: the recording is lost, the ring keeps moving
            lk.unlock();
            int wrc = BF_OK;
            if (write) {
                if (!r->writer) wrc = bf_sensor_data_writer_create(r->tmp.c_str(), &r->info, &r->writer);
                if (wrc == BF_OK) wrc = bf_sensor_data_writer_add_frame_compressed(r->writer, I, 0, 0, a.jpeg.data(), a.jpegSize, a.z.data(), a.zSize);
            }
            lk.lock();
            if (wrc) recFail(r, wrc);
            a.state = bf_sens_recorder::FREE; r->nextAppend++;
            r->cvFree.notify_all();
        }
        r->appending = false;
    }
}

// the slot of the next frame, free to fill (waits while the ring is full); null with the worker's status when one has failed
int recAcquire(bf_sens_recorder* r, bf_sens_recorder::Slot** out) {
    std::unique_lock<std::mutex> lk(r->m);
    bf_sens_recorder::Slot& s = r->slots[r->nextRecord % r->slots.size()];
    r->cvFree.wait(lk, [&] { return s.state == bf_sens_recorder::FREE; });
    if (r->rc) { set_error("%s", r->err.c_str()); return r->rc; }
    s.state = bf_sens_recorder::FILLING; s.frame = r->nextRecord;
    *out = &s;
    return BF_OK;
}

void recSubmit(bf_sens_recorder* r, bf_sens_recorder::Slot* s, bool filled) {
    {
        std::lock_guard<std::mutex> lk(r->m);
        if (filled) { s->state = bf_sens_recorder::FILLED; r->nextRecord++; }
        else s->state = bf_sens_recorder::FREE;
    }
    r->cvWork.notify_all();
}

bool fileExists(const std::string& f) { if (FILE* fp = fopen(f.c_str(), "rb")) { fclose(fp); return true; } return false; }

}  // namespace

extern "C" {

int bf_sens_recorder_destroy(bf_sens_recorder* r) {
    if (!r) return BF_OK;
    {
        std::lock_guard<std::mutex> lk(r->m);
        r->stop = true;
    }
    r->cvWork.notify_all();
    for (std::thread& t : r->threads) t.join();
    if (r->writer) { bf_sensor_data_writer_close(r->writer); r->writer = nullptr; }
    std::remove(r->tmp.c_str());
    if (r->pinned) {
        if (r->copyStream) (void)hipStreamSynchronize(r->copyStream);
    } else {
        for (bf_sens_recorder::Slot& s : r->slots) { free(s.coef); free(s.depth); }
    }
    delete r;
    return BF_OK;
}

int bf_sens_recorder_create(bf_pipeline* pipeline, const bf_sensor_data_info* info, const char* tmpFilename, uint32_t numThreads, uint32_t numSlots, bf_sens_recorder** out) {
    return guarded([&]() -> int {
    BF_REQUIRE(info && tmpFilename && tmpFilename[0] && out, "null argument");
    BF_REQUIRE(numThreads <= 12, "at most 12 encode threads");
    BF_REQUIRE(numSlots == 0 || numSlots >= 2, "at least 2 slots");
    BF_REQUIRE(numSlots <= 1024, "at most 1024 slots");
    if (numThreads == 0) numThreads = 4;
    if (numSlots == 0) numSlots = 4;
    BF_REQUIRE(info->colorCompressionType == BF_SENS_COLOR_JPEG, "a recording's colour is JPEG");
    BF_REQUIRE(info->depthCompressionType == BF_SENS_DEPTH_RAW_USHORT || info->depthCompressionType == BF_SENS_DEPTH_ZLIB_USHORT, "depth compression must be raw or zlib u16");
    BF_REQUIRE(info->depthWidth > 0 && info->depthHeight > 0 && info->colorWidth > 0 && info->colorHeight > 0 && info->colorWidth < 65536 && info->colorHeight < 65536 &&
                   info->depthShift > 0.0f && std::isfinite(info->depthShift), "bad image geometry");
    BF_REQUIRE((uint64_t)info->depthWidth * info->depthHeight < 0xFFFFF000ull, "depth image too large");
    {   // the temporary file must be writable now, not at the first frame's append
        FILE* f = fopen(tmpFilename, "wb");
        if (!f) { set_error("could not open file %s for writing", tmpFilename); return BF_ERR_INVALID_ARG; }
        fclose(f);
    }
    bf_sens_recorder* r = new bf_sens_recorder;
    bf::CreateGuard<bf_sens_recorder> guard(r, bf_sens_recorder_destroy);
    r->info = *info; r->info.numFrames = 0; r->info.numIMUFrames = 0; r->tmp = tmpFilename; r->pinned = pipeline != nullptr;
    r->coefCount = (size_t)((info->colorWidth + 7) / 8) * ((info->colorHeight + 7) / 8) * 192;
    r->depthCount = (size_t)info->depthWidth * info->depthHeight;
    r->slots.resize(numSlots);
    if (r->pinned) {
        BF_HIP_TRY(hipGetDevice(&r->device));
        hipStream_t copy = nullptr;
        BF_HIP_TRY(hipStreamCreateWithFlags(&copy, hipStreamNonBlocking));
        BF_TRY(r->res.adopt(copy));
        r->copyStream = copy;
        for (bf_sens_recorder::Slot& s : r->slots) {
            BF_TRY(r->res.pinned(&s.coef, r->coefCount * 2)); BF_TRY(r->res.pinned(&s.depth, r->depthCount * 2));
            BF_TRY(r->res.device(&s.d_coef, r->coefCount)); BF_TRY(r->res.device(&s.d_depth, r->depthCount));
            BF_TRY(r->res.event(&s.packed, hipEventDisableTiming)); BF_TRY(r->res.event(&s.copied, hipEventDisableTiming));
        }
    } else {
        for (bf_sens_recorder::Slot& s : r->slots) {
            s.coef = (int16_t*)malloc(r->coefCount * 2); s.depth = (uint16_t*)malloc(r->depthCount * 2);
            if (!s.coef || !s.depth) throw std::bad_alloc();
        }
    }
    for (uint32_t t = 0; t < numThreads; ++t) r->threads.emplace_back(recWorker, r);
    *out = guard.dismiss();
    return BF_OK;
    });
}

int bf_sens_recorder_record_host(bf_sens_recorder* r, const uint8_t* rgbx, const float* depthFloat) {
    BF_REQUIRE(r && rgbx && depthFloat, "null argument");
    bf_sens_recorder::Slot* s = nullptr;
    BF_TRY(recAcquire(r, &s));
    const bf_sensor_data_info& h = r->info;
    const int rc = bf_jpeg_forward_host(rgbx, 4, h.colorWidth, h.colorHeight, RECORD_JPEG_QUALITY, s->coef, r->coefCount);
    if (rc == BF_OK) {
        const float shift = h.depthShift;
        for (size_t i = 0; i < r->depthCount; ++i) {
            const float v = depthFloat[i] * shift;                            // (unsigned short) round(m_depthShift * d[i]), RGBDSensor.cpp:305
            s->depth[i] = (v > 0.0f && v < 65535.5f) ? (uint16_t)(v + 0.5f) : (uint16_t)0;
        }
        s->onDevice = false;
    }
    recSubmit(r, s, rc == BF_OK);
    return rc;
}

int bf_sens_recorder_record_device(bf_sens_recorder* r, const float* d_depthFloat, const uint8_t* d_rgbx, void* stream) {
    BF_REQUIRE(r && d_depthFloat && d_rgbx, "null argument");
    if (!r->pinned) { set_error("bf_sens_recorder_record_device: the recorder was created without a pipeline (host frames only)"); return BF_ERR_STATE; }
    bf_sens_recorder::Slot* s = nullptr;
    BF_TRY(recAcquire(r, &s));
    const bf_sensor_data_info& h = r->info;
    hipStream_t st = (hipStream_t)stream;
    int rc = bf_image_convert_depth_to_u16(s->d_depth, d_depthFloat, h.depthShift, (uint32_t)r->depthCount, st);
    if (rc == BF_OK) rc = bf_jpeg_forward_device(d_rgbx, h.colorWidth, h.colorHeight, RECORD_JPEG_QUALITY, s->d_coef, st);
    if (rc == BF_OK) {
        const bool ok = hipEventRecord(s->packed, st) == hipSuccess && hipStreamWaitEvent(r->copyStream, s->packed, 0) == hipSuccess &&
                        hipMemcpyAsync(s->depth, s->d_depth, r->depthCount * 2, hipMemcpyDeviceToHost, r->copyStream) == hipSuccess &&
                        hipMemcpyAsync(s->coef, s->d_coef, r->coefCount * 2, hipMemcpyDeviceToHost, r->copyStream) == hipSuccess &&
                        hipEventRecord(s->copied, r->copyStream) == hipSuccess;
        if (!ok) { set_error("bf_sens_recorder_record_device: %s", hipGetErrorString(hipGetLastError())); rc = BF_ERR_HIP; }
        s->onDevice = true;
    }
    recSubmit(r, s, rc == BF_OK);
    return rc;
}

int bf_sens_recorder_get_num_recorded(bf_sens_recorder* r, uint64_t* numFrames) {
    BF_REQUIRE(r && numFrames, "null argument");
    std::lock_guard<std::mutex> lk(r->m);
    *numFrames = r->nextRecord;
    return BF_OK;
}

int bf_sens_recorder_finish(bf_sens_recorder* r, const char* filename, const float* trajectory, uint64_t numTransforms, int overwrite, char* actualName, uint64_t capacity,
                            uint64_t* numFramesWritten) {
    return guarded([&]() -> int {
    BF_REQUIRE(r && filename && filename[0] && (trajectory || numTransforms == 0), "null argument");
    if (numFramesWritten) *numFramesWritten = 0;
    if (actualName && capacity) actualName[0] = 0;
    uint64_t recorded = 0;
    int wrc = BF_OK; std::string werr;
    {
        std::unique_lock<std::mutex> lk(r->m);
        r->cvFree.wait(lk, [&] { return r->nextAppend == r->nextRecord; });      // the ring is drained: no worker touches the writer any more
        recorded = r->nextRecord; wrc = r->rc; werr = r->err;
        r->nextRecord = r->nextClaim = r->nextAppend = 0; r->rc = BF_OK; r->err.clear();          // the recorder starts over, whatever happens below
    }
    int rc = BF_OK;
    if (r->writer) { rc = bf_sensor_data_writer_close(r->writer); r->writer = nullptr; }
    if (wrc) { std::remove(r->tmp.c_str()); set_error("%s", werr.c_str()); return wrc; }
    if (rc) { std::remove(r->tmp.c_str()); return rc; }
    if (recorded == 0 || numTransforms == 0) { std::remove(r->tmp.c_str()); return BF_OK; }
    std::string actual = filename;
    if (!overwrite) {                                                             // RGBDSensor.cpp:382-396
        const size_t dot = actual.find_last_of('.');
        const std::string base = dot == std::string::npos ? actual : actual.substr(0, dot), ext = dot == std::string::npos ? "" : actual.substr(dot);
        for (unsigned int num = 1; fileExists(actual); ++num) actual = base + std::to_string(num) + ext;
    }
    bf_sensor_data* sd = nullptr;
    rc = bf_sensor_data_open(r->tmp.c_str(), &sd);
    if (rc == BF_OK) {
        rc = bf_sensor_data_save_recorded(sd, actual.c_str(), trajectory, numTransforms);
        bf_sensor_data_close(sd);
    }
    std::remove(r->tmp.c_str());
    if (rc) return rc;
    if (actualName && capacity) snprintf(actualName, (size_t)capacity, "%s", actual.c_str());
    if (numFramesWritten) *numFramesWritten = numTransforms;
    return BF_OK;
    });
}

}  // extern "C"
