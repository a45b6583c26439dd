// Sensor-format frames on the device (gfx950): what SensorDataReader::processDepth (SensorDataReader.cpp:98-111) and the reconstruction
// half of the colour decoder (imagecodec.cpp) do on one host thread, as kernels on the ingest stream.
//   k_depth_u16        u16 -> metres, 0 -> -inf, one IEEE division per pixel (no reciprocal: the bytes of bf_sensor_data_read_depth)
//   k_rgb8_to_rgbx     RGB8 -> RGBX8, X = 255
//   k_jpeg_idct        quantised int16 coefficients -> the components' 8-bit sample planes: dequantise + islow inverse DCT.  A workgroup
//                      of 256 lanes takes 32 blocks: one lane per (block, column) for the first pass, then one lane per (block, row) for the
//                      second, the 8x8 `int` workspace of each block in LDS in between.
//   k_jpeg_to_rgbx     planes -> RGBX8: per pixel the triangle-filtered chroma samples and the fixed-point colour conversion
// All of it is integer arithmetic shared with the host through bf_jpeg_recon.h, so the results are compared as bytes.  Streaming passes
// over ~1 MB in and ~1.2 MB out per VGA frame: a few microseconds each, far below the frame loop's other stages.
#include <hip/hip_runtime.h>

#include "bf_device.h"
#include "bf_internal.h"
#include "bf_jpeg_recon.h"

using namespace bf;

namespace {

__global__ __launch_bounds__(256) void k_depth_u16(float* __restrict__ out, const uint16_t* __restrict__ in, float shift, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint16_t r = in[i];
    out[i] = r == 0 ? BF_MINF : (float)r / shift;
}

__global__ __launch_bounds__(256) void k_rgb8_to_rgbx(uint32_t* __restrict__ out, const uint8_t* __restrict__ in, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint8_t* p = in + (size_t)i * 3;
    out[i] = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | 0xFF000000u;
}

// what the kernels need of bf_jpeg_info, by value
struct JpegDev {
    int width, height, numComponents;
    int blocksX[3], blockOffset[3], planeOffset[3], tq[3];
    int sw[3], sh[3], fh[3], fv[3];       // chroma: covering size of the plane and up-sampling factors
    int numBlocks;
    uint16_t qt[4][64];                   // natural order (read per lane from the kernel-argument segment, like the filters' tap tables)
};

constexpr int BLOCKS_PER_GROUP = 32;      // 256 lanes / 8
// Workspace rows are 9 ints apart and blocks 72: in the column pass the 32 lanes of a half wave (4 blocks x 8 columns) write banks 8 b + c (+ 9 r),
// in the row pass (4 blocks x 8 rows) they read banks 8 b + 9 r + k - all 32 different both times (ds_read_b32 / ds_write_b32: bank = dword % 32).
constexpr int WS_ROW = 9, WS_BLOCK = 72;

__global__ __launch_bounds__(256) void k_jpeg_idct(uint8_t* __restrict__ planes, const int16_t* __restrict__ coef, JpegDev J) {
    __shared__ int ws[BLOCKS_PER_GROUP * WS_BLOCK];
    const int lb = threadIdx.x >> 3, k = threadIdx.x & 7;
    const int block = blockIdx.x * BLOCKS_PER_GROUP + lb;
    const bool live = block < J.numBlocks;
    int ci = 0;
    if (J.numComponents == 3) ci = block >= J.blockOffset[2] ? 2 : (block >= J.blockOffset[1] ? 1 : 0);
    if (live) {                                        // pass 1: column k of the block
        const int16_t* ip = coef + (size_t)block * 64 + k;
        const uint16_t* q = J.qt[J.tq[ci]] + k;
        int64_t x[8];
        for (int r = 0; r < 8; ++r) x[r] = (int)ip[8 * r] * (int)q[8 * r];
        bfjpeg::idctColumn(x, ws + lb * WS_BLOCK + k, WS_ROW);
    }
    __syncthreads();
    if (live) {                                        // pass 2: row k of the block, 8 samples = one 8-byte store
        union { uint8_t b[8]; uint2 v; } o;
        bfjpeg::idctRow(ws + lb * WS_BLOCK + k * WS_ROW, o.b);
        const int inComp = block - J.blockOffset[ci];
        const int by = inComp / J.blocksX[ci], bx = inComp - by * J.blocksX[ci];
        *reinterpret_cast<uint2*>(planes + J.planeOffset[ci] + ((size_t)(by * 8 + k) * J.blocksX[ci] + bx) * 8) = o.v;
    }
}

__global__ __launch_bounds__(256) void k_jpeg_to_rgbx(uint32_t* __restrict__ out, const uint8_t* __restrict__ planes, JpegDev J) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= J.width || y >= J.height) return;
    const int Y = planes[J.planeOffset[0] + (size_t)y * (J.blocksX[0] * 8) + x];
    uint8_t c[3] = {(uint8_t)Y, (uint8_t)Y, (uint8_t)Y};
    if (J.numComponents == 3) {
        const int cb = bfjpeg::chromaAt(planes + J.planeOffset[1], J.blocksX[1] * 8, J.sw[1], J.sh[1], J.fh[1], J.fv[1], x, y);
        const int cr = bfjpeg::chromaAt(planes + J.planeOffset[2], J.blocksX[2] * 8, J.sw[2], J.sh[2], J.fh[2], J.fv[2], x, y);
        bfjpeg::yccToRgb(Y, cb, cr, c);
    }
    out[(size_t)y * J.width + x] = (uint32_t)c[0] | (uint32_t)c[1] << 8 | (uint32_t)c[2] << 16 | 0xFF000000u;
}

}  // namespace

namespace bf {

// the layouts bf_jpeg_reconstruct_device takes (bf_internal.h)
bool jpeg_on_device(const bf_jpeg_info& I) {
    if (I.numComponents == 1) return true;
    if (I.numComponents != 3 || I.comp[0].h != I.hmax || I.comp[0].v != I.vmax) return false;
    for (int ci = 1; ci < 3; ++ci) {
        const uint32_t fh = I.hmax / I.comp[ci].h, fv = I.vmax / I.comp[ci].v;
        if (!((fh == 1 && fv == 1) || (fh == 2 && fv == 1) || (fh == 2 && fv == 2))) return false;
    }
    return true;
}

}  // namespace bf

extern "C" {

int bf_image_convert_depth_u16(float* d_output, const uint16_t* d_input, float depthShift, uint32_t n, void* stream) {
    BF_REQUIRE(d_output && d_input && n > 0, "bad argument");
    k_depth_u16<<<div_up(n, 256), 256, 0, (hipStream_t)stream>>>(d_output, d_input, depthShift, n);
    BF_HIP_TRY(hipGetLastError());
    return BF_OK;
}

int bf_image_convert_rgb8_to_rgbx(uint8_t* d_output, const uint8_t* d_input, uint32_t n, void* stream) {
    BF_REQUIRE(d_output && d_input && n > 0, "bad argument");
    k_rgb8_to_rgbx<<<div_up(n, 256), 256, 0, (hipStream_t)stream>>>((uint32_t*)d_output, d_input, n);
    BF_HIP_TRY(hipGetLastError());
    return BF_OK;
}

int bf_jpeg_reconstruct_device(const bf_jpeg_info* info, const int16_t* d_coefficients, uint8_t* d_planes, uint8_t* d_rgbxOut, void* stream) {
    BF_REQUIRE(info && d_coefficients && d_planes && d_rgbxOut, "null argument");
    const bf_jpeg_info& I = *info;
    BF_REQUIRE((I.numComponents == 1 || I.numComponents == 3) && I.width > 0 && I.height > 0 && I.width < 65536 && I.height < 65536 && I.hmax >= 1 && I.hmax <= 2 &&
                   I.vmax >= 1 && I.vmax <= 2, "bad description");
    // the description is the caller's: every offset the kernels use is re-derived from the sizes here, and compared
    uint32_t blocks = 0;
    for (uint32_t ci = 0; ci < I.numComponents; ++ci) {
        const bf_jpeg_component& c = I.comp[ci];
        BF_REQUIRE(c.h >= 1 && c.h <= I.hmax && c.v >= 1 && c.v <= I.vmax && c.tq < 4 && I.qtPresent[c.tq], "bad component");
        BF_REQUIRE(c.blocksX == I.mcusX * c.h && c.blocksY == I.mcusY * c.v && c.blockOffset == blocks && c.planeOffset == blocks * 64, "bad block layout");
        blocks += c.blocksX * c.blocksY;
    }
    BF_REQUIRE(I.mcusX == (I.width + 8 * I.hmax - 1) / (8 * I.hmax) && I.mcusY == (I.height + 8 * I.vmax - 1) / (8 * I.vmax) && blocks == I.numBlocks &&
                   I.planeBytes == blocks * 64, "bad block layout");
    if (!jpeg_on_device(I)) { set_error("jpeg: this sampling layout is reconstructed on the host only"); return BF_ERR_NOT_ON_DEVICE; }
    JpegDev J;
    memset(&J, 0, sizeof J);
    J.width = (int)I.width; J.height = (int)I.height; J.numComponents = (int)I.numComponents; J.numBlocks = (int)I.numBlocks;
    for (uint32_t ci = 0; ci < I.numComponents; ++ci) {
        const bf_jpeg_component& c = I.comp[ci];
        J.blocksX[ci] = (int)c.blocksX; J.blockOffset[ci] = (int)c.blockOffset; J.planeOffset[ci] = (int)c.planeOffset; J.tq[ci] = (int)c.tq;
        J.fh[ci] = (int)(I.hmax / c.h); J.fv[ci] = (int)(I.vmax / c.v);
        J.sw[ci] = (int)((I.width * c.h + I.hmax - 1) / I.hmax); J.sh[ci] = (int)((I.height * c.v + I.vmax - 1) / I.vmax);
    }
    memcpy(J.qt, I.qt, sizeof J.qt);
    hipStream_t st = (hipStream_t)stream;
    k_jpeg_idct<<<div_up(I.numBlocks, BLOCKS_PER_GROUP), 256, 0, st>>>(d_planes, d_coefficients, J);
    BF_HIP_TRY(hipGetLastError());
    k_jpeg_to_rgbx<<<dim3(div_up(I.width, 64), div_up(I.height, 4)), dim3(64, 4), 0, st>>>((uint32_t*)d_rgbxOut, d_planes, J);
    BF_HIP_TRY(hipGetLastError());
    return BF_OK;
}

}  // extern "C"
