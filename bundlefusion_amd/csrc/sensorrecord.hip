// A frame packed for a recording on the device (gfx950): the two conversions RGBDSensor::recordFrame (RGBDSensor.cpp:264-312) does on the host before
// the entropy coder and zlib take over - the mirror image of sensoringest.hip.
//   k_depth_to_u16     metres -> u16 (the rule of :305): eight pixels per lane, two 16-byte loads and one 16-byte store; the tail and
//                      unaligned buffers go pixel by pixel, so not a byte behind the array is touched
//   k_jpeg_forward     RGBX8 -> quantised DCT coefficients in zigzag order (bf_jpeg_forward_host's layout and bytes).  A workgroup of 256 lanes
//                      takes 32 blocks that are consecutive in raster order of the block grid, so its output is one contiguous run of 12 288 bytes:
//                        row pass     lane = (block b = lane % 32, row r = lane / 32): eight pixels (two 16-byte loads where the block lies inside an image
//                                     whose rows are 16-byte aligned; consecutive lanes read consecutive 32-byte pieces of one image row), colour
//                                     conversion, 3 x 8 row results to LDS
//                        column pass  lane = (block b = lane / 8, column c = lane % 8): eight row results per component from LDS, transform, quantise,
//                                     the int16 to its zigzag position in a second LDS array
//                        copy out     768 16-byte stores per workgroup, three per lane
// The arithmetic is bf_jpeg_fwd.h's (binary32, one rounding per operation, IEEE division, no FMA: the library's flags), so the result is compared
// with the host's as bytes.  The cosine factors and the quantisation tables come from the host in the kernel arguments.
//
// LDS layout of the row results, per component: word (n * 8 + k) * 36 + b for row n, frequency k, block b (ds_write_b32 / ds_read_b32: bank = dword % 32,
// conflicts within each half of the wave).  Row pass, one store: a half wave holds b = 0..31 at one (n, k) -> banks 4 (n * 8 + k) + b, all different.
// Column pass, one load: a half wave holds four consecutive blocks (b0 a multiple of 4) x eight columns at one n -> banks 4 c + (b - b0) + const, all different.
#include <hip/hip_runtime.h>

#include "bf_device.h"
#include "bf_internal.h"
#include "bf_jpeg_fwd.h"

using namespace bf;

namespace {

__global__ __launch_bounds__(256) void k_depth_to_u16(uint16_t* __restrict__ out, const float* __restrict__ in, float shift, uint32_t n, int aligned) {
    const uint32_t first = (blockIdx.x * 256u + threadIdx.x) * 8u;
    if (first >= n) return;
    float d[8];
    const bool whole = aligned && n - first >= 8u;
    const uint32_t cnt = whole ? 8u : (n - first < 8u ? n - first : 8u);
    if (whole) {
        const float4 a = *reinterpret_cast<const float4*>(in + first), b = *reinterpret_cast<const float4*>(in + first + 4);
        d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w; d[4] = b.x; d[5] = b.y; d[6] = b.z; d[7] = b.w;
    } else {
        for (uint32_t j = 0; j < 8; ++j) d[j] = j < cnt ? in[first + j] : 0.0f;
    }
    uint32_t q[8];
    for (int j = 0; j < 8; ++j) {
        const float v = d[j] * shift;
        q[j] = (v > 0.0f && v < 65535.5f) ? (uint32_t)(v + 0.5f) : 0u;
    }
    if (whole) {
        *reinterpret_cast<uint4*>(out + first) = make_uint4(q[0] | q[1] << 16, q[2] | q[3] << 16, q[4] | q[5] << 16, q[6] | q[7] << 16);
    } else {
        for (uint32_t j = 0; j < 8; ++j) if (j < cnt) out[first + j] = (uint16_t)q[j];
    }
}

struct FwdArgs {
    int width, height, blocksX;
    uint32_t numBlocks;
    int vector;                       // rows of the image are 16-byte aligned: blocks inside the image are read with 16-byte loads
    float C[64];                      // C[k][n], bfjpegfwd::cosTable
    float q[2][64];                   // quantisation steps, natural order; [0] luma, [1] chroma
    uint8_t zz[64];                   // zigzag position of natural position i
};

constexpr int FWD_BLOCKS = 32;        // 256 lanes / 8
constexpr int FWD_STRIDE = 36;        // words between (n, k) planes of the row results, see the head of the file
constexpr int FWD_COMP = 64 * FWD_STRIDE;

__global__ __launch_bounds__(256) void k_jpeg_forward(int16_t* __restrict__ coef, const uint8_t* __restrict__ rgbx, FwdArgs A) {
    __shared__ float ws[3 * FWD_COMP];                                  // 27 648 bytes
    __shared__ __attribute__((aligned(16))) int16_t zq[FWD_BLOCKS * 192];      // 12 288 bytes: the workgroup's output
    const uint32_t group0 = blockIdx.x * (uint32_t)FWD_BLOCKS;
    {   // ---- row pass
        const int b = threadIdx.x & 31, r = threadIdx.x >> 5;
        const uint32_t block = group0 + (uint32_t)b;
        if (block < A.numBlocks) {
            const int y0 = (int)(block / (uint32_t)A.blocksX), x0 = (int)(block - (uint32_t)y0 * (uint32_t)A.blocksX);
            const int y = min(y0 * 8 + r, A.height - 1);
            const uint32_t* row = reinterpret_cast<const uint32_t*>(rgbx) + (size_t)y * A.width;
            uint32_t px[8];
            if (A.vector && x0 * 8 + 8 <= A.width) {
                const uint4 a = *reinterpret_cast<const uint4*>(row + x0 * 8), c = *reinterpret_cast<const uint4*>(row + x0 * 8 + 4);
                px[0] = a.x; px[1] = a.y; px[2] = a.z; px[3] = a.w; px[4] = c.x; px[5] = c.y; px[6] = c.z; px[7] = c.w;
            } else {
                for (int j = 0; j < 8; ++j) px[j] = row[min(x0 * 8 + j, A.width - 1)];      // edge replication
            }
            float Y[8], Cb[8], Cr[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) bfjpegfwd::rgbToYcc((float)(px[j] & 255u), (float)((px[j] >> 8) & 255u), (float)((px[j] >> 16) & 255u), Y[j], Cb[j], Cr[j]);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int w = (r * 8 + k) * FWD_STRIDE + b;
                ws[w] = bfjpegfwd::dct1(A.C + k * 8, Y);
                ws[FWD_COMP + w] = bfjpegfwd::dct1(A.C + k * 8, Cb);
                ws[2 * FWD_COMP + w] = bfjpegfwd::dct1(A.C + k * 8, Cr);
            }
        }
    }
    __syncthreads();
    {   // ---- column pass
        const int b = threadIdx.x >> 3, c = threadIdx.x & 7;
        if (group0 + (uint32_t)b < A.numBlocks) {
            for (int comp = 0; comp < 3; ++comp) {
                float x[8];
#pragma unroll
                for (int n = 0; n < 8; ++n) x[n] = ws[comp * FWD_COMP + (n * 8 + c) * FWD_STRIDE + b];
                const float* q = A.q[comp ? 1 : 0];
#pragma unroll
                for (int k = 0; k < 8; ++k) zq[(b * 3 + comp) * 64 + A.zz[k * 8 + c]] = bfjpegfwd::quantise(bfjpegfwd::dct1(A.C + k * 8, x), q[k * 8 + c]);
            }
        }
    }
    __syncthreads();
    {   // ---- copy out: 24 16-byte pieces per block
        const uint32_t live = min((uint32_t)FWD_BLOCKS, A.numBlocks - group0);
        uint4* dst = reinterpret_cast<uint4*>(coef + (size_t)group0 * 192);
        const uint4* src = reinterpret_cast<const uint4*>(zq);
        for (uint32_t i = threadIdx.x; i < live * 24u; i += 256u) dst[i] = src[i];
    }
}

}  // namespace

extern "C" {

int bf_image_convert_depth_to_u16(uint16_t* d_output, const float* d_input, float depthShift, uint32_t n, void* stream) {
    BF_REQUIRE(d_output && d_input && n > 0 && n < 0xFFFFF000u, "bad argument");            // (the lanes' first pixel is a 32-bit index)
    BF_REQUIRE(((uintptr_t)d_output & 1) == 0 && ((uintptr_t)d_input & 3) == 0, "misaligned buffer");
    const int aligned = (((uintptr_t)d_output | (uintptr_t)d_input) & 15) == 0;
    k_depth_to_u16<<<div_up(div_up(n, 8), 256), 256, 0, (hipStream_t)stream>>>(d_output, d_input, depthShift, n, aligned);
    BF_HIP_TRY(hipGetLastError());
    return BF_OK;
}

int bf_jpeg_forward_device(const uint8_t* d_rgbx, uint32_t width, uint32_t height, int32_t quality, int16_t* d_coefficients, void* stream) {
    BF_REQUIRE(d_rgbx && d_coefficients && width > 0 && height > 0 && width < 65536 && height < 65536, "bad argument");
    BF_REQUIRE(((uintptr_t)d_rgbx & 3) == 0 && ((uintptr_t)d_coefficients & 15) == 0, "d_rgbx must be 4-byte aligned and d_coefficients 16-byte aligned");
    FwdArgs A;
    memset(&A, 0, sizeof A);
    A.width = (int)width; A.height = (int)height; A.blocksX = (int)((width + 7) / 8);
    A.numBlocks = (uint32_t)A.blocksX * ((height + 7) / 8);                       // < 2^26
    A.vector = ((uintptr_t)d_rgbx & 15) == 0 && (width & 3) == 0;
    struct Cos { float c[64]; Cos() { bfjpegfwd::cosTable(c); } };
    static const Cos cosines;                                                     // the host's (float)std::cos(double), once; the device evaluates no cosine
    memcpy(A.C, cosines.c, sizeof A.C);
    uint8_t q[2][64];
    bfjpegfwd::quantTables(quality, q);
    for (int i = 0; i < 64; ++i) { A.q[0][i] = (float)q[0][i]; A.q[1][i] = (float)q[1][i]; A.zz[bfjpegfwd::ZIGZAG[i]] = (uint8_t)i; }
    k_jpeg_forward<<<div_up(A.numBlocks, FWD_BLOCKS), 256, 0, (hipStream_t)stream>>>(d_coefficients, d_rgbx, A);
    BF_HIP_TRY(hipGetLastError());
    return BF_OK;
}

}  // extern "C"
