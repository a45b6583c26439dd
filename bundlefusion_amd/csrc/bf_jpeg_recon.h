// The reconstruction half of the baseline JPEG decoder (everything behind the entropy decode), written once for the host
// (imagecodec.cpp) and the device (sensoringest.hip): IJG "islow" inverse DCT, triangle ("fancy") chroma up-sampling, 16-bit
// fixed-point YCbCr -> RGB.  Integer arithmetic only, so both sides give the same bytes.
//
// Width of the intermediates.  A coefficient is an int16 and a quantisation step at most 65535 (16-bit tables), so a dequantised
// value needs 32 bits (32767 * 65535 < 2^31).  The first butterfly multiplies sums of four such values by 13-bit constants: 2^33 * 2^15
// does not fit 32 bits, and a hostile stream reaches that range.  The host code has always used 64-bit intermediates; so does the
// device (the pass is bound by memory, not by the multiplier).  The workspace between the passes is the host's `int`.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define BF_JHD __host__ __device__ inline
#else
#define BF_JHD inline
#endif

namespace bfjpeg {

BF_JHD uint8_t clamp8(int v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }
BF_JHD int descale(int64_t x, int n) { return (int)((x + ((int64_t)1 << (n - 1))) >> n); }

constexpr int CONST_BITS = 13, PASS1_BITS = 2;

// the 8-point LL&M butterfly of jidctint.c, before the descale: y[k] is output sample k of the 1-D transform of x[0..7]
BF_JHD void butterfly(const int64_t x[8], int64_t y[8]) {
    const int64_t F0298 = 2446, F0390 = 3196, F0541 = 4433, F0765 = 6270, F0899 = 7373, F1175 = 9633, F1501 = 12299, F1847 = 15137, F1961 = 16069,
                  F2053 = 16819, F2562 = 20995, F3072 = 25172;
    int64_t z2 = x[2], z3 = x[6];
    int64_t z1 = (z2 + z3) * F0541;
    int64_t tmp2 = z1 + z3 * (-F1847), tmp3 = z1 + z2 * F0765;
    z2 = x[0]; z3 = x[4];
    int64_t tmp0 = (z2 + z3) * (1 << CONST_BITS), tmp1 = (z2 - z3) * (1 << CONST_BITS);
    const int64_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = x[7]; tmp1 = x[5]; tmp2 = x[3]; tmp3 = x[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    int64_t z4 = tmp1 + tmp3;
    const int64_t z5 = (z3 + z4) * F1175;
    tmp0 *= F0298; tmp1 *= F2053; tmp2 *= F3072; tmp3 *= F1501;
    z1 *= -F0899; z2 *= -F2562; z3 *= -F1961; z4 *= -F0390;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    y[0] = tmp10 + tmp3; y[7] = tmp10 - tmp3;
    y[1] = tmp11 + tmp2; y[6] = tmp11 - tmp2;
    y[2] = tmp12 + tmp1; y[5] = tmp12 - tmp1;
    y[3] = tmp13 + tmp0; y[4] = tmp13 - tmp0;
}

// pass 1 on one column of dequantised coefficients -> the column of the workspace (ws[r * wsStride])
BF_JHD void idctColumn(const int64_t x[8], int* ws, int wsStride) {
    int64_t y[8];
    butterfly(x, y);
    for (int r = 0; r < 8; ++r) ws[r * wsStride] = descale(y[r], CONST_BITS - PASS1_BITS);
}

// pass 2 on one row of the workspace -> 8 samples
BF_JHD void idctRow(const int* w, uint8_t out[8]) {
    int64_t x[8], y[8];
    for (int k = 0; k < 8; ++k) x[k] = w[k];
    butterfly(x, y);
    for (int k = 0; k < 8; ++k) out[k] = clamp8(descale(y[k], CONST_BITS + PASS1_BITS + 3) + 128);
}

// One sample of a chroma plane brought to full resolution (h2v1_fancy_upsample / h2v2_fancy_upsample of jdsample.c).  p: the plane
// (row stride pw), sw x sh: its part that covers the image, fh / fv: the up-sampling factors (1x1, 2x1, 2x2; 1x2 replicates rows).
BF_JHD int chromaAt(const uint8_t* p, int pw, int sw, int sh, int fh, int fv, int x, int y) {
    if (fh == 1) return p[(size_t)(fv == 2 ? y >> 1 : y) * pw + x];
    const int i = x >> 1, odd = x & 1;
    if (fv == 1) {
        const uint8_t* in = p + (size_t)y * pw;
        if (odd) return i == sw - 1 ? in[i] : (in[i] * 3 + in[i + 1] + 2) >> 2;
        return i == 0 ? in[0] : (in[i] * 3 + in[i - 1] + 1) >> 2;
    }
    const int ys = y >> 1;
    const uint8_t* near = p + (size_t)ys * pw;
    const uint8_t* far = p + (size_t)((y & 1) ? (ys < sh - 1 ? ys + 1 : sh - 1) : (ys > 0 ? ys - 1 : 0)) * pw;
    const int c = near[i] * 3 + far[i];
    if (odd) {
        if (i == sw - 1) return (c * 4 + (sw == 1 ? 8 : 7)) >> 4;
        return (c * 3 + (near[i + 1] * 3 + far[i + 1]) + 7) >> 4;
    }
    if (i == 0) return (c * 4 + 8) >> 4;
    return (c * 3 + (near[i - 1] * 3 + far[i - 1]) + 8) >> 4;
}

// jdcolor.c build_ycc_rgb_table: 16-bit fixed point
BF_JHD void yccToRgb(int Y, int cbRaw, int crRaw, uint8_t* o) {
    const int cb = cbRaw - 128, cr = crRaw - 128;
    o[0] = clamp8(Y + ((91881 * cr + 32768) >> 16));
    o[1] = clamp8(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    o[2] = clamp8(Y + ((116130 * cb + 32768) >> 16));
}

}  // namespace bfjpeg
