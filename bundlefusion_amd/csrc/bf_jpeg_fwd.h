// The forward half of the baseline JPEG encoder (everything in front of the entropy coder), written once for the host
// (imagecodec.cpp: bf_jpeg_forward_host) and the device (sensorrecord.hip: bf_jpeg_forward_device): colour conversion, the
// direct-form 8-point DCT-II in two passes (rows, then columns), quantisation.
//
// This is binary32 arithmetic, and the ORDER OF OPERATIONS IS THE DEFINITION: one IEEE rounding per written operation, sums
// evaluated left to right, no fused multiply-add (the library is built with -ffp-contract=off), IEEE division.  Host and device
// then give the same int16 coefficients, and the two are compared as bytes.  The 64 cosine factors are computed on the host only
// (cosTable: (float)std::cos(double), the expression the encoder has always used) and reach the device as data.
#pragma once
#include <stdint.h>

#include <cmath>

#if defined(__HIPCC__)
#define BF_JFHD __host__ __device__ inline
#else
#define BF_JFHD inline
#endif

namespace bfjpegfwd {

// RGB -> level-shifted Y, Cb, Cr
BF_JFHD void rgbToYcc(float r, float g, float b, float& y, float& cb, float& cr) {
    y = 0.299f * r + 0.587f * g + 0.114f * b - 128.0f;
    cb = -0.168736f * r - 0.331264f * g + 0.5f * b;
    cr = 0.5f * r - 0.418688f * g - 0.081312f * b;
}

// one output of one pass: factors C[k][0..7] (ck) against the eight samples of a row or column
BF_JFHD float dct1(const float* ck, const float* x) {
    float s = 0;
    for (int n = 0; n < 8; ++n) s += ck[n] * x[n];
    return s;
}

// transformed value / quantisation step, rounded half away from zero
BF_JFHD int16_t quantise(float t, float q) {
    const float v = t / q;
    return (int16_t)(v < 0 ? -(int)(-v + 0.5f) : (int)(v + 0.5f));
}

// C[k][n] of the orthonormal DCT-II, row-major; host only
inline void cosTable(float C[64]) {
    for (int k = 0; k < 8; ++k)
        for (int n = 0; n < 8; ++n) C[k * 8 + n] = (k == 0 ? 0.35355339059327373f : 0.5f) * (float)std::cos((2 * n + 1) * k * 3.14159265358979323846 / 16.0);
}

// the tables of Annex K scaled by `quality` (1..100, clamped) like the IJG code; natural order; q[0] luma, q[1] chroma
inline void quantTables(int quality, uint8_t q[2][64]) {
    static const uint8_t STD_LUMA_Q[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                                           18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
    static const uint8_t STD_CHROMA_Q[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                             99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
    quality = quality < 1 ? 1 : (quality > 100 ? 100 : quality);
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int i = 0; i < 64; ++i) {
        const int a = ((int)STD_LUMA_Q[i] * scale + 50) / 100, b = ((int)STD_CHROMA_Q[i] * scale + 50) / 100;
        q[0][i] = (uint8_t)(a < 1 ? 1 : (a > 255 ? 255 : a)); q[1][i] = (uint8_t)(b < 1 ? 1 : (b > 255 ? 255 : b));
    }
}

// natural (row-major) position of the i-th coefficient in zigzag order
static const uint8_t ZIGZAG[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

}  // namespace bfjpegfwd
