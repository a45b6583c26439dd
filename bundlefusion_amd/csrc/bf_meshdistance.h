// The distance of an indexed mesh A (the samples) to an indexed mesh B (the surface) on the device (meshdistance.hip): the arithmetic of the definition, shared by
// the kernels and bf_mesh_distance_host, the buffers a bf_marching_cubes object owns for it and the entry point mesh.hip calls.  DESIGN.md "Mesh distance: the
// definition" and include/bf_hip.h state the definition; every function below is one of its sentences.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bf_hip.h"
#include "bf_device.h"
#include "bf_resources.h"

namespace bf {
namespace md {

typedef unsigned long long u64;

constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint32_t MAX_FACES = 300000000u;
constexpr uint32_t MAX_VERTICES = 900000000u;
constexpr uint32_t MAX_N = 1024;                  // subdivisions per edge of one face: at most 2^20 samples per face
constexpr u64 MAX_SAMPLES = 1ull << 28;
constexpr u64 MAX_ENTRIES = 1ull << 27;           // (face, cell) pairs of the grid over B: 512 MiB of uint32
constexpr int WEIGHT_BITS = 6;                    // surface mode: a sample's weight is below 2^6 m^2
constexpr float MAX_D = 64.0f;

// ---- binary64 from the binary32 inputs, one rounding per operation (the library is built without contraction)
BF_HD double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
BF_HD void load3(const float* __restrict__ p, double* o) { o[0] = (double)p[0]; o[1] = (double)p[1]; o[2] = (double)p[2]; }
BF_HD bool valueOk(float x) { return x > -1024.0f && x < 1024.0f; }          // finite and |x| < 1024 (a NaN fails both comparisons)
BF_HD bool finiteButLarge(double x) { return (x >= 1024.0 || x <= -1024.0) && x - x == 0.0; }          // finite and |x| >= 1024 (inf - inf is a NaN)

// the squared length of (b - a) x (c - a); the face is degenerate where it is not in (0, inf)
BF_HD double crossNorm2(const double* a, const double* b, const double* c) {
    double u[3], v[3], n[3];
    for (int d = 0; d < 3; ++d) { u[d] = b[d] - a[d]; v[d] = c[d] - a[d]; }
    n[0] = u[1] * v[2] - u[2] * v[1]; n[1] = u[2] * v[0] - u[0] * v[2]; n[2] = u[0] * v[1] - u[1] * v[0];
    return dot3(n, n);
}
BF_HD bool degenerate(double n2) { return !(n2 > 0.0 && n2 < (double)BF_PINF); }

// the squared distance of p to the closest point of triangle abc: Ericson, Real-Time Collision Detection 5.1.5, the regions in his order
BF_HD double triDist2(const double* p, const double* a, const double* b, const double* c) {
    double ab[3], ac[3], ap[3], bp[3], cp[3], q[3], r[3];
    for (int d = 0; d < 3; ++d) { ab[d] = b[d] - a[d]; ac[d] = c[d] - a[d]; ap[d] = p[d] - a[d]; bp[d] = p[d] - b[d]; cp[d] = p[d] - c[d]; }
    const double d1 = dot3(ab, ap), d2 = dot3(ac, ap), d3 = dot3(ab, bp), d4 = dot3(ac, bp), d5 = dot3(ab, cp), d6 = dot3(ac, cp);
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    if (d1 <= 0.0 && d2 <= 0.0) { for (int d = 0; d < 3; ++d) q[d] = a[d]; }                                        // vertex a
    else if (d3 >= 0.0 && d4 <= d3) { for (int d = 0; d < 3; ++d) q[d] = b[d]; }                                    // vertex b
    else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) { const double t = d1 / (d1 - d3); for (int d = 0; d < 3; ++d) q[d] = a[d] + t * ab[d]; }          // edge ab
    else if (d6 >= 0.0 && d5 <= d6) { for (int d = 0; d < 3; ++d) q[d] = c[d]; }                                    // vertex c
    else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) { const double t = d2 / (d2 - d6); for (int d = 0; d < 3; ++d) q[d] = a[d] + t * ac[d]; }          // edge ac
    else if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {                                                   // edge bc
        const double t = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        for (int d = 0; d < 3; ++d) q[d] = b[d] + t * (c[d] - b[d]);
    } else {                                                                                                        // the face
        const double den = 1.0 / ((va + vb) + vc), v = vb * den, w = vc * den;
        for (int d = 0; d < 3; ++d) q[d] = (a[d] + ab[d] * v) + ac[d] * w;
    }
    for (int d = 0; d < 3; ++d) r[d] = p[d] - q[d];
    return dot3(r, r);
}

// the subdivisions per edge of a non-degenerate face of A in surface mode; 0: above MAX_N (a refusal)
BF_HD uint32_t subdivisions(const double* a, const double* b, const double* c, double spacing) {
    if (!(spacing > 0.0)) return 1u;
    double e0[3], e1[3], e2[3];
    for (int d = 0; d < 3; ++d) { e0[d] = b[d] - a[d]; e1[d] = c[d] - a[d]; e2[d] = c[d] - b[d]; }
    double l2 = dot3(e0, e0);
    const double m1 = dot3(e1, e1), m2 = dot3(e2, e2);
    if (m1 > l2) l2 = m1;
    if (m2 > l2) l2 = m2;
    const double t = __builtin_ceil(__builtin_sqrt(l2) / spacing);
    if (!(t <= (double)MAX_N)) return 0u;
    return t < 1.0 ? 1u : (uint32_t)t;
}
// sample k of the n * n of a face: row j holds 2 (n - j) - 1 sub-triangles and starts at n^2 - (n - j)^2; inside a row upright and inverted ones alternate
BF_HD void sampleOf(const double* a, const double* b, const double* c, uint32_t n, uint32_t k, double* p) {
    const uint32_t m = n * n - k;                             // 1 .. n^2: r = n - j is the least r with r^2 >= m
    uint32_t r = (uint32_t)__builtin_sqrt((double)m);
    while (r * r < m) ++r;
    while (r > 1u && (r - 1u) * (r - 1u) >= m) --r;
    const uint32_t j = n - r, t = k - (n * n - r * r), i = t >> 1, up = (t & 1u) ? 2u : 1u;
    const double u = (double)(3u * i + up) / (double)(3u * n), v = (double)(3u * j + up) / (double)(3u * n);
    for (int d = 0; d < 3; ++d) p[d] = (a[d] + u * (b[d] - a[d])) + v * (c[d] - a[d]);
}
BF_HD double sampleWeight(double n2, uint32_t n) { return (0.5 * __builtin_sqrt(n2)) / (double)(n * n); }

// ---- the sums: q(x) = (int64)floor(x * 2^k + 0.5).  With L the least integer with numSamples <= 2^L, E = 0 in vertex mode and WEIGHT_BITS in surface mode, and e
// the least integer in [-20, 6] with D <= 2^e: kW = 62 - L - E, kWD = kW - e, kWD2 = kW - 2 e.  A term is below 2^E, 2^(E + e), 2^(E + 2 e), so a sum of
// numSamples terms stays below 2^62 + numSamples.
struct Scales { int kW, kWD, kWD2; double sW, sWD, sWD2; };
inline double pow2(int k) { double s = 1.0; for (int i = 0; i < (k < 0 ? -k : k); ++i) s = k < 0 ? s * 0.5 : s * 2.0; return s; }
inline Scales scalesFor(u64 numSamples, int surfaceMode, float D) {
    int L = 0; while ((1ull << L) < numSamples) ++L;
    int e = -20; while (e < 6 && (double)D > pow2(e)) ++e;
    Scales s;
    s.kW = 62 - L - (surfaceMode ? WEIGHT_BITS : 0); s.kWD = s.kW - e; s.kWD2 = s.kW - 2 * e;
    s.sW = pow2(s.kW); s.sWD = pow2(s.kWD); s.sWD2 = pow2(s.kWD2);
    return s;
}
BF_HD long long quant(double x, double scale) { return (long long)__builtin_floor(x * scale + 0.5); }
// the histogram bin of a within-distance: binScale = 1024.0 / (double)D
BF_HD uint32_t binOf(double d, double binScale) { const double t = __builtin_floor(d * binScale); return t >= 1023.0 ? 1023u : (uint32_t)t; }

// ---- the grid (not part of the definition: every result equals the minimum over all faces).  Cell of x: floor(x * inv) per axis, biased by 2^20 into 21 bits.
BF_HD long long cellOf(double x, double inv) { return (long long)__builtin_floor(x * inv); }
BF_HD u64 cellKey(long long x, long long y, long long z) { return (u64)(x + 1048576ll) | (u64)(y + 1048576ll) << 21 | (u64)(z + 1048576ll) << 42; }
// the device grid's cell edge: above D, so that a face within D of a sample is binned in one of the 27 cells around it, with 2^-10 of slack for the roundings
// of the cell indices; at least 2^-9, so that |index| stays below 2^20
inline double deviceCell(float D) { const double h = (double)D > 0.001953125 ? (double)D : 0.001953125; return h * 1.0009765625; }
// whether the plane of a face may cross the cell (ix, iy, iz) of edge h (conservative: the box is taken 2^-8 larger)
BF_HD bool planeTouches(const double* a, const double* nrm, long long ix, long long iy, long long iz, double h) {
    const double cx = ((double)ix + 0.5) * h, cy = ((double)iy + 0.5) * h, cz = ((double)iz + 0.5) * h;
    const double s = nrm[0] * (cx - a[0]) + nrm[1] * (cy - a[1]) + nrm[2] * (cz - a[2]);
    const double r = (__builtin_fabs(nrm[0]) + __builtin_fabs(nrm[1]) + __builtin_fabs(nrm[2])) * (0.50390625 * h);
    return __builtin_fabs(s) <= r;
}

}  // namespace md

struct MeshDistance {
    // control words (uint32) and the accumulators (int64: 8 + 1024 histogram bins)
    uint32_t* d_words = nullptr;
    unsigned long long* d_acc = nullptr;
    // scratch over A: per face its sample count, then (one more entry) the first sample id; per scan tile its count / offset
    uint32_t *d_startA = nullptr, *d_tilesA = nullptr;
    uint32_t capFacesA = 0;
    // scratch over B: nine floats per face (NaN in the first: degenerate), the hashed cells (key, count then first entry, cursor), the entries, tile sums
    float* d_tri = nullptr;
    uint32_t capFacesB = 0;
    unsigned long long* d_keys = nullptr;
    uint32_t *d_cellStart = nullptr, *d_cellFill = nullptr, *d_tilesC = nullptr;
    uint32_t capTable = 0;
    uint32_t* d_entries = nullptr;
    uint32_t capEntries = 0;
    // the result, valid until the next measurement: per sample the distance, the nearest face and the weight
    double *d_distance = nullptr, *d_weight = nullptr;
    uint32_t* d_face = nullptr;
    uint32_t capSamples = 0;
    uint32_t numSamples = 0;
};

// Measures `a` against `b` (device arrays) on `stream` and waits for it twice (the refusals and counts, then the sums).  The buffers of `s` are taken from, and
// stay with, `res`.  A refusal leaves the last result as it was.
int meshdistance_run(MeshDistance& s, Resources& res, hipStream_t stream, const bf_indexed_mesh& a, const bf_indexed_mesh& b, const bf_mesh_distance_params& params,
                     bf_mesh_distance_stats* stats);

}  // namespace bf
