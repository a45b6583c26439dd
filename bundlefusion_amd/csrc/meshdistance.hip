// The distance of an indexed mesh A (the samples) to an indexed mesh B (the surface) on the device, for gfx950, without either mesh leaving HBM (DESIGN.md "Mesh
// distance: the definition"; include/bf_hip.h states it next to bf_marching_cubes_distance).  The reference has no counterpart; bf_mesh_distance_host below is the
// definition on one core over a grid of its own, tests/mesh_distance_ref.py restates it in numpy as a brute-force minimum over all faces, and the kernels are held
// to both as bits.  The arithmetic of the definition is bf_meshdistance.h's, compiled for both sides.
//
// Nothing here depends on the order in which threads run: a sample's result is a minimum over (d2, face index) pairs, the sums are int64 sums of quantised terms
// (no float sums, no float atomics), the maximum is one of bit patterns.
//
// The grid over B: hashed cells of edge max(D, 2^-9) * (1 + 2^-10) in an open-addressing table of 64-bit cell keys (linear probing; capacity a power of two >= 2 *
// the number of (face, cell) pairs, which bounds the occupied cells), so memory follows the occupied cells and not the bounding box.  A non-degenerate face is
// listed in every cell of its bounding box that its plane may cross.  Count (with the validation), scan over the table's slots, fill: three passes over the same
// cells.  The order of the faces inside a cell is the atomics' and no result depends on it.  A face within D of a sample is listed in one of the 27 cells around the
// sample's cell, so the search is a fixed neighbourhood with no early-out: one thread per sample walks the lists of its 27 cells and reads nine floats per face.
// Sums: k_md_reduce keeps the histogram in LDS (8 KiB of 64-bit bins), sums in registers, one set of atomics per workgroup; at most 64 workgroups, so an address
// of the accumulators takes at most 64 atomics.
// Every device loop is bounded: probe sequences by the table size, a face's cells by 2^24.  Exhaustion sets a bit of the error word; no kernel waits for another
// workgroup and nothing spins.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "bf_device.h"
#include "bf_resources.h"
#include "bf_meshdistance.h"

using namespace bf;
using namespace bf::md;

namespace {

constexpr uint32_t WG = 256;
constexpr uint32_t TILE = 1024;                 // 4 consecutive elements per thread
constexpr uint32_t MAX_GRID = 8192;
constexpr u64 EMPTY_KEY = ~0ull;
constexpr u64 MAX_FACE_CELLS = 1ull << 24;      // the cells of one face's bounding box

// the control words (uint32) and the accumulators (int64), zeroed before the validation
enum : uint32_t { W_ERR = 0, W_DEG_A = 1, W_DEG_B = 2, NUM_WORDS = 4 };
enum : uint32_t { A_SUM_W = 0, A_SUM_WD = 1, A_SUM_WD2 = 2, A_SUM_WB = 3, A_WITHIN = 4, A_BEYOND = 5, A_MAX = 6, A_ENTRIES = 7, A_SAMPLES = 8, A_SPARE = 9, A_HIST = 16, NUM_ACC = A_HIST + 1024 };
constexpr uint32_t ERR_FACE_ID = 1u, ERR_VALUE = 2u, ERR_N = 4u, ERR_WEIGHT = 8u, ERR_CELLS = 16u, ERR_LOOP = 32u;

// ---- what the validation learns of a face, shared with the host route
struct FaceInfo { uint32_t err; bool degenerate; uint32_t n; double N2; double a[3], b[3], c[3]; };
BF_HD FaceInfo faceInfo(const float* __restrict__ pos, const uint32_t* __restrict__ faces, uint32_t nv, uint32_t f) {
    FaceInfo r; r.err = 0; r.degenerate = true; r.n = 0; r.N2 = 0.0;
    const uint32_t ia = faces[3 * (size_t)f], ib = faces[3 * (size_t)f + 1], ic = faces[3 * (size_t)f + 2];
    if (ia >= nv || ib >= nv || ic >= nv) { r.err = ERR_FACE_ID; return r; }
    load3(pos + 3 * (size_t)ia, r.a); load3(pos + 3 * (size_t)ib, r.b); load3(pos + 3 * (size_t)ic, r.c);
    r.N2 = crossNorm2(r.a, r.b, r.c);
    r.degenerate = degenerate(r.N2);
    // a finite component of 1024 or more is refused on any face; one that is not finite makes the face degenerate (N2 is not finite then) and is not refused
    for (int d = 0; d < 3; ++d)
        if (finiteButLarge(r.a[d]) || finiteButLarge(r.b[d]) || finiteButLarge(r.c[d])) r.err = ERR_VALUE;
    return r;
}
// ... and of a face of A in surface mode: its n, 0 with an error bit
BF_HD uint32_t faceSamples(FaceInfo& r, double spacing) {
    r.n = subdivisions(r.a, r.b, r.c, spacing);
    if (r.n == 0u) { r.err |= ERR_N; return 0u; }
    if (!(sampleWeight(r.N2, r.n) < 64.0)) { r.err |= ERR_WEIGHT; return 0u; }
    return r.n * r.n;
}

// the cells of a face of B: the range of its bounding box and the plane's normal; false where the box covers more than MAX_FACE_CELLS cells
struct FaceCells { long long lo[3], hi[3]; double nrm[3]; bool usePlane; };
BF_HD bool faceCells(const double* a, const double* b, const double* c, double inv, FaceCells& fc) {
    u64 cells = 1ull;
    for (int d = 0; d < 3; ++d) {
        const double mn = a[d] < b[d] ? (a[d] < c[d] ? a[d] : c[d]) : (b[d] < c[d] ? b[d] : c[d]);
        const double mx = a[d] > b[d] ? (a[d] > c[d] ? a[d] : c[d]) : (b[d] > c[d] ? b[d] : c[d]);
        fc.lo[d] = cellOf(mn, inv); fc.hi[d] = cellOf(mx, inv);
        cells *= (u64)(fc.hi[d] - fc.lo[d] + 1);          // each factor <= 2^21: checked after every axis
        if (cells > MAX_FACE_CELLS) return false;
    }
    double u[3], v[3];
    for (int d = 0; d < 3; ++d) { u[d] = b[d] - a[d]; v[d] = c[d] - a[d]; }
    fc.nrm[0] = u[1] * v[2] - u[2] * v[1]; fc.nrm[1] = u[2] * v[0] - u[0] * v[2]; fc.nrm[2] = u[0] * v[1] - u[1] * v[0];
    // The plane test is trusted only where the normal's direction is: the cross product's components carry an absolute error of some 2^-51 |u| |v|, which is
    // 2^-51 / sin(angle) of its length.  With sin^2 >= 2^-20 that is below 2^-41, far inside the 2^-8 of slack; a sliver below that is listed in every cell of
    // its bounding box (which a sliver's box makes few).
    fc.usePlane = dot3(fc.nrm, fc.nrm) >= 9.5367431640625e-07 * (dot3(u, u) * dot3(v, v));
    return true;
}

BF_HD uint32_t hashKey(u64 k) {
    u64 h = k * 0x9E3779B97F4A7C15ull;
    h = (h ^ (h >> 31)) * 0xC2B2AE3D27D4EB4Full;
    return (uint32_t)(h >> 32) ^ (uint32_t)h;
}
// the slot of a key: inserted where absent.  NONE: the probe sequence ran out
BF_DEV uint32_t slotInsert(u64* keys, uint32_t mask, u64 key) {
    uint32_t h = hashKey(key) & mask;
    for (uint32_t probes = 0; probes <= mask; ++probes, h = (h + 1u) & mask) {
        const u64 prev = atomicCAS(&keys[h], EMPTY_KEY, key);
        if (prev == EMPTY_KEY || prev == key) return h;
    }
    return NONE;
}
// after the insert kernel.  NONE: no such cell
BF_DEV uint32_t slotFind(const u64* __restrict__ keys, uint32_t mask, u64 key) {
    uint32_t h = hashKey(key) & mask;
    for (uint32_t probes = 0; probes <= mask; ++probes, h = (h + 1u) & mask) {
        const u64 s = keys[h];
        if (s == key) return h;
        if (s == EMPTY_KEY) break;
    }
    return NONE;
}

BF_DEV u64 wave_sum_u64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
BF_DEV u64 wave_max_u64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const u64 y = __shfl_xor(v, o, 64); v = y > v ? y : v; }
    return v;
}

__global__ __launch_bounds__(256) void k_md_fill32(uint32_t* __restrict__ a, size_t n, uint32_t v) {
    for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) a[i] = v;
}
__global__ __launch_bounds__(256) void k_md_fill64(u64* __restrict__ a, size_t n, u64 v) {
    for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) a[i] = v;
}

// A: the refusals, the degenerate faces, the sample count of every face -> count[f] (surface mode; vertex mode: the vertices' components are checked instead)
__global__ __launch_bounds__(256) void k_md_faces_a(const float* __restrict__ pos, uint32_t nv, const uint32_t* __restrict__ faces, uint32_t nf, int surfaceMode, double spacing,
                                                    uint32_t* __restrict__ count, uint32_t* words) {
    uint32_t bad = 0, deg = 0;
    for (uint32_t f = blockIdx.x * WG + threadIdx.x; f < nf; f += gridDim.x * WG) {
        FaceInfo r = faceInfo(pos, faces, nv, f);
        uint32_t c = 0;
        if (!r.err && r.degenerate) ++deg;
        else if (!r.err && surfaceMode) c = faceSamples(r, spacing);
        bad |= r.err;
        count[f] = c;
    }
    if (!surfaceMode)
        for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < 3 * (size_t)nv; i += (size_t)gridDim.x * WG) if (!valueOk(pos[i])) bad |= ERR_VALUE;
    deg = (uint32_t)wave_sum_i((int)deg);
    if ((threadIdx.x & 63) == 0 && deg) atomicAdd(&words[W_DEG_A], deg);          // only the waves that met a degenerate face: rare in a mesh
    if (bad) atomicOr(&words[W_ERR], bad);
}

// B: the refusals, the degenerate faces, nine floats per face (the first a NaN on a degenerate face), and the cells: PASS 0 counts the (face, cell) pairs, PASS 1
// inserts the cells' keys and counts per cell, PASS 2 lists the faces
template <int PASS>
__global__ __launch_bounds__(256) void k_md_faces_b(const float* __restrict__ pos, uint32_t nv, const uint32_t* __restrict__ faces, uint32_t nf, double h, double inv,
                                                    float* __restrict__ tri, u64* keys, uint32_t mask, uint32_t* cellStart, uint32_t* cellFill, uint32_t* __restrict__ entries,
                                                    uint32_t capEntries, uint32_t* words, u64* acc) {
    uint32_t bad = 0, deg = 0;
    u64 pairs = 0;
    for (uint32_t f = blockIdx.x * WG + threadIdx.x; f < nf; f += gridDim.x * WG) {
        FaceInfo r;
        if (PASS == 0) {
            r = faceInfo(pos, faces, nv, f);
            bad |= r.err;
            const bool skip = r.err || r.degenerate;
            if (!r.err && r.degenerate) ++deg;
            float* t = tri + 9 * (size_t)f;
            for (int d = 0; d < 3; ++d) { t[d] = skip ? __builtin_nanf("") : (float)r.a[d]; t[3 + d] = skip ? 0.0f : (float)r.b[d]; t[6 + d] = skip ? 0.0f : (float)r.c[d]; }
            if (skip) continue;
        } else {
            const float* t = tri + 9 * (size_t)f;
            if (t[0] != t[0]) continue;
            load3(t, r.a); load3(t + 3, r.b); load3(t + 6, r.c);
        }
        FaceCells fc;
        if (!faceCells(r.a, r.b, r.c, inv, fc)) { bad |= ERR_CELLS; continue; }
        for (long long z = fc.lo[2]; z <= fc.hi[2]; ++z)
            for (long long y = fc.lo[1]; y <= fc.hi[1]; ++y)
                for (long long x = fc.lo[0]; x <= fc.hi[0]; ++x) {
                    if (fc.usePlane && !planeTouches(r.a, fc.nrm, x, y, z, h)) continue;
                    if (PASS == 0) { ++pairs; continue; }
                    const u64 key = cellKey(x, y, z);
                    if (PASS == 1) {
                        const uint32_t s = slotInsert(keys, mask, key);
                        if (s == NONE) bad |= ERR_LOOP; else atomicAdd(&cellStart[s], 1u);
                    } else {
                        const uint32_t s = slotFind(keys, mask, key);
                        if (s == NONE) { bad |= ERR_LOOP; continue; }
                        const uint32_t at = cellStart[s] + atomicAdd(&cellFill[s], 1u);
                        if (at < capEntries) entries[at] = f; else bad |= ERR_LOOP;
                    }
                }
    }
    if (PASS == 0) {                                     // one atomic per workgroup: one per wave on one word is what profiles/mesh_simplify.md measured at 639 us
        __shared__ u64 wpairs[4];
        __shared__ uint32_t wdeg[4];
        deg = (uint32_t)wave_sum_i((int)deg);
        pairs = wave_sum_u64(pairs);
        if ((threadIdx.x & 63) == 0) { wpairs[threadIdx.x >> 6] = pairs; wdeg[threadIdx.x >> 6] = deg; }
        __syncthreads();
        if (threadIdx.x == 0) {
            const u64 p4 = (wpairs[0] + wpairs[1]) + (wpairs[2] + wpairs[3]); const uint32_t d4 = wdeg[0] + wdeg[1] + wdeg[2] + wdeg[3];
            if (d4) atomicAdd(&words[W_DEG_B], d4);
            if (p4) atomicAdd(&acc[A_ENTRIES], p4);
        }
    }
    if (bad) atomicOr(&words[W_ERR], bad);
}

// ---- the exclusive scan of a uint32 array in place, a[n] = the total: sums of tiles of 1024, one scan of the tile sums by one workgroup (64-bit inside: a prefix
// beyond 2^32 - 1 is written as 2^32 - 1 and the total is exact in *total), the prefixes inside every tile
__global__ __launch_bounds__(256) void k_md_tile_sum(const uint32_t* __restrict__ a, uint32_t n, uint32_t numTiles, uint32_t* __restrict__ tileSums) {
    __shared__ uint32_t ws[4];
    for (uint32_t tile = blockIdx.x; tile < numTiles; tile += gridDim.x) {
        uint32_t c = 0;
        for (uint32_t k = 0; k < 4; ++k) { const uint32_t i = tile * TILE + threadIdx.x * 4 + k; if (i < n) c += a[i]; }          // <= 1024 * 2^20
        c = (uint32_t)wave_sum_i((int)c);
        if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = c;
        __syncthreads();
        if (threadIdx.x == 0) tileSums[tile] = ws[0] + ws[1] + ws[2] + ws[3];
        __syncthreads();
    }
}
BF_DEV uint32_t sat32(u64 v) { return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v; }
__global__ __launch_bounds__(256) void k_md_tile_scan(uint32_t* a, uint32_t n, u64* total) {
    __shared__ u64 wtot[4];
    __shared__ u64 carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t base = 0; base < n; base += WG) {
        const uint32_t i = base + threadIdx.x;
        const u64 x = i < n ? a[i] : 0u;
        u64 incl = x;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const u64 y = __shfl_up(incl, o, 64); if ((int)lane >= o) incl += y; }
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        u64 woff = 0;
        for (uint32_t w = 0; w < wave; ++w) woff += wtot[w];
        const u64 c0 = carry;
        if (i < n) a[i] = sat32(c0 + woff + incl - x);
        __syncthreads();
        if (threadIdx.x == WG - 1) carry = c0 + woff + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}
__global__ __launch_bounds__(256) void k_md_tile_apply(uint32_t* __restrict__ a, uint32_t n, uint32_t numTiles, const uint32_t* __restrict__ tileOffsets, const u64* __restrict__ total) {
    __shared__ uint32_t wscan[4];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (blockIdx.x == 0 && threadIdx.x == 0) a[n] = sat32(*total);
    for (uint32_t tile = blockIdx.x; tile < numTiles; tile += gridDim.x) {
        uint32_t x[4]; uint32_t c = 0;
        for (uint32_t k = 0; k < 4; ++k) { const uint32_t i = tile * TILE + threadIdx.x * 4 + k; x[k] = i < n ? a[i] : 0u; c += x[k]; }
        uint32_t incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(incl, o, 64); if ((int)lane >= o) incl += y; }
        if (lane == 63) wscan[wave] = incl;
        __syncthreads();
        uint32_t woff = 0;
        for (uint32_t w = 0; w < wave; ++w) woff += wscan[w];
        uint32_t at = tileOffsets[tile] + woff + incl - c;
        for (uint32_t k = 0; k < 4; ++k) { const uint32_t i = tile * TILE + threadIdx.x * 4 + k; if (i < n) a[i] = at; at += x[k]; }
        __syncthreads();
    }
}

// ---- the search: one thread per sample, results at the sample's id
struct SearchArgs {
    const float* posA; const uint32_t* facesA; const uint32_t* startA; uint32_t nfA; int surfaceMode; uint32_t numSamples;
    const float* tri; const u64* keys; uint32_t mask; const uint32_t* cellStart; const uint32_t* cellCount; const uint32_t* entries; uint32_t numEntries; uint32_t nfB;
    double inv, D2;
    double* distance; uint32_t* face; double* weight;
};
__global__ __launch_bounds__(256) void k_md_search(SearchArgs s, uint32_t* words) {
    uint32_t bad = 0;
    for (uint32_t id = blockIdx.x * WG + threadIdx.x; id < s.numSamples; id += gridDim.x * WG) {
        double p[3], w = 1.0;
        if (!s.surfaceMode) load3(s.posA + 3 * (size_t)id, p);
        else {
            uint32_t lo = 0, hi = s.nfA;                       // the last face f with startA[f] <= id: it has samples, since startA[f + 1] > id
            while (hi - lo > 1u) { const uint32_t mid = lo + (hi - lo) / 2u; if (s.startA[mid] <= id) lo = mid; else hi = mid; }
            double a[3], b[3], c[3];
            load3(s.posA + 3 * (size_t)s.facesA[3 * (size_t)lo], a); load3(s.posA + 3 * (size_t)s.facesA[3 * (size_t)lo + 1], b); load3(s.posA + 3 * (size_t)s.facesA[3 * (size_t)lo + 2], c);
            const uint32_t nn = s.startA[lo + 1] - s.startA[lo];
            uint32_t n = (uint32_t)__builtin_sqrt((double)nn);
            while (n * n < nn) ++n;
            while (n > 1u && (n - 1u) * (n - 1u) >= nn) --n;
            sampleOf(a, b, c, n, id - s.startA[lo], p);
            w = sampleWeight(crossNorm2(a, b, c), n);
        }
        double best = (double)BF_PINF; uint32_t bestF = NONE;
        const long long cx = cellOf(p[0], s.inv), cy = cellOf(p[1], s.inv), cz = cellOf(p[2], s.inv);
        for (int k = 0; k < 27; ++k) {
            const uint32_t slot = slotFind(s.keys, s.mask, cellKey(cx + (k % 3) - 1, cy + (k / 3) % 3 - 1, cz + k / 9 - 1));
            if (slot == NONE) continue;
            const uint32_t e0 = s.cellStart[slot], cnt = s.cellCount[slot];
            if (e0 > s.numEntries || cnt > s.numEntries - e0) { bad |= ERR_LOOP; continue; }          // (not reached)
            for (uint32_t e = e0; e < e0 + cnt; ++e) {
                const uint32_t f = s.entries[e];
                if (f >= s.nfB) { bad |= ERR_LOOP; continue; }                                         // (not reached)
                double a[3], b[3], c[3];
                const float* t = s.tri + 9 * (size_t)f;
                load3(t, a); load3(t + 3, b); load3(t + 6, c);
                const double d2 = triDist2(p, a, b, c);
                if (d2 < best || (d2 == best && f < bestF)) { best = d2; bestF = f; }
            }
        }
        const bool within = bestF != NONE && best <= s.D2;
        s.distance[id] = within ? __builtin_sqrt(best) : (double)BF_PINF;
        s.face[id] = within ? bestF : NONE;
        s.weight[id] = w;
    }
    if (bad) atomicOr(&words[W_ERR], bad);
}

// ---- the sums over the per-sample results
__global__ __launch_bounds__(256) void k_md_reduce(const double* __restrict__ distance, const double* __restrict__ weight, uint32_t numSamples, double sW, double sWD, double sWD2,
                                                   double binScale, u64* acc) {
    __shared__ u64 hist[1024];
    __shared__ u64 part[7];
    for (uint32_t i = threadIdx.x; i < 1024; i += WG) hist[i] = 0ull;
    if (threadIdx.x < 7) part[threadIdx.x] = 0ull;
    __syncthreads();
    u64 v[6] = {0, 0, 0, 0, 0, 0}, mx = 0;
    for (uint32_t id = blockIdx.x * WG + threadIdx.x; id < numSamples; id += gridDim.x * WG) {
        const double d = distance[id], w = weight[id];
        const u64 qw = (u64)quant(w, sW);
        if (d < (double)BF_PINF) {
            const double wd = w * d;
            v[A_SUM_W] += qw; v[A_SUM_WD] += (u64)quant(wd, sWD); v[A_SUM_WD2] += (u64)quant(wd * d, sWD2); v[A_WITHIN] += 1ull;
            const u64 bits = (u64)__double_as_longlong(d);
            mx = bits > mx ? bits : mx;
            atomicAdd(&hist[binOf(d, binScale)], qw);
        } else { v[A_SUM_WB] += qw; v[A_BEYOND] += 1ull; }
    }
    for (int j = 0; j < 6; ++j) v[j] = wave_sum_u64(v[j]);
    mx = wave_max_u64(mx);
    if ((threadIdx.x & 63) == 0) { for (int j = 0; j < 6; ++j) atomicAdd(&part[j], v[j]); atomicMax(&part[6], mx); }
    __syncthreads();
    if (threadIdx.x < 6 && part[threadIdx.x]) atomicAdd(&acc[threadIdx.x], part[threadIdx.x]);
    if (threadIdx.x == 6 && part[6]) atomicMax(&acc[A_MAX], part[6]);
    for (uint32_t i = threadIdx.x; i < 1024; i += WG) if (hist[i]) atomicAdd(&acc[A_HIST + i], hist[i]);
}

uint32_t gridFor(size_t n) { return (uint32_t)std::max<size_t>(1, std::min<size_t>((n + WG - 1) / WG, MAX_GRID)); }
uint32_t gridForTiles(uint32_t tiles) { return std::max(1u, std::min(tiles, MAX_GRID)); }

template <typename T>
int grow(Resources& res, T** p, size_t count) { return res.regrow(p, std::max<size_t>(count, 1)); }

// the refusals that need no mesh
int paramsOk(const bf_mesh_distance_params& p, const char* who) {
    if (!(p.maxDistance > 0.0f && p.maxDistance <= MAX_D)) { set_error("%s: maxDistance is not a finite number in (0, 64]", who); return BF_ERR_INVALID_ARG; }
    if (!(p.sampleSpacing >= 0.0f && p.sampleSpacing < BF_PINF)) { set_error("%s: sampleSpacing is negative or not finite", who); return BF_ERR_INVALID_ARG; }
    if (p.sampleMode != 0 && p.sampleMode != 1) { set_error("%s: sampleMode is not 0 or 1", who); return BF_ERR_INVALID_ARG; }
    return BF_OK;
}
int refusal(uint32_t err, const char* who) {
    const char* what = (err & ERR_FACE_ID) ? "a face id is not below numVertices"
                     : (err & ERR_VALUE)   ? "a position component that the measurement reads is not finite or not below 1024 in magnitude"
                     : (err & ERR_N)       ? "a face of A needs more than 1024 subdivisions per edge: raise sampleSpacing"
                     : (err & ERR_WEIGHT)  ? "a sample of A weighs 64 square metres or more: lower sampleSpacing" : nullptr;
    if (!what) return BF_OK;
    set_error("%s: %s", who, what);
    return BF_ERR_INVALID_ARG;
}
int tooManyPairs(const char* who) {
    set_error("%s: the search grid over B would hold more than 2^27 (face, cell) pairs, or one face's bounding box more than 2^24 cells: lower maxDistance's ratio to the largest faces", who);
    return BF_ERR_CAPACITY;
}

void fillStats(bf_mesh_distance_stats* st, u64 numSamples, uint32_t degA, uint32_t degB, const Scales& sc, const u64* acc) {
    if (!st) return;
    memset(st, 0, sizeof *st);
    st->numSamples = numSamples; st->numWithin = acc[A_WITHIN]; st->numBeyond = acc[A_BEYOND]; st->numDegenerateA = degA; st->numDegenerateB = degB;
    memcpy(&st->maxWithin, &acc[A_MAX], 8);
    st->sumW = (int64_t)acc[A_SUM_W]; st->sumWD = (int64_t)acc[A_SUM_WD]; st->sumWD2 = (int64_t)acc[A_SUM_WD2]; st->sumWBeyond = (int64_t)acc[A_SUM_WB];
    st->scaleW = sc.kW; st->scaleWD = sc.kWD; st->scaleWD2 = sc.kWD2;
    memcpy(st->histogram, acc + A_HIST, 8 * 1024);
}

}  // namespace

namespace bf {

int meshdistance_run(MeshDistance& s, Resources& res, hipStream_t st, const bf_indexed_mesh& A, const bf_indexed_mesh& B, const bf_mesh_distance_params& params,
                     bf_mesh_distance_stats* stats) {
    static const char* who = "bf_marching_cubes_distance";
    BF_TRY(paramsOk(params, who));
    const uint32_t nvA = A.numVertices, nfA = A.numFaces, nvB = B.numVertices, nfB = B.numFaces;
    BF_REQUIRE(nfA <= MAX_FACES && nfB <= MAX_FACES && nvA <= MAX_VERTICES && nvB <= MAX_VERTICES, "too many faces or vertices for one measurement");
    BF_REQUIRE((nvA == 0 || A.d_positions) && (nfA == 0 || A.d_faces) && (nvB == 0 || B.d_positions) && (nfB == 0 || B.d_faces), "null mesh array");
    const int surface = params.sampleMode;
    const double h = deviceCell(params.maxDistance), inv = 1.0 / h;
    if (!s.d_words) BF_TRY(res.device(&s.d_words, NUM_WORDS));
    if (!s.d_acc) BF_TRY(res.device(&s.d_acc, NUM_ACC));

    // ---- the refusals and the counts, in scratch: no buffer of the last result is touched
    const uint32_t tilesA = div_up(nfA + 1u, TILE);
    if (nfA > s.capFacesA || !s.d_startA) {
        s.capFacesA = 0;
        BF_TRY(grow(res, &s.d_startA, (size_t)nfA + 1)); BF_TRY(grow(res, &s.d_tilesA, tilesA));
        s.capFacesA = nfA;
    }
    if (nfB > s.capFacesB || !s.d_tri) { s.capFacesB = 0; BF_TRY(grow(res, &s.d_tri, 9 * (size_t)nfB)); s.capFacesB = nfB; }
    hipLaunchKernelGGL(k_md_fill32, dim3(1), dim3(WG), 0, st, s.d_words, (size_t)NUM_WORDS, 0u);
    hipLaunchKernelGGL(k_md_fill64, dim3(gridFor(NUM_ACC)), dim3(WG), 0, st, s.d_acc, (size_t)NUM_ACC, 0ull);
    hipLaunchKernelGGL(k_md_faces_a, dim3(gridFor(std::max<size_t>(nfA, surface ? 0 : 3 * (size_t)nvA))), dim3(WG), 0, st, A.d_positions, nvA, A.d_faces, nfA, surface, (double)params.sampleSpacing,
                       s.d_startA, s.d_words);
    hipLaunchKernelGGL(k_md_tile_sum, dim3(gridForTiles(tilesA)), dim3(WG), 0, st, (const uint32_t*)s.d_startA, nfA, tilesA, s.d_tilesA);
    hipLaunchKernelGGL(k_md_tile_scan, dim3(1), dim3(WG), 0, st, s.d_tilesA, tilesA, s.d_acc + A_SAMPLES);
    hipLaunchKernelGGL(k_md_tile_apply, dim3(gridForTiles(tilesA)), dim3(WG), 0, st, s.d_startA, nfA, tilesA, (const uint32_t*)s.d_tilesA, (const u64*)(s.d_acc + A_SAMPLES));
    hipLaunchKernelGGL(k_md_faces_b<0>, dim3(std::min(gridFor(nfB), 2048u)), dim3(WG), 0, st, B.d_positions, nvB, B.d_faces, nfB, h, inv, s.d_tri, (u64*)nullptr, 0u, (uint32_t*)nullptr, (uint32_t*)nullptr,
                       (uint32_t*)nullptr, 0u, s.d_words, s.d_acc);
    BF_HIP_TRY(hipGetLastError());
    uint32_t words[NUM_WORDS] = {0};
    u64 head[A_HIST] = {0};
    BF_HIP_TRY(hipMemcpyAsync(words, s.d_words, sizeof words, hipMemcpyDeviceToHost, st));
    BF_HIP_TRY(hipMemcpyAsync(head, s.d_acc, sizeof head, hipMemcpyDeviceToHost, st));
    BF_HIP_TRY(hipStreamSynchronize(st));
    BF_TRY(refusal(words[W_ERR], who));
    const u64 numSamples64 = surface ? head[A_SAMPLES] : (u64)nvA;
    BF_REQUIRE(numSamples64 <= MAX_SAMPLES, "more than 2^28 samples: raise sampleSpacing");
    if ((words[W_ERR] & ERR_CELLS) || head[A_ENTRIES] > MAX_ENTRIES) return tooManyPairs(who);
    const uint32_t N = (uint32_t)numSamples64, E = (uint32_t)head[A_ENTRIES];
    const uint32_t degA = words[W_DEG_A], degB = words[W_DEG_B];

    // ---- the grid over B
    s.numSamples = 0;
    uint32_t cap = 1024;
    while (cap < 2u * E) cap <<= 1;
    const uint32_t mask = cap - 1u, tilesC = div_up(cap + 1u, TILE);
    if (cap > s.capTable || !s.d_keys) {
        s.capTable = 0;
        BF_TRY(grow(res, &s.d_keys, cap)); BF_TRY(grow(res, &s.d_cellStart, (size_t)cap + 1)); BF_TRY(grow(res, &s.d_cellFill, cap)); BF_TRY(grow(res, &s.d_tilesC, tilesC));
        s.capTable = cap;
    }
    if (E > s.capEntries || !s.d_entries) { s.capEntries = 0; BF_TRY(grow(res, &s.d_entries, E)); s.capEntries = E; }
    if (N > s.capSamples || !s.d_distance) {
        s.capSamples = 0;
        BF_TRY(grow(res, &s.d_distance, N)); BF_TRY(grow(res, &s.d_weight, N)); BF_TRY(grow(res, &s.d_face, N));
        s.capSamples = N;
    }
    hipLaunchKernelGGL(k_md_fill64, dim3(gridFor(cap)), dim3(WG), 0, st, s.d_keys, (size_t)cap, EMPTY_KEY);
    hipLaunchKernelGGL(k_md_fill32, dim3(gridFor(cap)), dim3(WG), 0, st, s.d_cellStart, (size_t)cap + 1, 0u);
    hipLaunchKernelGGL(k_md_fill32, dim3(gridFor(cap)), dim3(WG), 0, st, s.d_cellFill, (size_t)cap, 0u);
    hipLaunchKernelGGL(k_md_faces_b<1>, dim3(gridFor(nfB)), dim3(WG), 0, st, B.d_positions, nvB, B.d_faces, nfB, h, inv, s.d_tri, s.d_keys, mask, s.d_cellStart, s.d_cellFill, s.d_entries, E,
                       s.d_words, s.d_acc);
    hipLaunchKernelGGL(k_md_tile_sum, dim3(gridForTiles(tilesC)), dim3(WG), 0, st, (const uint32_t*)s.d_cellStart, cap, tilesC, s.d_tilesC);
    hipLaunchKernelGGL(k_md_tile_scan, dim3(1), dim3(WG), 0, st, s.d_tilesC, tilesC, s.d_acc + A_SPARE);          // (the total is E again)
    hipLaunchKernelGGL(k_md_tile_apply, dim3(gridForTiles(tilesC)), dim3(WG), 0, st, s.d_cellStart, cap, tilesC, (const uint32_t*)s.d_tilesC, (const u64*)(s.d_acc + A_SPARE));
    hipLaunchKernelGGL(k_md_faces_b<2>, dim3(gridFor(nfB)), dim3(WG), 0, st, B.d_positions, nvB, B.d_faces, nfB, h, inv, s.d_tri, s.d_keys, mask, s.d_cellStart, s.d_cellFill, s.d_entries, E,
                       s.d_words, s.d_acc);

    // ---- the search and the sums
    const Scales sc = scalesFor(numSamples64, surface, params.maxDistance);
    const double D = (double)params.maxDistance;
    SearchArgs sa;
    sa.posA = A.d_positions; sa.facesA = A.d_faces; sa.startA = s.d_startA; sa.nfA = nfA; sa.surfaceMode = surface; sa.numSamples = N;
    sa.tri = s.d_tri; sa.keys = s.d_keys; sa.mask = mask; sa.cellStart = s.d_cellStart; sa.cellCount = s.d_cellFill; sa.entries = s.d_entries; sa.numEntries = E; sa.nfB = nfB;
    sa.inv = inv; sa.D2 = D * D;
    sa.distance = s.d_distance; sa.face = s.d_face; sa.weight = s.d_weight;
    hipLaunchKernelGGL(k_md_search, dim3(gridFor(N)), dim3(WG), 0, st, sa, s.d_words);
    hipLaunchKernelGGL(k_md_reduce, dim3(std::max(1u, std::min(div_up(N, 4096u), 64u))), dim3(WG), 0, st, (const double*)s.d_distance, (const double*)s.d_weight, N, sc.sW, sc.sWD, sc.sWD2,
                       1024.0 / D, s.d_acc);
    BF_HIP_TRY(hipGetLastError());
    std::vector<u64> acc(NUM_ACC);
    BF_HIP_TRY(hipMemcpyAsync(words, s.d_words, sizeof words, hipMemcpyDeviceToHost, st));
    BF_HIP_TRY(hipMemcpyAsync(acc.data(), s.d_acc, 8 * (size_t)NUM_ACC, hipMemcpyDeviceToHost, st));
    BF_HIP_TRY(hipStreamSynchronize(st));
    if ((words[W_ERR] & ERR_LOOP) || acc[A_WITHIN] + acc[A_BEYOND] != numSamples64) { set_error("%s: a bounded loop ran out of steps", who); return BF_ERR_INTERNAL; }
    s.numSamples = N;
    fillStats(stats, numSamples64, degA, degB, sc, acc.data());
    return BF_OK;
}

}  // namespace bf

// ---- the host route
namespace {

// validation and counts of A: start[f] the first sample id of face f (surface mode), start[nf] the total
int hostSamples(const float* pos, const uint32_t* faces, uint32_t nv, uint32_t nf, const bf_mesh_distance_params& p, std::vector<u64>* start, u64& numSamples, uint32_t& deg, const char* who) {
    BF_REQUIRE(nf <= MAX_FACES && nv <= MAX_VERTICES, "too many faces or vertices for one measurement");
    BF_REQUIRE((nv == 0 || pos) && (nf == 0 || faces), "null mesh array");
    uint32_t err = 0; deg = 0;
    u64 total = 0;
    if (start) start->assign((size_t)nf + 1, 0);
    for (uint32_t f = 0; f < nf; ++f) {
        FaceInfo r = faceInfo(pos, faces, nv, f);
        if (start) (*start)[f] = total;
        if (!r.err && r.degenerate) ++deg;
        else if (!r.err && p.sampleMode) total += faceSamples(r, (double)p.sampleSpacing);
        err |= r.err;
    }
    if (start) (*start)[nf] = total;
    if (!p.sampleMode) for (size_t i = 0; i < 3 * (size_t)nv; ++i) if (!valueOk(pos[i])) err |= ERR_VALUE;
    BF_TRY(refusal(err, who));
    numSamples = p.sampleMode ? total : (u64)nv;
    BF_REQUIRE(numSamples <= MAX_SAMPLES, "more than 2^28 samples: raise sampleSpacing");
    return BF_OK;
}

}  // namespace

extern "C" int bf_mesh_distance_sample_count_host(const float* posA, const uint32_t* facesA, uint32_t nvA, uint32_t nfA, const bf_mesh_distance_params* params, uint64_t* numSamples) {
    static const char* who = "bf_mesh_distance_sample_count_host";
    BF_REQUIRE(params && numSamples, "null argument");
    BF_TRY(paramsOk(*params, who));
    u64 n = 0; uint32_t deg = 0;
    BF_TRY(hostSamples(posA, facesA, nvA, nfA, *params, nullptr, n, deg, who));
    *numSamples = n;
    return BF_OK;
}

// The grid here is the host's own: its cell edge g follows the faces (twice the mean longest side of their bounding boxes, between max(2^-9, D / 16) and the device's
// cell), the (cell, face) pairs are sorted by cell, and a sample searches the cells around its own ring by ring: after ring r every face not yet met lies farther
// than 0.99 * r * g, so the search ends once the best squared distance is below that bound's square, or the bound is beyond D.
extern "C" int bf_mesh_distance_host(const float* posA, const uint32_t* facesA, uint32_t nvA, uint32_t nfA, const float* posB, const uint32_t* facesB, uint32_t nvB, uint32_t nfB,
                                     const bf_mesh_distance_params* params, double* h_distance, uint32_t* h_face, double* h_weight, uint32_t capacity, bf_mesh_distance_stats* stats) {
    static const char* who = "bf_mesh_distance_host";
    BF_REQUIRE(params, "null argument");
    BF_TRY(paramsOk(*params, who));
    const bf_mesh_distance_params& P = *params;
    std::vector<u64> start;
    u64 numSamples = 0; uint32_t degA = 0, degB = 0;
    BF_TRY(hostSamples(posA, facesA, nvA, nfA, P, &start, numSamples, degA, who));
    BF_REQUIRE(nfB <= MAX_FACES && nvB <= MAX_VERTICES, "too many faces or vertices for one measurement");
    BF_REQUIRE((nvB == 0 || posB) && (nfB == 0 || facesB), "null mesh array");
    // B: the refusals, the corners, the cell edge
    std::vector<float> tri(9 * (size_t)nfB);
    std::vector<uint8_t> live(nfB, 0);
    uint32_t err = 0;
    double extent = 0.0; u64 numLive = 0;
    for (uint32_t f = 0; f < nfB; ++f) {
        const FaceInfo r = faceInfo(posB, facesB, nvB, f);
        err |= r.err;
        if (r.err) continue;
        if (r.degenerate) { ++degB; continue; }
        live[f] = 1; ++numLive;
        double side = 0.0;
        for (int d = 0; d < 3; ++d) {
            tri[9 * (size_t)f + d] = (float)r.a[d]; tri[9 * (size_t)f + 3 + d] = (float)r.b[d]; tri[9 * (size_t)f + 6 + d] = (float)r.c[d];
            side = std::max(side, std::max(r.a[d], std::max(r.b[d], r.c[d])) - std::min(r.a[d], std::min(r.b[d], r.c[d])));
        }
        extent += side;
    }
    BF_TRY(refusal(err, who));
    const double D = (double)P.maxDistance, D2 = D * D;
    const double gMin = std::max(0.001953125, D / 16.0), gMax = deviceCell(P.maxDistance);
    const double g = std::min(gMax, std::max(gMin, numLive ? 2.0 * extent / (double)numLive : gMax)), inv = 1.0 / g;
    std::vector<std::pair<u64, uint32_t>> pairs;
    for (uint32_t f = 0; f < nfB; ++f) {
        if (!live[f]) continue;
        double a[3], b[3], c[3];
        load3(&tri[9 * (size_t)f], a); load3(&tri[9 * (size_t)f + 3], b); load3(&tri[9 * (size_t)f + 6], c);
        FaceCells fc;
        if (!faceCells(a, b, c, inv, fc)) return tooManyPairs(who);
        for (long long z = fc.lo[2]; z <= fc.hi[2]; ++z)
            for (long long y = fc.lo[1]; y <= fc.hi[1]; ++y)
                for (long long x = fc.lo[0]; x <= fc.hi[0]; ++x)
                    if (!fc.usePlane || planeTouches(a, fc.nrm, x, y, z, g)) pairs.emplace_back(cellKey(x, y, z), f);
        if (pairs.size() > MAX_ENTRIES) return tooManyPairs(who);
    }
    std::sort(pairs.begin(), pairs.end());
    std::unordered_map<u64, std::pair<uint32_t, uint32_t>> cells;          // key -> (first pair, count)
    for (size_t i = 0; i < pairs.size();) {
        size_t j = i;
        while (j < pairs.size() && pairs[j].first == pairs[i].first) ++j;
        cells.emplace(pairs[i].first, std::make_pair((uint32_t)i, (uint32_t)(j - i)));
        i = j;
    }
    // the samples
    const Scales sc = scalesFor(numSamples, P.sampleMode, P.maxDistance);
    const double binScale = 1024.0 / D;
    std::vector<u64> acc(NUM_ACC, 0);
    uint32_t face = 0;                                   // surface mode: the face of the current sample
    for (u64 id = 0; id < numSamples; ++id) {
        double p[3], w = 1.0;
        if (!P.sampleMode) load3(posA + 3 * (size_t)id, p);
        else {
            while (start[face + 1] <= id) ++face;
            const FaceInfo r = faceInfo(posA, facesA, nvA, face);
            const uint32_t n = subdivisions(r.a, r.b, r.c, (double)P.sampleSpacing);
            sampleOf(r.a, r.b, r.c, n, (uint32_t)(id - start[face]), p);
            w = sampleWeight(r.N2, n);
        }
        double best = (double)BF_PINF; uint32_t bestF = NONE;
        if (!pairs.empty()) {
            const long long cx = cellOf(p[0], inv), cy = cellOf(p[1], inv), cz = cellOf(p[2], inv);
            for (long long r = 0;; ++r) {
                for (long long z = -r; z <= r; ++z)
                    for (long long y = -r; y <= r; ++y) {
                        const bool shell = z == -r || z == r || y == -r || y == r;
                        for (long long x = -r; x <= r; x += (shell || r == 0) ? 1 : 2 * r) {
                            const auto it = cells.find(cellKey(cx + x, cy + y, cz + z));
                            if (it == cells.end()) continue;
                            for (uint32_t e = it->second.first; e < it->second.first + it->second.second; ++e) {
                                const uint32_t f = pairs[e].second;
                                double a[3], b[3], c[3];
                                load3(&tri[9 * (size_t)f], a); load3(&tri[9 * (size_t)f + 3], b); load3(&tri[9 * (size_t)f + 6], c);
                                const double d2 = triDist2(p, a, b, c);
                                if (d2 < best || (d2 == best && f < bestF)) { best = d2; bestF = f; }
                            }
                        }
                    }
                const double lb = 0.99 * (double)r * g;                    // a face first met in ring r + 1 is farther than r * g, less the roundings
                if (best < lb * lb || lb * lb > D2) break;
            }
        }
        const bool within = bestF != NONE && best <= D2;
        const double d = within ? std::sqrt(best) : (double)BF_PINF;
        if (id < capacity) {
            if (h_distance) h_distance[id] = d;
            if (h_face) h_face[id] = within ? bestF : NONE;
            if (h_weight) h_weight[id] = w;
        }
        const u64 qw = (u64)quant(w, sc.sW);
        if (within) {
            const double wd = w * d;
            acc[A_SUM_W] += qw; acc[A_SUM_WD] += (u64)quant(wd, sc.sWD); acc[A_SUM_WD2] += (u64)quant(wd * d, sc.sWD2); acc[A_WITHIN] += 1;
            u64 bits; memcpy(&bits, &d, 8);
            acc[A_MAX] = std::max(acc[A_MAX], bits);
            acc[A_HIST + binOf(d, binScale)] += qw;
        } else { acc[A_SUM_WB] += qw; acc[A_BEYOND] += 1; }
    }
    fillStats(stats, numSamples, degA, degB, sc, acc.data());
    return BF_OK;
}

// bf_write_ply_indexed with the distance as a colour ramp
extern "C" int bf_write_ply_indexed_error(const char* filename, const float* h_positions, const uint32_t* h_faces, const double* h_distance, float maxDistance, uint32_t numVertices,
                                          uint32_t numFaces) {
    BF_REQUIRE(filename && (numVertices == 0 || h_distance), "null argument");
    BF_REQUIRE(maxDistance > 0.0f && maxDistance < BF_PINF, "maxDistance is not a finite number above 0");
    std::vector<float> col(3 * (size_t)numVertices);
    for (size_t i = 0; i < numVertices; ++i) {
        const double d = h_distance[i];
        float* c = &col[3 * i];
        if (!(d <= (double)maxDistance)) { c[0] = 1.0f; c[1] = 0.0f; c[2] = 1.0f; continue; }
        const float t = (float)(d / (double)maxDistance), s = 2.0f * t - 1.0f;
        c[0] = std::max(0.0f, s); c[1] = 1.0f - std::fabs(s); c[2] = std::max(0.0f, 1.0f - 2.0f * t);
    }
    return bf_write_ply_indexed(filename, h_positions, col.data(), h_faces, numVertices, numFaces);
}
