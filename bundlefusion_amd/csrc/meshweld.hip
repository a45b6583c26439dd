// Weld of a triangle soup into an indexed mesh on the device, for gfx950: what bf_marching_cubes_save_mesh computes on the host - the
// definition - without the triangles leaving HBM.
//
// Definition (corner 3 * t + c = corner c of triangle t):
//  * key of a corner: (int64)floor((double)p[c] * (1.0 / 0.00001) + 0.5) per axis, in binary64, multiply then add (no FMA);
//  * the vertex of a key is its lowest-numbered corner (the representative); vertex ids count the representatives in increasing corner number - the order of first
//    occurrence; position and colour are the representative's.  Corners of faces dropped below still make vertices;
//  * a face whose three ids are not pairwise different is dropped; among the others, faces with the same sorted id triple keep the one with the lowest triangle
//    index; kept faces stay in triangle order with their winding;
//  * the optional transform is xform() of bf_device.h on the welded positions, op by op in binary32.
// Nothing here depends on the order in which threads run: "first occurrence" is a minimum over corner numbers, never "who arrived first".
//
// Table protocol: an open-addressing table of uint32 corner numbers (capacity: a power of two >= 2 * 3T, linear probing).  A slot holds a corner NUMBER, never a
// key; keys are recomputed from the read-only triangle buffer.  Insert of corner i at slot h: prev = atomicCAS(slot, EMPTY, i); EMPTY: done; key(prev) == key(i):
// atomicMin(slot, i), done; otherwise the next slot.  Every value ever written to a slot has the key of the slot's first occupant, so a probe sequence takes the
// same turns whatever the minimum has settled to.  Coherence: inside the insert kernel a slot is read through the CAS result only (an agent-scope atomic) - a
// plain load may be served stale from another XCD's L2; the later kernels start after the insert kernel has ended and read slots with plain loads.
// The faces' table is the same thing over triangle numbers keyed on the sorted id triple (it reuses the corners' table: 2 * 3T slots >= 2 * T).
//
// Counting and compaction: tiles of 1024 elements (count per tile, one scan of the tile counts, scatter) - no atomics on counters, no float atomics anywhere.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "bf_device.h"
#include "bf_resources.h"
#include "bf_meshweld.h"

using namespace bf;

namespace {

constexpr uint32_t WG = 256;
constexpr uint32_t TILE = 1024;                 // 4 consecutive elements per thread
constexpr uint32_t EMPTY = 0xFFFFFFFFu;
constexpr uint32_t MAX_GRID = 8192;
constexpr uint32_t MAX_TRIANGLES = 300000000u;  // 2 * 3T rounded up to a power of two stays below 2^32

struct Key3 { long long x, y, z; };

BF_DEV long long axisKey(float p) { return (long long)floor(__dadd_rn(__dmul_rn((double)p, 1.0 / 0.00001), 0.5)); }
BF_DEV Key3 cornerKey(const float* __restrict__ tris, uint32_t i) {
    const float* p = tris + (size_t)(i / 3u) * 18u + (i % 3u) * 6u;
    Key3 k; k.x = axisKey(p[0]); k.y = axisKey(p[1]); k.z = axisKey(p[2]);
    return k;
}
BF_DEV bool same(const Key3& a, const Key3& b) { return a.x == b.x && a.y == b.y && a.z == b.z; }
BF_DEV uint32_t mix(unsigned long long a, unsigned long long b, unsigned long long c) {
    unsigned long long h = a * 0x9E3779B97F4A7C15ull;
    h = (h ^ (h >> 31) ^ b) * 0xC2B2AE3D27D4EB4Full;
    h = (h ^ (h >> 29) ^ c) * 0x165667B19E3779F9ull;
    return (uint32_t)(h >> 32) ^ (uint32_t)h;
}
BF_DEV uint32_t hashKey(const Key3& k) { return mix((unsigned long long)k.x, (unsigned long long)k.y, (unsigned long long)k.z); }

struct Tri3 { uint32_t a, b, c; };          // sorted
BF_DEV Tri3 faceKey(const uint32_t* __restrict__ ids, uint32_t t, bool& degenerate) {
    uint32_t a = ids[3 * (size_t)t], b = ids[3 * (size_t)t + 1], c = ids[3 * (size_t)t + 2];
    degenerate = a == b || b == c || a == c;
    uint32_t x;
    if (a > b) { x = a; a = b; b = x; }
    if (b > c) { x = b; b = c; c = x; }
    if (a > b) { x = a; a = b; b = x; }
    Tri3 r; r.a = a; r.b = b; r.c = c;
    return r;
}
BF_DEV bool same(const Tri3& p, const Tri3& q) { return p.a == q.a && p.b == q.b && p.c == q.c; }
BF_DEV uint32_t hashKey(const Tri3& k) { return mix(k.a, k.b, k.c); }

// the key of number i in its source: a corner of the triangle buffer, or a triangle of the id buffer
BF_DEV Key3 keyAt(const float* __restrict__ tris, uint32_t i) { return cornerKey(tris, i); }
BF_DEV Tri3 keyAt(const uint32_t* __restrict__ ids, uint32_t t) { bool d; return faceKey(ids, t, d); }

__global__ __launch_bounds__(256) void k_weld_fill(uint32_t* __restrict__ a, uint32_t n, uint32_t v) {
    for (uint32_t i = blockIdx.x * WG + threadIdx.x; i < n; i += gridDim.x * WG) a[i] = v;
}

// the insert of the protocol above; slot values only ever decrease, so a corner above the value just seen has nothing to write
template <typename K, typename S>
BF_DEV void tableInsert(uint32_t* table, uint32_t mask, uint32_t i, const K& key, const S* __restrict__ src) {
    uint32_t h = hashKey(key) & mask;
    for (uint32_t probes = 0; probes <= mask; ++probes, h = (h + 1u) & mask) {
        const uint32_t prev = atomicCAS(&table[h], EMPTY, i);
        if (prev == EMPTY) return;
        if (same(keyAt(src, prev), key)) { if (i < prev) atomicMin(&table[h], i); return; }
    }
}
// after the insert kernel: the slot of the key holds its lowest number
template <typename K, typename S>
BF_DEV uint32_t tableFind(const uint32_t* __restrict__ table, uint32_t mask, uint32_t i, const K& key, const S* __restrict__ src) {
    uint32_t h = hashKey(key) & mask;
    for (uint32_t probes = 0; probes <= mask; ++probes, h = (h + 1u) & mask) {
        const uint32_t s = table[h];
        if (s == EMPTY) break;
        if (s == i) return i;
        if (same(keyAt(src, s), key)) return s;
    }
    return i;       // (not reached: every number was inserted)
}

__global__ __launch_bounds__(256) void k_weld_corner_insert(const float* __restrict__ tris, uint32_t n, uint32_t* table, uint32_t mask) {
    for (uint32_t i = blockIdx.x * WG + threadIdx.x; i < n; i += gridDim.x * WG) tableInsert(table, mask, i, cornerKey(tris, i), tris);
}
__global__ __launch_bounds__(256) void k_weld_corner_find(const float* __restrict__ tris, uint32_t n, const uint32_t* __restrict__ table, uint32_t mask, uint32_t* __restrict__ rep) {
    for (uint32_t i = blockIdx.x * WG + threadIdx.x; i < n; i += gridDim.x * WG) rep[i] = tableFind(table, mask, i, cornerKey(tris, i), tris);
}
__global__ __launch_bounds__(256) void k_weld_face_insert(const uint32_t* __restrict__ ids, uint32_t T, uint32_t* table, uint32_t mask) {
    for (uint32_t t = blockIdx.x * WG + threadIdx.x; t < T; t += gridDim.x * WG) {
        bool degenerate;
        const Tri3 k = faceKey(ids, t, degenerate);
        if (!degenerate) tableInsert(table, mask, t, k, ids);
    }
}
__global__ __launch_bounds__(256) void k_weld_face_find(const uint32_t* __restrict__ ids, uint32_t T, const uint32_t* __restrict__ table, uint32_t mask, uint32_t* __restrict__ faceRep) {
    for (uint32_t t = blockIdx.x * WG + threadIdx.x; t < T; t += gridDim.x * WG) {
        bool degenerate;
        const Tri3 k = faceKey(ids, t, degenerate);
        faceRep[t] = degenerate ? EMPTY : tableFind(table, mask, t, k, ids);
    }
}

// elements that are their own representative (rep[i] == i), per tile
__global__ __launch_bounds__(256) void k_weld_tile_count(const uint32_t* __restrict__ rep, uint32_t n, uint32_t numTiles, uint32_t* __restrict__ tileCounts) {
    __shared__ uint32_t ws[4];
    for (uint32_t tile = blockIdx.x; tile < numTiles; tile += gridDim.x) {
        uint32_t c = 0;
        for (uint32_t k = 0; k < 4; ++k) { const uint32_t i = tile * TILE + threadIdx.x * 4 + k; if (i < n && rep[i] == i) ++c; }
        c = (uint32_t)wave_sum_i((int)c);
        if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = c;
        __syncthreads();
        if (threadIdx.x == 0) tileCounts[tile] = ws[0] + ws[1] + ws[2] + ws[3];
        __syncthreads();
    }
}
// exclusive scan of the tile counts in place by one workgroup (3T / 1024 values, not 3T); the total -> *total
__global__ __launch_bounds__(256) void k_weld_tile_scan(uint32_t* a, uint32_t n, uint32_t* total) {
    __shared__ uint32_t wtot[4];
    __shared__ uint32_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t base = 0; base < n; base += WG) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t x = i < n ? a[i] : 0u;
        uint32_t incl = x;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(incl, o, 64); if ((int)lane >= o) incl += y; }
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        uint32_t woff = 0;
        for (uint32_t w = 0; w < wave; ++w) woff += wtot[w];
        const uint32_t c0 = carry;
        if (i < n) a[i] = c0 + woff + incl - x;
        __syncthreads();
        if (threadIdx.x == WG - 1) carry = c0 + woff + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}
// rank of the tile's own representatives behind the tile's offset; VERTS: write vid, position (transformed) and colour; else: write the kept face's ids
template <bool VERTS>
__global__ __launch_bounds__(256) void k_weld_tile_scatter(const uint32_t* __restrict__ rep, uint32_t n, uint32_t numTiles, const uint32_t* __restrict__ tileOffsets, uint32_t capacity,
                                                           const float* __restrict__ tris, m44 xf, int hasXf, uint32_t* __restrict__ vid, float* __restrict__ positions,
                                                           float* __restrict__ colors, const uint32_t* __restrict__ faceIds, uint32_t* __restrict__ faces) {
    __shared__ uint32_t wscan[4];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t tile = blockIdx.x; tile < numTiles; tile += gridDim.x) {
        bool own[4]; uint32_t c = 0;
        for (uint32_t k = 0; k < 4; ++k) { const uint32_t i = tile * TILE + threadIdx.x * 4 + k; own[k] = i < n && rep[i] == i; c += own[k] ? 1u : 0u; }
        uint32_t incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(incl, o, 64); if ((int)lane >= o) incl += y; }
        if (lane == 63) wscan[wave] = incl;
        __syncthreads();
        uint32_t woff = 0;
        for (uint32_t w = 0; w < wave; ++w) woff += wscan[w];
        uint32_t pos = tileOffsets[tile] + woff + incl - c;
        for (uint32_t k = 0; k < 4; ++k) {
            if (!own[k]) continue;
            const uint32_t i = tile * TILE + threadIdx.x * 4 + k;
            const uint32_t id = pos++;
            if (id >= capacity) continue;
            if (VERTS) {
                vid[i] = id;
                const float* p = tris + (size_t)(i / 3u) * 18u + (i % 3u) * 6u;
                f3 q = mk3(p[0], p[1], p[2]);
                if (hasXf) q = xform(xf, q);
                positions[3 * (size_t)id] = q.x; positions[3 * (size_t)id + 1] = q.y; positions[3 * (size_t)id + 2] = q.z;
                colors[3 * (size_t)id] = p[3]; colors[3 * (size_t)id + 1] = p[4]; colors[3 * (size_t)id + 2] = p[5];
            } else {
                faces[3 * (size_t)id] = faceIds[3 * (size_t)i]; faces[3 * (size_t)id + 1] = faceIds[3 * (size_t)i + 1]; faces[3 * (size_t)id + 2] = faceIds[3 * (size_t)i + 2];
            }
        }
        __syncthreads();
    }
}
__global__ __launch_bounds__(256) void k_weld_face_ids(const uint32_t* __restrict__ rep, const uint32_t* __restrict__ vid, uint32_t n, uint32_t* __restrict__ faceIds) {
    for (uint32_t i = blockIdx.x * WG + threadIdx.x; i < n; i += gridDim.x * WG) faceIds[i] = vid[rep[i]];
}

uint32_t gridFor(uint32_t n) { return std::max(1u, std::min(div_up(n, WG), MAX_GRID)); }

}  // namespace

namespace bf {

int meshweld_run(MeshWeld& w, Resources& res, hipStream_t st, const bf_mc_triangle* d_triangles, uint32_t T, const float transform[16]) {
    w.numVertices = w.numFaces = 0;
    if (T == 0) return BF_OK;
    BF_REQUIRE(d_triangles, "null triangle buffer");
    BF_REQUIRE(T <= MAX_TRIANGLES, "too many triangles for one weld");
    const uint32_t n = 3u * T;
    uint32_t cap = 1024;
    while (cap < 2u * n) cap <<= 1;
    const uint32_t mask = cap - 1u;
    const uint32_t tilesV = div_up(n, TILE), tilesF = div_up(T, TILE);
    if (cap > w.capTable) { w.capTable = 0; BF_TRY(res.regrow(&w.d_table, cap)); w.capTable = cap; }
    if (T > w.capTriangles) {
        w.capTriangles = 0;
        BF_TRY(res.regrow(&w.d_rep, n)); BF_TRY(res.regrow(&w.d_vid, n)); BF_TRY(res.regrow(&w.d_faceIds, n));
        BF_TRY(res.regrow(&w.d_faceRep, T)); BF_TRY(res.regrow(&w.d_tiles, tilesV));
        w.capTriangles = T;
    }
    if (!w.d_totals) BF_TRY(res.device(&w.d_totals, 2));
    const float* tris = (const float*)d_triangles;
    m44 xf; memset(&xf, 0, sizeof xf);
    if (transform) memcpy(xf.e, transform, 64);
    const int hasXf = transform ? 1 : 0;

    // ---- vertices
    hipLaunchKernelGGL(k_weld_fill, dim3(gridFor(cap)), dim3(WG), 0, st, w.d_table, cap, EMPTY);
    hipLaunchKernelGGL(k_weld_corner_insert, dim3(gridFor(n)), dim3(WG), 0, st, tris, n, w.d_table, mask);
    hipLaunchKernelGGL(k_weld_corner_find, dim3(gridFor(n)), dim3(WG), 0, st, tris, n, (const uint32_t*)w.d_table, mask, w.d_rep);
    hipLaunchKernelGGL(k_weld_tile_count, dim3(std::min(tilesV, MAX_GRID)), dim3(WG), 0, st, (const uint32_t*)w.d_rep, n, tilesV, w.d_tiles);
    hipLaunchKernelGGL(k_weld_tile_scan, dim3(1), dim3(WG), 0, st, w.d_tiles, tilesV, w.d_totals);
    BF_HIP_TRY(hipGetLastError());
    uint32_t nv = 0;
    BF_HIP_TRY(hipMemcpyAsync(&nv, w.d_totals, 4, hipMemcpyDeviceToHost, st));
    BF_HIP_TRY(hipStreamSynchronize(st));
    BF_REQUIRE(nv >= 1 && nv <= n, "vertex count out of range");
    if (nv > w.capVertices) {
        w.capVertices = 0;
        BF_TRY(res.regrow(&w.d_positions, 3 * (size_t)nv)); BF_TRY(res.regrow(&w.d_colors, 3 * (size_t)nv));
        w.capVertices = nv;
    }
    hipLaunchKernelGGL(k_weld_tile_scatter<true>, dim3(std::min(tilesV, MAX_GRID)), dim3(WG), 0, st, (const uint32_t*)w.d_rep, n, tilesV, (const uint32_t*)w.d_tiles, nv, tris, xf, hasXf,
                       w.d_vid, w.d_positions, w.d_colors, (const uint32_t*)nullptr, (uint32_t*)nullptr);
    hipLaunchKernelGGL(k_weld_face_ids, dim3(gridFor(n)), dim3(WG), 0, st, (const uint32_t*)w.d_rep, (const uint32_t*)w.d_vid, n, w.d_faceIds);

    // ---- faces
    hipLaunchKernelGGL(k_weld_fill, dim3(gridFor(cap)), dim3(WG), 0, st, w.d_table, cap, EMPTY);
    hipLaunchKernelGGL(k_weld_face_insert, dim3(gridFor(T)), dim3(WG), 0, st, (const uint32_t*)w.d_faceIds, T, w.d_table, mask);
    hipLaunchKernelGGL(k_weld_face_find, dim3(gridFor(T)), dim3(WG), 0, st, (const uint32_t*)w.d_faceIds, T, (const uint32_t*)w.d_table, mask, w.d_faceRep);
    hipLaunchKernelGGL(k_weld_tile_count, dim3(std::min(tilesF, MAX_GRID)), dim3(WG), 0, st, (const uint32_t*)w.d_faceRep, T, tilesF, w.d_tiles);
    hipLaunchKernelGGL(k_weld_tile_scan, dim3(1), dim3(WG), 0, st, w.d_tiles, tilesF, w.d_totals + 1);
    BF_HIP_TRY(hipGetLastError());
    uint32_t nf = 0;
    BF_HIP_TRY(hipMemcpyAsync(&nf, w.d_totals + 1, 4, hipMemcpyDeviceToHost, st));
    BF_HIP_TRY(hipStreamSynchronize(st));
    BF_REQUIRE(nf <= T, "face count out of range");
    if (nf > w.capFaces) { w.capFaces = 0; BF_TRY(res.regrow(&w.d_faces, 3 * (size_t)nf)); w.capFaces = nf; }
    if (nf) {
        hipLaunchKernelGGL(k_weld_tile_scatter<false>, dim3(std::min(tilesF, MAX_GRID)), dim3(WG), 0, st, (const uint32_t*)w.d_faceRep, T, tilesF, (const uint32_t*)w.d_tiles, nf,
                           (const float*)nullptr, xf, 0, (uint32_t*)nullptr, (float*)nullptr, (float*)nullptr, (const uint32_t*)w.d_faceIds, w.d_faces);
        BF_HIP_TRY(hipGetLastError());
    }
    w.numVertices = nv; w.numFaces = nf;
    return BF_OK;
}

}  // namespace bf

// The one PLY writer (binary little-endian, per-vertex colours): 16-byte vertex records (3 floats, RGBA bytes with alpha 255), 13-byte face records.  Host only.
extern "C" int bf_write_ply_indexed(const char* filename, const float* h_positions, const float* h_colors, const uint32_t* h_faces, uint32_t numVertices, uint32_t numFaces) {
    BF_REQUIRE(filename, "null argument");
    BF_REQUIRE((numVertices == 0 || (h_positions && h_colors)) && (numFaces == 0 || h_faces), "null array");
    FILE* f = fopen(filename, "wb");
    if (!f) { set_error("cannot open %s", filename); return BF_ERR_INVALID_ARG; }
    fprintf(f, "ply\nformat binary_little_endian 1.0\ncomment bundlefusion_amd marching cubes\nelement vertex %u\nproperty float x\nproperty float y\nproperty float z\n"
               "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\nelement face %u\nproperty list uchar int vertex_indices\nend_header\n", numVertices, numFaces);
    const size_t CH = 65536;            // records per write
    std::vector<uint8_t> buf(CH * 16);
    for (size_t base = 0; base < numVertices; base += CH) {
        const size_t m = std::min(CH, (size_t)numVertices - base);
        for (size_t j = 0; j < m; ++j) {
            const size_t i = base + j;
            uint8_t* r = buf.data() + 16 * j;
            memcpy(r, h_positions + 3 * i, 12);
            for (int k = 0; k < 3; ++k) r[12 + k] = (uint8_t)std::max(0.0f, std::min(255.0f, h_colors[3 * i + k] * 255.0f + 0.5f));
            r[15] = 255;
        }
        fwrite(buf.data(), 16, m, f);
    }
    for (size_t base = 0; base < numFaces; base += CH) {
        const size_t m = std::min(CH, (size_t)numFaces - base);
        for (size_t j = 0; j < m; ++j) {
            uint8_t* r = buf.data() + 13 * j;
            r[0] = 3;
            memcpy(r + 1, h_faces + 3 * (base + j), 12);          // int32 in the file: the same bits
        }
        fwrite(buf.data(), 13, m, f);
    }
    const bool bad = ferror(f) != 0;
    if (fclose(f) != 0 || bad) { set_error("cannot write %s", filename); return BF_ERR_INVALID_ARG; }
    return BF_OK;
}
