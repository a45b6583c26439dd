// The scan as a point cloud on the device, for gfx950: SiftVisualization::computePointCloud per frame and sparsifyUniform over the union (include/bf_pointcloud.h)
// without a frame leaving HBM.  DESIGN.md 1 "Point cloud" is the definition, bf_point_cloud_build_host below is that definition as the sequential loop, and
// tests/point_cloud_ref.py restates it in numpy; the three agree as bits.  Nothing here depends on the order in which threads run: "the first point of a cell" is a
// minimum over candidate numbers, never "who arrived first".
//
//   k_pc_candidates   a 64x4 tile of pixels per workgroup, one lane per pixel.  The tile's depths with a one-pixel halo (66 x 6) are loaded once and every camera
//                     position is formed once into LDS (three planes + the depth, row stride 67 words), not five times per pixel.  Banks: ds_read_b32 / ds_write_b32
//                     take bank = word mod 32 within each 32-lane half; a half reads words c .. c + 31 of one row (c, c - 1, c + 1, c - 67, c + 67 alike): 32
//                     different banks.  The fill walks t -> (t / 66) * 67 + t % 66: consecutive words except one skipped word where a half crosses a row end - at
//                     most one two-way conflict per half.  Output: one staging record per pixel, two float4 (P.xyz + colour, N.xyz + candidate flag).
//   k_pc_insert       the cell table: open addressing, linear probing, one uint32 per slot, the power of two >= 2 * (maxPoints + maxFramePixels) slots - never more
//                     than half full, even in a frame that overflows the cloud.  A slot holds the index of a point of the cloud (< 2^31) or TAG | pixel number of
//                     the current frame; its cell is recomputed from the cloud's stored position or from the staging record (the stored P is the value the cell was
//                     formed from).  Insert of candidate i at slot h: prev = atomicCAS(slot, EMPTY, TAG | i); EMPTY: done; cell(prev) == cell(i): done if prev is a
//                     point of the cloud, atomicMin(slot, TAG | i) otherwise; else the next slot.  Every value ever written to a slot has the cell of the slot's first
//                     occupant, so probe sequences take the same turns while the minimum settles; points of the cloud order below every tagged value.
//                     Coherence (DESIGN.md "Mesh weld"): inside this kernel a slot is read through the result of an agent-scope atomic only; the kernels after it
//                     start behind the kernel boundary and use plain loads.
//   k_pc_flag_count   per candidate the slot of its cell; it is a point iff the slot holds its own tagged number.  Per tile of 1024 pixels the number of points.
//   k_pc_tile_scan    exclusive scan of the tile counts by one workgroup; the frame's total.
//   k_pc_scatter      rank inside the tile; position, normal and colour behind the cloud's end, and the slot's tagged value replaced by the point's index.
// No float atomics, no atomics on counters.  One host read per frame: the total.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "bf_device.h"
#include "bf_pointcloud.h"
#include "bf_resources.h"

using namespace bf;

namespace {

constexpr int TW = 64, TH = 4;                        // pixels per tile of k_pc_candidates
constexpr int VW = TW + 2, VH = TH + 2;               // with the halo
constexpr int VS = VW + 1;                            // row stride in words (odd)
constexpr uint32_t WG = 256;
constexpr uint32_t TILE = 1024;                       // 4 consecutive pixels per thread
constexpr uint32_t EMPTY = 0xFFFFFFFFu, NONE = 0xFFFFFFFFu;
constexpr uint32_t TAG = 0x80000000u;
constexpr uint32_t MAX_GRID = 8192;
constexpr uint32_t MAX_ENTRIES = 1u << 30;            // maxPoints + maxFramePixels: twice that many slots still fit 32 bits, and TAG | pixel stays below EMPTY

struct Cell3 { long long x, y, z; };
BF_DEV Cell3 cellOf(float x, float y, float z, double inv) { Cell3 c; c.x = pcCell(x, inv); c.y = pcCell(y, inv); c.z = pcCell(z, inv); return c; }
BF_DEV bool same(const Cell3& a, const Cell3& b) { return a.x == b.x && a.y == b.y && a.z == b.z; }
BF_DEV uint32_t hashCell(const Cell3& k) {
    unsigned long long h = (unsigned long long)k.x * 0x9E3779B97F4A7C15ull;
    h = (h ^ (h >> 31) ^ (unsigned long long)k.y) * 0xC2B2AE3D27D4EB4Full;
    h = (h ^ (h >> 29) ^ (unsigned long long)k.z) * 0x165667B19E3779F9ull;
    return (uint32_t)(h >> 32) ^ (uint32_t)h;
}
// the cell of a slot's value: a tagged pixel of the frame (staging) or a point of the cloud
BF_DEV Cell3 cellAt(uint32_t v, const float4* __restrict__ stage, const float* __restrict__ positions, double inv) {
    if (v & TAG) { const float4 s = stage[2 * (size_t)(v & ~TAG)]; return cellOf(s.x, s.y, s.z, inv); }
    const float* p = positions + 3 * (size_t)v;
    return cellOf(p[0], p[1], p[2], inv);
}

__global__ __launch_bounds__(256) void k_pc_fill(uint32_t* __restrict__ a, uint32_t n, uint32_t v) {
    for (uint32_t i = blockIdx.x * WG + threadIdx.x; i < n; i += gridDim.x * WG) a[i] = v;
}

__global__ __launch_bounds__(256) void k_pc_candidates(const float* __restrict__ depth, const uint32_t* __restrict__ color, float4* __restrict__ stage, PcFrame F) {
    __shared__ float sD[VH * VS], sX[VH * VS], sY[VH * VS], sZ[VH * VS];
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    for (int t = threadIdx.y * TW + threadIdx.x; t < VH * VW; t += TW * TH) {
        const int ly = t / VW, lx = t - ly * VW, x = x0 - 1 + lx, y = y0 - 1 + ly;
        const bool in = x >= 0 && y >= 0 && x < F.w && y < F.h;
        const float d = in ? depth[(size_t)y * F.w + x] : 0.0f;                 // outside the image: no position
        const float dp = pcHasPosition(d) ? d : 0.0f;                           // (a position nobody uses)
        const f3 p = pcPosition(F, x, y, dp);
        const int o = ly * VS + lx;
        sD[o] = d; sX[o] = p.x; sY[o] = p.y; sZ[o] = p.z;
    }
    __syncthreads();
    const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
    if (x >= F.w || y >= F.h) return;
    const size_t idx = (size_t)y * F.w + x;
    const uint32_t texel = color[idx];
    const int c = (threadIdx.y + 1) * VS + threadIdx.x + 1;                     // this pixel; c - 1 / c + 1 / c - VS / c + VS: its neighbours
    bool ok = x > 0 && y > 0 && x + 1 < F.w && y + 1 < F.h;
    ok = ok && pcHasPosition(sD[c]) && pcHasPosition(sD[c - 1]) && pcHasPosition(sD[c + 1]) && pcHasPosition(sD[c - VS]) && pcHasPosition(sD[c + VS]);
    PcPoint q;
    q.P = mk3(0.0f, 0.0f, 0.0f); q.N = q.P; q.rgba = 0u;
    if (ok)
        ok = pcCandidate(F, mk3(sX[c], sY[c], sZ[c]), mk3(sX[c - 1], sY[c - 1], sZ[c - 1]), mk3(sX[c + 1], sY[c + 1], sZ[c + 1]), mk3(sX[c - VS], sY[c - VS], sZ[c - VS]),
                         mk3(sX[c + VS], sY[c + VS], sZ[c + VS]), texel, q);
    stage[2 * idx] = make_float4(q.P.x, q.P.y, q.P.z, __uint_as_float(q.rgba));
    stage[2 * idx + 1] = make_float4(q.N.x, q.N.y, q.N.z, __uint_as_float(ok ? 1u : 0u));
}

BF_DEV bool isCandidate(const float4* __restrict__ stage, uint32_t i) { return __float_as_uint(stage[2 * (size_t)i + 1].w) != 0u; }

__global__ __launch_bounds__(256) void k_pc_insert(const float4* __restrict__ stage, uint32_t n, const float* __restrict__ positions, uint32_t* table, uint32_t mask, double inv) {
    for (uint32_t i = blockIdx.x * WG + threadIdx.x; i < n; i += gridDim.x * WG) {
        if (!isCandidate(stage, i)) continue;
        const float4 s = stage[2 * (size_t)i];
        const Cell3 key = cellOf(s.x, s.y, s.z, inv);
        const uint32_t me = TAG | i;
        uint32_t h = hashCell(key) & mask;
        for (uint32_t probes = 0; probes <= mask; ++probes, h = (h + 1u) & mask) {
            const uint32_t prev = atomicCAS(&table[h], EMPTY, me);
            if (prev == EMPTY) break;
            if (same(cellAt(prev, stage, positions, inv), key)) { if ((prev & TAG) && me < prev) atomicMin(&table[h], me); break; }
        }
    }
}

// d_own[i]: the slot whose value is TAG | i (thin), 0 for every candidate (no thinning), NONE otherwise - also for the tile's pixels past the frame's end
__global__ __launch_bounds__(256) void k_pc_flag_count(const float4* __restrict__ stage, uint32_t n, uint32_t numTiles, const float* __restrict__ positions,
                                                       const uint32_t* __restrict__ table, uint32_t mask, double inv, int thin, uint32_t* __restrict__ own,
                                                       uint32_t* __restrict__ tileCounts) {
    __shared__ uint32_t ws[4];
    for (uint32_t tile = blockIdx.x; tile < numTiles; tile += gridDim.x) {
        uint32_t c = 0;
        uint32_t o[4];
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t i = tile * TILE + threadIdx.x * 4 + k;
            o[k] = NONE;
            if (i >= n || !isCandidate(stage, i)) continue;
            if (!thin) { o[k] = 0u; ++c; continue; }
            const float4 s = stage[2 * (size_t)i];
            const Cell3 key = cellOf(s.x, s.y, s.z, inv);
            const uint32_t me = TAG | i;
            uint32_t h = hashCell(key) & mask;
            for (uint32_t probes = 0; probes <= mask; ++probes, h = (h + 1u) & mask) {
                const uint32_t v = table[h];
                if (v == me) { o[k] = h; ++c; break; }
                if (v == EMPTY) break;                                           // (not reached: every candidate was inserted)
                if (same(cellAt(v, stage, positions, inv), key)) break;        // the cell has an older point or a lower candidate
            }
        }
        *reinterpret_cast<uint4*>(own + (size_t)tile * TILE + threadIdx.x * 4) = make_uint4(o[0], o[1], o[2], o[3]);
        c = (uint32_t)wave_sum_i((int)c);
        if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = c;
        __syncthreads();
        if (threadIdx.x == 0) tileCounts[tile] = ws[0] + ws[1] + ws[2] + ws[3];
        __syncthreads();
    }
}

// exclusive scan of the tile counts in place by one workgroup, 256 per step; the total -> *total
__global__ __launch_bounds__(256) void k_pc_tile_scan(uint32_t* a, uint32_t n, uint32_t* total) {
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

// points behind the cloud's end `base` in pixel order; a point past `capacity` is not written (the frame overflows: the host sees the total)
__global__ __launch_bounds__(256) void k_pc_scatter(const float4* __restrict__ stage, uint32_t numTiles, const uint32_t* __restrict__ own, const uint32_t* __restrict__ tileOffsets,
                                                    uint32_t base, uint32_t capacity, int thin, uint32_t* __restrict__ table, float* __restrict__ positions,
                                                    float* __restrict__ normals, uint32_t* __restrict__ colors) {
    __shared__ uint32_t wscan[4];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t tile = blockIdx.x; tile < numTiles; tile += gridDim.x) {
        const uint4 o4 = *reinterpret_cast<const uint4*>(own + (size_t)tile * TILE + threadIdx.x * 4);
        const uint32_t o[4] = {o4.x, o4.y, o4.z, o4.w};
        uint32_t c = 0;
        for (uint32_t k = 0; k < 4; ++k) c += o[k] != NONE ? 1u : 0u;
        uint32_t incl = c;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) { const uint32_t y = __shfl_up(incl, s, 64); if ((int)lane >= s) incl += y; }
        if (lane == 63) wscan[wave] = incl;
        __syncthreads();
        uint32_t woff = 0;
        for (uint32_t w = 0; w < wave; ++w) woff += wscan[w];
        uint32_t rank = tileOffsets[tile] + woff + incl - c;
        for (uint32_t k = 0; k < 4; ++k) {
            if (o[k] == NONE) continue;
            const uint32_t r = rank++;
            if (r >= capacity - base) continue;
            const uint32_t id = base + r;
            const size_t i = (size_t)tile * TILE + threadIdx.x * 4 + k;
            const float4 a = stage[2 * i], b = stage[2 * i + 1];
            positions[3 * (size_t)id] = a.x; positions[3 * (size_t)id + 1] = a.y; positions[3 * (size_t)id + 2] = a.z;
            normals[3 * (size_t)id] = b.x; normals[3 * (size_t)id + 1] = b.y; normals[3 * (size_t)id + 2] = b.z;
            colors[id] = __float_as_uint(a.w);
            if (thin) table[o[k]] = id;
        }
        __syncthreads();
    }
}

uint32_t gridFor(uint32_t n) { return std::max(1u, std::min(div_up(n, WG), MAX_GRID)); }

int failOverflowed(const bf_point_cloud* pc) {
    set_error("bf_point_cloud: the cloud overflowed its capacity of %u points (bf_point_cloud_params.maxPoints); bf_point_cloud_reset clears it", pc->params.maxPoints);
    return BF_ERR_CAPACITY;
}

void frameOf(PcFrame& F, const float intrinsicsInv[16], const float transform[16], float maxDepth, float cellSize, int w, int h) {
    memcpy(F.k, intrinsicsInv, 48); memcpy(F.t, transform, 48);
    F.maxDepth = maxDepth;
    F.thin = cellSize > 0.0f ? 1 : 0;
    F.inv = F.thin ? 1.0 / (double)cellSize : 0.0;
    F.w = w; F.h = h;
}
bool poseInvalid(const float transform[16]) { return transform[0] != transform[0] || transform[0] == BF_MINF; }      // computePointCloud's first test (:531)

}  // namespace

extern "C" {

int bf_point_cloud_create(const bf_point_cloud_params* params, bf_point_cloud** out) {
    BF_REQUIRE(params && out, "null argument");
    BF_REQUIRE(params->maxPoints >= 1 && params->maxFramePixels >= 1, "maxPoints and maxFramePixels must be at least 1");
    BF_REQUIRE((uint64_t)params->maxPoints + params->maxFramePixels <= MAX_ENTRIES, "maxPoints + maxFramePixels must not exceed 2^30");
    BF_REQUIRE(params->cellSize == params->cellSize && params->maxDepth == params->maxDepth, "cellSize / maxDepth is NaN");
    bf_point_cloud* pc = new bf_point_cloud;
    bf::CreateGuard<bf_point_cloud> guard(pc, bf_point_cloud_destroy);
    pc->params = *params;
    pc->thin = params->cellSize > 0.0f;
    pc->inv = pc->thin ? 1.0 / (double)params->cellSize : 0.0;
    const uint32_t tiles = div_up(params->maxFramePixels, TILE);
    BF_TRY(pc->res.device(&pc->d_positions, 3 * (size_t)params->maxPoints));
    BF_TRY(pc->res.device(&pc->d_normals, 3 * (size_t)params->maxPoints));
    BF_TRY(pc->res.device(&pc->d_colors, (size_t)params->maxPoints));
    BF_TRY(pc->res.device(&pc->d_stage, 2 * (size_t)params->maxFramePixels));
    BF_TRY(pc->res.device(&pc->d_own, (size_t)tiles * TILE));
    BF_TRY(pc->res.device(&pc->d_tiles, (size_t)tiles));
    BF_TRY(pc->res.device(&pc->d_total, 1));
    if (pc->thin) {
        uint32_t slots = 1024;
        while (slots < 2u * (params->maxPoints + params->maxFramePixels)) slots <<= 1;
        BF_TRY(pc->res.device(&pc->d_table, (size_t)slots));
        pc->slots = slots;
    }
    BF_TRY(bf_point_cloud_reset(pc));
    BF_HIP_TRY(hipStreamSynchronize(pc->stream));
    *out = guard.dismiss();
    return BF_OK;
}

int bf_point_cloud_destroy(bf_point_cloud* pc) {
    if (!pc) return BF_OK;
    (void)hipDeviceSynchronize();
    delete pc;
    return BF_OK;
}

int bf_point_cloud_set_stream(bf_point_cloud* pc, void* s) {
    BF_REQUIRE(pc, "null argument");
    BF_HIP_TRY(hipStreamSynchronize(pc->stream));          // the table's fill was enqueued there
    pc->stream = (hipStream_t)s;
    return BF_OK;
}

int bf_point_cloud_reset(bf_point_cloud* pc) {
    BF_REQUIRE(pc, "null argument");
    if (pc->thin) {
        hipLaunchKernelGGL(k_pc_fill, dim3(gridFor(pc->slots)), dim3(WG), 0, pc->stream, pc->d_table, pc->slots, EMPTY);
        BF_HIP_TRY(hipGetLastError());
    }
    pc->numPoints = 0;
    pc->overflowed = false;
    return BF_OK;
}

int bf_point_cloud_add_frame(bf_point_cloud* pc, const float* d_depth, const uint8_t* d_colorRGBX, uint32_t width, uint32_t height, const float intrinsicsInv[16],
                             const float transform[16], uint32_t* numAdded) {
    BF_REQUIRE(pc && d_depth && d_colorRGBX && intrinsicsInv && transform, "null argument");
    if (numAdded) *numAdded = 0;
    if (pc->overflowed) return failOverflowed(pc);
    BF_REQUIRE(width >= 1 && height >= 1 && height <= 4u * 65535u, "image size out of range");
    BF_REQUIRE((uint64_t)width * height <= pc->params.maxFramePixels, "width * height exceeds bf_point_cloud_params.maxFramePixels");
    if (poseInvalid(transform)) return BF_OK;
    const uint32_t n = width * height, tiles = div_up(n, TILE), mask = pc->slots ? pc->slots - 1u : 0u;
    PcFrame F;
    frameOf(F, intrinsicsInv, transform, pc->params.maxDepth, pc->params.cellSize, (int)width, (int)height);
    hipStream_t st = pc->stream;
    const int thin = pc->thin ? 1 : 0;
    hipLaunchKernelGGL(k_pc_candidates, dim3(div_up(width, TW), div_up(height, TH)), dim3(TW, TH), 0, st, d_depth, (const uint32_t*)d_colorRGBX, pc->d_stage, F);
    if (thin) hipLaunchKernelGGL(k_pc_insert, dim3(gridFor(n)), dim3(WG), 0, st, (const float4*)pc->d_stage, n, (const float*)pc->d_positions, pc->d_table, mask, pc->inv);
    hipLaunchKernelGGL(k_pc_flag_count, dim3(std::min(tiles, MAX_GRID)), dim3(WG), 0, st, (const float4*)pc->d_stage, n, tiles, (const float*)pc->d_positions,
                       (const uint32_t*)pc->d_table, mask, pc->inv, thin, pc->d_own, pc->d_tiles);
    hipLaunchKernelGGL(k_pc_tile_scan, dim3(1), dim3(WG), 0, st, pc->d_tiles, tiles, pc->d_total);
    hipLaunchKernelGGL(k_pc_scatter, dim3(std::min(tiles, MAX_GRID)), dim3(WG), 0, st, (const float4*)pc->d_stage, tiles, (const uint32_t*)pc->d_own, (const uint32_t*)pc->d_tiles,
                       pc->numPoints, pc->params.maxPoints, thin, pc->d_table, pc->d_positions, pc->d_normals, pc->d_colors);
    BF_HIP_TRY(hipGetLastError());
    uint32_t total = 0;
    BF_HIP_TRY(hipMemcpyAsync(&total, pc->d_total, 4, hipMemcpyDeviceToHost, st));
    BF_HIP_TRY(hipStreamSynchronize(st));
    BF_REQUIRE(total <= n, "point count out of range");
    if (total > pc->params.maxPoints - pc->numPoints) { pc->overflowed = true; return failOverflowed(pc); }
    pc->numPoints += total;
    if (numAdded) *numAdded = total;
    return BF_OK;
}

int bf_point_cloud_get_gpu(bf_point_cloud* pc, bf_point_cloud_view* out) {
    BF_REQUIRE(pc && out, "null argument");
    if (pc->overflowed) return failOverflowed(pc);
    out->d_positions = pc->d_positions; out->d_normals = pc->d_normals; out->d_colors = (const uint8_t*)pc->d_colors; out->numPoints = pc->numPoints;
    return BF_OK;
}

int bf_point_cloud_download(bf_point_cloud* pc, float* h_positions, float* h_normals, uint8_t* h_colors, uint32_t capacity, uint32_t* numPoints) {
    BF_REQUIRE(pc, "null argument");
    if (pc->overflowed) return failOverflowed(pc);
    if (numPoints) *numPoints = pc->numPoints;
    const size_t m = std::min(capacity, pc->numPoints);
    if (m) {
        if (h_positions) BF_HIP_TRY(hipMemcpyAsync(h_positions, pc->d_positions, 12 * m, hipMemcpyDeviceToHost, pc->stream));
        if (h_normals) BF_HIP_TRY(hipMemcpyAsync(h_normals, pc->d_normals, 12 * m, hipMemcpyDeviceToHost, pc->stream));
        if (h_colors) BF_HIP_TRY(hipMemcpyAsync(h_colors, pc->d_colors, 4 * m, hipMemcpyDeviceToHost, pc->stream));
    }
    BF_HIP_TRY(hipStreamSynchronize(pc->stream));
    return BF_OK;
}

int bf_point_cloud_save(bf_point_cloud* pc, const char* filename, uint32_t* numPoints) {
    BF_REQUIRE(pc && filename, "null argument");
    if (pc->overflowed) return failOverflowed(pc);
    const size_t n = pc->numPoints;
    std::vector<float> pos(3 * std::max<size_t>(n, 1)), nrm(3 * std::max<size_t>(n, 1));
    std::vector<uint8_t> col(4 * std::max<size_t>(n, 1));
    BF_TRY(bf_point_cloud_download(pc, pos.data(), nrm.data(), col.data(), pc->numPoints, nullptr));
    BF_TRY(bf_write_ply_points(filename, pos.data(), nrm.data(), col.data(), pc->numPoints));
    if (numPoints) *numPoints = pc->numPoints;
    return BF_OK;
}

// Host only.  The header follows bf_write_ply_indexed's; there is no face element.
int bf_write_ply_points(const char* filename, const float* h_positions, const float* h_normals, const uint8_t* h_colors, uint32_t numPoints) {
    BF_REQUIRE(filename, "null argument");
    BF_REQUIRE(numPoints == 0 || (h_positions && h_normals && h_colors), "null array");
    FILE* f = fopen(filename, "wb");
    if (!f) { set_error("cannot open %s", filename); return BF_ERR_INVALID_ARG; }
    fprintf(f, "ply\nformat binary_little_endian 1.0\ncomment bundlefusion_amd point cloud\nelement vertex %u\nproperty float x\nproperty float y\nproperty float z\n"
               "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\nend_header\n", numPoints);
    const size_t CH = 65536;            // records per write
    std::vector<uint8_t> buf(CH * 28);
    for (size_t base = 0; base < numPoints; base += CH) {
        const size_t m = std::min(CH, (size_t)numPoints - base);
        for (size_t j = 0; j < m; ++j) {
            const size_t i = base + j;
            uint8_t* r = buf.data() + 28 * j;
            memcpy(r, h_positions + 3 * i, 12); memcpy(r + 12, h_normals + 3 * i, 12); memcpy(r + 24, h_colors + 4 * i, 4);
        }
        fwrite(buf.data(), 28, m, f);
    }
    const bool bad = ferror(f) != 0;
    if (fclose(f) != 0 || bad) { set_error("cannot write %s", filename); return BF_ERR_INVALID_ARG; }
    return BF_OK;
}

// The definition as the sequential loop: frames in order, pixels in raster order, the first candidate of a cell stays.
int bf_point_cloud_build_host(const float* const* h_depths, const uint8_t* const* h_colors, uint32_t numFrames, uint32_t width, uint32_t height, const float intrinsicsInv[16],
                              const float* h_transforms, float cellSize, float maxDepth, uint32_t capacity, float* h_positions, float* h_normals, uint8_t* h_colors_out,
                              uint32_t* numPoints) {
    BF_REQUIRE(numPoints && intrinsicsInv && (numFrames == 0 || (h_depths && h_colors && h_transforms)), "null argument");
    BF_REQUIRE(cellSize == cellSize && maxDepth == maxDepth, "cellSize / maxDepth is NaN");
    BF_REQUIRE(numFrames == 0 || (width >= 1 && height >= 1 && (uint64_t)width * height < (1ull << 31)), "image size out of range");
    struct Key { long long x, y, z; bool operator==(const Key& o) const { return x == o.x && y == o.y && z == o.z; } };
    struct KeyHash { size_t operator()(const Key& k) const { return (size_t)(k.x * 73856093ll ^ k.y * 19349669ll ^ k.z * 83492791ll); } };
    std::unordered_map<Key, uint32_t, KeyHash> cells;
    uint64_t count = 0;
    const int w = (int)width, h = (int)height;
    for (uint32_t f = 0; f < numFrames; ++f) {
        const float* T = h_transforms + 16 * (size_t)f;
        if (poseInvalid(T)) continue;
        BF_REQUIRE(h_depths[f] && h_colors[f], "null frame");
        PcFrame F;
        frameOf(F, intrinsicsInv, T, maxDepth, cellSize, w, h);
        const float* D = h_depths[f];
        auto pos = [&](int x, int y) { return pcPosition(F, x, y, D[(size_t)y * w + x]); };
        for (int y = 1; y + 1 < h; ++y)
            for (int x = 1; x + 1 < w; ++x) {
                const size_t i = (size_t)y * w + x;
                if (!(pcHasPosition(D[i]) && pcHasPosition(D[i - 1]) && pcHasPosition(D[i + 1]) && pcHasPosition(D[i - w]) && pcHasPosition(D[i + w]))) continue;
                uint32_t texel;
                memcpy(&texel, h_colors[f] + 4 * i, 4);
                PcPoint q;
                if (!pcCandidate(F, pos(x, y), pos(x - 1, y), pos(x + 1, y), pos(x, y - 1), pos(x, y + 1), texel, q)) continue;
                if (F.thin) {
                    const Key key = {pcCell(q.P.x, F.inv), pcCell(q.P.y, F.inv), pcCell(q.P.z, F.inv)};
                    if (!cells.emplace(key, (uint32_t)count).second) continue;
                }
                if (count < capacity) {
                    if (h_positions) { h_positions[3 * count] = q.P.x; h_positions[3 * count + 1] = q.P.y; h_positions[3 * count + 2] = q.P.z; }
                    if (h_normals) { h_normals[3 * count] = q.N.x; h_normals[3 * count + 1] = q.N.y; h_normals[3 * count + 2] = q.N.z; }
                    if (h_colors_out) memcpy(h_colors_out + 4 * count, &q.rgba, 4);
                }
                ++count;
                if (count > 0xFFFFFFFFull) { set_error("bf_point_cloud_build_host: more than 2^32 - 1 points"); return BF_ERR_CAPACITY; }
            }
    }
    *numPoints = (uint32_t)count;
    return BF_OK;
}

}  // extern "C"
