// The device cleaning of an indexed mesh (meshclean.hip): the buffers a bf_marching_cubes object owns for it and the entry point mesh.hip calls.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bf_hip.h"
#include "bf_resources.h"

namespace bf {

// Per-vertex normals of an indexed mesh in HBM (the clean's definition; meshclean.hip): per vertex its number of corners (counted, then counted down by the fill)
// and the start of its segment (numVertices + 1 of them); the corners of every vertex as filled and, for segments longer than a wave, in increasing order; the
// vertices with such segments and their count; the result, numVertices x 3 float
struct MeshNormals {
    uint32_t *d_degree = nullptr, *d_offset = nullptr, *d_corners = nullptr, *d_sorted = nullptr, *d_long = nullptr, *d_tilesN = nullptr, *d_numLong = nullptr;
    uint32_t capNormalVertices = 0, capNormalFaces = 0;
    float* d_normals = nullptr;
    uint32_t capNormals = 0;
};

struct MeshClean {
    // per input vertex, grown on demand: the union-find parent, the component label (kept for bf_marching_cubes_clean_labels), the face count of the component a
    // root stands for, the new vertex id; per scan tile of vertices / faces / output vertices its count, then its offset; the control words (meshclean.hip)
    uint32_t *d_parent = nullptr, *d_label = nullptr, *d_count = nullptr, *d_newId = nullptr, *d_tilesV = nullptr, *d_tilesF = nullptr, *d_words = nullptr;
    uint32_t capVerticesIn = 0, capFacesIn = 0;
    MeshNormals normals;          // of the output mesh
    // the result, valid until the next clean: nv x 3 float (normals.d_normals: only when the last clean computed them), nf x 3 uint32
    float *d_positions = nullptr, *d_colors = nullptr; uint32_t* d_faces = nullptr;
    uint32_t capVertices = 0, capFaces = 0;
    uint32_t numVertices = 0, numFaces = 0, numVerticesIn = 0;
    bool hasNormals = false, hasResult = false;          // hasResult: a clean has succeeded on this object (bf_marching_cubes_simplify's default input)
};

// Cleans the mesh at the device arrays of `in` on `stream` (see meshclean.hip for the definition and the kernels); waits for the stream twice (the refusal of a bad face id, then the counts).
// The buffers of `c` are taken from, and stay with, `res`.
int meshclean_run(MeshClean& c, Resources& res, hipStream_t stream, const bf_indexed_mesh& in, const bf_mesh_clean_params& params, bf_mesh_clean_stats* stats);

// The clean's normal pass on its own, over any indexed mesh in HBM (numVertices x 3 positions, numFaces x 3 ids below numVertices) on `stream`: n.d_normals holds
// the normals when the launched kernels have ended.  Does not wait.  bf_marching_cubes_simplify calls it for its output mesh.
int meshnormals_run(MeshNormals& n, Resources& res, hipStream_t stream, const float* d_positions, const uint32_t* d_faces, uint32_t numVertices, uint32_t numFaces);
// the same definition on one core: host arrays, h_normalsOut numVertices x 3
void meshnormals_host(const float* h_positions, const uint32_t* h_faces, uint32_t numVertices, uint32_t numFaces, float* h_normalsOut);

}  // namespace bf
