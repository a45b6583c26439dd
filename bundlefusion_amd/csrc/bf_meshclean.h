// The device cleaning of an indexed mesh (meshclean.hip): the buffers a bf_marching_cubes object owns for it and the entry point mesh.hip calls.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bf_hip.h"
#include "bf_resources.h"

namespace bf {

struct MeshClean {
    // per input vertex, grown on demand: the union-find parent, the component label (kept for bf_marching_cubes_clean_labels), the face count of the component a
    // root stands for, the new vertex id; per scan tile of vertices / faces / output vertices its count, then its offset; the control words (meshclean.hip)
    uint32_t *d_parent = nullptr, *d_label = nullptr, *d_count = nullptr, *d_newId = nullptr, *d_tilesV = nullptr, *d_tilesF = nullptr, *d_words = nullptr;
    uint32_t capVerticesIn = 0, capFacesIn = 0;
    // normals: per output vertex its number of corners (counted, then counted down by the fill) and the start of its segment (numVertices + 1 of them); the corners
    // of every vertex as filled and, for segments longer than a wave, in increasing order; the vertices with such segments
    uint32_t *d_degree = nullptr, *d_offset = nullptr, *d_corners = nullptr, *d_sorted = nullptr, *d_long = nullptr, *d_tilesN = nullptr;
    uint32_t capNormalVertices = 0, capNormalFaces = 0;
    // the result, valid until the next clean: nv x 3 float (normals: only when the last clean computed them), nf x 3 uint32
    float *d_positions = nullptr, *d_colors = nullptr, *d_normals = nullptr; uint32_t* d_faces = nullptr;
    uint32_t capVertices = 0, capFaces = 0, capNormals = 0;
    uint32_t numVertices = 0, numFaces = 0, numVerticesIn = 0;
    bool hasNormals = false;
};

// Cleans the mesh at the device arrays of `in` on `stream` (see meshclean.hip for the definition and the kernels); waits for the stream twice (the refusal of a bad face id, then the counts).
// The buffers of `c` are taken from, and stay with, `res`.
int meshclean_run(MeshClean& c, Resources& res, hipStream_t stream, const bf_indexed_mesh& in, const bf_mesh_clean_params& params, bf_mesh_clean_stats* stats);

}  // namespace bf
