// The device weld of a triangle soup into an indexed mesh (meshweld.hip): the buffers a bf_marching_cubes object owns for it and the entry points mesh.hip calls.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bf_hip.h"
#include "bf_resources.h"

namespace bf {

struct MeshWeld {
    // scratch, grown on demand: the open-addressing table (corner indices, then face indices), per corner its representative and its vertex id, per triangle its
    // three vertex ids and its representative face, per scan tile its count / offset
    uint32_t *d_table = nullptr, *d_rep = nullptr, *d_vid = nullptr, *d_faceIds = nullptr, *d_faceRep = nullptr, *d_tiles = nullptr, *d_totals = nullptr;
    uint32_t capTable = 0, capTriangles = 0;
    // the result, valid until the next weld: nv x 3 float, nv x 3 float, nf x 3 uint32
    float *d_positions = nullptr, *d_colors = nullptr; uint32_t* d_faces = nullptr;
    uint32_t capVertices = 0, capFaces = 0;
    uint32_t numVertices = 0, numFaces = 0;
};

// Welds numTriangles triangles at d_triangles on `stream` (see meshweld.hip for the definition); waits for the stream twice (vertex count, face count).
// The buffers of `w` are taken from, and stay with, `res`: the owner of the handle that holds `w`.
int meshweld_run(MeshWeld& w, Resources& res, hipStream_t stream, const bf_mc_triangle* d_triangles, uint32_t numTriangles, const float transform[16]);

}  // namespace bf
