/*
 * bf_pointcloud.h — the scan as a coloured, oriented point cloud.  SiftVisualization::saveToPointCloud (SiftVisualization.cpp:607-644, with computePointCloud
 * :527-561, getNormal :505-525 and depthToCamera :498-503) and its siblings RGBDSensor::recordPointCloud / saveRecordedPointCloud (RGBDSensor.cpp:528-616):
 * every skip-th frame with a valid pose is back-projected, each point gets a normal and its colour, is moved into the world by the frame's pose, and the union is
 * thinned to one point per cell (pc.sparsifyUniform(0.005f, true)) and written as a PLY.
 *
 * The thinning and the file are this library's own definition (mLib's are not in the reference tree): DESIGN.md 1 "Point cloud" states it, tests/point_cloud_ref.py
 * restates it in numpy, and the device object, the host route and the file are compared with that as bits.  In short: a pixel is a candidate iff its depth and
 * its four neighbours' depths are finite and > 0, its camera z is < maxDepth, it is not on the image border, its normal has a finite length > 0, its colour is not
 * (0, 0, 0) and its world position is finite with a cell index that fits an int32; candidates are numbered by add_frame call and then in raster order; the point
 * of a cell floor((double)P * (1.0 / (double)cellSize)) is its lowest-numbered candidate; the cloud lists the points in increasing candidate number.
 */
#ifndef BF_POINTCLOUD_H
#define BF_POINTCLOUD_H

#include "bf_hip.h"
#include "bf_pipeline.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bf_point_cloud_params {
    uint32_t maxPoints;          /* capacity of the cloud */
    uint32_t maxFramePixels;     /* largest width * height one add_frame may bring; maxPoints + maxFramePixels <= 2^30 */
    float cellSize;              /* sparsifyUniform's cell, metres; <= 0: no thinning, every candidate is a point */
    float maxDepth;              /* saveToPointCloud's maxDepth: candidates have camera z < maxDepth */
} bf_point_cloud_params;

/* the cloud in device memory, valid until the next add_frame / reset / destroy: numPoints x 3 float, numPoints x 3 float, numPoints x 4 uint8 (r g b 255) */
typedef struct bf_point_cloud_view {
    const float* d_positions;
    const float* d_normals;
    const uint8_t* d_colors;
    uint32_t numPoints;
} bf_point_cloud_view;

/* ---- the accumulator: RGBDSensor::recordPointCloud per frame (RGBDSensor.cpp:528-560), thinned as it grows ----
 * All device memory is taken at create: the cloud's three arrays, the cell table (the power of two >= 2 * (maxPoints + maxFramePixels) slots of 4 bytes) and one
 * frame's staging.  The calling thread's current device is used. */
typedef struct bf_point_cloud bf_point_cloud;
BF_API int bf_point_cloud_create(const bf_point_cloud_params* params, bf_point_cloud** out);
BF_API int bf_point_cloud_destroy(bf_point_cloud* pc);
BF_API int bf_point_cloud_set_stream(bf_point_cloud* pc, void* hip_stream);
/* RGBDSensor.cpp:610-615 (the recorded clouds are cleared after a save): an empty cloud again, also out of the overflowed state; nothing is reallocated */
BF_API int bf_point_cloud_reset(bf_point_cloud* pc);
/* SiftVisualization::computePointCloud (:527-561) + the thinning, for one frame in device memory: width x height float depth in metres and RGBX8 colour of the
 * same size, the 4x4 row-major inverse intrinsics and camera-to-world pose (host).  A pose whose first element is NaN or -inf adds nothing and is no error
 * (:531).  Refuses width * height > maxFramePixels.  *numAdded (may be NULL): points this frame appended.  Waits for the stream once (the count).
 * A frame that would take the cloud past maxPoints fails with BF_ERR_CAPACITY and leaves the object overflowed: every later add / get / download / save fails
 * the same way until bf_point_cloud_reset. */
BF_API int bf_point_cloud_add_frame(bf_point_cloud* pc, const float* d_depth, const uint8_t* d_colorRGBX, uint32_t width, uint32_t height, const float intrinsicsInv[16],
                                    const float transform[16], uint32_t* numAdded);
BF_API int bf_point_cloud_get_gpu(bf_point_cloud* pc, bf_point_cloud_view* out);
/* host copies of the first min(capacity, numPoints) points; any of the three arrays may be NULL; *numPoints (may be NULL): the cloud's size */
BF_API int bf_point_cloud_download(bf_point_cloud* pc, float* h_positions, float* h_normals, uint8_t* h_colors, uint32_t capacity, uint32_t* numPoints);
/* RGBDSensor::saveRecordedPointCloud's file (RGBDSensor.cpp:562-616; PointCloudIOf::saveToFile): download + bf_write_ply_points */
BF_API int bf_point_cloud_save(bf_point_cloud* pc, const char* filename, uint32_t* numPoints);

/* PointCloudIOf::saveToFile's counterpart, host only: binary little-endian PLY, one vertex = x y z, nx ny nz (float), red green blue alpha (uchar): 28 bytes; no
 * face element.  h_colors: numPoints x 4 bytes, written as they are. */
BF_API int bf_write_ply_points(const char* filename, const float* h_positions, const float* h_normals, const uint8_t* h_colors, uint32_t numPoints);

/* SiftVisualization::saveToPointCloud's loop (:607-644) as the definition itself: the sequential loop over frames and pixels on one core, the cells in a
 * std::unordered_map.  Needs no device.  h_depths / h_colors: numFrames pointers to width x height images; h_transforms: numFrames x 16.  Every frame is used
 * (the caller applies its stride).  Writes at most `capacity` points (the arrays may be NULL) and always reports the full count. */
BF_API int bf_point_cloud_build_host(const float* const* h_depths, const uint8_t* const* h_colors, uint32_t numFrames, uint32_t width, uint32_t height,
                                     const float intrinsicsInv[16], const float* h_transforms, float cellSize, float maxDepth, uint32_t capacity, float* h_positions,
                                     float* h_normals, uint8_t* h_colors_out, uint32_t* numPoints);

/* ---- the frame loop: SiftVisualization::saveToPointCloud(filename, depthImages, colorImages, trajectory, depthIntrinsicsInv, skip, numFrames, maxDepth) ----
 * Completes the frames handed in so far, takes bf_trajectory_manager_get_optimized_transforms (TrajectoryManager::getOptimizedTransforms) and adds the stored
 * integration frames 0, frameStride, 2 * frameStride, ... < numTransforms (frameStride >= 1) that have a valid pose, straight from HBM, with the inverse of the
 * intrinsics the pipeline integrates with (the colour camera's when depth is registered to it), on the pipeline's ingest stream; then writes the PLY.  The
 * accumulator is created by the first call (maxPoints 0: 4 Mi points) and kept.  The reconstruction is not touched: no volume command, no new stream.
 * *numFramesUsed: frames on the stride with a valid pose. */
BF_API int bf_pipeline_save_point_cloud(bf_pipeline* p, const char* filename, uint32_t frameStride, float cellSize, float maxDepth, uint32_t maxPoints, uint32_t* numPoints,
                                        uint32_t* numFramesUsed);

#ifdef __cplusplus
}
#endif
#endif /* BF_POINTCLOUD_H */
