/* bf_sensordata.h — recorded RGB-D sequences (".sens") for the BundleFusion path.
 *
 * Replaces, for the frame loop, the reference's `SensorDataReader` (FriedLiver/Source/SensorDataReader.h/.cpp) and the part
 * of mLib's `ml::SensorData` it calls (`loadFromFile`, `RGBDFrameCacheRead::getNext`, `decompressDepthAlloc`,
 * `decompressColorAlloc`; call sites SensorDataReader.cpp:40-83, 85-128).  mLib is a git submodule of the reference that is
 * NOT vendored under /root/reference (external/mLib is empty, .gitmodules pins no commit), so the container format is restated
 * from its published description (the ScanNet "SensorData" reader documents the same byte layout):
 *
 *   u32  version (= 4)
 *   u64  strlen, char[strlen] sensor name
 *   f32[16] colour intrinsic, f32[16] colour extrinsic, f32[16] depth intrinsic, f32[16] depth extrinsic   (row-major mat4f)
 *   i32  colour compression (-1 unknown, 0 raw RGB8, 1 PNG, 2 JPEG)
 *   i32  depth compression  (-1 unknown, 0 raw u16, 1 zlib-compressed u16, 2 "occi" u16)
 *   u32  colourWidth, colourHeight, depthWidth, depthHeight
 *   f32  depthShift          (depth in metres = u16 / depthShift; 0 = invalid)
 *   u64  numFrames, then per frame:
 *        f32[16] cameraToWorld, u64 timeStampColour, u64 timeStampDepth, u64 colourSizeBytes, u64 depthSizeBytes,
 *        colour bytes, depth bytes
 *   u64  numIMUFrames, then per IMU frame 5 x f64[3] + u64 time stamp (128 B)      (may be absent in older files)
 *
 * All functions run on the host only (no GPU needed), with one exception: a bf_sens_player created over a pipeline feeds that pipeline's
 * device ingest (bf_sens_player_next).  Status / error conventions as in bf_hip.h.
 */
#ifndef BF_SENSORDATA_H
#define BF_SENSORDATA_H

#include "bf_pipeline.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { BF_SENS_COLOR_UNKNOWN = -1, BF_SENS_COLOR_RAW = 0, BF_SENS_COLOR_PNG = 1, BF_SENS_COLOR_JPEG = 2 };
enum { BF_SENS_DEPTH_UNKNOWN = -1, BF_SENS_DEPTH_RAW_USHORT = 0, BF_SENS_DEPTH_ZLIB_USHORT = 1, BF_SENS_DEPTH_OCCI_USHORT = 2 };

typedef struct bf_sensor_data_info {          /* ml::SensorData header fields */
    uint32_t versionNumber;
    char sensorName[256];
    float colorIntrinsic[16], colorExtrinsic[16], depthIntrinsic[16], depthExtrinsic[16];
    int32_t colorCompressionType, depthCompressionType;
    uint32_t colorWidth, colorHeight, depthWidth, depthHeight;
    float depthShift;
    uint64_t numFrames, numIMUFrames;
} bf_sensor_data_info;

typedef struct bf_sensor_data bf_sensor_data;               /* a .sens file opened for reading */
typedef struct bf_sensor_data_writer bf_sensor_data_writer; /* a .sens file being written      */

/* colour decoder for PNG / JPEG frames: decode `size` bytes into width*height RGB8; return 0 on success.  ml::SensorData decodes
 * with stb_image; this library has a built-in decoder (baseline JPEG, 8-bit non-interlaced PNG: bf_decode_color_rgb) that is used
 * unless the host application installs its own with bf_sensor_data_set_color_decoder (e.g. for progressive JPEG). */
typedef int (*bf_sens_color_decoder)(void* user, const uint8_t* data, uint64_t size, int32_t compressionType, uint32_t width,
                                     uint32_t height, uint8_t* rgbOut);
BF_API int bf_decode_color_rgb(const uint8_t* data, uint64_t size, int32_t compressionType, uint32_t width, uint32_t height, uint8_t* rgbOut);
/* baseline JPEG (4:4:4, image-optimised Huffman tables) of an RGB8 image, for recording colour frames the way the reference does
 * (TYPE_JPEG, RGBDSensor.cpp:276).  out == NULL: only *size is returned (the stream is kept for the following call with a buffer). */
BF_API int bf_encode_jpeg_rgb(const uint8_t* rgb, uint32_t width, uint32_t height, int32_t quality, uint8_t* out, uint64_t capacity, uint64_t* size);
/* The encoder in its two stages, for callers that run the first on the device (bf_jpeg_forward_device, bf_hip.h); bf_encode_jpeg_rgb is the two in sequence.
 *   bf_jpeg_forward_host     colour conversion, edge replication, DCT, quantisation, zigzag -> ceil(width/8) * ceil(height/8) * 192 int16: per block
 *                            (raster order of the block grid) Y, Cb, Cr, 64 values each in zigzag order.  pixelStride 3 (RGB8) or 4 (RGBX8, X ignored);
 *                            capacity in int16.  The arithmetic is binary32 with a defined order (csrc/bf_jpeg_fwd.h, DESIGN.md "Recording").
 *   bf_jpeg_entropy_encode   two Huffman passes with image-optimised tables, headers, scan; out == NULL as in bf_encode_jpeg_rgb. */
BF_API int bf_jpeg_forward_host(const uint8_t* pixels, uint32_t pixelStride, uint32_t width, uint32_t height, int32_t quality, int16_t* coefficients, uint64_t capacity);
BF_API int bf_jpeg_entropy_encode(uint32_t width, uint32_t height, int32_t quality, const int16_t* coefficients, uint8_t* out, uint64_t capacity, uint64_t* size);

/* The built-in JPEG decoder in its stages, for callers that reconstruct on the device (bf_jpeg_info, bf_jpeg_reconstruct_device: bf_hip.h):
 *   bf_jpeg_parse           headers up to the scan -> *info.  expectWidth x expectHeight: the size the container states (0 x 0: any)
 *   bf_jpeg_entropy_decode  Huffman decode of the scan into info->numBlocks * 64 int16 (layout: bf_jpeg_info); capacity in int16.
 *                           BF_ERR_NOT_ON_DEVICE for a (hostile) stream whose DC values leave int16: bf_decode_color_rgb still reads it
 *   bf_jpeg_reconstruct_host  the coefficients -> width*height RGB8: what bf_jpeg_reconstruct_device computes, on the host
 * bf_decode_color_rgb is these three in one pass; they reject what it rejects, with the same messages. */
BF_API int bf_jpeg_parse(const uint8_t* data, uint64_t size, uint32_t expectWidth, uint32_t expectHeight, bf_jpeg_info* info);
BF_API int bf_jpeg_entropy_decode(const uint8_t* data, uint64_t size, const bf_jpeg_info* info, int16_t* coefficients, uint64_t capacity);
BF_API int bf_jpeg_reconstruct_host(const bf_jpeg_info* info, const int16_t* coefficients, uint8_t* rgbOut);

/* SensorData::loadFromFile (frames are indexed and read on demand, so a file larger than host memory can be played) */
BF_API int bf_sensor_data_open(const char* filename, bf_sensor_data** out);
BF_API int bf_sensor_data_close(bf_sensor_data* sd);
BF_API int bf_sensor_data_get_info(bf_sensor_data* sd, bf_sensor_data_info* out);
/* RGBDSensor::init + initializeDepth/ColorIntrinsics/Extrinsics as done by createFirstConnected (SensorDataReader.cpp:57-63) */
BF_API int bf_sensor_data_get_sensor_desc(bf_sensor_data* sd, bf_rgbd_sensor_desc* out);
BF_API int bf_sensor_data_set_color_decoder(bf_sensor_data* sd, bf_sens_color_decoder fn, void* user);
/* RGBDFrame fields */
BF_API int bf_sensor_data_get_frame_pose(bf_sensor_data* sd, uint64_t frame, float cameraToWorld[16], uint64_t* timeStampColor,
                                         uint64_t* timeStampDepth);
BF_API int bf_sensor_data_get_frame_sizes(bf_sensor_data* sd, uint64_t frame, uint64_t* colorSizeBytes, uint64_t* depthSizeBytes);
/* decompressDepthAlloc: depthWidth*depthHeight u16 */
BF_API int bf_sensor_data_read_depth_raw(bf_sensor_data* sd, uint64_t frame, uint16_t* h_out);
/* what SensorDataReader::processDepth hands to the image manager (:98-103): metres, 0 -> -inf */
BF_API int bf_sensor_data_read_depth(bf_sensor_data* sd, uint64_t frame, float* h_depthMetres);
/* the stored colour bytes as they are (for an external decoder) */
BF_API int bf_sensor_data_read_color_compressed(bf_sensor_data* sd, uint64_t frame, uint8_t* h_out, uint64_t capacity, uint64_t* size);
/* decompressColorAlloc + the vec4uc(vec3uc) widening of processDepth (:107-111): colourWidth*colourHeight RGBX, X = 255.
 * A file without colour (size 0) yields zeros like the reference's untouched m_colorRGBX. */
BF_API int bf_sensor_data_read_color_rgbx(bf_sensor_data* sd, uint64_t frame, uint8_t* h_rgbx);

/* Decode-ahead player: `numThreads` worker threads (0: 4; at most 12) read, inflate and entropy-decode the frames of `sd` in order into a ring of
 * pinned slots; bf_sens_player_next hands the next frame, strictly in frame order, to the pipeline's device ingest
 * (bf_pipeline_process_frame_raw_decoded) and recycles its slot.  JPEG colour in a layout the device reconstructs travels as quantised
 * coefficients; everything else (PNG, other JPEG layouts, a decoder installed with bf_sensor_data_set_color_decoder) is decoded to RGB8 by the
 * worker.  The result does not depend on numThreads.  A frame that fails to decode fails the bf_sens_player_next call of THAT frame (status and
 * bf_last_error of the worker); the frames before it are delivered.  *gotFrame = 0 with BF_OK at the end of the file (or when the pipeline is full).
 * `pipeline` may be NULL: the player then only decodes, and bf_sens_player_peek is the way to look at the slots (no GPU needed).  `sd` must outlive
 * the player and must not be read through other calls meanwhile. */
typedef struct bf_sens_player bf_sens_player;
typedef struct bf_sens_frame {                /* one decoded slot; the pointers are valid until the next bf_sens_player_next / _destroy */
    uint64_t frame;
    const uint16_t* depthU16;                 /* depthWidth * depthHeight */
    const void* colour;                       /* jpegCoefficients ? int16 coefficients (jpeg.numBlocks * 64) : RGB8 (colourWidth * colourHeight * 3; NULL: no colour stored) */
    uint64_t colourBytes;
    int32_t jpegCoefficients;
    bf_jpeg_info jpeg;                        /* valid when jpegCoefficients */
} bf_sens_frame;
BF_API int bf_sens_player_create(bf_pipeline* pipeline, bf_sensor_data* sd, uint32_t numThreads, bf_sens_player** out);
BF_API int bf_sens_player_next(bf_sens_player* pl, int* gotFrame);
/* the frame bf_sens_player_next would hand over (waits for its worker); *gotFrame = 0 at the end of the file */
BF_API int bf_sens_player_peek(bf_sens_player* pl, bf_sens_frame* out, int* gotFrame);
BF_API int bf_sens_player_destroy(bf_sens_player* pl);

/* SensorData::saveToFile, incrementally.  info: sensorName, calibration, compression types (colour: frames are stored as
 * given; depth: RAW_USHORT or ZLIB_USHORT, compressed here), sizes, depthShift; numFrames is filled in by _close. */
BF_API int bf_sensor_data_writer_create(const char* filename, const bf_sensor_data_info* info, bf_sensor_data_writer** out);
BF_API int bf_sensor_data_writer_add_frame(bf_sensor_data_writer* w, const float cameraToWorld[16], uint64_t timeStampColor,
                                           uint64_t timeStampDepth, const uint8_t* colorBytes, uint64_t colorSizeBytes,
                                           const uint16_t* depth);
/* the same with the depth bytes as they go into the file: already compressed for ZLIB_USHORT (compress2 level 8 is what _add_frame uses), the plane itself for RAW_USHORT */
BF_API int bf_sensor_data_writer_add_frame_compressed(bf_sensor_data_writer* w, const float cameraToWorld[16], uint64_t timeStampColor, uint64_t timeStampDepth,
                                                      const uint8_t* colorBytes, uint64_t colorSizeBytes, const uint8_t* depthBytes, uint64_t depthSizeBytes);
BF_API int bf_sensor_data_writer_close(bf_sensor_data_writer* w);

/* SensorDataReader::saveToFile(filename, trajectory) (SensorDataReader.cpp:152-165, "kind of a hack"): the same frames with
 * cameraToWorld replaced by trajectory[i] (16 floats each) for i < numTransforms and by an all -inf matrix for the rest. */
BF_API int bf_sensor_data_save_with_trajectory(bf_sensor_data* sd, const char* filename, const float* trajectory, uint64_t numTransforms);
/* RGBDSensor::saveRecordedFramesToFile (RGBDSensor.cpp:353-398): only the first numTransforms frames, each with its pose; more
 * transforms than frames is an error ("something went wrong; found more transforms than frames"). */
BF_API int bf_sensor_data_save_recorded(bf_sensor_data* sd, const char* filename, const float* trajectory, uint64_t numTransforms);

/* PoseHelper::evaluateAteRmse (PoseHelper.h:35-79): absolute trajectory error after a rigid (Kabsch) alignment of the camera
 * positions; transforms whose first element is -inf are skipped on either side.  *rmse = -inf when fewer than 3 transforms are
 * given (except the reference's special case for 2).  *numEvaluated = number of positions used.  mLib's EigenWrapperf::kabsch is
 * not in the tree: the alignment here is the textbook SVD solution (double precision). */
BF_API int bf_evaluate_ate_rmse(const float* trajectory, const float* referenceTrajectory, uint32_t numTransforms, float* rmse,
                                uint32_t* numEvaluated);
/* PoseHelper::getAlignmentBetweenTrajectories (PoseHelper.h:81-108): the rigid transform itself (all -inf when it cannot be evaluated) */
BF_API int bf_trajectory_alignment(const float* trajectory, const float* referenceTrajectory, uint32_t numTransforms, float align[16]);
/* PoseHelper::evaluateErr2PerImage (:110-146): squared position error of every pose that is valid on both sides, after the alignment;
 * imageIndices / err2 need room for numTransforms entries */
BF_API int bf_evaluate_err2_per_image(const float* trajectory, const float* referenceTrajectory, uint32_t numTransforms, uint32_t* imageIndices,
                                      float* err2, uint32_t* count);
/* SensorDataReader::evaluateTrajectory (:167-189): the file's cameraToWorld poses, re-based so that the first is identity, are
 * the reference. */
BF_API int bf_sensor_data_evaluate_trajectory(bf_sensor_data* sd, const float* trajectory, uint64_t numTransforms, float* rmse,
                                              uint32_t* numEvaluated);

#ifdef __cplusplus
}
#endif
#endif /* BF_SENSORDATA_H */
