/*
 * bf_record.h — s_recordData: record the scan.  RGBDSensor::recordFrame (RGBDSensor.cpp:264-312) for every accepted frame
 * (DepthSensing.cpp:1042-1045) and RGBDSensor::saveRecordedFramesToFile (RGBDSensor.cpp:353-398) with the optimised trajectory at the end of the
 * scan (DepthSensing.cpp:475-483), as a threaded back end that needs no GPU and a device front end for the frame loop.
 *
 * A recorded frame is the sensor's own: getDepthFloat() as u16 = round(depthShift * metres) (invalid -> 0) and getColorRGBX() as a baseline 4:4:4
 * JPEG of quality 90 - the bytes bf_sensor_data_writer_add_frame + bf_encode_jpeg_rgb write.  The front half of both (bf_image_convert_depth_to_u16,
 * bf_jpeg_forward_device: bf_hip.h; or their host forms) fills a slot of a ring; worker threads entropy-code the colour and deflate the depth
 * (compress2 level 8), and the blobs are appended to a temporary .sens strictly in frame order.  The file's bytes depend on the frames only.
 * The legacy uncompressed ".sensor" container (s_recordCompression = false) is not written; s_recordDataWidth / Height resample in that path only.
 */
#ifndef BF_RECORD_H
#define BF_RECORD_H

#include "bf_hip.h"
#include "bf_pipeline.h"
#include "bf_sensordata.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the recording keys of zParametersDefault.txt (GlobalAppState.h); bf_global_app_state keeps ignoring them */
typedef struct bf_record_state {
    int32_t s_recordData;                  /* master flag */
    int32_t s_recordCompression;           /* true: .sens (the only container written here) */
    uint32_t s_recordDataWidth, s_recordDataHeight;      /* parsed and stored; they apply to the uncompressed container only */
    char s_recordDataFile[512];
} bf_record_state;
#define BF_RECORD_STATE_NUM_FIELDS 5

BF_API int bf_record_state_default(bf_record_state* out);                                    /* false, true, 640, 480, "dump/recording.sens" */
/* reads the same parameter file bf_global_app_state_read reads; *numMissing: fields of bf_record_state the file does not name */
BF_API int bf_record_state_read(const char* filename, bf_record_state* out, uint32_t* numMissing);

/* ---- the recorder ----
 * info: header of the recording (sensor name, calibration, sizes, depthShift; colour JPEG, depth RAW_USHORT or ZLIB_USHORT).  tmpFilename: the temporary
 * .sens the frames are appended to.  numThreads workers (0: 4; at most 12), numSlots ring slots (0: 4; at least 2), each one frame's int16
 * coefficients and u16 depth plane - pinned host memory plus a device twin when `pipeline` is given (then the calling thread's current device is used),
 * plain memory otherwise (no GPU needed; only _record_host may then be called).
 * A record call waits while every slot is in use - a recording never drops a frame - and otherwise never for a copy, an encode or the disk.  A worker's
 * failure (disk full, encoder error) fails the next record or finish call with the worker's status and message. */
typedef struct bf_sens_recorder bf_sens_recorder;
BF_API int bf_sens_recorder_create(bf_pipeline* pipelineOrNull, const bf_sensor_data_info* info, const char* tmpFilename, uint32_t numThreads, uint32_t numSlots,
                                   bf_sens_recorder** out);
/* colourWidth * colourHeight RGBX8 (X ignored) and depthWidth * depthHeight float metres on the host; packed on the calling thread */
BF_API int bf_sens_recorder_record_host(bf_sens_recorder* rec, const uint8_t* h_rgbx, const float* h_depthFloat);
/* the same two images in device memory: the two packing kernels run on `hip_stream` into the slot's device twin, the copy to the pinned slot on the
 * recorder's own stream behind an event, and a worker takes the slot when that copy's event has fired.  The caller's buffers are free as soon as
 * `hip_stream` has passed the two kernels. */
BF_API int bf_sens_recorder_record_device(bf_sens_recorder* rec, const float* d_depthFloat, const uint8_t* d_rgbx, void* hip_stream);
BF_API int bf_sens_recorder_get_num_recorded(bf_sens_recorder* rec, uint64_t* numFrames);    /* frames handed in since create / the last finish */
/* drains the ring, closes the temporary file, writes `filename` through bf_sensor_data_save_recorded - the first numTransforms frames, each with its
 * pose (trajectory: numTransforms x 16 floats); more transforms than frames is the reference's error - and removes the temporary file.  Unless
 * `overwrite`, an existing name gets a numeric suffix before its extension (RGBDSensor.cpp:382-396); the name written goes to actualName (capacity
 * bytes; may be NULL).  Nothing recorded since the last finish, or numTransforms == 0: *numFramesWritten = 0 and no file.  The recorder can be used again. */
BF_API int bf_sens_recorder_finish(bf_sens_recorder* rec, const char* filename, const float* trajectory, uint64_t numTransforms, int overwrite, char* actualName,
                                   uint64_t capacity, uint64_t* numFramesWritten);
/* joins the workers; without a finish the temporary file is removed */
BF_API int bf_sens_recorder_destroy(bf_sens_recorder* rec);

/* ---- the frame loop ----
 * Before the first frame (refused after it).  With state->s_recordData the pipeline owns a recorder (numThreads as above) whose header describes the
 * pipeline's sensor: JPEG colour, ZLIB_USHORT depth, depthShift 1000 (RGBDSensor.cpp:269-280); its temporary file is <tmpPrefix><id>.rec.sens
 * (tmpPrefix NULL: "./bf_").  s_recordData with s_recordCompression = false is refused.  Every frame the image manager accepts is recorded, in every
 * form of bf_pipeline_process_frame*: the depth before registration, erosion and the depth filter, the colour before resampling, at sensor
 * resolution; the packing kernels run on the ingest stream.  Without a record state the loop launches, records and allocates nothing for it. */
BF_API int bf_pipeline_set_record_state(bf_pipeline* p, const bf_record_state* state, uint32_t numThreads, const char* tmpPrefix);
/* completes the frames handed in, takes bf_trajectory_manager_get_optimized_transforms (DepthSensing.cpp:480-482) and finishes the recorder;
 * filename NULL: s_recordDataFile.  A second call without new frames returns 0 frames and writes nothing. */
BF_API int bf_pipeline_save_recording(bf_pipeline* p, const char* filenameOrNull, int overwrite, char* actualName, uint64_t capacity, uint64_t* numFramesWritten);

#ifdef __cplusplus
}
#endif
#endif /* BF_RECORD_H */
