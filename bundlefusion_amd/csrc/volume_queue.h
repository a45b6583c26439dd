// The frame loop's command queue to the volume (bf_pipeline::vol).  It depends on the bf_scene_* C ABI only - the caller resolves frame pointers, texels and
// events - so it builds and runs on the CPU against a fake scene (tests/volume_queue_harness.cpp).
#pragma once
#include <condition_variable>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/bf_hip.h"

namespace bf {

// The volume stream is fed by its own host thread: the main thread decides WHAT to integrate (TrajectoryManager lists, poses)
// and posts commands; the worker issues the launches (three per operator + the event operations: 13 us of HIP calls per operator,
// 12 % of the wall time), so they do not serialize with the ~60 launches of the detect and bundling streams on one CPU thread.
class VolumeQueue {
public:
    enum class Op : int { Integrate = BF_SCENE_OP_INTEGRATE, Deintegrate = BF_SCENE_OP_DEINTEGRATE, Reintegrate = BF_SCENE_OP_REINTEGRATE, Collect, Flush, Render, SaveMesh, SaveMeshSimplified, SaveMeshRecoloured, SaveMeshTextured, MeasureMesh };
    // what the poster of a Render command waits for: the command's own status and message (not the worker's sticky error, unless the flush before it failed)
    struct Reply { bool done = false; int rc = BF_OK; std::string message; };
    // The three operators carry the frame (data, optional interleaved texels), its pose T0 (a re-integration: from T0 to T1) and the event that completes the
    // frame, or null; Collect (garbage collection) and Flush (issue what is held back for the next batch) carry nothing.  Render (a picture of the volume between
    // two frames' batches, bf_render.h) issues what is pending, then calls render(renderCtx) - the queue knows nothing about ray casters - and answers in *reply.
    // The queue does not own renderCtx and reply: both must stay valid until the command has been handled, which postAndWait (the only way a Render is posted)
    // guarantees by keeping them on the poster's stack until the worker has set reply->done.  SaveMesh (the mesh of the volume between two frames' batches,
    // bf_pipeline_save_mesh and bf_pipeline_save_mesh_clean) is posted and answered the same way, with its job in render / renderCtx: the queue knows nothing
    // about marching cubes either; SaveMeshSimplified (bf_pipeline_save_mesh_simplified), SaveMeshRecoloured (bf_pipeline_save_mesh_recoloured) and SaveMeshTextured
    // (bf_pipeline_save_mesh_textured) likewise, and MeasureMesh (bf_pipeline_measure_mesh), which writes no file.
    struct Cmd {
        Op op = Op::Flush; bf_depth_camera_data data = {nullptr, nullptr}; const void* texels = nullptr; float T0[16] = {}, T1[16] = {}; void* waitEvent = nullptr;
        int (*render)(void*) = nullptr; void* renderCtx = nullptr; Reply* reply = nullptr;
    };

    ~VolumeQueue() { stop(); }
    void start(bf_scene* scene, const bf_depth_camera_params& cam, int device);      // the worker thread begins with hipSetDevice(device)
    void stop();                       // what is queued is still handled, then the thread is joined
    int post(const Cmd& c);            // returns the worker's first error, if it has one (message prefixed "volume worker: ")
    int postAndWait(Cmd c);            // a Render or one of the SaveMesh commands: returns when THAT command has been handled (not the ones posted after it), with its status
    int drain();                       // everything posted so far, what was held back for a batch included, has been issued; the worker's first error
    void setBatching(bool enable) { batching_ = enable; }      // (drain first)
    void setInline(bool enable) { inline_ = enable; }          // post() handles the command on the calling thread, one by one (drain first)
    // where the volume thread's time goes: seconds spent handling commands (HIP API calls) and commands handled since the last reset
    void profile(double* busySeconds, double* commands, bool reset);

private:
    int dispatch(const Cmd& c, bool batch);
    int issueSingle(const Cmd& c);
    int submitPending();
    void work();

    bf_scene* scene_ = nullptr;
    bf_depth_camera_params cam_ = {};
    // Batched volume operators (round 5, bf_scene_run_batch): the volume thread collects a frame's operators - the integration of the previous frame, which
    // arrives last in that frame's body, and this frame's re-integrations - and issues them as ONE batch when the frame's garbage collection arrives
    // (DepthSensing.cpp:854-902 order kept: ..., integrate(k-1), fixes(k), GC(k), integrate(k), ...); a flush command (every accessor, bf_pipeline_synchronize)
    // issues what is pending.  Per batch: four launches and one pass over the touched blocks instead of 3 launches and one pass per operator.
    bool batching_ = true;
    bool inline_ = false;              // stage timings are taken with everything issued from the calling thread
    std::vector<Cmd> pending_;         // worker-thread only; inline dispatch finds it empty and the worker idle: the drain that precedes setInline saw to both
    static const size_t MAX_QUEUE = 48;          // back-pressure: the volume thread may lag the bundling thread by a few frames at most
    std::thread worker_;
    std::mutex mu_;
    std::condition_variable cvWork_, cvIdle_;
    std::deque<Cmd> queue_;
    bool stop_ = false, busy_ = false;
    int workerError_ = BF_OK;
    std::string workerMessage_;
    double busySeconds_ = 0.0, commands_ = 0.0;
};

}  // namespace bf
