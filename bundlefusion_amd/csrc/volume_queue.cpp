#include "volume_queue.h"

#include <chrono>
#include <cstring>

#include "bf_internal.h"

namespace bf {

int VolumeQueue::issueSingle(const Cmd& c) {                                                          // DepthSensing.cpp:723-762
    if (c.waitEvent) BF_TRY(bf_scene_wait_event(scene_, c.waitEvent));
    if (c.texels) BF_TRY(bf_scene_set_frame_texels(scene_, c.texels));
    if (c.op == Op::Integrate) return bf_scene_integrate(scene_, c.T0, &c.data, &cam_, nullptr);
    if (c.op == Op::Deintegrate) return bf_scene_deintegrate(scene_, c.T0, &c.data, &cam_, nullptr);
    return bf_scene_reintegrate(scene_, c.T0, c.T1, &c.data, &cam_);
}

int VolumeQueue::submitPending() {
    if (pending_.empty()) return BF_OK;
    bf_scene_batch_op ops[BF_SCENE_BATCH_MAX];
    const uint32_t n = (uint32_t)pending_.size();
    for (uint32_t k = 0; k < n; ++k) {
        const Cmd& c = pending_[k];
        ops[k].kind = (int32_t)c.op; ops[k].reserved = 0;
        memcpy(ops[k].T0, c.T0, 64); memcpy(ops[k].T1, c.op == Op::Reintegrate ? c.T1 : c.T0, 64);
        ops[k].data = c.data; ops[k].d_texels = c.texels;
        ops[k].wait_event = c.waitEvent;
    }
    pending_.clear();
    return bf_scene_run_batch(scene_, ops, n, &cam_);
}

// The handling of one command, by the worker (batch: the batching setting) or inline on the posting thread (batch off).  No default: a new Op must get its arm.
int VolumeQueue::dispatch(const Cmd& c, bool batch) {
    switch (c.op) {
    case Op::Integrate: case Op::Deintegrate: case Op::Reintegrate:
        if (!batch) return issueSingle(c);
        pending_.push_back(c);
        return pending_.size() == BF_SCENE_BATCH_MAX ? submitPending() : BF_OK;
    case Op::Collect:
        BF_TRY(submitPending());
        return bf_scene_garbage_collect(scene_);
    case Op::Flush:
        return submitPending();
    case Op::Render: case Op::SaveMesh: case Op::SaveMeshSimplified: case Op::SaveMeshRecoloured: case Op::SaveMeshTextured: case Op::MeasureMesh: {
        BF_TRY(submitPending());
        const int rc = c.render ? c.render(c.renderCtx) : BF_ERR_INVALID_ARG;
        if (c.reply) { c.reply->rc = rc; if (rc != BF_OK) c.reply->message = bf_last_error(); }
        return BF_OK;               // a picture or a mesh that failed is its poster's business, not the volume's
    }
    }
    return BF_ERR_INVALID_ARG;      // (not an Op)
}

void VolumeQueue::work() {
    for (;;) {
        Cmd c;
        {
            std::unique_lock<std::mutex> lk(mu_);
            cvWork_.wait(lk, [this] { return stop_ || !queue_.empty(); });
            if (queue_.empty()) return;             // stop requested and drained
            c = queue_.front(); queue_.pop_front();
            busy_ = true;
        }
        const double tv = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
        const int rc = dispatch(c, batching_);
        const double dv = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count() - tv;
        {
            std::lock_guard<std::mutex> lk(mu_);
            busySeconds_ += dv; commands_ += 1.0;
            if (rc != BF_OK && workerError_ == BF_OK) { workerError_ = rc; workerMessage_ = bf_last_error(); }
            if (c.reply) { if (rc != BF_OK) { c.reply->rc = rc; c.reply->message = bf_last_error(); } c.reply->done = true; }
            busy_ = false;
            cvIdle_.notify_all();
        }
    }
}

void VolumeQueue::start(bf_scene* scene, const bf_depth_camera_params& cam, int device) {
    scene_ = scene; cam_ = cam;
    worker_ = std::thread([this, device] { (void)hipSetDevice(device); work(); });
}

void VolumeQueue::stop() {
    if (!worker_.joinable()) return;
    { std::lock_guard<std::mutex> lk(mu_); stop_ = true; }
    cvWork_.notify_all();
    worker_.join();
}

int VolumeQueue::post(const Cmd& c) {
    if (inline_) return dispatch(c, false);
    std::unique_lock<std::mutex> lk(mu_);
    cvIdle_.wait(lk, [this] { return queue_.size() < MAX_QUEUE || workerError_ != BF_OK; });
    if (workerError_ != BF_OK) { set_error("volume worker: %s", workerMessage_.c_str()); return workerError_; }
    queue_.push_back(c);
    cvWork_.notify_one();
    return BF_OK;
}

int VolumeQueue::postAndWait(Cmd c) {
    Reply reply;
    c.reply = &reply;
    if (inline_) {
        const int rc = dispatch(c, false);
        if (rc != BF_OK) return rc;
    } else {
        BF_TRY(post(c));
        std::unique_lock<std::mutex> lk(mu_);
        cvIdle_.wait(lk, [&reply] { return reply.done; });
    }
    if (reply.rc != BF_OK) set_error("%s", reply.message.c_str());
    return reply.rc;
}

int VolumeQueue::drain() {
    std::unique_lock<std::mutex> lk(mu_);
    if (worker_.joinable() && workerError_ == BF_OK) {      // what the volume thread holds back for the next batch is issued now
        queue_.push_back(Cmd());                            // (a flush)
        cvWork_.notify_one();
    }
    cvIdle_.wait(lk, [this] { return queue_.empty() && !busy_; });
    if (workerError_ != BF_OK) { set_error("volume worker: %s", workerMessage_.c_str()); return workerError_; }
    return BF_OK;
}

void VolumeQueue::profile(double* busySeconds, double* commands, bool reset) {
    std::lock_guard<std::mutex> lk(mu_);
    if (busySeconds) *busySeconds = busySeconds_;
    if (commands) *commands = commands_;
    if (reset) { busySeconds_ = 0.0; commands_ = 0.0; }
}

}  // namespace bf
