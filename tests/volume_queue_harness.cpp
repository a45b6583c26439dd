// Stand-alone CPU harness of bf::VolumeQueue (bundlefusion_amd/csrc/volume_queue.cpp): the queue against a fake scene that records every call, its arguments
// and the calling thread, can hold a call on a latch and can fail its n-th call.  Built and run under the thread and the address sanitizer by
// tests/test_host_cpu.py::test_volume_queue_harness_under_sanitizers; exit status 0 = every case passed.
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "../bundlefusion_amd/csrc/volume_queue.h"
#include "../bundlefusion_amd/csrc/bf_internal.h"

using bf::VolumeQueue;
typedef VolumeQueue::Op Op;

// ------------------------------------------------------------------------------------------------ the fakes
namespace {

enum Fn { SET_DEVICE, WAIT_EVENT, SET_TEXELS, INTEGRATE, DEINTEGRATE, REINTEGRATE, RUN_BATCH, COLLECT };
struct Call {
    Fn fn; std::thread::id tid; bf_scene* scene = nullptr;
    int device = -1; void* event = nullptr; const void* texels = nullptr;
    float T0[16] = {}, T1[16] = {}; bf_depth_camera_data data = {nullptr, nullptr}; uint32_t camWidth = 0;
    std::vector<bf_scene_batch_op> ops;
};
struct Fake {
    std::mutex mu;
    std::condition_variable cv;
    std::vector<Call> log;
    int sceneCalls = 0;          // every bf_scene_* call counts
    int blockOn = 0;             // the n-th scene call waits until `open` (0: none)
    bool open = false, blocked = false;
    int failOn = 0, failCode = 0;      // the n-th scene call fails
} F;
thread_local std::string lastError;

int record(Call c) {
    std::unique_lock<std::mutex> lk(F.mu);
    c.tid = std::this_thread::get_id();
    F.log.push_back(c);
    if (c.fn == SET_DEVICE) return BF_OK;
    const int n = ++F.sceneCalls;
    if (n == F.blockOn) { F.blocked = true; F.cv.notify_all(); F.cv.wait(lk, [] { return F.open; }); }
    if (n == F.failOn) { bf::set_error("fake failure at call %d", n); return F.failCode; }
    return BF_OK;
}
void resetFake() { std::lock_guard<std::mutex> lk(F.mu); F.log.clear(); F.sceneCalls = 0; F.blockOn = 0; F.open = false; F.blocked = false; F.failOn = 0; F.failCode = 0; }
std::vector<Call> takeLog() { std::lock_guard<std::mutex> lk(F.mu); return F.log; }
Call operatorCall(Fn fn, bf_scene* s, const float* T0, const float* T1, const bf_depth_camera_data* d, const bf_depth_camera_params* cam) {
    Call c; c.fn = fn; c.scene = s; memcpy(c.T0, T0, 64); memcpy(c.T1, T1, 64); c.data = *d; c.camWidth = cam->m_imageWidth;
    return c;
}

}  // namespace

namespace bf {
void set_error(const char* fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    lastError = buf;
}
}  // namespace bf

extern "C" {
const char* bf_last_error(void) { return lastError.c_str(); }
hipError_t hipSetDevice(int device) { Call c; c.fn = SET_DEVICE; c.device = device; record(c); return hipSuccess; }
int bf_scene_wait_event(bf_scene* s, void* ev) { Call c; c.fn = WAIT_EVENT; c.scene = s; c.event = ev; return record(c); }
int bf_scene_set_frame_texels(bf_scene* s, const void* t) { Call c; c.fn = SET_TEXELS; c.scene = s; c.texels = t; return record(c); }
int bf_scene_integrate(bf_scene* s, const float T[16], const bf_depth_camera_data* d, const bf_depth_camera_params* cam, const uint32_t* mask) {
    if (mask) return BF_ERR_INVALID_ARG;
    return record(operatorCall(INTEGRATE, s, T, T, d, cam));
}
int bf_scene_deintegrate(bf_scene* s, const float T[16], const bf_depth_camera_data* d, const bf_depth_camera_params* cam, const uint32_t* mask) {
    if (mask) return BF_ERR_INVALID_ARG;
    return record(operatorCall(DEINTEGRATE, s, T, T, d, cam));
}
int bf_scene_reintegrate(bf_scene* s, const float oldT[16], const float newT[16], const bf_depth_camera_data* d, const bf_depth_camera_params* cam) {
    return record(operatorCall(REINTEGRATE, s, oldT, newT, d, cam));
}
int bf_scene_run_batch(bf_scene* s, const bf_scene_batch_op* ops, uint32_t n, const bf_depth_camera_params* cam) {
    Call c; c.fn = RUN_BATCH; c.scene = s; c.camWidth = cam->m_imageWidth; c.ops.assign(ops, ops + n);
    return record(c);
}
int bf_scene_garbage_collect(bf_scene* s) { Call c; c.fn = COLLECT; c.scene = s; return record(c); }
}

// ------------------------------------------------------------------------------------------------ the cases
namespace {

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

bf_scene* const SCENE = reinterpret_cast<bf_scene*>(0x5ce0);
const int DEVICE = 3;
bf_depth_camera_params camera() { bf_depth_camera_params c; memset(&c, 0, sizeof c); c.m_imageWidth = 321; c.m_imageHeight = 7; return c; }

// command `id` (1, 2, ...): every field distinct and derived from the id
VolumeQueue::Cmd command(Op op, int id, bool event = true, bool texels = true) {
    VolumeQueue::Cmd c;
    c.op = op;
    c.data.d_depthData = reinterpret_cast<const float*>((uintptr_t)0x10000 * id);
    c.data.d_colorData = reinterpret_cast<const uint8_t*>((uintptr_t)0x10000 * id + 0x800);
    c.texels = texels ? reinterpret_cast<const void*>((uintptr_t)0x20000 * id) : nullptr;
    c.waitEvent = event ? reinterpret_cast<void*>((uintptr_t)0x30000 * id) : nullptr;
    for (int i = 0; i < 16; ++i) { c.T0[i] = id + 0.03125f * i; c.T1[i] = -(id + 0.03125f * i); }
    return c;
}
VolumeQueue::Cmd bare(Op op) { VolumeQueue::Cmd c; c.op = op; return c; }

struct Started {
    VolumeQueue q;
    Started() { resetFake(); q.start(SCENE, camera(), DEVICE); }
};

bool samePose(const float* a, const float* b) { return memcmp(a, b, 64) == 0; }
void checkBatchOp(const bf_scene_batch_op& o, const VolumeQueue::Cmd& c) {
    CHECK(o.kind == (int)c.op && o.reserved == 0);
    CHECK(samePose(o.T0, c.T0));
    CHECK(samePose(o.T1, c.op == Op::Reintegrate ? c.T1 : c.T0));
    CHECK(o.data.d_depthData == c.data.d_depthData && o.data.d_colorData == c.data.d_colorData);
    CHECK(o.d_texels == c.texels && o.wait_event == c.waitEvent);
}
// log[i ...] is the single issue of c: its event wait and texel hand-over when present, then the operator; returns the index behind it
size_t checkSingle(const std::vector<Call>& log, size_t i, const VolumeQueue::Cmd& c, std::thread::id tid) {
    if (c.waitEvent) { CHECK(i < log.size() && log[i].fn == WAIT_EVENT && log[i].event == c.waitEvent && log[i].tid == tid); ++i; }
    if (c.texels) { CHECK(i < log.size() && log[i].fn == SET_TEXELS && log[i].texels == c.texels && log[i].tid == tid); ++i; }
    CHECK(i < log.size());
    const Call& k = log[i];
    CHECK(k.fn == (c.op == Op::Integrate ? INTEGRATE : c.op == Op::Deintegrate ? DEINTEGRATE : REINTEGRATE));
    CHECK(k.tid == tid && k.scene == SCENE && k.camWidth == 321);
    CHECK(samePose(k.T0, c.T0));
    if (c.op == Op::Reintegrate) CHECK(samePose(k.T1, c.T1));
    CHECK(k.data.d_depthData == c.data.d_depthData && k.data.d_colorData == c.data.d_colorData);
    return i + 1;
}

// the command sequence of cases 1, 3 and 4
struct Sequence {
    VolumeQueue::Cmd a = command(Op::Integrate, 1), b = command(Op::Reintegrate, 2, false, true), c = command(Op::Deintegrate, 3, true, false), d = command(Op::Integrate, 4, false, false);
    void post(VolumeQueue& q) {
        CHECK(q.post(a) == BF_OK); CHECK(q.post(b) == BF_OK); CHECK(q.post(c) == BF_OK); CHECK(q.post(bare(Op::Collect)) == BF_OK);
        CHECK(q.post(d) == BF_OK); CHECK(q.post(bare(Op::Flush)) == BF_OK);
    }
    // the calls of the one-by-one issue, from log[i] on, all on thread tid; Flush makes no call
    void checkSingles(const std::vector<Call>& log, size_t i, std::thread::id tid) {
        i = checkSingle(log, i, a, tid); i = checkSingle(log, i, b, tid); i = checkSingle(log, i, c, tid);
        CHECK(i < log.size() && log[i].fn == COLLECT && log[i].tid == tid && log[i].scene == SCENE); ++i;
        i = checkSingle(log, i, d, tid);
        CHECK(i == log.size());
    }
};

void caseBatched() {
    Started t; Sequence s;
    s.post(t.q);
    CHECK(t.q.drain() == BF_OK);
    const std::vector<Call> log = takeLog();
    CHECK(log.size() == 4);
    CHECK(log[0].fn == SET_DEVICE && log[0].device == DEVICE);
    const std::thread::id worker = log[0].tid;
    CHECK(worker != std::this_thread::get_id());
    for (const Call& k : log) CHECK(k.tid == worker);
    CHECK(log[1].fn == RUN_BATCH && log[1].scene == SCENE && log[1].camWidth == 321 && log[1].ops.size() == 3);
    checkBatchOp(log[1].ops[0], s.a); checkBatchOp(log[1].ops[1], s.b); checkBatchOp(log[1].ops[2], s.c);
    CHECK(samePose(log[1].ops[0].T1, s.a.T0) && samePose(log[1].ops[2].T1, s.c.T0) && samePose(log[1].ops[1].T1, s.b.T1));
    CHECK(log[2].fn == COLLECT && log[2].scene == SCENE);
    CHECK(log[3].fn == RUN_BATCH && log[3].ops.size() == 1);
    checkBatchOp(log[3].ops[0], s.d);
}

void caseThirteen() {
    Started t;
    std::vector<VolumeQueue::Cmd> cmds;
    for (int i = 0; i < 13; ++i) cmds.push_back(command(i % 3 == 0 ? Op::Integrate : i % 3 == 1 ? Op::Deintegrate : Op::Reintegrate, i + 1));
    for (const auto& c : cmds) CHECK(t.q.post(c) == BF_OK);
    CHECK(t.q.drain() == BF_OK);
    const std::vector<Call> log = takeLog();
    CHECK(log.size() == 3 && log[1].fn == RUN_BATCH && log[2].fn == RUN_BATCH);
    CHECK(log[1].ops.size() == BF_SCENE_BATCH_MAX && log[2].ops.size() == 1);
    for (int i = 0; i < 12; ++i) checkBatchOp(log[1].ops[i], cmds[i]);
    checkBatchOp(log[2].ops[0], cmds[12]);
}

void caseUnbatched() {
    Started t; Sequence s;
    t.q.setBatching(false);
    s.post(t.q);
    CHECK(t.q.drain() == BF_OK);
    const std::vector<Call> log = takeLog();
    CHECK(!log.empty() && log[0].fn == SET_DEVICE && log[0].tid != std::this_thread::get_id());
    s.checkSingles(log, 1, log[0].tid);
}

void caseInline() {
    {
        Started t;
        CHECK(t.q.drain() == BF_OK);
        resetFake();                     // (the worker's hipSetDevice is behind us: drain returned)
        t.q.setInline(true);
        CHECK(t.q.post(bare(Op::Flush)) == BF_OK);          // a frame boundary with timings on and collection off
        CHECK(takeLog().empty());
    }
    Started t; Sequence s;
    CHECK(t.q.drain() == BF_OK);
    t.q.setInline(true);
    s.post(t.q);
    const std::vector<Call> log = takeLog();      // no drain: the calls were made when post returned
    CHECK(!log.empty() && log[0].fn == SET_DEVICE && log[0].tid != std::this_thread::get_id());
    s.checkSingles(log, 1, std::this_thread::get_id());
    double busy = -1.0, commands = -1.0;
    t.q.profile(&busy, &commands, false);
    CHECK(commands == 1.0);                       // the worker handled the one flush of the drain above and nothing else
}

void waitBlocked() { std::unique_lock<std::mutex> lk(F.mu); F.cv.wait(lk, [] { return F.blocked; }); }
void openLatch() { { std::lock_guard<std::mutex> lk(F.mu); F.open = true; } F.cv.notify_all(); }

void caseBackPressure() {
    Started t;
    t.q.setBatching(false);
    { std::lock_guard<std::mutex> lk(F.mu); F.blockOn = 1; }
    std::atomic<int> returned{0};
    std::thread poster([&] { for (int i = 0; i < 60; ++i) { CHECK(t.q.post(command(Op::Integrate, i + 1, false, false)) == BF_OK); returned++; } });
    waitBlocked();                                // the worker holds command 1 inside the fake
    while (returned.load() < 48) std::this_thread::yield();      // the queue fills behind it (the room the worker made by taking command 1 is announced when it
    std::this_thread::sleep_for(std::chrono::milliseconds(50));  // has handled it: 48 posts return if the queue was full by then, else 49)
    CHECK(returned.load() <= 49);                 // the next post waits
    openLatch();
    poster.join();
    CHECK(t.q.drain() == BF_OK);
    const std::vector<Call> log = takeLog();
    CHECK(log.size() == 61);
    for (int i = 0; i < 60; ++i) CHECK(log[1 + i].fn == INTEGRATE && log[1 + i].T0[0] == (float)(i + 1));
}

void caseError() {
    Started t;
    t.q.setBatching(false);
    { std::lock_guard<std::mutex> lk(F.mu); F.failOn = 2; F.failCode = BF_ERR_HIP; F.blockOn = 2; }      // (held until all three are queued)
    for (int i = 0; i < 3; ++i) CHECK(t.q.post(command(Op::Integrate, i + 1, false, false)) == BF_OK);
    waitBlocked();
    openLatch();
    CHECK(t.q.drain() == BF_ERR_HIP);
    const std::string msg = bf_last_error();
    CHECK(msg.rfind("volume worker: ", 0) == 0 && msg.find("fake failure at call 2") != std::string::npos);
    bf::set_error("");
    CHECK(t.q.post(command(Op::Integrate, 9, false, false)) == BF_ERR_HIP);      // returns at once: nothing is queued behind an error
    CHECK(std::string(bf_last_error()).rfind("volume worker: ", 0) == 0);
    CHECK(t.q.drain() == BF_ERR_HIP);
    const std::vector<Call> log = takeLog();
    CHECK(log.size() == 4);                       // the worker went on consuming behind the failed call; the post after the error was not queued
    for (size_t i = 1; i < log.size(); ++i) CHECK(log[i].fn == INTEGRATE && log[i].T0[0] == (float)i);
    t.q.stop();                                   // joins
}

void caseStopWithQueued() {
    Started t;
    t.q.setBatching(false);
    { std::lock_guard<std::mutex> lk(F.mu); F.blockOn = 1; }
    for (int i = 0; i < 5; ++i) CHECK(t.q.post(command(Op::Integrate, i + 1, false, false)) == BF_OK);
    waitBlocked();
    std::atomic<bool> stopping{false};
    std::thread stopper([&] { stopping = true; t.q.stop(); });
    while (!stopping.load()) std::this_thread::yield();
    std::this_thread::sleep_for(std::chrono::milliseconds(20));      // stop is requested with four commands queued and one in flight
    openLatch();
    stopper.join();
    const std::vector<Call> log = takeLog();
    CHECK(log.size() == 6);
    for (int i = 0; i < 5; ++i) CHECK(log[1 + i].fn == INTEGRATE && log[1 + i].T0[0] == (float)(i + 1));
}

void caseProfile() {
    Started t;
    for (int i = 0; i < 5; ++i) CHECK(t.q.post(command(Op::Integrate, i + 1)) == BF_OK);
    CHECK(t.q.post(bare(Op::Collect)) == BF_OK);
    CHECK(t.q.drain() == BF_OK);
    CHECK(t.q.drain() == BF_OK);
    double busy = -1.0, commands = -1.0;
    t.q.profile(&busy, &commands, true);
    CHECK(commands == 6.0 + 2.0 && busy >= 0.0);
    t.q.profile(&busy, &commands, false);
    CHECK(commands == 0.0 && busy == 0.0);
    CHECK(t.q.drain() == BF_OK);
    t.q.profile(nullptr, &commands, false);
    CHECK(commands == 1.0);
}

}  // namespace

int main() {
    caseBatched();
    caseThirteen();
    caseUnbatched();
    caseInline();
    caseBackPressure();
    caseError();
    caseStopWithQueued();
    caseProfile();
    printf("volume queue harness: 8 cases passed\n");
    return 0;
}
