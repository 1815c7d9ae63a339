// side.cpp (host code only, compiled as HIP like the kernels' files) — fork / join of the library's side stream: work that nothing on the caller's stream reads for a while (a conv block's weight-grad: its
// GEMM, reduce and output launches) runs there beside the caller's next bandwidth-bound passes.
//   s = cvk_side_begin(main): everything queued on `main` so far happens before whatever is launched on s from now on;
//   cvk_side_join(main):      everything launched on s so far happens before whatever is queued on `main` from now on.
// One side stream per device, created on first use: non-blocking (no implicit ordering against the legacy default stream, which is the stream
// PyTorch launches on unless told otherwise) and at the lowest priority, so that the caller's stream is served first where both have waves to
// place.  Which CUs the side stream's kernels leave free is decided by the capped grids of the *_wg entry points, not by a CU mask:
// hipExtStreamCreateWithCUMask takes neither the non-blocking flag nor a priority, and a blocking stream is ordered against every launch on the
// default stream — no overlap at all.  The library opens this one stream and no other.
#include "cvk_common.h"
#include <atomic>
#include <mutex>

namespace {

constexpr int kMaxDev = 64;
struct Side {
    hipStream_t stream = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
};
Side g_side[kMaxDev];
std::mutex g_mu;
std::atomic<long> g_forks{0};

// the current device's side stream and events (created on first use); nullptr with the error set.  The caller holds g_mu.
Side* side_of_current_device(const char* who) {
    int dev = -1;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess || dev < 0 || dev >= kMaxDev) {
        cvk_set_error("%s: no current device (%s)", who, hipGetErrorString(e));
        return nullptr;
    }
    Side& sd = g_side[dev];
    if (sd.stream == nullptr) {
        int least = 0, greatest = 0;
        e = hipDeviceGetStreamPriorityRange(&least, &greatest);          // lower numbers are greater priorities
        if (e == hipSuccess) e = hipEventCreateWithFlags(&sd.fork, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&sd.join, hipEventDisableTiming);
        hipStream_t s = nullptr;
        if (e == hipSuccess) e = hipStreamCreateWithPriority(&s, hipStreamNonBlocking, least);
        if (e != hipSuccess) {
            cvk_set_error("%s: creating the side stream failed: %s", who, hipGetErrorString(e));
            if (sd.fork) (void)hipEventDestroy(sd.fork);
            if (sd.join) (void)hipEventDestroy(sd.join);
            sd.fork = sd.join = nullptr;
            return nullptr;
        }
        sd.stream = s;
    }
    return &sd;
}

}  // namespace

// Each pair below (record on one stream, wait on the other) reuses one event per device, so the lock is held across the pair: two host threads
// that fork or join on one device cannot re-record the event between the other's record and wait.
extern "C" void* cvk_side_begin(void* main_stream) {
    std::lock_guard<std::mutex> lock(g_mu);
    Side* sd = side_of_current_device("cvk_side_begin");
    if (sd == nullptr) return nullptr;
    hipError_t e = hipEventRecord(sd->fork, (hipStream_t)main_stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(sd->stream, sd->fork, 0);
    if (e != hipSuccess) {
        cvk_set_error("cvk_side_begin: %s", hipGetErrorString(e));
        return nullptr;
    }
    g_forks.fetch_add(1, std::memory_order_relaxed);
    return sd->stream;
}

extern "C" int cvk_side_join(void* main_stream) {
    std::lock_guard<std::mutex> lock(g_mu);
    Side* sd = side_of_current_device("cvk_side_join");
    if (sd == nullptr) return CVK_EINVAL;
    hipError_t e = hipEventRecord(sd->join, sd->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent((hipStream_t)main_stream, sd->join, 0);
    if (e != hipSuccess) {
        cvk_set_error("cvk_side_join: %s", hipGetErrorString(e));
        return (int)e;
    }
    return CVK_OK;
}

// how often the side stream was handed out in this process: every group of launches that reaches the side stream starts with one cvk_side_begin
extern "C" long cvk_side_launches(void) { return g_forks.load(std::memory_order_relaxed); }
