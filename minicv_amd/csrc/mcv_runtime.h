// mcv_runtime.h — host runtime helpers for the C-ABI shim: per-thread last error, HIP error
// checking, device-buffer RAII, the per-thread, per-device workspace every host driver keeps its
// buffers in, and the counted stream calls behind the mcvTest*Stats exports. No exception crosses an
// extern "C" boundary: every export wraps its body in MCV_GUARD, which records the message and
// returns the export's failure value.
#pragma once

#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <initializer_list>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>
#include <cstdio>
#include <cstdarg>

namespace mcv {

struct Error : std::runtime_error {
    explicit Error(const std::string& m) : std::runtime_error(m) {}
};

void set_last_error(const char* msg);
void clear_last_error();

[[noreturn]] inline void fail(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    throw Error(buf);
}

#define MCV_HIP(call)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (call);                                                                         \
        if (e_ != hipSuccess) ::mcv::fail("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, \
                                          __LINE__);                                                    \
    } while (0)

// Throws unless a HIP device is usable: the product path has no CPU fallback.
void require_device();

#define MCV_GUARD(failval, ...)                                                     \
    try {                                                                           \
        ::mcv::clear_last_error();                                                  \
        __VA_ARGS__                                                                 \
    } catch (const std::exception& ex) {                                            \
        ::mcv::set_last_error(ex.what());                                           \
        return failval;                                                             \
    } catch (...) {                                                                 \
        ::mcv::set_last_error("unknown exception");                                 \
        return failval;                                                             \
    }

// Device allocation that grows on demand (never shrinks) and is freed on destruction.
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    void ensure(size_t count) {
        if (count <= n) return;
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
        MCV_HIP(hipMalloc((void**)&p, (count ? count : 1) * sizeof(T)));
        n = count;
    }
    void reset() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};

template <class T>
struct PinnedBuf {
    T* p = nullptr;
    size_t n = 0;
    void ensure(size_t count) {
        if (count <= n) return;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        n = 0;
        MCV_HIP(hipHostMalloc((void**)&p, (count ? count : 1) * sizeof(T), hipHostMallocPortable));
        n = count;
    }
    ~PinnedBuf() {
        if (p) (void)hipHostFree(p);
    }
};

// Orders the uses of one workspace (below: per thread and device) across streams: the device-level matchers are
// asynchronous on the caller's stream, so a call on stream B right after one on stream A would race on
// the shared buffers (and on their finish counters). enter(s) makes s wait for the previous use when
// that ran on another stream; leave(s) records this use's completion.
struct StreamFence {
    hipEvent_t ev = nullptr;
    hipStream_t last = nullptr;
    bool used = false;
    // The null stream and the per-thread default stream live as long as the process; a caller's own
    // stream may be destroyed right after the call.
    static bool persistent(hipStream_t s) { return s == nullptr || s == hipStreamPerThread; }
    // A call on another stream than the previous one waits for the previous call's completion event.
    // A call on a caller-created stream records that event when it leaves (one reused event), so a
    // stream the caller destroys after the call is never touched again. A call on the null / per-thread
    // stream defers the record to the next call that switches streams (an event record costs the stream
    // a marker packet, ~3 us per call, which back-to-back calls on the default stream would otherwise
    // pay on every call): those streams cannot be destroyed, so the deferred record is always valid.
    void enter(hipStream_t s) {
        if (!used || last == s) return;
        if (persistent(last)) {
            if (!ev) MCV_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            MCV_HIP(hipEventRecord(ev, last));
        }
        MCV_HIP(hipStreamWaitEvent(s, ev, 0));
    }
    void leave(hipStream_t s) {
        if (!persistent(s)) {
            if (!ev) MCV_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            MCV_HIP(hipEventRecord(ev, s));
        }
        last = s;
        used = true;
    }
    ~StreamFence() {
        if (ev) (void)hipEventDestroy(ev);
    }
};

// ---- workspaces. Device buffers, streams and events belong to one device and do not follow a device
// switch of the calling thread, so a host driver keeps them in a workspace per (thread, device, slot):
// thread_device_ws<Ws>(slot) is the calling thread's Ws for the current device, made on first use and kept
// until the thread ends. The slot tells apart several workspaces of one kind on one device (the query
// shards of cvMatch*Multi, as thread_plan(model, shard) does for plans). A caller that already knows the
// current device passes it to thread_device_ws_on and spares the query.
template <class Ws>
Ws& thread_device_ws_on(int dev, int slot = 0) {
    struct Entry {
        int dev, slot;
        Ws ws;
    };
    thread_local std::vector<std::unique_ptr<Entry>> all;
    for (auto& e : all)
        if (e->dev == dev && e->slot == slot) return e->ws;
    all.emplace_back(new Entry{dev, slot, {}});
    return all.back()->ws;
}
template <class Ws>
Ws& thread_device_ws(int slot = 0) {
    int dev = 0;
    MCV_HIP(hipGetDevice(&dev));
    return thread_device_ws_on<Ws>(dev, slot);
}
// Base of a workspace that runs on a stream of its own (non-blocking, made on first use). A workspace
// that runs on its caller's stream (the matcher kernels', the pipeline's) does not derive from it.
struct DeviceWs {
    hipStream_t stream() {
        if (!s_) MCV_HIP(hipStreamCreateWithFlags(&s_, hipStreamNonBlocking));
        return s_;
    }
    DeviceWs() = default;
    DeviceWs(const DeviceWs&) = delete;
    DeviceWs& operator=(const DeviceWs&) = delete;
    ~DeviceWs() {
        if (s_) (void)hipStreamDestroy(s_);
    }

private:
    hipStream_t s_ = nullptr;
};

// ---- what a call enqueued, for the mcvTest*Stats exports. A driver keeps the record of its last call
// in a plain thread_local of its own (never in the workspace: reading it must not touch HIP) and
// derives from CallStats to add its own fields.
struct CallStats {
    long long launches = 0, syncs = 0, copies = 0, memsets = 0;
};
// Copies and memsets are counted by the call's form: one of zero bytes issues no HIP call and counts.
inline void counted_copy(CallStats& st, void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s) {
    if (bytes) MCV_HIP(hipMemcpyAsync(dst, src, bytes, kind, s));
    ++st.copies;
}
inline void counted_zero(CallStats& st, void* p, size_t bytes, hipStream_t s) {
    if (bytes) MCV_HIP(hipMemsetAsync(p, 0, bytes, s));
    ++st.memsets;
}
// The bare synchronisation of the geometry drivers (they check their launches as they enqueue them), and
// the batches' form, which asks for the launches' last error first.
inline void counted_wait(CallStats& st, hipStream_t s) {
    MCV_HIP(hipStreamSynchronize(s));
    ++st.syncs;
}
inline void counted_sync(CallStats& st, hipStream_t s) {
    MCV_HIP(hipGetLastError());
    counted_wait(st, s);
}
// The body of a mcvTest*Stats export: launches, syncs, copies, memsets, then up to four of the driver's own.
inline int stats8_out(const char* who, long long* stats8, const CallStats& st, std::initializer_list<long long> own) {
    if (!stats8) fail("%s: null argument", who);
    const long long v[8] = {st.launches, st.syncs, st.copies, st.memsets};
    std::copy(v, v + 8, stats8);
    std::copy(own.begin(), own.end(), stats8 + 4);
    return 0;
}
inline long long us_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
}

// CUs of the current device (256 when they cannot be read).
inline int device_cus() {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
        cus = 256;
    return cus;
}

// Waves of `kernel` (blocks of `threads`) the current device holds at once: its occupancy x the CUs.
template <class K>
inline int64_t resident_waves(K kernel, int threads) {
    const int cus = device_cus();
    int per = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kernel, threads, 0) != hipSuccess || per <= 0) per = 1;
    return (int64_t)per * cus * (threads / 64);
}

// Point chunks of a (model waves) x (point chunks) sweep: with c chunks the launch takes
// ceil(waves c / resident) rounds of waves 1 / c as long, so the idle tail of the last round is what
// the count changes. Returns the smallest c in [1, hi] within 1 % of the fewest one-chunk-wave
// durations (more chunks cost per-wave model setup and count atomics).
inline int tail_chunks(int64_t waves, int64_t resident, int hi) {
    if (waves <= 0 || resident <= 0 || hi <= 1) return 1;
    double best = 1e300;
    for (int c = 1; c <= hi; ++c) {
        const double cost = (double)((waves * c + resident - 1) / resident) / c;
        if (cost < best) best = cost;
    }
    for (int c = 1; c <= hi; ++c)
        if ((double)((waves * c + resident - 1) / resident) / c <= best * 1.01) return c;
    return 1;
}

}  // namespace mcv
