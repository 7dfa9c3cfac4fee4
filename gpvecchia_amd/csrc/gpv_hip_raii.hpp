// gpv_hip_raii.hpp — what the C-ABI layer (gpv_api.hip, the only file that includes this) owns on a device: the error
// record behind gpv_last_hip_error(), move-only owners of device / pinned buffers, events, streams and graphs, and the one
// place where a sweep is captured into a graph and replayed.  A resource is released by its owner's destructor and by
// nothing else: a new plan resource is a member of gpv_plan of one of these types, and no other code needs to know of it.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/gpvecchia.h"

#include <cstdio>
#include <cstdlib>
#include <utility>

namespace gpv {

// Every HIP failure is remembered (per host thread) with the call that produced it, so that a caller that gets
// GPV_ERR_HIP can tell out-of-memory from a bad stream from a failed launch: gpv_last_hip_error().
inline thread_local int g_hip_code = 0;
inline thread_local char g_hip_text[256] = "";
inline int note_hip(hipError_t e, const char *what, int line)
{
    g_hip_code = (int)e;
    (void)hipGetLastError();          // HIP keeps a failure until it is read: the launch wrappers' hipGetLastError() would report it again
    std::snprintf(g_hip_text, sizeof(g_hip_text), "%s: %s [%s, gpv_api.hip:%d]", hipGetErrorName(e), hipGetErrorString(e),
                  what, line);
    return GPV_ERR_HIP;
}
#define GPV_HIP(expr)                                                   \
    do {                                                                \
        hipError_t e_ = (expr);                                         \
        if (e_ != hipSuccess) return note_hip(e_, #expr, __LINE__);     \
    } while (0)
// the same for code that cleans up before it returns: evaluates to true on failure
#define GPV_HIP_FAILED(expr) ([&]() { hipError_t e_ = (expr); if (e_ != hipSuccess) { note_hip(e_, #expr, __LINE__); return true; } return false; }())

// A device buffer (Pinned: a page-locked host buffer).  Converts to T* wherever a pointer is wanted, so kernel arguments and
// launch calls name the member itself.  Every operation returns the HIP status and is invoked through GPV_BUF / GPV_BUF_FAILED,
// which record the failing call, the buffer's name and the caller's line.
inline thread_local const char *g_buf_call = "";      // the HIP call the latest buffer operation made
template <class T, bool Pinned = false>
class DevBuf {
    T *p_ = nullptr;
public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
    DevBuf &operator=(DevBuf &&o) noexcept { std::swap(p_, o.p_); return *this; }
    ~DevBuf() { (void)reset(); }
    operator T *() const { return p_; }
    T *get() const { return p_; }
    hipError_t reset()
    {
        T *q = std::exchange(p_, nullptr);
        g_buf_call = Pinned ? "hipHostFree" : "hipFree";
        return !q ? hipSuccess : (Pinned ? hipHostFree(q) : hipFree(q));
    }
    hipError_t resize(size_t count)                   // free, then allocate `count` elements (never less than 8 bytes)
    {
        (void)reset();
        const size_t bytes = count ? count * sizeof(T) : 8;
        g_buf_call = Pinned ? "hipHostMalloc" : "hipMalloc";
        const hipError_t e = Pinned ? hipHostMalloc((void **)&p_, bytes, hipHostMallocDefault) : hipMalloc((void **)&p_, bytes);
        if (e != hipSuccess) p_ = nullptr;
        return e;
    }
    hipError_t ensure(size_t count) { return p_ ? hipSuccess : resize(count); }      // allocate if empty
    hipError_t upload(const T *src, size_t count)     // resize, then a blocking copy from the host
    {
        hipError_t e = resize(count);
        if (e == hipSuccess && count) {
            g_buf_call = "hipMemcpy";
            e = hipMemcpy(p_, src, count * sizeof(T), hipMemcpyHostToDevice);
        }
        return e;
    }
};
template <class T> using PinnedBuf = DevBuf<T, true>;
inline void note_buf(hipError_t e, const char *buf, int line)
{
    char what[160];
    std::snprintf(what, sizeof(what), "%s(%s, ...)", g_buf_call, buf);
    note_hip(e, what, line);
}
#define GPV_BUF_FAILED(buf, op) ([&]() { const hipError_t e_ = (buf).op; if (e_ != hipSuccess) note_buf(e_, #buf, __LINE__); return e_ != hipSuccess; }())
#define GPV_BUF(buf, op) do { if (GPV_BUF_FAILED(buf, op)) return GPV_ERR_HIP; } while (0)

// An event, stream, graph or executable graph: destroyed with its owner.  put() hands the empty slot to the creating call.
template <class H, hipError_t (*Destroy)(H)>
class Owned {
    H h_ = nullptr;
public:
    Owned() = default;
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    ~Owned() { reset(); }
    operator H() const { return h_; }
    H *put() { reset(); return &h_; }
    void adopt(H h) { reset(); h_ = h; }
    void reset() { if (h_) (void)Destroy(std::exchange(h_, nullptr)); }
};
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using Event = Owned<hipEvent_t, hipEventDestroy>;
using Graph = Owned<hipGraph_t, hipGraphDestroy>;
using GraphExec = Owned<hipGraphExec_t, hipGraphExecDestroy>;

// Replays the plan-owned executable graph `exec` on `st`; captures it from `enqueue` first when there is none yet or the
// caller calls it `stale` (*captured says that a capture succeeded).  A sweep of many launches of a few microseconds each is
// more than the host can enqueue as fast as the device retires them.  Plain enqueue() instead when capture or instantiation
// fails, when `st` is already being captured by the caller, or under GPV_NO_GRAPH=1.
inline bool graphs_off() { static const bool off = getenv("GPV_NO_GRAPH") != nullptr; return off; }   // read once
template <class F>
hipError_t graph_replay(GraphExec &exec, hipStream_t st, F &&enqueue, bool stale = false, bool *captured = nullptr)
{
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess) { (void)hipGetLastError(); cap = hipStreamCaptureStatusNone; }
    if (graphs_off() || cap != hipStreamCaptureStatusNone) return enqueue();
    if (!exec || stale) {
        exec.reset();
        if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) == hipSuccess) {
            const hipError_t e = enqueue();
            Graph graph;
            hipGraphExec_t x = nullptr;
            const hipError_t e2 = hipStreamEndCapture(st, graph.put());
            if (e == hipSuccess && e2 == hipSuccess && graph && hipGraphInstantiate(&x, graph, nullptr, nullptr, 0) == hipSuccess) {
                exec.adopt(x);
                if (captured) *captured = true;
            }
            graph.reset();
            (void)hipGetLastError();
        }
    }
    return exec ? hipGraphLaunch(exec, st) : enqueue();
}

}  // namespace gpv
