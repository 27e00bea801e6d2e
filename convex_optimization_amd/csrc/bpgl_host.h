// Host-side helpers shared by the two C-ABI translation units of libbpgl.so
// (bpgl.hip: single right-hand side; bpgl_panel_abi.hip: k right-hand sides) and by bpgl_panel_pos.hip,
// which holds kernel variants only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/bpgl.h"

namespace bpgl_host {
// thread-local message behind bpgl_last_error(); returns `code`
int fail(int code, const char* fmt, ...);

inline int64_t up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }
inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// bump allocator over the caller's scratch buffer (256-byte aligned pieces)
struct Carve {
    int64_t off = 0;
    int64_t take(int64_t bytes) {
        int64_t o = off;
        off = up(off + bytes, 256);
        return o;
    }
};

constexpr int kGraphIters = 8;   // iterations captured per replayed hipGraph (panel; RCCL contexts' cap)
// single-RHS solver: hipGraphs of 1, 2, 4, ..., kGraphMaxIters iterations, so a run of n iterations
// costs about log2(n) replays instead of n / 8
constexpr int kGraphLevels = 7;
constexpr int kGraphMaxIters = 1 << (kGraphLevels - 1);

constexpr int kMaskWords = 32;   // CU mask words queried (1024 CUs)

inline int popcount_mask(const uint32_t* mask, int words, int cus) {
    int n = 0;
    for (int i = 0; i < words; ++i) {
        uint32_t v = mask[i];
        if (32 * i >= cus) break;
        if (32 * (i + 1) > cus) v &= (1u << (cus - 32 * i)) - 1u;
        n += __builtin_popcount(v);
    }
    return n;
}

// CUs a stream may use (its CU mask, hipExtStreamGetCUMask), 0 if unknown
inline int stream_cus(hipStream_t s, int dev_cus) {
    uint32_t mask[kMaskWords] = {};
    if (hipExtStreamGetCUMask(s, kMaskWords, mask) != hipSuccess) {
        (void)hipGetLastError();   // the query's own error only: not sticky, later launch checks read it
        return 0;
    }
    return popcount_mask(mask, kMaskWords, dev_cus);
}

// CUs a kernel launched on stream s can occupy: the stream's CU mask when it has one, else the device's
inline int usable_cus(hipStream_t s, int device) {
    int dev = 0;
    if (hipDeviceGetAttribute(&dev, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || dev <= 0) {
        (void)hipGetLastError();
        return 0;
    }
    const int n = stream_cus(s, dev);
    return (n > 0 && n < dev) ? n : dev;
}
}  // namespace bpgl_host

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) return bpgl_host::fail(BPGL_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

#define LAUNCH_CHECK(what)                                                                   \
    do {                                                                                     \
        hipError_t e_ = hipGetLastError();                                                   \
        if (e_ != hipSuccess) return bpgl_host::fail(BPGL_E_HIP, "launch %s: %s", what, hipGetErrorString(e_)); \
    } while (0)

namespace bpgl_host {
// f(std::integral_constant<int, V>{}) for the V among V0, Vs... that equals v (the last one when none
// does): a run-time value picks a template argument, as static_for does on the device
template <int V0, int... Vs, typename F>
auto dispatch(int v, F&& f) {
    if constexpr (sizeof...(Vs) == 0) {
        return f(std::integral_constant<int, V0>{});
    } else {
        if (v == V0) return f(std::integral_constant<int, V0>{});
        return dispatch<Vs...>(v, f);
    }
}

// HIP-event timing of the kernels of an iteration, KINDS kinds of them: event
// 2 * (it * KINDS + kind) + {0: start, 1: end} of timed iteration `it` (the caller counts `iters`)
// Hidden visibility: its member functions are weak symbols, and libbpgl.so exports none beyond its ABI.
template <int KINDS>
struct __attribute__((visibility("hidden"))) KernelTimes {
    hipStream_t stream = nullptr;
    bool on = false;
    std::vector<hipEvent_t> evs;   // the context's destroy function destroys them
    int64_t iters = 0;
    bool kind_used[KINDS] = {};   // kinds recorded in the current window

    void record(int64_t it, int kind, int end) {
        kind_used[kind] = true;
        const size_t idx = 2 * ((size_t)it * KINDS + kind) + end;
        while (evs.size() <= idx) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return;
            evs.push_back(e);
        }
        (void)hipEventRecord(evs[idx], stream);
    }
    // fn() between the two events of (it, kind); nothing but fn() when timing is off (graph capture relies
    // on it), and no end event when fn fails
    template <typename F>
    int timed(int kind, int64_t it, F&& fn) {
        if (!on) return fn();
        record(it, kind, 0);
        const int rc = fn();
        if (!rc) record(it, kind, 1);
        return rc;
    }
    void reset() {
        iters = 0;
        for (bool& u : kind_used) u = false;
    }
    // per kind, the time of the window's iterations; the stream must be idle
    int sums(double* sum_ms) const {
        for (int k = 0; k < KINDS; ++k) sum_ms[k] = 0.0;
        for (int64_t it = 0; it < iters; ++it)
            for (int k = 0; k < KINDS; ++k) {
                const size_t i0 = 2 * ((size_t)it * KINDS + k);
                if (!kind_used[k] || i0 + 1 >= evs.size()) continue;
                float ms = 0.f;
                HIP_TRY(hipEventElapsedTime(&ms, evs[i0], evs[i0 + 1]));
                sum_ms[k] += ms;
            }
        return 0;
    }
    // ... averaged over the iterations; ends the window
    int collect(double* avg_ms, int64_t* samples) {
        if (int rc = sums(avg_ms)) return rc;
        for (int k = 0; k < KINDS; ++k) avg_ms[k] = iters ? avg_ms[k] / iters : 0.0;
        if (samples) *samples = iters;
        reset();
        return 0;
    }
};

// enqueue() captured on `stream` as a hipGraph, instantiated into *exec and uploaded to the device, so
// the first replay inside a caller's timed region pays no upload.  A failing enqueue() ends the
// capture and returns its code.
template <typename F>
int capture_graph(hipStream_t stream, hipGraphExec_t* exec, F&& enqueue) {
    hipGraph_t graph = nullptr;
    hipError_t e = hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess)   // the text callers have always seen, whatever the stream is called here
        return fail(BPGL_E_HIP, "hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal): %s",
                    hipGetErrorString(e));
    const int rc = enqueue();
    e = hipStreamEndCapture(stream, &graph);
    if (rc) {
        if (graph) (void)hipGraphDestroy(graph);
        return rc;
    }
    if (e != hipSuccess) return fail(BPGL_E_HIP, "hipStreamEndCapture: %s", hipGetErrorString(e));
    e = hipGraphInstantiate(exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) return fail(BPGL_E_HIP, "hipGraphInstantiate: %s", hipGetErrorString(e));
    if ((e = hipGraphUpload(*exec, stream)) != hipSuccess)
        return fail(BPGL_E_HIP, "hipGraphUpload: %s", hipGetErrorString(e));
    return 0;
}
}  // namespace bpgl_host
