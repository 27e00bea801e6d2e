// The column gather (DESIGN.md sections 9 and 12): one kernel for bpgl_gather_columns (bpgl.hip) and
// bpgl_panel_gather_columns (bpgl_panel_abi.hip).  A checkpoint operation, not a per-iteration one.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "bpgl_device.h"
#include "bpgl_host.h"

namespace bpgl {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------
// gather: A_out[i * lda_out + c] = A(i, cols[c]), c < n_out; cols[c] is a global column index
// b w + j (element A + b block_stride + i lda + j); an index outside [0, nblock w) -- -1 by
// convention -- writes 0, and so do the columns c in [n_out, lda_out).
// One thread owns 16 bytes of an output row (E = 16 / BYTES consecutive columns) for the rows
// blockIdx.y, blockIdx.y + gridDim.y, ...: consecutive lanes store consecutive 16-byte pieces of
// one row, and read increasing addresses of the source row when cols is sorted.
// ---------------------------------------------------------------------------
template <int BYTES> struct GatherElem;
template <> struct GatherElem<2> { using type = uint16_t; };
template <> struct GatherElem<4> { using type = uint32_t; };
template <> struct GatherElem<8> { using type = uint64_t; };

struct GatherArgs {
    const void* A;
    long long lda, block_stride, w, ncols, m;
    const int* cols;
    long long n_out;
    void* out;
    long long lda_out;
};

template <int BYTES>
__global__ __launch_bounds__(kThreads) void k_gather_cols(GatherArgs a) {
    using T = typename GatherElem<BYTES>::type;
    constexpr int E = 16 / BYTES;
    const long long chunk = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (chunk >= a.lda_out / E) return;
    long long off[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const long long c = chunk * E + e;
        const long long col = c < a.n_out ? (long long)a.cols[c] : -1;
        const bool ok = col >= 0 && col < a.ncols;
        off[e] = ok ? (col / a.w) * a.block_stride + col % a.w : -1;
    }
    const T* __restrict__ src = reinterpret_cast<const T*>(a.A);
    T* __restrict__ dst = reinterpret_cast<T*>(a.out) + chunk * E;
    for (long long i = blockIdx.y; i < a.m; i += gridDim.y) {
        union { T v[E]; u32x4 q; } o;
#pragma unroll
        for (int e = 0; e < E; ++e) o.v[e] = off[e] >= 0 ? src[i * a.lda + off[e]] : (T)0;
        *reinterpret_cast<u32x4*>(dst + i * a.lda_out) = o.q;
    }
}

// Host side of both entry points: checks a.cols, a.n_out, a.out and a.lda_out (elements of `bytes`
// bytes, one of BYTES...), then extra() (0, or the failure it reported), and launches about 4096 blocks:
// each thread walks rows blockIdx.y, + gridDim.y, ... with its column offsets in registers.
template <int... BYTES, typename Extra>
int gather_columns(int device, hipStream_t stream, int bytes, const GatherArgs& a, Extra&& extra) {
    using bpgl_host::fail;
    if (!a.cols || !a.out) return fail(BPGL_E_ARG, "cols and A_out must be non-null");
    const int V = 16 / bytes;
    if (a.n_out <= 0) return fail(BPGL_E_ARG, "n_out must be > 0");
    if (a.lda_out < a.n_out || a.lda_out % V)
        return fail(BPGL_E_ARG, "lda_out (%lld) must be >= n_out (%lld) and a multiple of %d", a.lda_out, a.n_out, V);
    if (((uintptr_t)a.out) % 16) return fail(BPGL_E_ARG, "A_out must be 16-byte aligned");
    if (a.lda_out / V > (int64_t)0x7fffffff * kThreads) return fail(BPGL_E_ARG, "lda_out too large");
    if (int rc = extra()) return rc;
    HIP_TRY(hipSetDevice(device));
    const int64_t gx = bpgl_host::cdiv(a.lda_out / V, kThreads);
    const int64_t gy = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(a.m, 65535), bpgl_host::cdiv(4096, gx)));
    const auto kernel = bpgl_host::dispatch<BYTES...>(bytes, [](auto b) { return &k_gather_cols<decltype(b)::value>; });
    hipLaunchKernelGGL(kernel, dim3((unsigned)gx, (unsigned)gy), dim3(kThreads), 0, stream, a);
    LAUNCH_CHECK("k_gather_cols");
    return 0;
}
template <int... BYTES>
int gather_columns(int device, hipStream_t stream, int bytes, const GatherArgs& a) {
    return gather_columns<BYTES...>(device, stream, bytes, a, [] { return 0; });
}

}  // namespace bpgl
