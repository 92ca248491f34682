// common.h - what the units share: the error and profiler hooks (defined in core.hip), the launch macro, the shape
// lists and their dispatch (ShapeList), workspace carving and a few device helpers.  It declares nothing that
// gnn_kernels.hip, sell_pipeline.hip or backward.hip define: each of them owns its entry points.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gnn_hip.h"

namespace gnn {

int fail(int code, const char *fmt, ...);
void prof_pre(const char *name, hipStream_t s);
void prof_post(hipStream_t s);
// gnn_profile_begin/end: the launches of ONE library call are timed from one event per kernel boundary
// (see Profiler::chain); put one at the top of an entry point that launches several kernels
struct ProfChain {
    bool prev;
    ProfChain();
    ~ProfChain();
    ProfChain(const ProfChain &) = delete;
    ProfChain &operator=(const ProfChain &) = delete;
};

#define GNN_LAUNCH(NAME, KERNEL, GRID, BLOCK, STREAM, ...)                                       \
    do {                                                                                         \
        gnn::prof_pre(NAME, STREAM);                                                             \
        hipLaunchKernelGGL(KERNEL, dim3(GRID), dim3(BLOCK), 0, STREAM, __VA_ARGS__);             \
        gnn::prof_post(STREAM);                                                                  \
        hipError_t err_ = hipGetLastError();                                                     \
        if (err_ != hipSuccess)                                                                  \
            return gnn::fail(-(int)err_, "%s launch failed: %s", NAME, hipGetErrorString(err_)); \
    } while (0)

// same with dynamic LDS bytes
#define GNN_LAUNCH_SH(NAME, KERNEL, GRID, BLOCK, SHMEM, STREAM, ...)                             \
    do {                                                                                         \
        gnn::prof_pre(NAME, STREAM);                                                             \
        hipLaunchKernelGGL(KERNEL, dim3(GRID), dim3(BLOCK), SHMEM, STREAM, __VA_ARGS__);         \
        gnn::prof_post(STREAM);                                                                  \
        hipError_t err_ = hipGetLastError();                                                     \
        if (err_ != hipSuccess)                                                                  \
            return gnn::fail(-(int)err_, "%s launch failed: %s", NAME, hipGetErrorString(err_)); \
    } while (0)

constexpr int kBlock = 256;   // 4 waves of 64

// a shape as a type: hit rows [H'(D) | X(F) | 0-pad] of C floats, stored LDH = gnn_h_stride(F, D) apart
template <int F_, int D_>
struct Shape {
    static constexpr int F = F_, D = D_, C = F + D;
    static constexpr int LDH = (C + 3) & ~3;
};

// The one shape dispatch: a list of Shape<F, D> types, written once per kernel family, that answers "is (F, D)
// listed" and runs a generic lambda at the caller's (F, D) - `fn(sh)` may use sh.F / sh.D as template arguments.
template <typename... S>
struct ShapeList {
    static constexpr bool has(int F, int D) { return ((F == S::F && D == S::D) || ...); }
    // fn(Shape<F, D>{}) for the listed shape (F, D); `miss` where there is none
    template <typename R, typename Fn>
    static R find(int F, int D, R miss, Fn fn)
    {
        (void)((F == S::F && D == S::D && (miss = fn(S{}), true)) || ...);
        return miss;
    }
};

// The (input_dim, hidden_dim) pairs the per-pass forward (gnn_kernels.hip) and the backward (backward.hip) have kernels
// for: one list, so that a shape cannot be trained without a forward or the other way round.
// (input_dim 4: the hit classifier of gnn/MPNN_HitClassifier.ipynb - r, phi, z and the seed label - and the first
// shapes whose hit rows [H' | X] have no zero pad column, C == LDH)
using ModelShapes = ShapeList<Shape<2, 4>, Shape<2, 8>, Shape<2, 16>, Shape<2, 32>, Shape<3, 4>, Shape<3, 8>, Shape<3, 16>,
                              Shape<3, 32>, Shape<3, 64>, Shape<4, 8>, Shape<4, 16>, Shape<4, 32>, Shape<4, 64>,
                              Shape<11, 4>, Shape<11, 8>, Shape<11, 16>>;

// every weight (gradient) pointer of a whole-model call is there
inline bool params_complete(const gnn_params_t *p)
{
    return p && p->Win && p->bin && p->W1 && p->b1 && p->W2 && p->b2 && p->W3 && p->b3 && p->W4 && p->b4;
}
inline bool grads_complete(const gnn_grads_t *gr)
{
    return gr && gr->Win && gr->bin && gr->W1 && gr->b1 && gr->W2 && gr->b2 && gr->W3 && gr->b3 && gr->W4 && gr->b4;
}

// csr_build.hip's device-wide scan, shared: exclusive scans of n_arrays (1 or 2) int32 count arrays stored `stride`
// apart into ptr_a / ptr_b [n + 1] (entry n = the total); `sums` = scan_sums_words(n) int32 of scratch
int64_t scan_sums_words(int64_t n);
int scan_counts(const int32_t *cnt, int64_t stride, int n_arrays, int32_t *ptr_a, int32_t *ptr_b, int64_t n,
                int32_t *sums, hipStream_t s);

// One-time per-DEVICE set-up (hipFuncSetAttribute opt-ins for > 64 KB of dynamic LDS, CU counts):
// a process may drive several devices, and a function attribute set while device 0 was current
// says nothing about device 1.  `static DevOnce once; if (once.need()) { ... }`.
struct DevOnce {
    unsigned long long done = 0;
    bool need()
    {
        int d = 0;
        if (hipGetDevice(&d) != hipSuccess) return true;
        const unsigned long long bit = 1ull << (d & 63);
        if (done & bit) return false;
        done |= bit;
        return true;
    }
};

// CU count of the CURRENT device (cached per device)
inline int device_cus()
{
    static int cus[64] = {0};
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess) return 256;
    int &c = cus[d & 63];
    if (!c) {
        hipDeviceProp_t prop;
        c = (hipGetDeviceProperties(&prop, d) == hipSuccess && prop.multiProcessorCount > 0)
                ? prop.multiProcessorCount : 256;
    }
    return c;
}

// one item per thread; grids beyond 8 workgroups are rounded up to a multiple of 8 so that
// xcd_block() below is a bijection (the surplus workgroups find nothing to do)
inline unsigned grid_for(int64_t n)
{
    const unsigned g = (unsigned)((n + kBlock - 1) / kBlock);
    return g > 8 ? (g + 7) & ~7u : g;
}

// Workgroups are dealt round-robin to the 8 XCDs, each with its own L2.  Items are stored graph
// by graph (hits, segments), and a kernel's gathers stay inside the item's graph: with the plain
// blockIdx order every XCD works on every graph in flight and its L2 thrashes; here XCD x takes
// a CONTIGUOUS eighth of the items, a few graphs at a time.
__device__ __forceinline__ int64_t xcd_block()
{
    const unsigned g = gridDim.x, b = blockIdx.x;
    return (g & 7) ? b : (b & 7) * (g >> 3) + (b >> 3);
}
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

inline int bits_for(unsigned long long v)              // bits to hold 0 .. v (the key bits of a radix sort)
{
    int b = 1;
    while (b < 64 && (v >> b) != 0) ++b;
    return b;
}

// workspaces: the caller's pointer rounded up to 256 bytes, then carved
inline char *align_ws(void *ws) { return reinterpret_cast<char *>((reinterpret_cast<uintptr_t>(ws) + 255) & ~(uintptr_t)255); }

// hands out a workspace piece by piece, each piece 256-byte aligned; a null base only adds up the sizes
struct Carver {
    char *base;
    size_t off = 0;
    template <typename T>
    T *take(size_t count)
    {
        char *p = base ? base + off : nullptr;
        off += align256(count * sizeof(T));
        return reinterpret_cast<T *>(p);
    }
    size_t bytes() const { return off + 256; }         // + what align_ws may skip
};

inline int check_workspace(const void *ws, size_t have, size_t need)
{
    if (!ws || have < need) return fail(GNN_ERR_WORKSPACE, "workspace too small: need %zu bytes", need);
    return 0;
}

// tanh(x) = 1 - 2 / (2^(2 log2(e) x) + 1): v_exp_f32 + v_rcp_f32 (1 ulp each), absolute error
// ~1e-7 everywhere (the score tolerance is absolute, 1e-5).  Saturates correctly at +-inf.
__device__ __forceinline__ float tanh_f(float x)
{
    float t = __builtin_amdgcn_exp2f(x * 2.8853900817779268f);
    return 1.0f - 2.0f * __builtin_amdgcn_rcpf(t + 1.0f);
}

__device__ __forceinline__ float sigmoid_f(float x)
{
    float t = __builtin_amdgcn_exp2f(x * -1.4426950408889634f);
    return __builtin_amdgcn_rcpf(1.0f + t);
}

// Walk CSR entries [k0, k1) of one hit: `row_of(k)` gives the float row entry k points at (an
// index load), `w_of(k)` its weight (an index load and a dependent gather), `use(w, row)` consumes
// them IN ENTRY ORDER (the sums stay bit-identical to a plain loop).  A plain loop is two
// dependent memory latencies per entry; here the index loads, weights and rows of U entries are
// all in flight together before the first one is consumed.
template <int N4, int U = 4, typename RowOf, typename WOf, typename Use>
__device__ __forceinline__ void csr_walk(int k0, int k1, RowOf row_of, WOf w_of, Use use)
{
    int k = k0;
    for (; k + U <= k1; k += U) {
        const float *rp[U];
        float w[U], r[U][4 * N4];
#pragma unroll
        for (int u = 0; u < U; ++u) rp[u] = row_of(k + u);
#pragma unroll
        for (int u = 0; u < U; ++u) w[u] = w_of(k + u);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float4 *r4 = reinterpret_cast<const float4 *>(rp[u]);
#pragma unroll
            for (int i = 0; i < N4; ++i) {
                const float4 a = r4[i];
                r[u][4 * i] = a.x; r[u][4 * i + 1] = a.y; r[u][4 * i + 2] = a.z; r[u][4 * i + 3] = a.w;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) use(w[u], r[u]);
    }
    for (; k < k1; ++k) {
        const float *rp = row_of(k);
        const float w = w_of(k);
        float r[4 * N4];
        const float4 *r4 = reinterpret_cast<const float4 *>(rp);
#pragma unroll
        for (int i = 0; i < N4; ++i) {
            const float4 a = r4[i];
            r[4 * i] = a.x; r[4 * i + 1] = a.y; r[4 * i + 2] = a.z; r[4 * i + 3] = a.w;
        }
        use(w, r);
    }
}

}  // namespace gnn
