// fixed_ops.h - the arithmetic of DESIGN.md "Fixed point" as device functions, shared by the per-module kernels
// (fixed_point.hip) and the one-workgroup-per-graph kernel (fixed_events.hip): requant, lookup, quant, the overflow
// counter of a wave, the LDS copies of weights, and the host's reading of a gnn_fx_format_t.  One copy, so that the
// two routes cannot drift apart by a bit.
#pragma once
#include "common.h"
#include "gnn_hip_fixed.h"

namespace gnn {

struct Fx {
    int32_t Fb, W, sat, tb;
    int32_t lo, hi;
    int64_t half;       // what "rnd" adds before the shift: 2^(Fb-1), or 0
};

__device__ __forceinline__ int32_t fx_requant(int64_t acc, const Fx &f, int &over)
{
    int64_t k = (acc + f.half) >> f.Fb;
    if (k < f.lo || k > f.hi) {
        ++over;
        if (f.sat)
            k = k < f.lo ? f.lo : f.hi;
        else
            k = (int64_t)((uint64_t)k << (64 - f.W)) >> (64 - f.W);
    }
    return (int32_t)k;
}

// T[clamp(((int64) k << s >> Fb) + 2^(tb-1), 0, 2^tb - 1)]
__device__ __forceinline__ int32_t fx_lookup(const int32_t *T, int32_t k, int s, const Fx &f)
{
    int64_t idx = (((int64_t)k << s) >> f.Fb) + (1 << (f.tb - 1));
    const int64_t last = (1 << f.tb) - 1;
    idx = idx < 0 ? 0 : (idx > last ? last : idx);
    return T[idx];
}
__device__ __forceinline__ int32_t fx_tanh(const int32_t *T, int32_t k, const Fx &f) { return fx_lookup(T, k, f.tb - 3, f); }
__device__ __forceinline__ int32_t fx_sigmoid(const int32_t *T, int32_t k, const Fx &f) { return fx_lookup(T, k, f.tb - 4, f); }

// clip(rint(x 2^Fb), lo, hi): the scaling is exact in float32 (a power of two), rintf rounds half to even
__device__ __forceinline__ int32_t fx_quant(float x, float scale, const Fx &f)
{
    const float v = rintf(x * scale);
    if (v != v) return 0;
    return (int32_t)fminf(fmaxf(v, (float)f.lo), (float)f.hi);
}

// adds a lane's count of one stage over the wave; lane 0 adds the wave's sum into the counter.  Every lane of the wave
// must arrive (the kernels return nowhere before it).
__device__ __forceinline__ void fx_count(int over, int64_t *counter)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) over += __shfl_xor(over, o);
    if ((threadIdx.x & 63) == 0 && over)
        atomicAdd(reinterpret_cast<unsigned long long *>(counter), (unsigned long long)over);
}

// LDS copies --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void lds_copy(int32_t *dst, const int32_t *__restrict__ src, int n)
{
    for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
}
// columns [col0, col0 + K) of W [Dout, ldw] as dst[k * Dout + d], rows K .. KP of dst zero
__device__ __forceinline__ void lds_copy_T(int32_t *dst, const int32_t *__restrict__ W, int Dout, int ldw, int col0, int K,
                                           int KP)
{
    for (int i = threadIdx.x; i < KP * Dout; i += blockDim.x) {
        const int k = i / Dout, d = i - k * Dout;
        dst[i] = k < K ? W[d * ldw + col0 + k] : 0;
    }
}

inline int fx_format_ok(int W, int I, int tb) { return W >= 4 && W <= 24 && I >= 2 && I <= W && tb >= 4 && tb <= 12; }

// the kernels' view of a format the entry point has checked
inline Fx fx_of(const gnn_fx_format_t &fmt)
{
    Fx f;
    f.W = fmt.total_bits;
    f.Fb = fmt.total_bits - fmt.int_bits;
    f.sat = fmt.overflow == GNN_FX_SAT;
    f.tb = fmt.table_bits;
    f.lo = -(1 << (f.W - 1));
    f.hi = (1 << (f.W - 1)) - 1;
    f.half = fmt.rounding == GNN_FX_RND && f.Fb > 0 ? (int64_t)1 << (f.Fb - 1) : 0;
    return f;
}

}  // namespace gnn
