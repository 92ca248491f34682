// lane_ops.h - the lane primitives shared by gnn_kernels.hip, sell_pipeline.hip and backward.hip: DPP moves inside a
// quad or a row of 16 lanes, vector loads / stores of a lane's piece of a row, and the float vector types.
#pragma once
#include <hip/hip_runtime.h>

namespace gnn {

typedef float f2_t __attribute__((ext_vector_type(2)));
typedef float f3_t __attribute__((ext_vector_type(3)));
typedef float f4_t __attribute__((ext_vector_type(4)));

// v of the lane that the DPP control CTRL names (quad_perm, row_ror: ...)
template <int CTRL>
__device__ __forceinline__ float dpp(float v)
{
    // quad_perm reads only lanes of the own quad, row_ror only lanes of the own row of 16 (always valid), so no "old"
    // value is needed: mov_dpp (old = undef) saves the v_mov that update_dpp(0, ...) needs to set it up
    return __builtin_bit_cast(
        float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}

// v of lane J of the own quad, in all 4 lanes
template <int J>
__device__ __forceinline__ int quad_bcast(int v)
{
    return __builtin_amdgcn_mov_dpp(v, J * 0x55, 0xF, 0xF, true);
}
template <int J>
__device__ __forceinline__ float quad_bcast(float v)
{
    return dpp<J * 0x55>(v);
}

// sum over the 4 lanes of a quad, identical bits in all 4 lanes
__device__ __forceinline__ float quad_sum(float v)
{
    v += dpp<0xB1>(v);   // quad_perm [1,0,3,2]: lane ^ 1
    v += dpp<0x4E>(v);   // quad_perm [2,3,0,1]: lane ^ 2
    return v;
}

// N floats (1, 2 or a multiple of 4; aligned to their own size, 16 bytes from 4 on) as one load / store per 16 bytes
template <int N>
__device__ __forceinline__ void load_vec(const float *__restrict__ src, float *dst)
{
    if constexpr (N == 1) {
        dst[0] = src[0];
    } else if constexpr (N == 2) {
        const float2 v = *reinterpret_cast<const float2 *>(src);
        dst[0] = v.x; dst[1] = v.y;
    } else {
        static_assert(N % 4 == 0, "vector length");
#pragma unroll
        for (int i = 0; i < N / 4; ++i) {
            const float4 v = reinterpret_cast<const float4 *>(src)[i];
            dst[4 * i] = v.x; dst[4 * i + 1] = v.y; dst[4 * i + 2] = v.z; dst[4 * i + 3] = v.w;
        }
    }
}

template <int N>
__device__ __forceinline__ void store_vec(float *__restrict__ dst, const float *src)
{
    if constexpr (N == 1) {
        dst[0] = src[0];
    } else if constexpr (N == 2) {
        *reinterpret_cast<float2 *>(dst) = make_float2(src[0], src[1]);
    } else {
        static_assert(N % 4 == 0, "vector length");
#pragma unroll
        for (int i = 0; i < N / 4; ++i)
            reinterpret_cast<float4 *>(dst)[i] =
                make_float4(src[4 * i], src[4 * i + 1], src[4 * i + 2], src[4 * i + 3]);
    }
}

}   // namespace gnn
