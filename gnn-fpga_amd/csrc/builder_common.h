// builder_common.h - what the GPU builders (graph_build, hit_samples, muon_graph, event_graphs, select_hits) share:
// the reference's float32 arithmetic, the event of a row, the hit builders' status bits and argument checks.
// Include it AFTER the unit's own `#pragma clang fp contract(off)`: these functions are compiled under the includer's setting.
#pragma once
#include "common.h"

#include <cmath>

namespace gnn {

typedef unsigned long long u64;

constexpr float kPiF = (float)M_PI;                    // numpy rounds np.pi / 2 np.pi to float32 against float32 data
constexpr float kTwoPiF = (float)(2.0 * M_PI);
constexpr int64_t kInt32End = (int64_t)1 << 31;        // the first count an int32 index cannot hold

// status bits of the hit builders (GB_ / HS_ / EG_ / SH_STATUS_* in Python); muon_graph.hip has its own
constexpr int kStatusLayer = 1, kStatusInt32 = 2, kStatusEvents = 4, kStatusFinite = 8, kStatusDup = 16;

// the references' phi wrap (calc_dphi: gnn/graph.py:38-42, gnn/Muon_graph.py:54-58, cell 9 of the hit classifier's
// notebook, cell 7 of the full-event one), float32
__device__ __forceinline__ float wrap_dphi(float d)
{
    if (d > kPiF) d = d - kTwoPiF;
    if (d < -kPiF) d = d + kTwoPiF;
    return d;
}

// phi_slope and z0 of a hit pair (gnn/graph.py:57-62, gnn/Muon_graph.py:75-80), float32, in the references' order of
// operations; dr = 0 gives inf or NaN
__device__ __forceinline__ void pair_slope_z0(float r1, float p1, float z1, float r2, float p2, float z2, float &slope,
                                              float &z0)
{
    const float dphi = wrap_dphi(p2 - p1);
    const float dz = z2 - z1, dr = r2 - r1;
    slope = dphi / dr;
    z0 = z1 - (r1 * dz) / dr;
}

// the phi-slope and z0 cut of gnn/graph.py:43-66 and gnn/Muon_graph.py:60-83
__device__ __forceinline__ bool keep_pair(float r1, float p1, float z1, float r2, float p2, float z2, float slope_max,
                                          float z0_max)
{
    float slope, z0;
    pair_slope_z0(r1, p1, z1, r2, p2, z2, slope, z0);
    return fabsf(slope) < slope_max && fabsf(z0) < z0_max;   // NaN (dr = 0, dphi = 0) compares false
}

// a feature: the references divide a float32 column by a float64 scale and round the quotient to float32
__device__ __forceinline__ float feature(float v, double scale) { return (float)((double)v / scale); }

// the largest e in [0, n) with a[e] <= v (0 when there is none)
template <typename T>
__device__ __forceinline__ int64_t last_le(const T *a, int64_t n, int64_t v)
{
    int64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

// the first position p in [0, n) with key[p] >= v (n when there is none)
__device__ __forceinline__ int64_t lower_bound(const u64 *key, int64_t n, u64 v)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (key[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// lane i < E tests entry i of event_ptr: it must run non-decreasing from 0 to n
__device__ __forceinline__ void check_event_ptr(const int64_t *ep, int64_t E, int64_t n, int64_t i,
                                                int32_t *status)
{
    if (i < E && (ep[i] > ep[i + 1] || (i == 0 && (ep[0] != 0 || ep[E] != n)))) atomicOr(status, kStatusEvents);
}

// does event e = last_le(ep, E, i) own row i?  (Not where event_ptr is malformed: check_event_ptr flags that.)
__device__ __forceinline__ bool event_owns(const int64_t *ep, int64_t e, int64_t i)
{
    return ep[e] <= i && i < ep[e + 1];
}

inline int check_scales(const char *who, double scale_r, double scale_phi, double scale_z)
{
    if (!(scale_r != 0.0 && scale_phi != 0.0 && scale_z != 0.0))
        return fail(GNN_ERR_BADARG, "%s: a feature scale is zero or NaN", who);
    return 0;
}

}  // namespace gnn
