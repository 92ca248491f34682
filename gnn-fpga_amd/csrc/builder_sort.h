// builder_sort.h - the stable radix sort of (u64 key, int32 value) pairs of hit_samples.hip, event_graphs.hip and select_hits.hip, out
// of a workspace piece carved beforehand (the only includers of rocprim among the builders).
#pragma once
#include <rocprim/rocprim.hpp>

#include "builder_common.h"

namespace gnn {

// the temporary storage a sort of n pairs on any number of key bits needs
inline size_t sort_temp_bytes(int64_t n)
{
    size_t t = 0;
    (void)rocprim::radix_sort_pairs(nullptr, t, (const u64 *)nullptr, (u64 *)nullptr, (const int32_t *)nullptr,
                                    (int32_t *)nullptr, (size_t)n, 0u, 64u, (hipStream_t)0, false);
    return t + 256;
}

// sorts by the low `bits` bits of the keys; `who` (the entry point) and `what` (the sort) name a failure
inline int sort_pairs(const char *who, const char *what, void *temp, size_t temp_bytes, const u64 *kin, u64 *kout,
                      const int32_t *vin, int32_t *vout, int64_t n, int bits, hipStream_t s)
{
    size_t tb = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, tb, kin, kout, vin, vout, (size_t)n, 0u, (unsigned)bits, s, false);
    if (e == hipSuccess && tb > temp_bytes) e = hipErrorInvalidValue;
    tb = temp_bytes;
    if (e == hipSuccess)
        e = rocprim::radix_sort_pairs(temp, tb, kin, kout, vin, vout, (size_t)n, 0u, (unsigned)bits, s, false);
    if (e != hipSuccess) return fail(-(int)e, "%s: radix sort %s: %s", who, what, hipGetErrorString(e));
    return 0;
}

}  // namespace gnn
