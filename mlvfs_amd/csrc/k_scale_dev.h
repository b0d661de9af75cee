// k_scale_dev.h -- what the averaging kernels share (k_scale.hip, k_resample.hip): the division by a launch-wide constant as a
// multiplication (ScDiv, scdiv_make: clip.h).
#pragma once
#include "clip.h"
#include "render_route.h"

namespace mlv {
namespace {                    // every including file's own copy

// floor(n / d) for every n below 2^32 (scdiv_make, clip.h)
__device__ __forceinline__ uint32_t sc_div(uint32_t n, const ScDiv &d)
{
    const uint32_t t = __umulhi(n, d.m);
    return (t + ((n - t) >> d.s1)) >> d.s2;
}

}  // namespace
}  // namespace mlv
