// swr_user_math.hip.h -- what every run-time compiled contract shares: the fixed-width types hiprtc does not bring, and the scalar
// helpers of the build's System.Numerics model under the names user text calls them by.  Included by swr_program.hip.h (fragment and
// vertex programs) and swr_post.hip.h (post-process programs): one definition, so a `swr_lerp` in a post program is the `swr_lerp` of
// a fragment program in every library build.
#pragma once

#ifdef __HIPCC_RTC__
typedef __INT8_TYPE__ int8_t;
typedef __UINT8_TYPE__ uint8_t;
typedef __INT16_TYPE__ int16_t;
typedef __UINT16_TYPE__ uint16_t;
typedef __INT32_TYPE__ int32_t;
typedef __UINT32_TYPE__ uint32_t;
typedef __INT64_TYPE__ int64_t;
typedef __UINT64_TYPE__ uint64_t;
typedef __UINTPTR_TYPE__ uintptr_t;
#ifndef offsetof
#define offsetof(T, m) __builtin_offsetof(T, m)
#endif
#endif

#include "swr_device.h"

// Lerp's a * (1 - t) + b * t as the build's System.Numerics model evaluates it (SWR_NUMERICS_FMA)
__device__ __forceinline__ float swr_lerp(float a, float b, float t) { return swr::nm_lerp(a, b, t); }
__device__ __forceinline__ float4 swr_lerp(float4 a, float4 b, float t) {
    return make_float4(swr_lerp(a.x, b.x, t), swr_lerp(a.y, b.y, t), swr_lerp(a.z, b.z, t), swr_lerp(a.w, b.w, t));
}
// MathF.Max / Math.Clamp as .NET evaluates them
__device__ __forceinline__ float swr_max(float a, float b) { return swr::mathf_max(a, b); }
__device__ __forceinline__ float swr_clamp(float v, float lo, float hi) { return swr::math_clamp(v, lo, hi); }
