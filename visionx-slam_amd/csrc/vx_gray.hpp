// vx_gray.hpp — the one gray conversion of the library (orb.hip's pyramid level 0, init_gate.hip's sums).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace vx {

// cvtColor BGR2GRAY fixed point (B 1868, G 9617, R 4899, >> 14)
__device__ __forceinline__ uint8_t gray_bgr(int b, int g, int r) {
    return (uint8_t)((b * 1868 + g * 9617 + r * 4899 + (1 << 13)) >> 14);
}

// the same on a pixel in memory; 1 channel passes through
__device__ __forceinline__ uint8_t gray_px(const uint8_t* s, int ch) {
    if (ch == 1) return s[0];
    return gray_bgr(s[0], s[1], s[2]);
}

}  // namespace vx
