// vx_rows.hpp — a byte range copied by every thread of a grid (k_frame_capture, k_track_final).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace vx {

// Bytes [0, nbytes) from src to dst by threads t of nt: nbytes a multiple of 4, both pointers 4-byte
// aligned.  A dword head up to the first 16-byte boundary, uint4 loads and stores over the body, a
// dword tail — when both sides reach that boundary after the same head; otherwise dwords throughout.
// (Rows of 20 bytes, vx_keypoint, are no vector; a block of them is such a range.)
__device__ __forceinline__ void grid_copy_range(void* dst_v, const void* src_v, size_t nbytes, size_t t, size_t nt) {
    uint8_t* dst = static_cast<uint8_t*>(dst_v);
    const uint8_t* src = static_cast<const uint8_t*>(src_v);
    const size_t ms = (16 - (reinterpret_cast<uintptr_t>(src) & 15)) & 15, md = (16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15;
    size_t head = ms == md ? ms : nbytes;
    if (head > nbytes) head = nbytes;
    const size_t nvec = (nbytes - head) / 16, tail0 = head + nvec * 16;
    const uint32_t* s32 = reinterpret_cast<const uint32_t*>(src);
    uint32_t* d32 = reinterpret_cast<uint32_t*>(dst);
    for (size_t k = t; k < head / 4; k += nt) d32[k] = s32[k];
    const uint4* s4 = reinterpret_cast<const uint4*>(src + head);
    uint4* d4 = reinterpret_cast<uint4*>(dst + head);
    for (size_t k = t; k < nvec; k += nt) d4[k] = s4[k];
    for (size_t k = tail0 / 4 + t; k < nbytes / 4; k += nt) d32[k] = s32[k];
}

}  // namespace vx
