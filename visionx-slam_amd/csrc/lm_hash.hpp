// lm_hash.hpp — the resident map's landmark id -> row table (vx_dmap::ht_key / ht_val), shared by
// its users: the lean LocalBA build (ba_lean.hip, which also owns the insert kernels) and the
// TrackWithPnP pair gather (track.hip).  Open addressing, linear probing, splitmix64 of the id;
// a removed landmark's entry stays (its lm_bad row says kLmRemoved).
#pragma once
#include <cstdint>

#include "dmap.hpp"

namespace vx {

constexpr uint64_t kEmptyKey = ~0ull;

__device__ __forceinline__ uint64_t mix(uint64_t x) {  // splitmix64
    x += 0x9e3779b97f4a7c15ull;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

// Map::GetLandmark(k): the landmark's row, -1 when the id was never inserted
__device__ __forceinline__ int ht_get(const uint64_t* key, const int* val, unsigned mask, uint64_t k) {
    unsigned h = (unsigned)mix(k) & mask;
    for (unsigned probe = 0; probe <= mask; ++probe) {
        const uint64_t x = key[h];
        if (x == k) return val[h];
        if (x == kEmptyKey) return -1;
        h = (h + 1) & mask;
    }
    return -1;
}

// the table covers rows [0, n_lm) of m afterwards: new rows added, the whole table rebuilt when it
// has to grow (enqueued on c's stream; ba_lean.hip)
int ht_sync(vx_ctx* c, vx_dmap* m);

}  // namespace vx
