// keys.hpp — classification from compact 5-tuple keys (internal; keys.hip,
// keys_encap.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "classify.hpp"
#include "engine.hpp"
#include "nffacl.h"

namespace nffacl {

// Keys per lane per batch of the key kernels (keys.hip: the work split).
constexpr int kKeysU = 2;

// Classify n keys against `t` (launch_slots' conventions: records the launch
// on `t`, n == 0 is a no-op).  d_keys / d_key6 are 16-byte aligned.
int launch_keys(nffacl_engine *eng, DevTable *t, const nffacl_key *d_keys, const nffacl_key6 *d_key6,
                uint32_t n_key6, uint64_t n, uint32_t *d_port, uint64_t *d_permit, hipStream_t stream);

namespace dev {

constexpr uint32_t kFam4 = 4u, kFam6 = 6u;

// Packet idx's key from its parsed fields: each lane writes its own 16-byte
// key (lane-contiguous dwordx4 stores), IPv6 lanes their 32-byte record at
// their packet's index.  Shared by the three extraction kernels.
__device__ __forceinline__ void store_key(const Fields &f, uint64_t idx, bool live, u32x4 *__restrict__ keys,
                                          u32x4 *__restrict__ key6) {
    u32x4 k = {0u, 0u, 0u, 0u};  // neither family: the zero key
    if (f.is4) k = u32x4{f.s[0], f.t[0], f.ports, (f.proto & 0xFFu) | kFam4 << 8};
    if (f.is6) k = u32x4{static_cast<uint32_t>(idx), 0u, f.ports, (f.proto & 0xFFu) | kFam6 << 8};
    if (live) keys[idx] = k;
    if (f.is6) {  // (is6 implies live)
        key6[2 * idx] = u32x4{f.s[0], f.s[1], f.s[2], f.s[3]};
        key6[2 * idx + 1] = u32x4{f.t[0], f.t[1], f.t[2], f.t[3]};
    }
}

}  // namespace dev

}  // namespace nffacl
