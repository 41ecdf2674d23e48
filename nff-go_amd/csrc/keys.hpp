// keys.hpp — classification from compact 5-tuple keys (internal; keys.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "engine.hpp"
#include "nffacl.h"

namespace nffacl {

// Keys per lane per batch of the key kernels (keys.hip: the work split).
constexpr int kKeysU = 2;

// Classify n keys against `t` (launch_slots' conventions: records the launch
// on `t`, n == 0 is a no-op).  d_keys / d_key6 are 16-byte aligned.
int launch_keys(nffacl_engine *eng, DevTable *t, const nffacl_key *d_keys, const nffacl_key6 *d_key6,
                uint32_t n_key6, uint64_t n, uint32_t *d_port, uint64_t *d_permit, hipStream_t stream);

}  // namespace nffacl
