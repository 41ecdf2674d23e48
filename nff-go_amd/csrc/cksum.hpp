// cksum.hpp — checksums of packed frames (internal; cksum.hip).
#pragma once

#include <cstdint>

namespace nffacl {

// A tile is kCkTile consecutive frames, one per thread of a kCkBlock
// workgroup (nffacl_checksum_frames_plan reports ceil(n / kCkTile) tiles).
constexpr uint32_t kCkBlock = 1024;
constexpr uint32_t kCkTile = kCkBlock;

}  // namespace nffacl
