// route.hpp — the routing stage behind the nffacl_router handle (internal).
//
// The reference does not hand verdicts back: segmentProcess appends every
// packet of a burst to OutputMbufs[answer] in arrival order and enqueues one
// slice per output flow (flow/flow.go:1462-1486; the vector form through
// asm.GenerateMask, flow.go:1505-1517).  That is a stable partition of the
// burst by answer.  Here the burst is a batch of up to 2^31 verdicts in HBM
// and the partition is three ordinary launches (route.hip): per-tile counts,
// one exclusive scan of them, a per-tile stable scatter.  No workgroup waits
// on another one.
//
// A tile is kRouteTile = 1024 threads x 8 keys.  A packet's bucket is
//   SEPARATE  port != 0                       (separate, flow.go:1795-1797)
//   SPLIT     min(port, n_out)                (makeSplitter, flow.go:1161)
// so there are n_out + 1 buckets, the last one holding the out-of-range
// answers (empty in SEPARATE mode).  The scratch is the count matrix
// counts[bucket * tiles + tile] (bucket-major: its exclusive scan in memory
// order is every (bucket, tile)'s first position in d_index).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "nffacl.h"

namespace nffacl {

constexpr uint32_t kRouteBlock = 1024;                      // threads per tile workgroup (16 waves)
constexpr uint32_t kRouteRounds = 8;                        // keys per thread
constexpr uint32_t kRouteTile = kRouteBlock * kRouteRounds; // 8192 keys
constexpr uint64_t kRouteMaxN = uint64_t(1) << 31;
constexpr uint32_t kRouteMaxOut = 255;

// Key bits of the kernels' template parameter: the smallest of 1, 2, 4, 8
// that holds a bucket number 0..n_out.
inline int route_key_bits(uint32_t n_out) { return n_out < 2 ? 1 : n_out < 4 ? 2 : n_out < 16 ? 4 : 8; }

// Packed-frame gather (route_frames.hip): a tile is kGatherfTile output
// positions, one per thread of a kRouteBlock workgroup; the scratch is one
// 64-bit sum per tile, the tile's rooms in 16-byte chunks (after the scan:
// the tile's first output chunk).
constexpr uint32_t kGatherfTile = kRouteBlock;

namespace dev {

// Inclusive wave sum: row_shr 1, 2, 4, 8 inside the four 16-lane rows, then
// lane 15 of rows 0 / 2 into rows 1 / 3 (row_bcast:15) and lane 31 into the
// upper half (row_bcast:31).  A lane without a source adds `old` = 0.
template <int CTRL, int ROWS>
__device__ __forceinline__ uint32_t dpp_add(uint32_t x) {
    return x + static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(x), CTRL, ROWS, 0xf, false));
}
__device__ __forceinline__ uint32_t wave_scan_incl(uint32_t x) {
    x = dpp_add<0x111, 0xf>(x);
    x = dpp_add<0x112, 0xf>(x);
    x = dpp_add<0x114, 0xf>(x);
    x = dpp_add<0x118, 0xf>(x);
    x = dpp_add<0x142, 0xa>(x);
    x = dpp_add<0x143, 0xc>(x);
    return x;
}

// The packed-frame gathers (route_frames.hip, route_decap.hip).  Position j's
// frame: its descriptor (0: an empty frame, for j >= m and for an index past
// the batch) and its room in chunks.  `amask` = align - 1.
__device__ __forceinline__ uint64_t frame_at(const uint64_t *__restrict__ desc, uint64_t n,
                                             const uint32_t *__restrict__ index, uint64_t j, uint64_t m,
                                             uint32_t amask, uint32_t &room) {
    uint64_t ds = 0;
    if (j < m) {
        const uint32_t i = index[j];
        if (i < n) ds = desc[i];
    }
    room = (((static_cast<uint32_t>(ds) & 0xFFFFu) + amask) & ~amask) >> 4;  // <= 4096
    return ds;
}

// Defined in route_frames.hip; the decapsulating gather (route_decap.hip) launches it too.
__global__ __launch_bounds__(kRouteBlock) void k_gatherf_scan(uint64_t *sums, uint32_t tiles,
                                                              uint64_t *__restrict__ out_bytes);

}  // namespace dev

}  // namespace nffacl

struct nffacl_router {
    int device = 0;
    uint32_t mode = NFFACL_ROUTE_SEPARATE;
    uint32_t n_out = 2;
    uint64_t max_n = 0;
    uint32_t *d_counts = nullptr;  // (n_out + 1) * tiles(max_n) dwords
    uint64_t *d_fsums = nullptr;   // nffacl_route_frames_plan(max_n): one sum per gather tile
    hipEvent_t last = nullptr;     // recorded behind every launch; destroy waits on it
    bool used = false;
};
