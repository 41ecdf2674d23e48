// route_frames.hip — the per-output packet lists of segmentProcess
// (flow/flow.go:1462-1486) for packed variable-length frames: output frame j
// is frame d_index[j] of a (frames, desc) batch, the outputs packed back to
// back with descriptors of their own (desc = offset << 16 | len, the layout
// nffacl_classify_frames_device reads).
//
// All sizes are counted in 16-byte chunks: room(len) = len rounded up to
// `align`, a multiple of 16, and frames start 16-byte aligned on both sides.
// Three launches on the caller's stream, none of which waits on another
// workgroup, no global atomics:
//   k_gatherf_sums   one workgroup per tile of kGatherfTile positions j: lane
//                    j reads d_index[j], gathers that frame's descriptor and
//                    the workgroup sums the rooms into sums[tile]
//   k_gatherf_scan   one workgroup: exclusive 64-bit scan of sums in place
//                    (a tile's first output chunk) and *d_out_bytes
//   k_gatherf_copy   one workgroup per tile: re-reads the tile's indices and
//                    descriptors (L2), scans the rooms into LDS, writes the
//                    output descriptors, then copies output-stationary
// Output-stationary: the tile's output chunks are numbered 0..start[T) and
// thread t of round k owns chunk c = 1024 k + t.  It finds the frame that
// chunk lies in (binary search over start[] in LDS), loads the frame's chunk
// c - start[f] with one nontemporal 16-byte load (a source byte is read once)
// if that chunk starts inside the frame, zeroes the bytes past len and stores
// 16 bytes at chunk base + c.  Every store instruction of a wave writes 1 KiB
// contiguous whatever the frame lengths are; every output chunk is written
// exactly once (data, clipped data or the zeros of a pad); a tile of 64-byte
// frames and one of 1518-byte frames differ in their round count only.
// Registers / LDS per kernel and the measured figures: DESIGN.md §4.10.
#include <hip/hip_runtime.h>

#include "classify.hpp"
#include "devutil.hpp"
#include "nffacl.h"
#include "route.hpp"

namespace nffacl {
namespace dev {

constexpr uint32_t kWaves = kRouteBlock / 64;

// A tile's rooms fit 22 bits (1024 frames x 4096 chunks): summed in u32.
__global__ __launch_bounds__(kRouteBlock) void k_gatherf_sums(const uint64_t *__restrict__ desc, uint64_t n,
                                                              const uint32_t *__restrict__ index, uint64_t m,
                                                              uint32_t amask, uint64_t *__restrict__ sums) {
    __shared__ uint32_t wsum[kWaves];
    const uint32_t tid = threadIdx.x, lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    uint32_t room;
    frame_at(desc, n, index, uint64_t(blockIdx.x) * kGatherfTile + tid, m, amask, room);
    const uint32_t incl = wave_scan_incl(room);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    if (wave == 0) {  // the 16 partials: one more DPP scan, in wave 0
        const uint32_t s = wave_scan_incl(lane < kWaves ? wsum[lane] : 0u);
        if (lane == 63) sums[blockIdx.x] = s;
    }
}

// Exclusive scan of sums[0, tiles) in place, one workgroup, shaped like
// k_route_scan: every thread sums its own run of tiles, the run sums are
// scanned (DPP inside a wave, LDS across the 16 waves), every thread rewrites
// its run.  The sums are 64-bit (up to 2^31 frames x 4096 chunks = 2^43); the
// DPP scan is 32-bit, so a run sum goes through it as two limbs, its low 24
// bits and the rest, neither of which can carry out of 32 bits over 64 lanes.
__global__ __launch_bounds__(kRouteBlock) void k_gatherf_scan(uint64_t *sums, uint32_t tiles,
                                                              uint64_t *__restrict__ out_bytes) {
    __shared__ uint64_t wsum[kWaves];
    const uint32_t tid = threadIdx.x, lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t per = (tiles + kRouteBlock - 1) / kRouteBlock;  // <= 2^11
    const uint32_t lo = min(tid * per, tiles), hi = min(lo + per, tiles);
    uint64_t sum = 0;
    for (uint32_t i = lo; i < hi; ++i) sum += sums[i];
    const uint32_t s0 = wave_scan_incl(static_cast<uint32_t>(sum) & 0xFFFFFFu);
    const uint32_t s1 = wave_scan_incl(static_cast<uint32_t>(sum >> 24));
    const uint64_t incl = (uint64_t(s1) << 24) + s0;
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint64_t run = incl - sum, total = 0;
    for (uint32_t w = 0; w < kWaves; ++w) {
        run += w < wave ? wsum[w] : 0;
        total += wsum[w];
    }
    for (uint32_t i = lo; i < hi; ++i) {
        const uint64_t c = sums[i];
        sums[i] = run;
        run += c;
    }
    if (tid == 0) *out_bytes = total << 4;
}

__global__ __launch_bounds__(kRouteBlock) void k_gatherf_copy(const uint8_t *__restrict__ frames,
                                                              const uint64_t *__restrict__ desc, uint64_t n,
                                                              const uint32_t *__restrict__ index, uint64_t m,
                                                              uint32_t amask, const uint64_t *__restrict__ starts,
                                                              u32x4 *__restrict__ out, uint64_t cap_chunks,
                                                              uint64_t *__restrict__ out_desc) {
    __shared__ uint32_t start[kGatherfTile + 1];  // a frame's first chunk inside the tile; [T] = the tile's chunks
    __shared__ uint64_t sdesc[kGatherfTile];      // its source descriptor
    __shared__ uint32_t wsum[kWaves];
    const uint32_t tid = threadIdx.x, lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint64_t j = uint64_t(blockIdx.x) * kGatherfTile + tid;
    const uint64_t base = starts[blockIdx.x];  // the tile's first output chunk

    // A: exclusive scan of the tile's rooms
    uint32_t room;
    const uint64_t ds = frame_at(desc, n, index, j, m, amask, room);
    const uint32_t incl = wave_scan_incl(room);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t first = incl - room;
    for (uint32_t w = 0; w < wave; ++w) first += wsum[w];
    start[tid] = first;
    sdesc[tid] = ds;
    if (tid == kGatherfTile - 1) start[kGatherfTile] = first + room;
    if (j < m) out_desc[j] = (base + first) << 20 | (ds & 0xFFFFu);  // byte offset << 16 | len
    __syncthreads();

    // B: one output chunk per thread and round
    const uint32_t total = start[kGatherfTile];
    const u32x4 *src = reinterpret_cast<const u32x4 *>(frames);
    for (uint32_t c = tid; c < total; c += kRouteBlock) {
        uint32_t f = 0;  // the last frame that starts at or before c: start[f] <= c < start[f + 1]
#pragma unroll
        for (uint32_t s = kGatherfTile / 2; s; s >>= 1) f += start[f + s] <= c ? s : 0u;
        const uint64_t fd = sdesc[f];
        const uint32_t k = c - start[f];
        const int rem = static_cast<int>(static_cast<uint32_t>(fd) & 0xFFFFu) - static_cast<int>(16u * k);
        // (branch-free: a chunk that starts past its frame's end is a pad, read from the zero block)
        const u32x4 v = __builtin_nontemporal_load(rem > 0 ? src + (fd >> 20) + k : &g_zero16);
        uint32_t d[4] = {v.x, v.y, v.z, v.w};
        if (rem < 16) clip_dwords<4>(d, static_cast<uint32_t>(max(rem, 0)));
        if (base + c < cap_chunks) out[base + c] = u32x4{d[0], d[1], d[2], d[3]};
    }
}

}  // namespace dev
}  // namespace nffacl

using namespace nffacl;

extern "C" {

int nffacl_route_frames_plan(uint64_t m, uint64_t *tiles, uint64_t *scratch_bytes) {
    if (!tiles || !scratch_bytes || m > kRouteMaxN) return NFFACL_ERR_INVALID_ARG;
    *tiles = (m + kGatherfTile - 1) / kGatherfTile;
    *scratch_bytes = *tiles * sizeof(uint64_t);
    return NFFACL_OK;
}

int nffacl_route_gather_frames_device(nffacl_router *r, const uint8_t *d_frames, const uint64_t *d_desc, uint64_t n,
                                      const uint32_t *d_index, uint64_t m, uint32_t align, uint8_t *d_out,
                                      uint64_t out_cap, uint64_t *d_out_desc, uint64_t *d_out_bytes, void *stream) {
    if (!r || !d_out_bytes || m > r->max_n || align < 16 || align > 4096 || (align & (align - 1)) != 0 ||
        (out_cap % 16) != 0)
        return NFFACL_ERR_INVALID_ARG;
    if (m && (!d_index || !d_out_desc || !d_out || (reinterpret_cast<uintptr_t>(d_out) % 16) != 0 ||
              (n && (!d_desc || !d_frames || (reinterpret_cast<uintptr_t>(d_frames) % 16) != 0))))
        return NFFACL_ERR_INVALID_ARG;
    HIP_TRY(hipSetDevice(r->device));
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const uint32_t tiles = static_cast<uint32_t>((m + kGatherfTile - 1) / kGatherfTile);  // <= 2^21
    const uint32_t amask = align - 1;
    if (tiles)
        hipLaunchKernelGGL(dev::k_gatherf_sums, dim3(tiles), dim3(kRouteBlock), 0, s, d_desc, n, d_index, m, amask,
                           r->d_fsums);
    hipLaunchKernelGGL(dev::k_gatherf_scan, dim3(1), dim3(kRouteBlock), 0, s, r->d_fsums, tiles, d_out_bytes);
    if (tiles)
        hipLaunchKernelGGL(dev::k_gatherf_copy, dim3(tiles), dim3(kRouteBlock), 0, s, d_frames, d_desc, n, d_index, m,
                           amask, r->d_fsums, reinterpret_cast<dev::u32x4 *>(d_out), out_cap / 16, d_out_desc);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(r->last, s));
    r->used = true;
    return NFFACL_OK;
}

}  // extern "C"
