// route_decap.hip — the packed-frame gather of route_frames.hip that drops the
// shims on the way: output frame j is frame d_index[j] without its bytes
// [14, cursor), the cursor being what nffacl_extract_keys_encap_frames_device
// reported for it (RemoveVLANTag / RemoveMPLS / DecapsulateIPv4GTP followed by
// the enqueue of segmentProcess, packet/packet.go:789-798, gtp.go:132-140), the
// EtherType set to what the inner header is.  Semantics: nffacl.h.
//
// Counting, packing and the three launches are those of route_frames.hip (its
// k_gatherf_scan is launched as it is); a frame's room comes from its output
// length L' = L - s, s = cursor - 14 the strip, a multiple of 4.
//   k_gatherd_sums   k_gatherf_sums plus a 2-byte gather of the cursor
//   k_gatherd_copy   output-stationary as k_gatherf_copy: thread t of round k
//                    owns output chunk 1024 k + t of the tile
// A stripped frame's output chunk q >= 1 is source dwords 4q + s/4 .. + 3: not
// an aligned source chunk.  With a = q + (s >> 4) and r = (s >> 2) & 3 it is
// the upper 4 - r dwords of aligned source chunk a and the lower r of chunk
// a + 1.  Consecutive lanes own consecutive output chunks, so inside a frame
// lane l + 1 has loaded exactly the chunk a + 1 that lane l needs: every lane
// issues ONE aligned nontemporal 16-byte load (a source byte is still read
// once), takes three dwords of its right neighbour's registers (DPP
// wave_shl:1) and rotates the seven dwords by r with selects.  Only a lane
// whose right neighbour is not in its frame, or holds a pad — lane 63 and a
// frame's last data chunk — loads chunk a + 1 itself, in a branch a ballot
// skips (issued before anything waits for chunk a), and only if that chunk
// starts inside the frame: no read ever runs past a frame's last 16-byte
// chunk.  Two rounds are located and loaded together before either is
// finished.  Output chunk 0 is source chunk 0 with dword 3 (EtherType | the
// inner header's first two bytes) settled in phase A.
// Registers / LDS and the measured figures: DESIGN.md §4.12.
#include <hip/hip_runtime.h>

#include "classify.hpp"
#include "devutil.hpp"
#include "nffacl.h"
#include "route.hpp"

namespace nffacl {
namespace dev {

constexpr uint32_t kWaves = kRouteBlock / 64;
constexpr uint32_t kDecapRounds = 2;  // rounds of the copy whose searches and loads are in flight together

// frame_at with the strip: `s` = cursor - 14 where the cursor is one the rule
// accepts (14 < cursor < len, a whole number of dwords behind byte 14), else 0;
// `room` is that of the output length len - s.  `i` is the source frame (only
// meaningful where s != 0, which implies a frame of the batch).
__device__ __forceinline__ uint64_t decap_at(const uint64_t *__restrict__ desc, uint64_t n,
                                             const uint16_t *__restrict__ inner_off,
                                             const uint32_t *__restrict__ index, uint64_t j, uint64_t m,
                                             uint32_t amask, uint32_t &i, uint32_t &s, uint32_t &room) {
    uint64_t ds = 0;
    uint32_t c = 0;
    i = 0;
    if (j < m) {
        i = index[j];
        if (i < n) {
            ds = desc[i];
            c = inner_off[i];
        }
    }
    const uint32_t len = static_cast<uint32_t>(ds) & 0xFFFFu;
    s = (c > 14u && c < len && ((c - 14u) & 3u) == 0u) ? c - 14u : 0u;
    room = ((len - s + amask) & ~amask) >> 4;
    return ds;
}

__global__ __launch_bounds__(kRouteBlock) void k_gatherd_sums(const uint64_t *__restrict__ desc, uint64_t n,
                                                              const uint16_t *__restrict__ inner_off,
                                                              const uint32_t *__restrict__ index, uint64_t m,
                                                              uint32_t amask, uint64_t *__restrict__ sums) {
    __shared__ uint32_t wsum[kWaves];
    const uint32_t tid = threadIdx.x, lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    uint32_t i, s, room;
    decap_at(desc, n, inner_off, index, uint64_t(blockIdx.x) * kGatherfTile + tid, m, amask, i, s, room);
    const uint32_t incl = wave_scan_incl(room);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    if (wave == 0) {
        const uint32_t t = wave_scan_incl(lane < kWaves ? wsum[lane] : 0u);
        if (lane == 63) sums[blockIdx.x] = t;
    }
}

// Lane l <- lane l + 1's x (wave_shl:1); lane 63, which has no right neighbour, <- old.
__device__ __forceinline__ uint32_t from_next_lane(uint32_t old, uint32_t x) {
    return static_cast<uint32_t>(
        __builtin_amdgcn_update_dpp(static_cast<int>(old), static_cast<int>(x), 0x130, 0xf, 0xf, false));
}

__global__ __launch_bounds__(kRouteBlock) void k_gatherd_copy(
    const uint8_t *__restrict__ frames, const uint64_t *__restrict__ desc, uint64_t n,
    const uint16_t *__restrict__ inner_off, const uint32_t *__restrict__ keys, const uint32_t *__restrict__ index,
    uint64_t m, uint32_t amask, const uint64_t *__restrict__ starts, u32x4 *__restrict__ out, uint64_t cap_chunks,
    uint64_t *__restrict__ out_desc) {
    __shared__ uint32_t start[kGatherfTile + 1];  // a frame's first output chunk inside the tile; [T] = the tile's chunks
    __shared__ uint64_t sdesc[kGatherfTile];      // its source descriptor
    __shared__ uint32_t sd3[kGatherfTile];        // its output dword 3 where it is stripped
    __shared__ uint16_t sstrip[kGatherfTile];     // its strip s
    __shared__ uint32_t wsum[kWaves];
    const uint32_t tid = threadIdx.x, lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint64_t j = uint64_t(blockIdx.x) * kGatherfTile + tid;
    const uint64_t base = starts[blockIdx.x];  // the tile's first output chunk

    // A: strips, exclusive scan of the tile's rooms, every stripped frame's dword 3
    uint32_t i, s, room;
    const uint64_t ds = decap_at(desc, n, inner_off, index, j, m, amask, i, s, room);
    const uint32_t incl = wave_scan_incl(room);
    if (lane == 63) wsum[wave] = incl;
    uint32_t d3 = 0;
    if (s) {
        // The dword at byte cursor - 2 = s + 12 (dword aligned, inside the frame: cursor < len): the inner
        // EtherType, or what stands in its place, below the inner header's first two bytes.
        d3 = reinterpret_cast<const uint32_t *>(frames + (ds >> 16))[(s + 12u) >> 2];
        const uint32_t fam = (keys[4 * uint64_t(i) + 3] >> 8) & 0xFFu;  // nffacl_key.meta
        if (fam == 4u) d3 = (d3 & 0xFFFF0000u) | 0x0008u;                // 08 00
        if (fam == 6u) d3 = (d3 & 0xFFFF0000u) | 0xDD86u;                // 86 DD
    }
    __syncthreads();
    uint32_t first = incl - room;
    for (uint32_t w = 0; w < wave; ++w) first += wsum[w];
    start[tid] = first;
    sdesc[tid] = ds;
    sd3[tid] = d3;
    sstrip[tid] = static_cast<uint16_t>(s);
    if (tid == kGatherfTile - 1) start[kGatherfTile] = first + room;
    if (j < m) out_desc[j] = (base + first) << 20 | ((ds & 0xFFFFu) - s);  // byte offset << 16 | len - s
    __syncthreads();

    // B: one output chunk per thread and round, kDecapRounds rounds in flight together; a wave stays whole
    // through its last round (the lane exchange)
    const uint32_t total = start[kGatherfTile];
    const u32x4 *src = reinterpret_cast<const u32x4 *>(frames);
    for (uint32_t c0 = wave * 64u; c0 < total; c0 += kDecapRounds * kRouteBlock) {
        uint32_t f[kDecapRounds], q[kDecapRounds], st[kDecapRounds], r[kDecapRounds];
        int rem[kDecapRounds];
        bool own[kDecapRounds];
        u32x4 v[kDecapRounds], u[kDecapRounds];
        // where each chunk lies and what it loads
#pragma unroll
        for (uint32_t k = 0; k < kDecapRounds; ++k) {
            const uint32_t c = c0 + k * kRouteBlock + lane;
            const bool live = c < total;
            uint32_t g = 0;  // the last frame that starts at or before c: start[g] <= c < start[g + 1]
#pragma unroll
            for (uint32_t h = kGatherfTile / 2; h; h >>= 1) g += start[g + h] <= c ? h : 0u;
            const uint64_t fd = sdesc[g];
            const uint32_t len = static_cast<uint32_t>(fd) & 0xFFFFu;
            f[k] = g, st[k] = sstrip[g], q[k] = c - start[g];
            rem[k] = static_cast<int>(len - st[k]) - static_cast<int>(16u * q[k]);  // output bytes from this chunk on
            const bool data = live && rem[k] > 0;
            r[k] = q[k] ? (st[k] >> 2) & 3u : 0u;
            const uint32_t a = q[k] ? q[k] + (st[k] >> 4) : 0u;  // 16 a <= 16 q + s < len: chunk a starts in the frame
            const u32x4 *p = src + (fd >> 20) + a;
            v[k] = __builtin_nontemporal_load(data ? p : &g_zero16);
            // chunk a + 1 is the right neighbour's if that is this frame's next data chunk; else it is loaded here,
            // if it starts inside the frame, before anything waits for chunk a
            const uint32_t fid = live ? g : 0xFFFFFFFFu;
            const bool apart = from_next_lane(0xFFFFFFFEu, fid) != fid || rem[k] <= 16;  // (every lane takes part)
            own[k] = data && r[k] != 0u && 16u * (a + 1u) < len && apart;
            // (wave-uniform branch, branch-free inside: both loads are in flight together)
            u[k] = u32x4{0u, 0u, 0u, 0u};
            if (ballot(own[k]) != 0) u[k] = __builtin_nontemporal_load(own[k] ? p + 1 : &g_zero16);
        }
#pragma unroll
        for (uint32_t k = 0; k < kDecapRounds; ++k) {
            const uint32_t c = c0 + k * kRouteBlock + lane;
            const uint32_t nx = from_next_lane(0u, v[k].x), ny = from_next_lane(0u, v[k].y),
                           nz = from_next_lane(0u, v[k].z);
            const uint32_t hx = own[k] ? u[k].x : nx, hy = own[k] ? u[k].y : ny, hz = own[k] ? u[k].z : nz;
            // dwords r .. r + 3 of (chunk a, chunk a + 1): rotate by bit 0 of r, then by bit 1
            const bool b0 = (r[k] & 1u) != 0u, b1 = (r[k] & 2u) != 0u;
            const uint32_t t0 = b0 ? v[k].y : v[k].x, t1 = b0 ? v[k].z : v[k].y, t2 = b0 ? v[k].w : v[k].z,
                           t3 = b0 ? hx : v[k].w, t4 = b0 ? hy : hx, t5 = b0 ? hz : hy;
            uint32_t d[4] = {b1 ? t2 : t0, b1 ? t3 : t1, b1 ? t4 : t2, b1 ? t5 : t3};
            if (q[k] == 0u && st[k] != 0u) d[3] = sd3[f[k]];
            if (rem[k] < 16) clip_dwords<4>(d, static_cast<uint32_t>(max(rem[k], 0)));
            if (c < total && base + c < cap_chunks) out[base + c] = u32x4{d[0], d[1], d[2], d[3]};
        }
    }
}

}  // namespace dev
}  // namespace nffacl

using namespace nffacl;

extern "C" int nffacl_route_gather_decap_frames_device(nffacl_router *r, const uint8_t *d_frames,
                                                       const uint64_t *d_desc, uint64_t n,
                                                       const uint16_t *d_inner_off, const nffacl_key *d_keys,
                                                       const uint32_t *d_index, uint64_t m, uint32_t align,
                                                       uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_desc,
                                                       uint64_t *d_out_bytes, void *stream) {
    if (!r || !d_out_bytes || m > r->max_n || align < 16 || align > 4096 || (align & (align - 1)) != 0 ||
        (out_cap % 16) != 0 || !d_inner_off || (reinterpret_cast<uintptr_t>(d_inner_off) % 2) != 0 || !d_keys ||
        (reinterpret_cast<uintptr_t>(d_keys) % 16) != 0)
        return NFFACL_ERR_INVALID_ARG;
    if (m && (!d_index || !d_out_desc || !d_out || (reinterpret_cast<uintptr_t>(d_out) % 16) != 0 ||
              (n && (!d_desc || !d_frames || (reinterpret_cast<uintptr_t>(d_frames) % 16) != 0))))
        return NFFACL_ERR_INVALID_ARG;
    HIP_TRY(hipSetDevice(r->device));
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const uint32_t tiles = static_cast<uint32_t>((m + kGatherfTile - 1) / kGatherfTile);  // <= 2^21
    const uint32_t amask = align - 1;
    if (tiles)
        hipLaunchKernelGGL(dev::k_gatherd_sums, dim3(tiles), dim3(kRouteBlock), 0, s, d_desc, n, d_inner_off, d_index, m,
                           amask, r->d_fsums);
    hipLaunchKernelGGL(dev::k_gatherf_scan, dim3(1), dim3(kRouteBlock), 0, s, r->d_fsums, tiles, d_out_bytes);
    if (tiles)
        hipLaunchKernelGGL(dev::k_gatherd_copy, dim3(tiles), dim3(kRouteBlock), 0, s, d_frames, d_desc, n, d_inner_off,
                           reinterpret_cast<const uint32_t *>(d_keys), d_index, m, amask, r->d_fsums,
                           reinterpret_cast<dev::u32x4 *>(d_out), out_cap / 16, d_out_desc);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(r->last, s));
    r->used = true;
    return NFFACL_OK;
}
