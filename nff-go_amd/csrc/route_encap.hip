// route_encap.hip — the packed-frame gather of route_frames.hip that rewrites
// for the next hop on the way: output frame j is frame d_index[j] with the
// adjacency record d_adj[d_hop[i]] applied — next-hop MACs, an EtherType, a
// shim of up to 48 bytes pushed behind the Ethernet header (AddVLANTag
// vlan.go:119-131, AddMPLS mpls.go:81-91, EncapsulateIPv4GTP gtp.go:117-130 =
// EncapsulateHead packet.go:758-771), the shim's length fields and outer IPv4
// header checksum filled, the inner TTL / hop limit decremented and the inner
// header checksum patched (examples/decrementTTL.go:27-40).  Semantics: nffacl.h.
//
// Counting, packing and the three launches are those of route_frames.hip (its
// k_gatherf_scan is launched as it is); a frame's room comes from its output
// length L' = L + s, s the record's shim length where the record applies.
//   k_gathere_sums   k_gatherf_sums plus a 4-byte gather of the hop and one of
//                    the record's dword 3 (EtherType, shim_len, flags)
//   k_gathere_copy   output-stationary as k_gatherf_copy: thread t of round k
//                    owns output chunk 1024 k + t of the tile
// Payload.  Output dword D >= 3 + s/4 of a frame is source dword D - s/4, so
// output chunk q is the upper r = (s >> 2) & 3 dwords of aligned source chunk
// a - 1 and the lower 4 - r of chunk a, a = q - (s >> 4).  Consecutive lanes
// own consecutive output chunks, so the lane to the LEFT has loaded exactly
// chunk a - 1: every lane issues ONE aligned nontemporal 16-byte load, takes
// y, z, w of its left neighbour's registers (DPP wave_shr:1) and rotates the
// seven dwords by r with selects.  Inside a wave the left neighbour of a
// frame's chunk q >= 1 is always that frame's chunk q - 1 (header lanes load
// their source chunk like any other), so only lane 0 has to load chunk a - 1
// itself, in a branch a ballot skips, issued before anything waits.  Chunk
// a - 1 starts inside the frame whenever the lane holds output bytes; chunk a
// is loaded only if it does.
// Header.  The chunks below ceil((14 + s + 12) / 16) of a frame whose record
// applies are composed in registers: output byte b in [14, 14 + s) is record
// byte b + 2, so output dword D is alignbyte(rec[D + 1], rec[D], 2) — a lane
// loads the record's chunk q (16 bytes, through the caches) and dword 4q + 4.
// Dword 3 takes the EtherType below, dword 3 + s/4 the source's bytes 14-15
// above (and its bytes 12-13 below under INNER_ETYPE, which makes it source
// dword 3 whole).  The length fields are ALU from L and s; the outer header
// checksum and the inner dwords 5 and 6 with TTL and checksum patched are
// settled once per frame in phase A and kept in LDS.  No lane walks a header.
// Registers / LDS and the measured figures: DESIGN.md §4.15.
#include <hip/hip_runtime.h>

#include "classify.hpp"
#include "devutil.hpp"
#include "nffacl.h"
#include "route.hpp"

// 1: one load per lane and the lane exchange; 0: every lane loads both chunks (the correctness baseline)
#ifndef NFFACL_ENCAP_EXCHANGE
#define NFFACL_ENCAP_EXCHANGE 1
#endif
// rounds of the copy whose searches and loads are in flight together
#ifndef NFFACL_ENCAP_ROUNDS
#define NFFACL_ENCAP_ROUNDS 2
#endif

namespace nffacl {
namespace dev {

constexpr uint32_t kWaves = kRouteBlock / 64;
constexpr uint32_t kEncapRounds = NFFACL_ENCAP_ROUNDS;
constexpr uint32_t kAdjKnown = NFFACL_ADJ_MACS | NFFACL_ADJ_TTL | NFFACL_ADJ_INNER_ETYPE | NFFACL_ADJ_IP4_LEN |
                               NFFACL_ADJ_UDP_LEN | NFFACL_ADJ_GTP_LEN;
// A frame's word in LDS: s (6 bits) | flags << 6 | applied | the record names an EtherType | inner dwords 5, 6
// patched | the outer header checksum (as its two bytes lie in memory) << 16
constexpr uint32_t kMetaApplied = 1u << 12, kMetaEtype = 1u << 13, kMetaPatched = 1u << 14;

__device__ __forceinline__ uint32_t bswap16(uint32_t x) { return ((x & 0xFFu) << 8) | ((x >> 8) & 0xFFu); }
// reduceChecksum (checksum.go:179-184) of a sum of at most 2^16 words
__device__ __forceinline__ uint32_t fold16(uint32_t x) {
    x = (x >> 16) + (x & 0xFFFFu);
    return (x >> 16) + (x & 0xFFFFu);
}

// frame_at with the rewrite: `w` = dword 3 of the frame's record (ether_type | shim_len << 16 | flags << 24) where
// the record applies, else 0 with applied = false; `room` is that of the output length len + s.  Decided from the
// descriptor, the hop and the record alone.  `i`, `h`: source frame and record (meaningful where applied).
__device__ __forceinline__ uint64_t encap_at(const uint64_t *__restrict__ desc, uint64_t n,
                                             const uint32_t *__restrict__ hop, const uint32_t *__restrict__ adj,
                                             uint32_t n_adj, const uint32_t *__restrict__ index, uint64_t j,
                                             uint64_t m, uint32_t amask, uint32_t &h, uint32_t &w, bool &applied,
                                             uint32_t &room) {
    uint64_t ds = 0;
    w = 0, h = 0;
    bool rec = false;
    if (j < m) {
        const uint32_t i = index[j];
        if (i < n) {
            ds = desc[i];
            h = hop[i] & 0xFFFFFFu;
            rec = h < n_adj;
            if (rec) w = adj[16 * uint64_t(h) + 3];
        }
    }
    const uint32_t len = static_cast<uint32_t>(ds) & 0xFFFFu, s = (w >> 16) & 0xFFu, fl = w >> 24;
    applied = rec && len >= 14u && (s & 3u) == 0u && s <= 48u && (fl & ~kAdjKnown) == 0u && len + s <= 65535u &&
              (!(fl & NFFACL_ADJ_INNER_ETYPE) || s >= 4u) && (!(fl & NFFACL_ADJ_IP4_LEN) || s >= 20u) &&
              (!(fl & NFFACL_ADJ_UDP_LEN) || ((fl & NFFACL_ADJ_IP4_LEN) && s >= 28u)) &&
              (!(fl & NFFACL_ADJ_GTP_LEN) || ((fl & NFFACL_ADJ_UDP_LEN) && s >= 36u));
    if (!applied) w = 0;
    room = ((len + ((w >> 16) & 0xFFu) + amask) & ~amask) >> 4;  // <= 4096
    return ds;
}

__global__ __launch_bounds__(kRouteBlock) void k_gathere_sums(const uint64_t *__restrict__ desc, uint64_t n,
                                                              const uint32_t *__restrict__ hop,
                                                              const uint32_t *__restrict__ adj, uint32_t n_adj,
                                                              const uint32_t *__restrict__ index, uint64_t m,
                                                              uint32_t amask, uint64_t *__restrict__ sums) {
    __shared__ uint32_t wsum[kWaves];
    const uint32_t tid = threadIdx.x, lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    uint32_t h, w, room;
    bool applied;
    encap_at(desc, n, hop, adj, n_adj, index, uint64_t(blockIdx.x) * kGatherfTile + tid, m, amask, h, w, applied, room);
    const uint32_t incl = wave_scan_incl(room);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    if (wave == 0) {
        const uint32_t t = wave_scan_incl(lane < kWaves ? wsum[lane] : 0u);
        if (lane == 63) sums[blockIdx.x] = t;
    }
}

// Lane l <- lane l - 1's x (wave_shr:1); lane 0, which has no left neighbour, <- 0.
__device__ __forceinline__ uint32_t from_prev_lane(uint32_t x) {
    return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(x), 0x138, 0xf, 0xf, false));
}

__global__ __launch_bounds__(kRouteBlock) void k_gathere_copy(
    const uint8_t *__restrict__ frames, const uint64_t *__restrict__ desc, uint64_t n,
    const uint32_t *__restrict__ hop, const uint32_t *__restrict__ adj, uint32_t n_adj,
    const uint32_t *__restrict__ index, uint64_t m, uint32_t amask, const uint64_t *__restrict__ starts,
    u32x4 *__restrict__ out, uint64_t cap_chunks, uint64_t *__restrict__ out_desc, uint8_t *__restrict__ status) {
    __shared__ uint32_t start[kGatherfTile + 1];  // a frame's first output chunk inside the tile; [T] = the tile's chunks
    __shared__ uint64_t sdesc[kGatherfTile];      // its source descriptor
    __shared__ uint32_t smeta[kGatherfTile];      // s, flags, kMeta*, outer header checksum
    __shared__ uint32_t shop[kGatherfTile];       // its record
    __shared__ uint32_t sp5[kGatherfTile], sp6[kGatherfTile];  // source dwords 5, 6 as they leave (kMetaPatched)
    __shared__ uint32_t wsum[kWaves];
    const uint32_t tid = threadIdx.x, lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint64_t j = uint64_t(blockIdx.x) * kGatherfTile + tid;
    const uint64_t base = starts[blockIdx.x];  // the tile's first output chunk

    // A: which records apply, exclusive scan of the tile's rooms, every rewritten frame's patch words
    uint32_t h, w, room;
    bool applied;
    const uint64_t ds = encap_at(desc, n, hop, adj, n_adj, index, j, m, amask, h, w, applied, room);
    const uint32_t incl = wave_scan_incl(room);
    if (lane == 63) wsum[wave] = incl;
    const uint32_t len = static_cast<uint32_t>(ds) & 0xFFFFu, s = (w >> 16) & 0xFFu, fl = w >> 24;
    uint32_t meta = 0, p5 = 0, p6 = 0, st = 0;
    if (applied) {
        st = NFFACL_RW_APPLIED;
        meta = s | fl << 6 | kMetaApplied | ((w & 0xFFFFu) ? kMetaEtype : 0u);
        const uint32_t *sp = reinterpret_cast<const uint32_t *>(frames + (ds >> 16));
        const bool tail20 = (fl & NFFACL_ADJ_IP4_LEN) && (fl & NFFACL_ADJ_INNER_ETYPE) && s == 20u;
        uint32_t d3 = 0;  // source bytes 12-15 (len >= 14: chunk 0 starts inside the frame)
        if ((fl & NFFACL_ADJ_TTL) || tail20) d3 = sp[3];
        if (fl & NFFACL_ADJ_TTL) {
            const uint32_t et = bswap16(d3), vb = (d3 >> 16) & 0xFFu;
            const bool v4 = et == 0x0800u && (vb >> 4) == 4u && (vb & 15u) >= 5u && len >= 34u;
            const bool v6 = et == 0x86DDu && (vb >> 4) == 6u && len >= 54u;
            if (v4 || v6) {
                p5 = sp[5], p6 = sp[6];  // bytes 20-27: IPv4 TTL 22, protocol 23, checksum 24-25; IPv6 hop limit 21
                const uint32_t ttl = v4 ? (p5 >> 16) & 0xFFu : (p5 >> 8) & 0xFFu;
                st |= ttl >= 2u ? NFFACL_RW_TTL_DONE : NFFACL_RW_TTL_EXPIRED;
                if (ttl >= 2u) {
                    meta |= kMetaPatched;
                    if (v4) {
                        // RFC 1624 eq. 3 on the words as they lie in memory (the one's complement sum commutes
                        // with the byte swap): m = (TTL, protocol), m' = m with TTL - 1
                        const uint32_t mw = p5 >> 16, hc = p6 & 0xFFFFu;
                        const uint32_t sum = fold16((~hc & 0xFFFFu) + (~mw & 0xFFFFu) + (mw - 1u));
                        p5 -= 0x10000u;
                        p6 = (p6 & 0xFFFF0000u) | (~sum & 0xFFFFu);
                    } else {
                        p5 -= 0x100u;
                    }
                }
            }
        }
        if (fl & NFFACL_ADJ_IP4_LEN) {
            // the outer header as it leaves: shim [0, 20) = record dwords 4..8, TotalLength in, checksum field 0,
            // and with s = 20 under INNER_ETYPE its last two bytes the source's bytes 12-13
            const uint32_t *rp = adj + 16 * uint64_t(h);
            const u32x4 a = *reinterpret_cast<const u32x4 *>(rp + 4);
            uint32_t e = rp[8];
            if (tail20) e = (e & 0xFFFFu) | d3 << 16;
            const uint32_t x = (a.x & 0xFFFFu) | bswap16(len + s - 14u) << 16, z = a.z & 0xFFFFu;
            const uint32_t sum = (x & 0xFFFFu) + (x >> 16) + (a.y & 0xFFFFu) + (a.y >> 16) + z + (a.w & 0xFFFFu) +
                                 (a.w >> 16) + (e & 0xFFFFu) + (e >> 16);
            meta |= (~fold16(sum) & 0xFFFFu) << 16;
        }
    }
    __syncthreads();
    uint32_t first = incl - room;
    for (uint32_t k = 0; k < wave; ++k) first += wsum[k];
    start[tid] = first;
    sdesc[tid] = ds;
    smeta[tid] = meta;
    shop[tid] = h;
    sp5[tid] = p5;
    sp6[tid] = p6;
    if (tid == kGatherfTile - 1) start[kGatherfTile] = first + room;
    if (j < m) {
        out_desc[j] = (base + first) << 20 | (len + s);  // byte offset << 16 | len + s
        if (status) status[j] = static_cast<uint8_t>(st);
    }
    __syncthreads();

    // B: one output chunk per thread and round, kEncapRounds rounds in flight together; a wave stays whole through
    // its last round (the lane exchange)
    const uint32_t total = start[kGatherfTile];
    const u32x4 *src = reinterpret_cast<const u32x4 *>(frames);
    for (uint32_t c0 = wave * 64u; c0 < total; c0 += kEncapRounds * kRouteBlock) {
        uint32_t f[kEncapRounds], q[kEncapRounds], me[kEncapRounds], ln[kEncapRounds], r5[kEncapRounds];
        int rem[kEncapRounds];
        bool own[kEncapRounds], hdr[kEncapRounds];
        u32x4 v[kEncapRounds], u[kEncapRounds], rv[kEncapRounds];
        // where each chunk lies and what it loads
#pragma unroll
        for (uint32_t k = 0; k < kEncapRounds; ++k) {
            const uint32_t c = c0 + k * kRouteBlock + lane;
            const bool live = c < total;
            uint32_t g = 0;  // the last frame that starts at or before c: start[g] <= c < start[g + 1]
#pragma unroll
            for (uint32_t t = kGatherfTile / 2; t; t >>= 1) g += start[g + t] <= c ? t : 0u;
            const uint64_t fd = sdesc[g];
            f[k] = g, me[k] = smeta[g], q[k] = c - start[g], ln[k] = static_cast<uint32_t>(fd) & 0xFFFFu;
            const uint32_t sh = me[k] & 63u;
            rem[k] = static_cast<int>(ln[k] + sh) - static_cast<int>(16u * q[k]);  // output bytes from this chunk on
            const bool data = live && rem[k] > 0;
            hdr[k] = data && (me[k] & kMetaApplied) != 0u && q[k] < ((sh + 41u) >> 4);
            // chunk 0 of the output is chunk 0 of the source in place; where s >= 16 it is lane s >> 4 that holds
            // source chunk 0 for the exchange, and lane 0 reads it only for what the record does not supply
            const int a = q[k] ? static_cast<int>(q[k]) - static_cast<int>(sh >> 4) : 0;
            const bool rec0 = (me[k] & (NFFACL_ADJ_MACS << 6)) != 0u && (me[k] & kMetaEtype) != 0u;
            const bool ld = data && a >= 0 && 16 * a < static_cast<int>(ln[k]) && (q[k] != 0u || sh < 16u || !rec0);
            const u32x4 *p = src + (fd >> 20) + a;
            v[k] = __builtin_nontemporal_load(ld ? p : &g_zero16);
            // chunk a - 1: the left neighbour's; lane 0 has none and loads it here, before anything waits for
            // chunk a (wave-uniform branch, branch-free inside)
            const bool prev = data && q[k] != 0u && (sh & 12u) != 0u && a >= 1;
            own[k] = prev && (NFFACL_ENCAP_EXCHANGE ? lane == 0u : true);
            u[k] = u32x4{0u, 0u, 0u, 0u};
            if (ballot(own[k]) != 0) u[k] = __builtin_nontemporal_load(own[k] ? p - 1 : &g_zero16);
            // the record's chunk q and the dword behind it, where they lie (through the caches)
            const uint32_t *rp = adj + 16 * uint64_t(shop[g]) + 4u * q[k];
            rv[k] = u32x4{0u, 0u, 0u, 0u}, r5[k] = 0u;
            if (ballot(hdr[k]) != 0) {
                const bool rq = hdr[k] && q[k] <= 3u;
                rv[k] = *(rq ? reinterpret_cast<const u32x4 *>(rp) : &g_zero16);
                r5[k] = *(rq && q[k] <= 2u ? rp + 4 : reinterpret_cast<const uint32_t *>(&g_zero16));
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < kEncapRounds; ++k) {
            const uint32_t c = c0 + k * kRouteBlock + lane;
            const uint32_t sh = me[k] & 63u, r = q[k] ? (sh >> 2) & 3u : 0u;
            const uint32_t ny = from_prev_lane(v[k].y), nz = from_prev_lane(v[k].z), nw = from_prev_lane(v[k].w);
            const uint32_t py = own[k] ? u[k].y : ny, pz = own[k] ? u[k].z : nz, pw = own[k] ? u[k].w : nw;
            // dwords 3 - r .. 6 - r of (py, pz, pw, chunk a): by bit 1 of r, then by bit 0
            const bool b0 = (r & 1u) != 0u, b1 = (r & 2u) != 0u;
            const uint32_t t0 = b1 ? py : pw, t1 = b1 ? pz : v[k].x, t2 = b1 ? pw : v[k].y, t3 = b1 ? v[k].x : v[k].z,
                           t4 = b1 ? v[k].y : v[k].w;
            uint32_t d[4] = {b0 ? t0 : t1, b0 ? t1 : t2, b0 ? t2 : t3, b0 ? t3 : t4};
            if (ballot(hdr[k]) != 0 && hdr[k]) {
                const uint32_t g[4] = {__builtin_amdgcn_alignbyte(rv[k].y, rv[k].x, 2),
                                       __builtin_amdgcn_alignbyte(rv[k].z, rv[k].y, 2),
                                       __builtin_amdgcn_alignbyte(rv[k].w, rv[k].z, 2),
                                       __builtin_amdgcn_alignbyte(r5[k], rv[k].w, 2)};
                const uint32_t fl2 = me[k] >> 6, mixed = 3u + (sh >> 2), lo = 0xFFFFu, hi = 0xFFFF0000u;
                if (q[k] == 0u) {
                    if (fl2 & NFFACL_ADJ_MACS) d[0] = rv[k].x, d[1] = rv[k].y, d[2] = rv[k].z;
                    if (sh) d[3] = ((me[k] & kMetaEtype) ? bswap16(rv[k].w) : d[3] & lo) | (g[3] & hi);
                } else {
                    const uint32_t l2 = ln[k] + sh;
#pragma unroll
                    for (uint32_t e = 0; e < 4; ++e) {
                        const uint32_t D = 4u * q[k] + e;
                        const uint32_t mix = (fl2 & NFFACL_ADJ_INNER_ETYPE) ? d[e] : (g[e] & lo) | (d[e] & hi);
                        d[e] = D < mixed ? g[e] : D == mixed ? mix : d[e];
                        if (me[k] & kMetaPatched) d[e] = D == mixed + 2u ? sp5[f[k]] : D == mixed + 3u ? sp6[f[k]] : d[e];
                    }
                    // TotalLength, HdrChecksum (output bytes 16-17, 24-25), DgramLen (38-39), MessageLength (44-45)
                    if ((fl2 & NFFACL_ADJ_IP4_LEN) && q[k] == 1u)
                        d[0] = (d[0] & hi) | bswap16(l2 - 14u), d[2] = (d[2] & hi) | me[k] >> 16;
                    if ((fl2 & NFFACL_ADJ_UDP_LEN) && q[k] == 2u) d[1] = (d[1] & lo) | bswap16(l2 - 34u) << 16;
                    if ((fl2 & NFFACL_ADJ_GTP_LEN) && q[k] == 2u) d[3] = (d[3] & hi) | bswap16(ln[k] - 14u);
                }
            }
            if (rem[k] < 16) clip_dwords<4>(d, static_cast<uint32_t>(max(rem[k], 0)));
            if (c < total && base + c < cap_chunks) out[base + c] = u32x4{d[0], d[1], d[2], d[3]};
        }
    }
}

}  // namespace dev
}  // namespace nffacl

using namespace nffacl;

extern "C" int nffacl_route_gather_encap_frames_device(nffacl_router *r, const uint8_t *d_frames,
                                                       const uint64_t *d_desc, uint64_t n, const uint32_t *d_hop,
                                                       const nffacl_adj *d_adj, uint32_t n_adj,
                                                       const uint32_t *d_index, uint64_t m, uint32_t align,
                                                       uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_desc,
                                                       uint64_t *d_out_bytes, uint8_t *d_status, void *stream) {
    if (!r || !d_out_bytes || m > r->max_n || align < 16 || align > 4096 || (align & (align - 1)) != 0 ||
        (out_cap % 16) != 0 || n_adj > (1u << 24) || (n_adj && !d_adj) ||
        (reinterpret_cast<uintptr_t>(d_adj) % 16) != 0 || (n && !d_hop) || (reinterpret_cast<uintptr_t>(d_hop) % 4) != 0)
        return NFFACL_ERR_INVALID_ARG;
    if (m && (!d_index || !d_out_desc || !d_out || (reinterpret_cast<uintptr_t>(d_out) % 16) != 0 ||
              (n && (!d_desc || !d_frames || (reinterpret_cast<uintptr_t>(d_frames) % 16) != 0))))
        return NFFACL_ERR_INVALID_ARG;
    HIP_TRY(hipSetDevice(r->device));
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const uint32_t tiles = static_cast<uint32_t>((m + kGatherfTile - 1) / kGatherfTile);  // <= 2^21
    const uint32_t amask = align - 1;
    const uint32_t *adj = reinterpret_cast<const uint32_t *>(d_adj);
    if (tiles)
        hipLaunchKernelGGL(dev::k_gathere_sums, dim3(tiles), dim3(kRouteBlock), 0, s, d_desc, n, d_hop, adj, n_adj,
                           d_index, m, amask, r->d_fsums);
    hipLaunchKernelGGL(dev::k_gatherf_scan, dim3(1), dim3(kRouteBlock), 0, s, r->d_fsums, tiles, d_out_bytes);
    if (tiles)
        hipLaunchKernelGGL(dev::k_gathere_copy, dim3(tiles), dim3(kRouteBlock), 0, s, d_frames, d_desc, n, d_hop, adj,
                           n_adj, d_index, m, amask, r->d_fsums, reinterpret_cast<dev::u32x4 *>(d_out), out_cap / 16,
                           d_out_desc, d_status);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(r->last, s));
    r->used = true;
    return NFFACL_OK;
}
