// cksum.hip — checksums of packed frames (nffacl.h,
// nffacl_checksum_frames_device): HIP kernel (gfx950) and launcher.
//
// Hot path replaced: what the reference's users get from the NIC's RX offload,
// or from packet/checksum.go on the CPU (CalculateIPv4Checksum,
// CalculateIPv{4,6}{TCP,UDP,ICMP}Checksum), for a batch that stays in HBM: the
// IPv4 header sum and the L4 sum of every frame, compared with what the frame
// carries.  Semantics: nffacl.h.
//
// This kernel reduces every byte of every L4 span — 8 to 1 500 bytes that
// start and end anywhere — where every other frame kernel reads one to three
// lines per frame.  One kCkBlock-thread workgroup takes a tile of kCkTile
// consecutive frames, grid-striding over the tiles:
//   A  one thread per frame: descriptor and cursor lane-contiguous; the lane
//      reads the header words it needs (dword loads inside the frame's first
//      chunks), settles family, header length, the L4 span [b, e), the status
//      bits known so far, the IPv4 header sum, the pseudo-header sum (each
//      sum's loads issued together) and the stored L4 field.  LDS gets the span, the span's first source chunk, a
//      zeroed u32 accumulator per frame and the exclusive scan start[] of the
//      spans' 16-byte chunk counts ((e + 15) / 16 - b / 16, 0 where no L4 sum
//      is due).
//   B  chunk-stationary: thread t of round k owns span chunk 1024 k + t of the
//      tile, finds its frame by binary search over start[] (as the gathers do),
//      issues ONE aligned nontemporal 16-byte load, zeroes the bytes outside
//      [b, e) and sums its eight big-endian words as the even bytes and the odd
//      bytes of the four dwords separately (b is even: a frame's even bytes are
//      the words' high bytes; no per-word swap).  A frame's chunks are
//      consecutive lanes, so a wave holds a few segments: one unsegmented DPP
//      scan S of the 64 values, the segments' last lanes found by one DPP
//      compare of the frame numbers, and each of those lanes takes S of the
//      lane before its segment's head (ds_bpermute; the head from the ballot of
//      the tails) and does one ds_add_u32 of the difference into its frame's
//      accumulator, which is what joins the waves a 1 518-byte frame crosses.
//      kCkRounds rounds are located and loaded before either is reduced.
//   C  one thread per frame: total = accumulator - stored field + pseudo-header
//      (plain integer sums: the field need not be zeroed on the way), fold,
//      the UDP rules, the compare; one 8-byte record per lane and one ballot
//      per wave for d_bad_bits.
// A u32 cannot overflow: 32 768 words x 0xFFFF < 2^31.  With what ==
// NFFACL_CK_IP4 the instantiation without phase B, LDS or barriers runs.
// No global atomics, no scratch, nothing allocated.
// Registers / LDS and the measured figures: DESIGN.md §4.13.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "classify.hpp"
#include "cksum.hpp"
#include "devutil.hpp"
#include "nffacl.h"
#include "route.hpp"

namespace nffacl {
namespace dev {

constexpr uint32_t kCkWaves = kCkBlock / 64;
constexpr uint32_t kCkRounds = 2;  // rounds of phase B whose searches and loads are in flight together

// What phase A settles for one frame.
struct CkFrame {
    uint32_t status = 0, ip = 0;
    uint32_t b = 0, e = 0;   // the L4 span, where `due`
    uint32_t stored = 0;     // the L4 checksum field as the frame carries it
    uint32_t pseudo = 0;     // pseudo-header sum
    bool due = false, udp = false, v6 = false;
};

// One frame's bytes through aligned dword loads (every offset asked for lies inside the frame).
struct CkReader {
    const uint32_t *p;
    __device__ __forceinline__ uint32_t dword(uint32_t k, bool want) const { return want ? p[k] : 0u; }
    __device__ __forceinline__ uint32_t byte(uint32_t off, bool want) const {
        return (dword(off >> 2, want) >> (8u * (off & 3u))) & 0xFFu;
    }
    // the big-endian word at an even offset
    __device__ __forceinline__ uint32_t be16(uint32_t off, bool want) const {
        const uint32_t w = dword(off >> 2, want), h = (off & 2u) ? w >> 16 : w;
        return (h & 0xFFu) << 8 | ((h >> 8) & 0xFFu);
    }
    // sum of the big-endian words of [lo, hi), both even, at most kMax dwords; 0 unless `want`.  The first
    // kEager dwords' loads are issued together; the rest only if a lane of the wave has more.
    template <int kEager, int kMax>
    __device__ __forceinline__ uint32_t sum(uint32_t lo, uint32_t hi, bool want) const {
        const uint32_t j0 = lo >> 2, cnt = want ? ((hi + 3u) >> 2) - j0 : 0u;
        uint32_t ev = 0, od = 0;  // two 16-bit lanes each: the dwords' bytes 0 | 2 and 1 | 3
        uint32_t w[kMax];
        auto add = [&](uint32_t k) {
            const uint32_t o = 4u * (j0 + k);
            const uint32_t x = w[k] & (((o >= lo && o + 2u <= hi) ? 0x0000FFFFu : 0u) |
                                       ((o + 2u >= lo && o + 4u <= hi) ? 0xFFFF0000u : 0u));
            ev += x & 0x00FF00FFu;
            od += (x >> 8) & 0x00FF00FFu;
        };
#pragma unroll
        for (uint32_t k = 0; k < static_cast<uint32_t>(kEager); ++k) w[k] = dword(j0 + k, k < cnt);
#pragma unroll
        for (uint32_t k = 0; k < static_cast<uint32_t>(kEager); ++k) add(k);
        if (kMax > kEager && ballot(cnt > static_cast<uint32_t>(kEager))) {
#pragma unroll
            for (uint32_t k = kEager; k < static_cast<uint32_t>(kMax); ++k) w[k] = dword(j0 + k, k < cnt);
#pragma unroll
            for (uint32_t k = kEager; k < static_cast<uint32_t>(kMax); ++k) add(k);
        }
        return ((ev & 0xFFFFu) + (ev >> 16)) * 256u + (od & 0xFFFFu) + (od >> 16);
    }
};

// reduceChecksum (checksum.go:179-184): two steps settle any u32.
__device__ __forceinline__ uint32_t ck_fold(uint32_t s) {
    s = (s >> 16) + (s & 0xFFFFu);
    return (s >> 16) + (s & 0xFFFFu);
}
// A stored field against the computed one, 0x0000 and 0xFFFF being the same number.
__device__ __forceinline__ bool ck_differ(uint32_t a, uint32_t b) { return (a ? a : 0xFFFFu) != (b ? b : 0xFFFFu); }

// Phase A for one frame (ds = 0 for a lane past the batch: the zero record).
template <bool L4>
__device__ __forceinline__ CkFrame ck_settle(const uint8_t *__restrict__ frames, uint64_t ds, uint32_t c,
                                             uint32_t what) {
    CkFrame f;
    const uint32_t len = static_cast<uint32_t>(ds) & 0xFFFFu;
    const CkReader rd{reinterpret_cast<const uint32_t *>(frames + (ds >> 16))};
    const bool ok = (c & 1u) == 0u && c >= 14u && c < len;  // (0xFFFF is odd)
    const uint32_t v0 = rd.byte(c, ok), nib = v0 >> 4;
    uint32_t fam = nib == 4u || nib == 6u ? nib : 0u;
    if (c == 14u) {
        const uint32_t et = rd.be16(12u, ok);
        fam = (et == 0x0800u && nib == 4u) ? 4u : (et == 0x86DDu && nib == 6u) ? 6u : 0u;
    }
    if (!ok) fam = 0u;
    const bool is4 = fam == 4u, is6 = fam == 6u;
    const uint32_t hlen = is4 ? 4u * (v0 & 15u) : 40u;
    const bool hdr = (is4 && hlen >= 20u && c + hlen <= len) || (is6 && L4 && c + 40u <= len);
    if ((is4 || (is6 && L4)) && !hdr) f.status = NFFACL_CK_LENGTH;
    const bool ip4 = is4 && hdr && (what & NFFACL_CK_IP4) != 0u;
    const uint32_t hstored = rd.be16(c + 10u, ip4);
    const uint32_t hsum = rd.sum<6, 16>(c, c + hlen, ip4);  // the field's own word comes off again: no masking
    if (ip4) {
        f.ip = ~ck_fold(hsum - hstored) & 0xFFFFu;
        f.status |= NFFACL_CK_IP4_DONE | (ck_differ(f.ip, hstored) ? NFFACL_CK_IP4_BAD : 0u);
    }
    if (!L4) return f;
    // the span: TotalLength (IPv4), PayloadLen (IPv6) against the frame
    const uint32_t tl = rd.be16(c + (is4 ? 2u : 4u), hdr);
    const uint32_t end = is4 ? tl : 40u + tl;  // the packet's end from the cursor on
    const bool fits = hdr && end >= hlen && c + end <= len;
    if (hdr && !fits) f.status |= NFFACL_CK_LENGTH;
    const bool frag = is4 && fits && (rd.be16(c + 6u, is4 && fits) & 0x3FFFu) != 0u;
    if (frag) f.status |= NFFACL_CK_FRAGMENT;
    const uint32_t proto = rd.byte(c + (is4 ? 9u : 6u), fits);
    const bool tcp = proto == 6u, udp = proto == 17u, icmp = proto == (is4 ? 1u : 58u);
    const bool l4 = fits && !frag && (tcp || udp || icmp);
    const uint32_t b = c + hlen, e = c + end, m = e - b;
    bool sound = l4 && m >= (tcp ? 20u : 8u);
    sound = sound && (!udp || rd.be16(b + 4u, sound && udp) == m);  // DgramLen
    if (l4 && !sound) f.status |= NFFACL_CK_LENGTH;
    f.due = sound, f.udp = udp, f.v6 = is6;
    f.b = sound ? b : 0u, f.e = sound ? e : 0u;
    f.stored = rd.be16(b + (tcp ? 16u : udp ? 6u : 2u), sound);
    // source and destination words, the protocol and m; none for ICMP over IPv4
    const bool ph = sound && !(is4 && icmp);
    f.pseudo = rd.sum<9, 9>(c + (is4 ? 12u : 8u), c + (is4 ? 20u : 40u), ph) + (ph ? proto + m : 0u);
    return f;
}

// Lane l <- lane l + 1's x (wave_shl:1); lane 63 <- old.
__device__ __forceinline__ uint32_t ck_next_lane(uint32_t old, uint32_t x) {
    return static_cast<uint32_t>(
        __builtin_amdgcn_update_dpp(static_cast<int>(old), static_cast<int>(x), 0x130, 0xf, 0xf, false));
}

template <bool L4>
__global__ __launch_bounds__(kCkBlock) void k_cksum(const uint8_t *__restrict__ frames,
                                                    const uint64_t *__restrict__ desc, uint64_t n,
                                                    const uint16_t *__restrict__ inner_off, uint32_t what,
                                                    uint64_t *__restrict__ sums, uint64_t *__restrict__ bad_bits,
                                                    uint32_t tiles) {
    __shared__ uint32_t start[L4 ? kCkTile + 1 : 1];  // a frame's first span chunk inside the tile; [T] = the tile's
    __shared__ uint64_t schunk[L4 ? kCkTile : 1];     // its span's first 16-byte chunk in d_frames
    __shared__ uint32_t sspan[L4 ? kCkTile : 1];      // b | e << 16
    __shared__ uint32_t acc[L4 ? kCkTile : 1];        // the sum of its span's words
    __shared__ uint32_t wsum[kCkWaves];
    const uint32_t tid = threadIdx.x, lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const u32x4 *src = reinterpret_cast<const u32x4 *>(frames);

    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        // A
        const uint64_t i = uint64_t(tile) * kCkTile + tid;
        const bool live = i < n;
        const uint64_t ds = live ? desc[i] : 0;
        const uint32_t c = !live ? 0u : inner_off ? inner_off[i] : 14u;
        const CkFrame f = ck_settle<L4>(frames, ds, c, what);
        uint32_t total_words = 0;
        if constexpr (L4) {
            const uint32_t room = f.due ? ((f.e + 15u) >> 4) - (f.b >> 4) : 0u;  // <= 95
            const uint32_t incl = wave_scan_incl(room);
            if (lane == 63) wsum[wave] = incl;
            schunk[tid] = (ds >> 20) + (f.b >> 4);
            sspan[tid] = f.b | f.e << 16;
            acc[tid] = 0u;
            __syncthreads();
            uint32_t first = incl - room;
            for (uint32_t w = 0; w < wave; ++w) first += wsum[w];
            start[tid] = first;
            if (tid == kCkTile - 1) start[kCkTile] = first + room;
            __syncthreads();

            // B: one span chunk per thread and round; a wave stays whole through its last round (the scan)
            const uint32_t total = start[kCkTile];
            for (uint32_t c0 = wave * 64u; c0 < total; c0 += kCkRounds * kCkBlock) {
                uint32_t g[kCkRounds], km[kCkRounds];
                u32x4 v[kCkRounds];
#pragma unroll
                for (uint32_t k = 0; k < kCkRounds; ++k) {
                    const uint32_t ch = c0 + k * kCkBlock + lane;
                    const bool in = ch < total;
                    uint32_t fr = 0;  // the last frame that starts at or before ch: start[fr] <= ch < start[fr + 1]
#pragma unroll
                    for (uint32_t h = kCkTile / 2; h; h >>= 1) fr += start[fr + h] <= ch ? h : 0u;
                    const uint32_t q = ch - start[fr], sp = sspan[fr];
                    // the chunk covers frame bytes [16 a, 16 a + 16), a = b / 16 + q; 16 a < e: it starts in the frame
                    const int lo = q ? 0 : static_cast<int>(sp & 15u);
                    const int left = static_cast<int>(sp >> 16) - static_cast<int>(((sp & 0xFFF0u) + 16u * q));
                    const int hi = in ? min(left, 16) : 0;
                    km[k] = ((1u << hi) - 1u) & ~((1u << lo) - 1u);  // the chunk's bytes inside [b, e)
                    g[k] = in ? fr : 0xFFFFFFFFu;
                    v[k] = __builtin_nontemporal_load(in ? src + schunk[fr] + q : &g_zero16);
                }
#pragma unroll
                for (uint32_t k = 0; k < kCkRounds; ++k) {
                    uint32_t ev = 0, od = 0;
#pragma unroll
                    for (uint32_t j = 0; j < 4; ++j) {
                        // bits 4 j .. 4 j + 3 of km -> the byte mask of dword j
                        const uint32_t keep = ((((km[k] >> (4u * j)) & 15u) * 0x00204081u) & 0x01010101u) * 0xFFu;
                        const uint32_t w = v[k][j] & keep;
                        ev += w & 0x00FF00FFu;
                        od += (w >> 8) & 0x00FF00FFu;
                    }
                    const uint32_t x = ((ev & 0xFFFFu) + (ev >> 16)) * 256u + (od & 0xFFFFu) + (od >> 16);
                    const uint32_t S = wave_scan_incl(x);  // <= 64 x 8 x 0xFFFF
                    const bool tail = lane == 63 || ck_next_lane(0u, g[k]) != g[k];
                    const uint64_t heads = ballot(tail) << 1 | 1u;  // a segment starts behind every tail
                    const uint32_t head = 63u - static_cast<uint32_t>(__builtin_clzll(heads & (~0ull >> (63u - lane))));
                    const uint32_t before = static_cast<uint32_t>(
                        __builtin_amdgcn_ds_bpermute(static_cast<int>((head - 1u) << 2), static_cast<int>(S)));
                    if (tail && g[k] != 0xFFFFFFFFu)
                        __hip_atomic_fetch_add(&acc[g[k]], S - (head ? before : 0u), __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
            __syncthreads();
            total_words = acc[tid];
        }

        // C
        uint32_t status = f.status, l4 = 0;
        if (L4 && f.due) {
            l4 = ~ck_fold(total_words - f.stored + f.pseudo) & 0xFFFFu;
            if (f.udp && l4 == 0u) l4 = 0xFFFFu;
            status |= NFFACL_CK_L4_DONE;
            if (f.udp && f.stored == 0u) status |= f.v6 ? NFFACL_CK_L4_BAD : NFFACL_CK_L4_ABSENT;
            else if (ck_differ(l4, f.stored)) status |= NFFACL_CK_L4_BAD;
        }
        if (sums && live) sums[i] = uint64_t(status) << 32 | l4 << 16 | f.ip;
        const uint64_t bad = ballot((status & (NFFACL_CK_IP4_BAD | NFFACL_CK_L4_BAD)) != 0u);
        if (bad_bits && lane == 0 && live) bad_bits[i >> 6] = bad;
    }
}

}  // namespace dev
}  // namespace nffacl

using namespace nffacl;

extern "C" int nffacl_checksum_frames_plan(uint64_t n, uint64_t *tiles) {
    if (!tiles || n >> 32) return NFFACL_ERR_INVALID_ARG;
    *tiles = std::max<uint64_t>((n + kCkTile - 1) / kCkTile, 1);
    return NFFACL_OK;
}

extern "C" int nffacl_checksum_frames_device(const uint8_t *d_frames, const uint64_t *d_desc, uint64_t n,
                                             const uint16_t *d_inner_off, uint32_t what, nffacl_cksum *d_sums,
                                             uint64_t *d_bad_bits, void *stream) {
    auto misaligned = [](const void *p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a != 0; };
    if (what == 0 || (what & ~(NFFACL_CK_IP4 | NFFACL_CK_L4)) != 0 || n >> 32 || (!d_sums && !d_bad_bits))
        return NFFACL_ERR_INVALID_ARG;
    if (!d_frames || misaligned(d_frames, 16) || !d_desc || misaligned(d_desc, 8) || misaligned(d_inner_off, 2) ||
        misaligned(d_sums, 8) || misaligned(d_bad_bits, 8))
        return NFFACL_ERR_INVALID_ARG;
    if (n == 0) return NFFACL_OK;
    // 1024-thread workgroups, two per CU: 256 CUs x 2 hold any gfx950 part, grid stride beyond
    const uint32_t tiles = static_cast<uint32_t>((n + kCkTile - 1) / kCkTile);  // <= 2^22
    const dim3 grid(std::min<uint32_t>(tiles, 512)), block(kCkBlock);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    uint64_t *sums = reinterpret_cast<uint64_t *>(d_sums);
    if (what & NFFACL_CK_L4)
        hipLaunchKernelGGL(dev::k_cksum<true>, grid, block, 0, s, d_frames, d_desc, n, d_inner_off, what, sums,
                           d_bad_bits, tiles);
    else
        hipLaunchKernelGGL(dev::k_cksum<false>, grid, block, 0, s, d_frames, d_desc, n, d_inner_off, what, sums,
                           d_bad_bits, tiles);
    HIP_TRY(hipGetLastError());
    return NFFACL_OK;
}
