// keys_encap.hip — keys from encapsulated packed frames (nffacl.h,
// nffacl_extract_keys_encap_frames_device): HIP kernel (gfx950) and launcher.
//
// Hot path replaced: the decapsulation step the reference's users run on the
// CPU before they classify the inner 5-tuple — vlan.go:66-76 (tags),
// mpls.go:38-41, 65-74 (ParseL3CheckMPLS / RemoveMPLS), gre.go:13-16,
// gtp.go:132-140 (DecapsulateIPv4GTP) — resolved once, here, without
// rewriting the frame: the key is that of the inner header, and every key
// kernel downstream (keys.hip) works on it unchanged.
//
// The shim chain is a chain of dependent reads (tag -> label -> label -> IHL
// -> UDP -> GTP flags -> extension).  Work split (one wave64 = 64 consecutive
// frames, as k_extract_keys_frames):
//  * stage: the wave loads its 64 descriptors lane-contiguous and copies the
//    first kW bytes of every frame into its own LDS region, cooperatively in
//    the shape of load_frames_rs: per 64-byte line, lane 16r + c loads chunk r
//    of frame 16j + c for j = 0..3 (whole lines per instruction,
//    nontemporal), a chunk only if it starts inside its frame, bytes past the
//    frame's length zeroed on the way in.  A line no frame of the wave
//    reaches is not loaded at all (zeros are stored).  Frame f lies at dword
//    f * kStride; kStride is odd, so the 64 lanes' reads of "my frame, dword
//    k" fall into 64 different banks;
//  * resolve: each lane walks its own frame's chain with ds_read_b32 at
//    data-dependent dword indices.  Every shim is a multiple of 4 bytes, so
//    the walk's state is one dword index q: the EtherType (or what stands for
//    it) is the low half of dword q and the L3 header starts in its high
//    half.  Loops are bounded by the caps (2 tags, 8 labels, 4 extensions) and
//    predicated; the encap bits are tested wave-uniformly, the label and
//    extension loops are skipped by ballot when no lane of the wave needs them;
//  * re-base: the lane reads dwords q - 3 .. q + 12 of its frame from LDS as
//    the d[16] of parse_fields, sets the low half of d[3] to the resolved
//    EtherType and parses as a plain frame; ports that inner IP options push
//    past the window come through far_dwords based at the inner frame;
//  * deep frames: a lane whose chain or window touches a dword at or past kW
//    of a frame longer than kW repeats the resolution against global memory
//    (one dword per read, clipped at the frame's length) in a branch only
//    such lanes take; the ragged last wave (and n < 64) takes that path
//    throughout.
// No global atomics, no workgroup waits on another, nothing is allocated.
// Registers / LDS and the measurements: DESIGN.md §4.11.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "classify.hpp"
#include "devutil.hpp"
#include "keys.hpp"

namespace nffacl {
namespace dev {

constexpr uint32_t kW = 192;                    // staged bytes per frame
constexpr uint32_t kWDwords = kW / 4;           // 48
constexpr uint32_t kStride = kWDwords + 1;      // dwords between frames in LDS (odd: no bank shared)
constexpr uint32_t kWaveDwords = 64 * kStride;  // 12544 bytes per wave
constexpr uint32_t kEncapWaves = 4;             // 256-thread workgroups: 50176 bytes of LDS, 3 per CU

// EtherTypes as the little-endian low half of a frame dword
constexpr uint32_t kEt4 = 0x0008u, kEt6 = 0xDD86u, kEtTag = 0x0081u, kEtSTag = 0xA888u, kEtMpls = 0x4788u;

typedef u32x4 u32x4_a4 __attribute__((aligned(4)));  // a 16-byte LDS store at a dword-aligned address

// Stage the first kW bytes of the wave's 64 frames (ds = this lane's
// descriptor; every lane active) into wl[frame * kStride + dword].
__device__ __forceinline__ void stage_frames(const uint8_t *__restrict__ frames, uint64_t ds, uint32_t lane,
                                             uint32_t *__restrict__ wl) {
    const uint32_t lo = static_cast<uint32_t>(ds), hi = static_cast<uint32_t>(ds >> 32);
    const uint32_t r = lane >> 4, c = lane & 15u;
    uint32_t fl[4];
    const uint8_t *fp[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int src = static_cast<int>((16u * j + c) << 2);
        const uint32_t l = static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(src, static_cast<int>(lo)));
        const uint32_t h = static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(src, static_cast<int>(hi)));
        fl[j] = l & 0xFFFFu;
        fp[j] = frames + ((uint64_t(h) << 32 | l) >> 16);
    }
#pragma unroll
    for (uint32_t L = 0; L < kW / 64; ++L) {
        const uint32_t o = 64u * L + 16u * r;  // this lane's chunk of the line
        u32x4 v[4];
        if (L == 0 || ballot((lo & 0xFFFFu) > 64u * L)) {  // some frame of the wave reaches line L
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const u32x4 *p = o < fl[j] ? reinterpret_cast<const u32x4 *>(fp[j] + o) : &g_zero16;
                v[j] = __builtin_nontemporal_load(p);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t rem = fl[j] - o;       // valid bytes from the chunk's start (if o < len)
                if (ballot(o < fl[j] && rem < 16u)) {  // the frame ends inside this chunk: zero its tail
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        const int left = o < fl[j] ? static_cast<int>(rem) - 4 * m : 16;
                        v[j][m] &= left >= 4 ? 0xFFFFFFFFu : left <= 0 ? 0u : (1u << (8 * left)) - 1u;
                    }
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            *reinterpret_cast<u32x4_a4 *>(wl + (16u * j + c) * kStride + o / 4u) = v[j];
    }
}

// Frame dwords from the wave's LDS stage: dword k < kWDwords of this lane's
// frame; a predicated-off read gives 0.  `over` records a wanted dword past
// the stage (it reads as 0: right for a frame that ends inside the stage).
struct LdsReader {
    const uint32_t *my;
    bool over;
    __device__ __forceinline__ uint32_t operator()(uint32_t k, bool want) {
        const bool in = k < kWDwords;
        over |= want && !in;
        const uint32_t v = my[in ? k : 0u];
        return want && in ? v : 0u;
    }
};

// The same from global memory, one lane's frame (4-byte aligned loads that
// start inside the frame), bytes at or past `len` as 0.
struct GlobalReader {
    const uint32_t *p;
    uint32_t len;
    __device__ __forceinline__ uint32_t operator()(uint32_t k, bool want) {
        const int rem = 4u * k < len ? static_cast<int>(len - 4u * k) : 0;
        uint32_t v = 0u;
        if (want && rem > 0) v = p[k];
        return rem >= 4 ? v : v & ((1u << (8 * rem)) - 1u);
    }
};

// One frame's encapsulation resolved (the rules: nffacl.h, nffacl_encap_flags)
// and its inner header re-based: d[3..15] = frame dwords q .. q + 12 with the
// low half of d[3] set to the resolved EtherType (d[0..2] are not read by
// parse_fields).  Returns q, the dword whose high half starts the inner L3
// header (cursor = 4 q + 2), or 0 for a malformed frame (d[3]'s EtherType is
// then 0: neither family).
template <class Reader>
__device__ __forceinline__ uint32_t resolve_encap(Reader &rd, uint32_t len, uint32_t encap, uint32_t (&d)[16]) {
    uint32_t q = 3u;
    uint32_t w = rd(q, true);  // invariant: w = dword q
    uint32_t et = w & 0xFFFFu;
    bool bad = false;
    if (encap & NFFACL_ENCAP_VLAN) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const bool tag = et == kEtTag || et == kEtSTag;
            const uint32_t wn = rd(q + 1u, tag);
            q += tag ? 1u : 0u;
            w = tag ? wn : w;
            et = w & 0xFFFFu;
        }
    }
    if (encap & NFFACL_ENCAP_MPLS) {
        const bool mpls = et == kEtMpls;
        if (ballot(mpls)) {
            bool open = mpls;  // label i's S bit is bit 0 of dword q + 1 + i
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (!ballot(open)) break;
                const uint32_t wn = rd(q + 1u, open);
                q += open ? 1u : 0u;
                w = open ? wn : w;
                open = open && !(wn & 1u);
            }
            bad |= open;  // more than 8 labels, or no bottom of stack before the frame ends
            const uint32_t nib = (w >> 20) & 0xFu;  // the usual rule: the payload's version nibble
            if (mpls) et = nib == 4u ? kEt4 : nib == 6u ? kEt6 : 0u;
        }
    }
    if (encap & (NFFACL_ENCAP_GRE | NFFACL_ENCAP_GTPU)) {
        const bool is6 = et == kEt6;
        const uint32_t ihl = (w >> 16) & 0xFu;
        const bool ip = !bad && (is6 || (et == kEt4 && ihl >= 5u));
        const uint32_t w2 = rd(q + 2u, ip);  // IPv4 protocol: byte 3; IPv6 next header: byte 0
        const uint32_t proto = is6 ? w2 & 0xFFu : w2 >> 24;
        const uint32_t q4 = q + (is6 ? 10u : ihl);  // the L4 header starts in the high half of dword q4
        const bool l4gre = ip && (encap & NFFACL_ENCAP_GRE) && proto == 47u;
        const bool l4udp = ip && (encap & NFFACL_ENCAP_GTPU) && proto == 17u;
        if (ballot(l4gre || l4udp)) {
            const uint32_t wa = rd(q4, l4gre);               // GRE flags, version
            const uint32_t wb = rd(q4 + 1u, l4gre || l4udp);  // GRE NextProto / UDP destination port
            const uint32_t wc = rd(q4 + 2u, l4udp);           // GTP flags, message type
            const uint32_t gfl = wa >> 16;
            const bool gre = l4gre && ((gfl >> 8) & 7u) == 0u;  // version 0
            const uint32_t tfl = (wc >> 16) & 0xFFu;
            // UDP dport 2152, GTPv1, PT 1, G-PDU
            const bool gtp = l4udp && (wb & 0xFFFFu) == 0x6808u && (tfl >> 4) == 3u && (wc >> 24) == 255u;
            uint32_t qn = q4 + 1u + ((gfl >> 7) & 1u) + ((gfl >> 5) & 1u) + ((gfl >> 4) & 1u);  // + C, K, S
            uint32_t etn = wb & 0xFFFFu;
            etn = etn == kEt4 || etn == kEt6 ? etn : 0u;
            if (ballot(gtp)) {
                uint32_t qe = q4 + 4u + ((tfl & 7u) ? 1u : 0u);  // 8 bytes, 12 with any of E / S / PN
                bool walk = gtp && (tfl & 4u);
                uint32_t we = rd(qe, gtp);  // byte 1: next extension type, byte 2: that extension's length
                if (ballot(walk)) {
#pragma unroll
                    for (int i = 0; i < 5; ++i) {
                        walk = walk && ((we >> 8) & 0xFFu) != 0u;
                        if (!ballot(walk)) break;
                        const uint32_t el = (we >> 16) & 0xFFu;  // 4-octet units, its last octet the next type
                        if (walk && (i == 4 || el == 0u)) {      // a fifth extension, or one of length 0
                            bad = true;
                            walk = false;
                        }
                        qe += walk ? el : 0u;
                        const uint32_t wn = rd(qe, walk);
                        we = walk ? wn : we;
                    }
                }
                const uint32_t nib = (we >> 20) & 0xFu;
                qn = gtp ? qe : qn;
                etn = gtp ? (nib == 4u ? kEt4 : nib == 6u ? kEt6 : 0u) : etn;
            }
            if (gre || gtp) {
                q = qn;
                et = etn;
            }
        }
    }
    // a frame whose shims reach its end has no inner header; an unencapsulated
    // frame keeps its plain key whatever its length
    bad |= q != 3u && 4u * q + 2u >= len;
#pragma unroll
    for (uint32_t k = 3; k < 16; ++k) d[k] = rd(q - 3u + k, !bad);
    d[3] = (d[3] & 0xFFFF0000u) | (bad ? 0u : et);
    return bad ? 0u : q;
}

// Packed frames -> keys of their inner headers (desc = offset << 16 | len).
__global__ void __launch_bounds__(64 * kEncapWaves)
k_extract_keys_encap(const uint8_t *__restrict__ frames, const uint64_t *__restrict__ desc, uint64_t n,
                     uint32_t encap, u32x4 *__restrict__ keys, u32x4 *__restrict__ key6,
                     uint16_t *__restrict__ inner_off) {
    __shared__ uint32_t stage[kEncapWaves * kWaveDwords];
    uint32_t *wl = stage + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * kWaveDwords;
    NFFACL_WAVE_LOOP(n) {
        const uint64_t idx = base + lane;
        const bool live = idx < n;
        const uint64_t ds = live ? desc[idx] : 0;
        const uint32_t len = static_cast<uint32_t>(ds & 0xFFFFu);
        const uint8_t *pkt = frames + (ds >> 16);
        uint32_t d[16] = {};
        uint32_t q = 0;
        bool deep = true;  // the ragged last wave: one frame per lane from global memory
        if (base + 64 <= n) {
            wave_lds_sync();  // the previous batch's reads are done
            stage_frames(frames, ds, lane, wl);
            wave_lds_sync();
            LdsReader rd{wl + lane * kStride, false};
            q = resolve_encap(rd, len, encap, d);
            deep = rd.over && len > kW;
        }
        if (deep) {
            GlobalReader rd{reinterpret_cast<const uint32_t *>(pkt), len};
            q = resolve_encap(rd, len, encap, d);
        }
        // the inner frame: bytes [14, cursor) removed
        const uint32_t skip = q ? 4u * (q - 3u) : 0u;
        Fields f;
        parse_fields<true>(d, live, f, [&](uint32_t k, uint32_t &lo, uint32_t &hi) {
            far_dwords(pkt + skip, len > skip ? len - skip : 0u, k, lo, hi);
        }, 0u);
        store_key(f, idx, live, keys, key6);
        if (inner_off && live) inner_off[idx] = static_cast<uint16_t>(q ? 4u * q + 2u : 0xFFFFu);
    }
}

}  // namespace dev
}  // namespace nffacl

using namespace nffacl;

extern "C" int nffacl_extract_keys_encap_frames_device(const uint8_t *d_frames, const uint64_t *d_desc, uint64_t n,
                                                       uint32_t encap, nffacl_key *d_keys, nffacl_key6 *d_key6,
                                                       uint16_t *d_inner_off, void *stream) {
    constexpr uint32_t all = NFFACL_ENCAP_VLAN | NFFACL_ENCAP_MPLS | NFFACL_ENCAP_GRE | NFFACL_ENCAP_GTPU;
    auto misaligned = [](const void *p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a != 0; };
    if ((encap & ~all) != 0 || n >> 32) return NFFACL_ERR_INVALID_ARG;
    if (!d_frames || misaligned(d_frames, 16) || !d_desc || misaligned(d_desc, 8) || !d_keys ||
        misaligned(d_keys, 16) || !d_key6 || misaligned(d_key6, 16) || misaligned(d_inner_off, 2))
        return NFFACL_ERR_INVALID_ARG;
    if (n == 0) return NFFACL_OK;
    // a streaming kernel with no table; its LDS stage lets three workgroups
    // share a CU, so 256 CUs x 3 of them hold any gfx950 part, grid stride beyond
    const uint64_t blocks = (n + 64 * dev::kEncapWaves - 1) / (64 * dev::kEncapWaves);
    const uint32_t grid = static_cast<uint32_t>(std::min<uint64_t>(blocks, 768));
    hipLaunchKernelGGL(dev::k_extract_keys_encap, dim3(grid), dim3(64 * dev::kEncapWaves), 0,
                       static_cast<hipStream_t>(stream), d_frames, d_desc, n, encap,
                       reinterpret_cast<dev::u32x4 *>(d_keys), reinterpret_cast<dev::u32x4 *>(d_key6), d_inner_off);
    HIP_TRY(hipGetLastError());
    return NFFACL_OK;
}
