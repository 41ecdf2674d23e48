// keys.hip — classification from compact 5-tuple keys (nffacl_key, nffacl.h):
// HIP kernels (gfx950) and their launchers.
//
// Hot path replaced: the same (*Packet).l3ACL (packet/acl.go:522-565) as
// engine.hip, fed with the fields ParseAllKnownL3 / ParseL4ForIPv4/6 yield
// instead of the packet bytes they are parsed from.  The walks are those of
// classify.hpp, unchanged; what differs is everything around them.
//
// Work split (one wave64, a batch = 64 U consecutive keys):
//  * one lane owns one key per load: load u of a batch is ONE lane-contiguous
//    global_load_dwordx4 (1 KiB per instruction, nontemporal — a key is read
//    once) that gives lane l key base + 64 u + l whole.  No transpose, no
//    parse: the four dwords ARE the walk's Fields;
//  * a wave issues the U loads of its NEXT batch (a grid stride ahead) before
//    it walks the current one, so the stream's latency hides behind U walks;
//    the grid is persistent (static grid stride, no pull counters);
//  * IPv6 lanes gather their two dwordx4 from the key6 side array in a
//    divergent branch, bounds-checked against n_key6; the gather of key u + 1
//    is issued before the walk of key u starts, which covers it;
//  * per-lane walks (LINEAR, INDEXED, HYBRID lane) run once per key; the
//    wave-cooperative flat walks take one 64-key batch at a time;
//  * lane l holds key b + l, so the permit word is a plain ballot (no
//    ds_bpermute) and the port store a lane-contiguous dword store.
// Registers / LDS per kernel and the measured figures: DESIGN.md §4.9.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <type_traits>

#include "classify.hpp"
#include "devutil.hpp"
#include "engine.hpp"
#include "keys.hpp"
#include "launch.hpp"

namespace nffacl {
namespace dev {

// Key idx of the array, this lane's; lanes past n read the zero block (a key
// of family 0: verdict 0), so the load needs no branch.
__device__ __forceinline__ u32x4 load_key(const u32x4 *__restrict__ keys, uint64_t idx, uint64_t n) {
    return __builtin_nontemporal_load(idx < n ? keys + idx : &g_zero16);
}

struct Addr6 {
    u32x4 s, t;  // src / dst as little-endian dwords of the wire bytes: Fields::s, ::t
};

// The IPv6 record of key k (meta says family 6, index inside the array):
// issued here, used by key_fields.  Returns whether the lane is IPv6.
__device__ __forceinline__ bool gather6(const u32x4 &k, const u32x4 *__restrict__ key6, uint32_t n_key6, Addr6 &x) {
    const bool six = (k.w >> 8) == kFam6 && k.x < n_key6;
    x.s = x.t = u32x4{0, 0, 0, 0};
    if (six) {
        const u32x4 *p = key6 + 2u * uint64_t(k.x);
        x.s = __builtin_nontemporal_load(p);
        x.t = __builtin_nontemporal_load(p + 1);
    }
    return six;
}

// A key is the parse's result: no field is computed, only named.  (meta's
// bits 16-31 are 0; a key that sets them has an unknown family.)
__device__ __forceinline__ void key_fields(const u32x4 &k, const Addr6 &x, bool six, Fields &f) {
    f.is4 = (k.w >> 8) == kFam4;
    f.is6 = six;
    f.proto = k.w & 0xFFu;
    f.ports = k.z;
    f.s[0] = six ? x.s.x : k.x;
    f.t[0] = six ? x.t.x : k.y;
    f.s[1] = x.s.y;
    f.s[2] = x.s.z;
    f.s[3] = x.s.w;
    f.t[1] = x.t.y;
    f.t[2] = x.t.z;
    f.t[3] = x.t.w;
}

// Key walks over the table layouts of TableMode.  Walks that read the same
// layout share an instantiation: kTabFlat serves kTabFlat4 too (2 rounds in
// flight: the smaller scratch fits either launch), kTabFlatLds4 serves
// kTabFlatLds4U (predicated entry loads).
template <int NS, int TM>
__device__ __forceinline__ uint32_t walk_key(const IndexedArgs &a, const Fields &f, uint32_t lane) {
    const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if constexpr (TM == kTabFlatLdsP) {
        FlatScratch<4> *W = reinterpret_cast<FlatScratch<4> *>(lds_tab + a.stage_dwords);
        return classify_flat_pipe<NS>(a, f, W[w], lane, [] {});
    } else if constexpr (TM == kTabFlat) {
        FlatScratch<2> *W = reinterpret_cast<FlatScratch<2> *>(lds_tab);
        return classify_flat<NS, 2, false>(a, f, W[w], lane);
    } else if constexpr (TM == kTabFlatLds || TM == kTabFlatLds4 || TM == kTabFlatLdsG) {
        constexpr int R = TM == kTabFlatLds ? 2 : 4;
        FlatScratch<R> *W = reinterpret_cast<FlatScratch<R> *>(lds_tab + a.stage_dwords);
        return classify_flat<NS, R, true, TM == kTabFlatLdsG, true, TM == kTabFlatLdsG>(a, f, W[w], lane);
    } else {
        static_assert(NS <= 4, "per-lane walks: the positional four slots");
        if constexpr (TM == kTabLds) return classify_indexed<NS, 1>(LdsTab{}, a, f);
        else if constexpr (TM == kTabLdsNP) return classify_indexed<NS, 1, LdsTab, true>(LdsTab{}, a, f);
        else if constexpr (TM == kTabSplit) return classify_indexed<NS, 1>(SplitTab{a.tab}, a, f);
        else return classify_indexed<NS, 1>(GlobalTab{a.tab}, a, f);
    }
}

constexpr bool flat_tm(int tm) {
    return tm == kTabFlat || tm == kTabFlatLds || tm == kTabFlatLds4 || tm == kTabFlatLdsG || tm == kTabFlatLdsP;
}

// The batch loop shared by the LINEAR and the table kernels: `walk(f)` is the
// verdict of one key's fields, called with every lane of the wave active.
// What a wave holds across a walk is kept small, because the widest flat
// walks fill the 128 VGPRs of a 1024-thread workgroup on their own: during
// walk u < U - 1 the keys still to walk and the NEXT key's IPv6 record (its
// gather issued before walk u starts), during the last walk only the next
// batch's U keys (their loads issued before it starts).  Only a batch's
// first gather is waited for.
template <int U, bool NT_OUT, class Walk>
__device__ __forceinline__ void key_batches(const u32x4 *__restrict__ keys, const u32x4 *__restrict__ key6,
                                            uint32_t n_key6, uint64_t n, uint32_t *__restrict__ port_out,
                                            uint64_t *__restrict__ permit_out, Walk &&walk) {
    const uint32_t lane = lane_id();
    const uint32_t wpb = blockDim.x >> 6;
    const uint64_t wave0 = uint64_t(blockIdx.x) * wpb + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t step = uint64_t(gridDim.x) * wpb * (64u * U);
    uint64_t base = wave0 * (64u * U);
    if (base >= n) return;
    u32x4 k[U];
#pragma unroll
    for (int u = 0; u < U; ++u) k[u] = load_key(keys, base + 64u * u + lane, n);
    for (; base < n; base += step) {
        Addr6 x, xn;
        bool six = gather6(k[0], key6, n_key6, x), sixn = false;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t b = base + 64u * u;  // (wave-uniform; a batch past n holds zero keys: its walk is skipped)
            const u32x4 kk = k[u];
            if (u + 1 < U) {
                sixn = gather6(k[u + 1], key6, n_key6, xn);
            } else {
                const uint64_t nb = base + step;
                if (nb < n) {
#pragma unroll
                    for (int v = 0; v < U; ++v) k[v] = load_key(keys, nb + 64u * v + lane, n);
                }
            }
            if (b < n) {
                Fields f;
                key_fields(kk, x, six, f);
                const uint32_t res = walk(f);  // lanes past n hold the zero key: 0
                const bool live = b + lane < n;
                if (live && port_out) store_port<NT_OUT>(port_out + b + lane, res);
                if (permit_out) {
                    const uint64_t permit = ballot(live && res != 0u);
                    if (lane == 0) permit_out[b >> 6] = permit;
                }
            }
            x = xn;
            six = sixn;
        }
    }
}

template <int U>
__global__ void __launch_bounds__(256)
k_keys_linear(const u32x4 *__restrict__ keys, const u32x4 *__restrict__ key6, uint32_t n_key6, uint64_t n,
              LinearArgs a, uint32_t *__restrict__ port_out, uint64_t *__restrict__ permit_out) {
    key_batches<U, false>(keys, key6, n_key6, n, port_out, permit_out,
                                 [&](const Fields &f) { return classify_linear(f, a.rec4, a.n4, a.rec6, a.n6); });
}

// Tables and directories staged as the slot kernels stage them; the flat
// walks' FlatScratch per wave lies where theirs does.
template <int NS, int TM, int U>
__global__ void __launch_bounds__(1024)
k_keys(const u32x4 *__restrict__ keys, const u32x4 *__restrict__ key6, uint32_t n_key6, uint64_t n, IndexedArgs a,
       uint32_t *__restrict__ port_out, uint64_t *__restrict__ permit_out) {
    if (TM != kTabGlobal && TM != kTabFlat) stage_table(a);
    const uint32_t lane = lane_id();
    // nontemporal verdict stores where the table should keep L2 (devutil.hpp store_port)
    key_batches<U, TM == kTabFlatLdsP>(keys, key6, n_key6, n, port_out, permit_out,
                                                    [&](const Fields &f) { return walk_key<NS, TM>(a, f, lane); });
}

// Slots -> keys.  Dense 64-byte slots load lane-contiguous (devutil.hpp
// load_rowswap: lane l ends with packet l); wider strides one row per lane.
__global__ void __launch_bounds__(256)
k_extract_keys(const uint8_t *__restrict__ slots, uint32_t stride, uint64_t n, uint32_t flags,
               u32x4 *__restrict__ keys, u32x4 *__restrict__ key6) {
    NFFACL_WAVE_LOOP(n) {
        const uint64_t idx = base + lane;
        const bool live = idx < n;
        const uint8_t *pkt = slots + (live ? idx : 0) * stride;
        uint32_t d[16];
        if (stride == 64u && base + 64 <= n) {
            u32x4 v[4];
            load_rowswap<true>(slots + base * 64, lane, v);
            rowswap_batch(v, d);
        } else {
            load16(pkt, d);
        }
        Fields f;
        parse_fields(d, live, f, [&](uint32_t k, uint32_t &lo, uint32_t &hi) {
            far_dwords(pkt, stride, k, lo, hi);
        }, flags);
        store_key(f, idx, live, keys, key6);
    }
}

// Packed frames -> keys (desc = offset << 16 | len, as k_linear_frames).  A
// full wave loads its 64 descriptors lane-contiguous and its frame lines
// cooperatively (load_frames_rs: whole 64-byte lines per instruction); the
// ragged last wave reads one frame per lane.  Ports past byte 63 (IHL >= 12,
// VLAN) come through the frames far reader: bytes past len read as 0.
__global__ void __launch_bounds__(256)
k_extract_keys_frames(const uint8_t *__restrict__ frames, const uint64_t *__restrict__ desc, uint64_t n,
                      uint32_t flags, u32x4 *__restrict__ keys, u32x4 *__restrict__ key6) {
    NFFACL_WAVE_LOOP(n) {
        const uint64_t idx = base + lane;
        const bool live = idx < n;
        const uint64_t ds = live ? desc[idx] : 0;
        const uint32_t len = static_cast<uint32_t>(ds & 0xFFFFu);
        const uint8_t *pkt = frames + (ds >> 16);
        uint32_t d[16];
        if (base + 64 <= n) {
            u32x4 v[4];
            load_frames_rs(frames, ds, lane, v);
            rowswap_batch(v, d);
            if (ballot(len < 64u)) clip16(d, len);
        } else {
            load16_frame(pkt, len, d);
        }
        Fields f;
        parse_fields(d, live, f, [&](uint32_t k, uint32_t &lo, uint32_t &hi) {
            far_dwords(pkt, len, k, lo, hi);
        }, flags);
        store_key(f, idx, live, keys, key6);
    }
}

}  // namespace dev

namespace {

// The key instantiation that walks the layout of slot-kernel mode tm.
int key_tm(int tm) {
    if (tm == dev::kTabFlat4) return dev::kTabFlat;
    if (tm == dev::kTabFlatLds4U) return dev::kTabFlatLds4;
    return tm;
}

// Calls f(integral_constant<NS>, integral_constant<TM>) for a key kernel.
template <class F>
void dispatch_keys(int ns, int tm, F &&f) {
    auto lane_walks = [&](auto nsc) {
        switch (tm) {
        case dev::kTabLds: f(nsc, std::integral_constant<int, dev::kTabLds>{}); break;
        case dev::kTabLdsNP: f(nsc, std::integral_constant<int, dev::kTabLdsNP>{}); break;
        case dev::kTabSplit: f(nsc, std::integral_constant<int, dev::kTabSplit>{}); break;
        default: f(nsc, std::integral_constant<int, dev::kTabGlobal>{}); break;
        }
    };
    auto flat_walks = [&](auto nsc) {
        switch (tm) {
        case dev::kTabFlat: f(nsc, std::integral_constant<int, dev::kTabFlat>{}); break;
        case dev::kTabFlatLds: f(nsc, std::integral_constant<int, dev::kTabFlatLds>{}); break;
        case dev::kTabFlatLdsG: f(nsc, std::integral_constant<int, dev::kTabFlatLdsG>{}); break;
        case dev::kTabFlatLdsP: f(nsc, std::integral_constant<int, dev::kTabFlatLdsP>{}); break;
        default: f(nsc, std::integral_constant<int, dev::kTabFlatLds4>{}); break;
        }
    };
    auto with_ns = [&](auto nsc) {
        if (dev::flat_tm(tm)) flat_walks(nsc);
        else if constexpr (decltype(nsc)::value <= 4) lane_walks(nsc);
    };
    switch (ns) {
    case 2: with_ns(std::integral_constant<int, 2>{}); break;
    case 3: with_ns(std::integral_constant<int, 3>{}); break;
    case 4: with_ns(std::integral_constant<int, 4>{}); break;
    case 5: with_ns(std::integral_constant<int, 5>{}); break;
    case 6: with_ns(std::integral_constant<int, 6>{}); break;
    case 7: with_ns(std::integral_constant<int, 7>{}); break;
    default: with_ns(std::integral_constant<int, 8>{}); break;
    }
}

// Every key kernel may take the CU's whole LDS (once per process).
int prepare_key_kernels() {
    static std::once_flag once;
    static hipError_t err = hipSuccess;
    std::call_once(once, [] {
        for (int ns = 2; ns <= int(kMaxSlots); ++ns)
            for (int tm : {int(dev::kTabLds), int(dev::kTabLdsNP), int(dev::kTabSplit), int(dev::kTabFlat),
                           int(dev::kTabFlatLds), int(dev::kTabFlatLds4), int(dev::kTabFlatLdsG),
                           int(dev::kTabFlatLdsP)}) {
                if (ns > 4 && !dev::flat_tm(tm)) continue;
                dispatch_keys(ns, tm, [&](auto nsc, auto tmc) {
                    constexpr int NS = decltype(nsc)::value, TM = decltype(tmc)::value;
                    const hipError_t e = hipFuncSetAttribute(
                        reinterpret_cast<const void *>(dev::k_keys<NS, TM, kKeysU>),
                        hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(kLdsBytes));
                    if (e != hipSuccess) err = e;
                });
            }
    });
    if (err != hipSuccess) {
        set_last_error(std::string("hipFuncSetAttribute(LDS): ") + hipGetErrorString(err));
        return NFFACL_ERR_HIP;
    }
    return NFFACL_OK;
}

}  // namespace

// Launch shape: the slot kernels' choice for the same table (indexed_launch:
// block, workgroups per CU, LDS bytes — the staged image and scratch are the
// same), over batches of 64 U keys.
int launch_keys(nffacl_engine *eng, DevTable *t, const nffacl_key *d_keys, const nffacl_key6 *d_key6,
                uint32_t n_key6, uint64_t n, uint32_t *d_port, uint64_t *d_permit, hipStream_t stream) {
    if (n == 0) return NFFACL_OK;
    const dev::u32x4 *keys = reinterpret_cast<const dev::u32x4 *>(d_keys);
    const dev::u32x4 *key6 = reinterpret_cast<const dev::u32x4 *>(d_key6);
    if (t->meta.algo != NFFACL_ALGO_LINEAR) {
        if (!table_consistent(t)) {
            set_last_error("compiled table layout does not match its kernel");
            return NFFACL_ERR_INVALID_ARG;
        }
        const int st = prepare_key_kernels();
        if (st != NFFACL_OK) return st;
        const dev::IndexedArgs a = indexed_args(t);
        const IndexedLaunch L = indexed_launch(eng, t);
        if (L.lds_bytes > kLdsBytes) {
            set_last_error("compiled table's LDS image and scratch exceed the CU's LDS");
            return NFFACL_ERR_INVALID_ARG;
        }
        const int tm = key_tm(L.tm);
        if (L.ns > 4 && !dev::flat_tm(tm)) {  // (no compiler output: per-lane walks have four slots)
            set_last_error("no key kernel for a per-lane walk over more than 4 slots");
            return NFFACL_ERR_UNSUPPORTED;
        }
        dispatch_keys(L.ns, tm, [&](auto nsc, auto tmc) {
            constexpr int NS = decltype(nsc)::value, TM = decltype(tmc)::value, U = kKeysU;
            const uint32_t grid = grid_for(eng, (n + U - 1) / U, L.block, L.per_cu);
            const size_t lds = TM == dev::kTabGlobal ? 0 : L.lds_bytes;
            hipLaunchKernelGGL((dev::k_keys<NS, TM, U>), dim3(grid), dim3(L.block), lds, stream, keys, key6, n_key6, n,
                               a, d_port, d_permit);
        });
    } else {
        const uint32_t block = 256;
        const dev::LinearArgs a{t->d_blob + t->meta.off_rec4, t->meta.n4, t->d_blob + t->meta.off_rec6, t->meta.n6, 0u};
        const uint32_t grid = grid_for(eng, (n + kKeysU - 1) / kKeysU, block, 8);
        hipLaunchKernelGGL(dev::k_keys_linear<kKeysU>, dim3(grid), dim3(block), 0, stream, keys, key6, n_key6, n, a,
                           d_port, d_permit);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(t->note_use(stream));
    return NFFACL_OK;
}

}  // namespace nffacl

// ---------------------------------------------------------------------------
// C-ABI (include/nffacl.h); nffacl_classify_keys_host: capi.cpp (the engine's
// host staging)
// ---------------------------------------------------------------------------

using namespace nffacl;

static bool aligned16(const void *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

extern "C" {

int nffacl_classify_keys_device(nffacl_engine *eng, const nffacl_key *d_keys, const nffacl_key6 *d_key6,
                                uint32_t n_key6, uint64_t n, uint32_t *d_port, uint64_t *d_permit_bits,
                                void *stream) {
    if (!eng || (!d_port && !d_permit_bits)) return NFFACL_ERR_INVALID_ARG;
    if (n == 0) return NFFACL_OK;
    if (!d_keys || !aligned16(d_keys) || (n_key6 && !d_key6) || !aligned16(d_key6)) return NFFACL_ERR_INVALID_ARG;
    HIP_TRY(hipSetDevice(eng->device));
    const TablePtr t = acquire_table(eng);  // held while the launch is enqueued
    return launch_keys(eng, t.get(), d_keys, d_key6, n_key6, n, d_port, d_permit_bits,
                       static_cast<hipStream_t>(stream));
}

int nffacl_extract_keys_device(const uint8_t *d_slots, uint32_t stride, uint64_t n, uint32_t flags,
                               nffacl_key *d_keys, nffacl_key6 *d_key6, void *stream) {
    if ((flags & ~uint32_t(NFFACL_PARSE_VLAN)) != 0 || n >> 32) return NFFACL_ERR_INVALID_ARG;
    if (n == 0) return NFFACL_OK;
    if (!d_slots || stride < 64 || (stride % 16) != 0 || !aligned16(d_slots) || !d_keys || !aligned16(d_keys) ||
        !d_key6 || !aligned16(d_key6))
        return NFFACL_ERR_INVALID_ARG;
    // a streaming kernel with no table: 256-thread workgroups, enough of them
    // to fill any gfx950 part (256 CUs x 8), grid stride beyond
    const uint64_t blocks = (n + 255) / 256;
    const uint32_t grid = static_cast<uint32_t>(std::min<uint64_t>(blocks, 2048));
    hipLaunchKernelGGL(dev::k_extract_keys, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), d_slots,
                       stride, n, flags, reinterpret_cast<dev::u32x4 *>(d_keys),
                       reinterpret_cast<dev::u32x4 *>(d_key6));
    HIP_TRY(hipGetLastError());
    return NFFACL_OK;
}

int nffacl_extract_keys_frames_device(const uint8_t *d_frames, const uint64_t *d_desc, uint64_t n, uint32_t flags,
                                      nffacl_key *d_keys, nffacl_key6 *d_key6, void *stream) {
    if ((flags & ~uint32_t(NFFACL_PARSE_VLAN)) != 0 || n >> 32) return NFFACL_ERR_INVALID_ARG;
    if (n == 0) return NFFACL_OK;
    if (!d_frames || !aligned16(d_frames) || !d_desc || !d_keys || !aligned16(d_keys) || !d_key6 ||
        !aligned16(d_key6))
        return NFFACL_ERR_INVALID_ARG;
    const uint64_t blocks = (n + 255) / 256;  // (launch shape: as nffacl_extract_keys_device)
    const uint32_t grid = static_cast<uint32_t>(std::min<uint64_t>(blocks, 2048));
    hipLaunchKernelGGL(dev::k_extract_keys_frames, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream),
                       d_frames, d_desc, n, flags, reinterpret_cast<dev::u32x4 *>(d_keys),
                       reinterpret_cast<dev::u32x4 *>(d_key6));
    HIP_TRY(hipGetLastError());
    return NFFACL_OK;
}

// Plain C++ for the flow-function clones: the field rules of parse_fields
// (classify.hpp) on one frame at a time.
int nffacl_extract_keys_host(const uint8_t *const *frames, const uint32_t *lens, uint64_t n, uint32_t flags,
                             nffacl_key *keys, nffacl_key6 *key6, uint64_t key6_cap, uint64_t *n_key6) {
    if ((flags & ~uint32_t(NFFACL_PARSE_VLAN)) != 0 || !n_key6) return NFFACL_ERR_INVALID_ARG;
    *n_key6 = 0;
    if (n == 0) return NFFACL_OK;
    if (!frames || !lens || !keys || (key6_cap && !key6)) return NFFACL_ERR_INVALID_ARG;
    uint64_t n6 = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint8_t *p = frames[i];
        const uint32_t len = lens[i];
        auto at = [&](uint32_t o) -> uint32_t { return o < len ? p[o] : 0u; };  // bytes past the frame read as 0
        auto be16 = [&](uint32_t o) { return at(o) << 8 | at(o + 1); };
        auto le32 = [&](uint32_t o) { return at(o) | at(o + 1) << 8 | at(o + 2) << 16 | at(o + 3) << 24; };
        uint32_t l3 = 14, et = be16(12);
        if ((flags & NFFACL_PARSE_VLAN) && et == 0x8100u) {  // ParseAllKnownL3CheckVLAN
            l3 = 18;
            et = be16(16);
        }
        nffacl_key k{0, 0, 0, 0};
        if (et == 0x0800u) {
            const uint32_t l4 = l3 + 4u * (at(l3) & 0xFu);  // wherever IHL puts it
            k = nffacl_key{le32(l3 + 12), le32(l3 + 16), be16(l4) | be16(l4 + 2) << 16, at(l3 + 9) | 4u << 8};
        } else if (et == 0x86DDu) {
            if (n6 >= key6_cap) return NFFACL_ERR_INVALID_ARG;
            if (n6 >> 32) return NFFACL_ERR_INVALID_ARG;
            for (uint32_t j = 0; j < 16; ++j) {
                key6[n6].src[j] = static_cast<uint8_t>(at(l3 + 8 + j));
                key6[n6].dst[j] = static_cast<uint8_t>(at(l3 + 24 + j));
            }
            const uint32_t l4 = l3 + 40;
            k = nffacl_key{static_cast<uint32_t>(n6), 0u, be16(l4) | be16(l4 + 2) << 16, at(l3 + 6) | 6u << 8};
            ++n6;
        }
        keys[i] = k;
    }
    *n_key6 = n6;
    return NFFACL_OK;
}

}  // extern "C"
