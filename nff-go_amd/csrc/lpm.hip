// lpm.hip — longest-prefix-match next hops of a batch in HBM (nffacl.h,
// nffacl_lpm_commit / nffacl_lpm_lookup_device / _keys_device): HIP kernels
// (gfx950), the committed table's lifetime and the launchers.
//
// Hot path replaced: (*LPM).Lookup (packet/packet.go:880-895, DPDK's
// rte_lpm_lookup) called per packet by the user's flow function
// (examples/netlink.go:60-68).  Table format: lpm.hpp (16-8-8, top level in
// LDS).  Unlike every other kernel of the library this is a trie walk of
// dependent loads, not a list walk with a rule test, so the shape is chosen
// to keep many independent chains in flight:
//   * one 1024-thread workgroup per CU stages L0 and the hop words (<= 144
//     KiB) into LDS once, 8 x 16-byte loads in flight per thread, then
//     grid-strides over tiles of kLpmTile addresses;
//   * a lane owns four consecutive addresses (one nontemporal dwordx4 load;
//     four in the key form, where only family-4 keys are looked up) and walks
//     them as four independent chains: four ds_read_u16 of L0 and four reads of
//     the hop words give four answer words (kLpmHit | hop, kLpmExt | group, or
//     0); all four level-1 loads are issued before one is consumed, then all
//     four level-2 loads.  A chain that is done reads the table's first
//     word instead (a select of the address, no branch), and a level is skipped
//     when no lane of the wave has an extension left;
//   * the four next hops leave in one nontemporal dwordx4 store;
//   * hit bits: a lane's four bits are a nibble, the 16 lanes of a DPP row own
//     one 64-bit word of the bitmap: an OR scan with row_shr 1, 2, 4, 8 over
//     the two halves and one 8-byte store by the row's last lane.  No LDS, no
//     ballots.
// The tail of a batch (n % 4, n % 64, n % kLpmTile) is handled by the lane
// that holds it: single loads and stores, zero bits past n, no word past
// ceil(n / 64).  LDS = false is the same walk with L0 and the hop words read
// from global memory, for batches too small to repay the staging.
// No atomics, no scratch, nothing allocated.  Registers / LDS and the measured
// figures: DESIGN.md §4.14.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <new>

#include "devutil.hpp"
#include "launch.hpp"
#include "lpm.hpp"
#include "nffacl.h"
#include "tables.hpp"

namespace nffacl {

// Batches of at least this many addresses take the LDS form (DESIGN.md §4.14:
// the measured crossover of the two forms).
constexpr uint64_t kLpmLdsMinN = uint64_t(1) << 12;

struct LpmTable : DeviceBlob {
    LpmLayout lay;
};

struct LpmDevice {
    int device = 0;
    uint32_t num_cus = 256;
    TableHome home;
    std::shared_ptr<LpmTable> active;  // guarded by nffacl_lpm::mu
};

void lpm_device_destroy(LpmDevice *d) {
    d->active.reset();  // retired onto the home's stream, which ~TableHome drains
    delete d;
}

namespace dev {

enum LpmSrc : int { kLpmDense = 0, kLpmKeys = 1 };

struct LpmArgs {
    const uint32_t *stage;  // L0, then the hop words; also the address a finished chain reads
    const uint32_t *l1, *l2;
    uint32_t hops;          // H
    uint32_t stage_vec;     // the staged image in 16-byte pieces
};

extern __shared__ u32x4 lpm_lds[];

template <int CTRL>
__device__ __forceinline__ uint32_t row_or(uint32_t x) {
    return x | static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(x), CTRL, 0xf, 0xf, false));
}
// Lane 15 of every row <- the OR of the row's 16 values.
__device__ __forceinline__ uint32_t row_or_scan(uint32_t x) {
    x = row_or<0x111>(x);
    x = row_or<0x112>(x);
    x = row_or<0x114>(x);
    return row_or<0x118>(x);
}

template <int SRC, bool LDS>
__global__ __launch_bounds__(kLpmBlock) void k_lpm(const void *__restrict__ src, uint64_t n, LpmArgs a,
                                                   uint32_t swap, uint32_t miss, uint32_t *__restrict__ next,
                                                   uint64_t *__restrict__ hit_bits, uint32_t tiles) {
    constexpr uint32_t U = kLpmPerLane;
    const uint32_t tid = threadIdx.x;
    if constexpr (LDS) {
        const u32x4 *from = reinterpret_cast<const u32x4 *>(a.stage);
        constexpr uint32_t F = 8;
        for (uint32_t i0 = tid; i0 < a.stage_vec; i0 += F * kLpmBlock) {
            u32x4 v[F];
#pragma unroll
            for (uint32_t u = 0; u < F; ++u)
                if (i0 + u * kLpmBlock < a.stage_vec) v[u] = from[i0 + u * kLpmBlock];
#pragma unroll
            for (uint32_t u = 0; u < F; ++u)
                if (i0 + u * kLpmBlock < a.stage_vec) lpm_lds[i0 + u * kLpmBlock] = v[u];
        }
        __syncthreads();
    }
    const uint32_t c = lane_id() & 15u;

    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t i0 = uint64_t(tile) * kLpmTile + U * tid;
        const uint32_t live = i0 >= n ? 0u : n - i0 >= U ? U : static_cast<uint32_t>(n - i0);
        uint32_t adr[U] = {0u, 0u, 0u, 0u};
        bool ok[U];
#pragma unroll
        for (uint32_t j = 0; j < U; ++j) ok[j] = j < live;
        if constexpr (SRC == kLpmDense) {
            const uint32_t *p = static_cast<const uint32_t *>(src) + i0;
            if (live == U) {
                const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(p));
#pragma unroll
                for (uint32_t j = 0; j < U; ++j) adr[j] = v[j];
            } else {
#pragma unroll
                for (uint32_t j = 0; j < U; ++j)
                    if (j < live) adr[j] = p[j];
            }
        } else {
            const u32x4 *keys = static_cast<const u32x4 *>(src);  // (n >= 1: key 0 stands in past the batch)
            u32x4 k[U];
#pragma unroll
            for (uint32_t j = 0; j < U; ++j) k[j] = __builtin_nontemporal_load(keys + (j < live ? i0 + j : 0));
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (uint32_t j = 0; j < U; ++j) {
                ok[j] = ok[j] && ((k[j][3] >> 8) & 0xFFu) == 4u;
                adr[j] = ok[j] ? k[j][1] : 0u;
            }
        }
        if (swap) {
#pragma unroll
            for (uint32_t j = 0; j < U; ++j) adr[j] = __builtin_bswap32(adr[j]);
        }

        // level 0: the answer word of every chain
        uint32_t e[U], r[U];
#pragma unroll
        for (uint32_t j = 0; j < U; ++j) {
            if constexpr (LDS) e[j] = reinterpret_cast<const uint16_t *>(lpm_lds)[adr[j] >> 16];
            else e[j] = reinterpret_cast<const uint16_t *>(a.stage)[adr[j] >> 16];
        }
#pragma unroll
        for (uint32_t j = 0; j < U; ++j) {
            const uint32_t h = e[j] <= a.hops ? e[j] : 0u;
            if constexpr (LDS) r[j] = reinterpret_cast<const uint32_t *>(lpm_lds)[kLpmL0Dwords + h];
            else r[j] = a.stage[kLpmL0Dwords + h];
        }
#pragma unroll
        for (uint32_t j = 0; j < U; ++j) {
            if (e[j] > a.hops) r[j] = kLpmExt | (e[j] - a.hops - 1u);
            if (!ok[j]) r[j] = 0u;
        }
        // levels 1 and 2: every chain's load issued before one is consumed
#pragma unroll
        for (int level = 1; level <= 2; ++level) {
            const uint32_t *grp = level == 1 ? a.l1 : a.l2;
            const int sh = level == 1 ? 8 : 0;
            if (ballot(((r[0] | r[1] | r[2] | r[3]) & kLpmExt) != 0u) == 0) continue;
            uint32_t t[U];
#pragma unroll
            for (uint32_t j = 0; j < U; ++j) {
                const uint64_t at = uint64_t(r[j] & kLpmValue) << 8 | ((adr[j] >> sh) & 0xFFu);
                t[j] = *((r[j] & kLpmExt) ? grp + at : a.stage);
            }
            __builtin_amdgcn_sched_barrier(0);  // (the scheduler otherwise consumes the first load before the last is issued)
#pragma unroll
            for (uint32_t j = 0; j < U; ++j)
                if (r[j] & kLpmExt) r[j] = t[j];
        }

        u32x4 out;
        uint32_t nib = 0;
#pragma unroll
        for (uint32_t j = 0; j < U; ++j) {
            const bool hit = (r[j] & kLpmHit) != 0u;
            out[j] = hit ? r[j] & kLpmValue : miss;
            nib |= hit ? 1u << j : 0u;
        }
        if (next) {
            uint32_t *q = next + i0;
            if (live == U) {
                __builtin_nontemporal_store(out, reinterpret_cast<u32x4 *>(q));
            } else {
#pragma unroll
                for (uint32_t j = 0; j < U; ++j)
                    if (j < live) q[j] = out[j];
            }
        }
        if (hit_bits) {  // (uniform) a dead chain's bit is 0; the row's word is written if it starts inside the batch
            const uint32_t lo = row_or_scan(c < 8u ? nib << (4u * c) : 0u);
            const uint32_t hi = row_or_scan(c >= 8u ? nib << (4u * (c - 8u)) : 0u);
            const uint64_t word = uint64_t(tile) * (kLpmTile / 64) + (tid >> 4);
            if (c == 15u && word * 64 < n) hit_bits[word] = uint64_t(hi) << 32 | lo;
        }
    }
}

}  // namespace dev

namespace {

bool aligned16(const void *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// Both LDS instantiations may take the staged image's dynamic LDS (once per process).
int prepare_lpm_kernels() {
    static std::once_flag once;
    static hipError_t err = hipSuccess;
    std::call_once(once, [] {
        for (const void *f : {reinterpret_cast<const void *>(dev::k_lpm<dev::kLpmDense, true>),
                              reinterpret_cast<const void *>(dev::k_lpm<dev::kLpmKeys, true>)}) {
            const hipError_t e =
                hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(kLdsBytes));
            if (e != hipSuccess) err = e;
        }
    });
    if (err != hipSuccess) {
        set_last_error(std::string("hipFuncSetAttribute(LDS): ") + hipGetErrorString(err));
        return NFFACL_ERR_HIP;
    }
    return NFFACL_OK;
}

template <int SRC>
int lpm_lookup(nffacl_lpm *lpm, const void *d_src, uint64_t n, uint32_t flags, uint32_t miss, uint32_t *d_next,
               uint64_t *d_hit_bits, void *stream) {
    constexpr uint32_t known = NFFACL_LPM_SWAP_BYTES | NFFACL_LPM_FORCE_LDS | NFFACL_LPM_FORCE_GLOBAL;
    constexpr uint32_t both = NFFACL_LPM_FORCE_LDS | NFFACL_LPM_FORCE_GLOBAL;
    if (!lpm || (flags & ~known) != 0 || (flags & both) == both || n >> 32 || (!d_next && !d_hit_bits))
        return NFFACL_ERR_INVALID_ARG;
    if (!aligned16(d_src) || !aligned16(d_next) || !aligned16(d_hit_bits)) return NFFACL_ERR_INVALID_ARG;
    std::shared_ptr<LpmTable> t;  // held while the launch is enqueued
    uint32_t cus = 0;
    int device = 0;
    {
        std::lock_guard<std::mutex> g(lpm->mu);
        if (lpm->dev) t = lpm->dev->active, cus = lpm->dev->num_cus, device = lpm->dev->device;
    }
    if (!t) {
        set_last_error("LPM lookup before any nffacl_lpm_commit");
        return NFFACL_ERR_INVALID_ARG;
    }
    if (n == 0) return NFFACL_OK;
    if (!d_src) return NFFACL_ERR_INVALID_ARG;
    HIP_TRY(hipSetDevice(device));
    const bool lds = (flags & NFFACL_LPM_FORCE_LDS) || (!(flags & NFFACL_LPM_FORCE_GLOBAL) && n >= kLpmLdsMinN);
    const LpmLayout &L = t->lay;
    const dev::LpmArgs a{t->d_blob + L.off_l0, t->d_blob + L.off_l1, t->d_blob + L.off_l2, L.hops,
                         L.stage_dwords / 4};
    const uint32_t tiles = static_cast<uint32_t>((n + kLpmTile - 1) / kLpmTile);  // <= 2^20
    const uint32_t swap = flags & NFFACL_LPM_SWAP_BYTES;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (lds) {
        // the staged image leaves room for one workgroup per CU
        const int st = prepare_lpm_kernels();
        if (st != NFFACL_OK) return st;
        hipLaunchKernelGGL((dev::k_lpm<SRC, true>), dim3(std::min(tiles, cus)), dim3(kLpmBlock),
                           size_t(L.stage_dwords) * 4, s, d_src, n, a, swap, miss, d_next, d_hit_bits, tiles);
    } else {
        hipLaunchKernelGGL((dev::k_lpm<SRC, false>), dim3(std::min(tiles, 2 * cus)), dim3(kLpmBlock), 0, s, d_src, n,
                           a, swap, miss, d_next, d_hit_bits, tiles);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(t->note_use(s));
    return NFFACL_OK;
}

}  // namespace
}  // namespace nffacl

using namespace nffacl;

extern "C" {

int nffacl_lpm_commit(nffacl_lpm *lpm, int hip_device) {
    if (!lpm) return NFFACL_ERR_INVALID_ARG;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        (void)hipGetLastError();
        set_last_error("no HIP device visible");
        return NFFACL_ERR_NO_DEVICE;
    }
    if (hip_device < 0 || hip_device >= count) return NFFACL_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(lpm->mu);
    if (lpm->dev && lpm->dev->device != hip_device) {
        set_last_error("an LPM table stays on the device of its first commit");
        return NFFACL_ERR_INVALID_ARG;
    }
    std::vector<uint32_t> words;
    auto t = std::make_shared<LpmTable>();
    const int st = lpm_compile(lpm->rules, words, t->lay);
    if (st != NFFACL_OK) return st;
    HIP_TRY(hipSetDevice(hip_device));
    if (!lpm->dev) {
        LpmDevice *d = new (std::nothrow) LpmDevice();
        if (!d) return NFFACL_ERR_NOMEM;
        d->device = hip_device;
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, hip_device) == hipSuccess && cus > 0)
            d->num_cus = static_cast<uint32_t>(cus);
        const hipError_t e = d->home.init(hip_device);
        if (e != hipSuccess) {
            set_last_error(std::string("LPM table stream: ") + hipGetErrorString(e));
            delete d;
            return NFFACL_ERR_HIP;
        }
        lpm->dev = d;
    }
    lpm->dev->home.reap(false);
    HIP_TRY(t->upload(&lpm->dev->home, words.data(), words.size()));
    lpm->dev->active = std::move(t);  // the table before it retires behind its launches
    return NFFACL_OK;
}

int nffacl_lpm_lookup_device(nffacl_lpm *lpm, const uint32_t *d_addr, uint64_t n, uint32_t flags,
                             uint32_t miss_value, uint32_t *d_next, uint64_t *d_hit_bits, void *stream) {
    return lpm_lookup<dev::kLpmDense>(lpm, d_addr, n, flags, miss_value, d_next, d_hit_bits, stream);
}

int nffacl_lpm_lookup_keys_device(nffacl_lpm *lpm, const nffacl_key *d_keys, uint64_t n, uint32_t flags,
                                  uint32_t miss_value, uint32_t *d_next, uint64_t *d_hit_bits, void *stream) {
    return lpm_lookup<dev::kLpmKeys>(lpm, d_keys, n, flags, miss_value, d_next, d_hit_bits, stream);
}

}  // extern "C"
