// route.hip — stable partition of a verdict vector into per-output index lists
// (the output slices of segmentProcess, flow/flow.go:1462-1486), on the GPU.
//
// Three launches on the caller's stream, none of which waits on another
// workgroup (route.hpp has the layout of the count matrix):
//   k_route_count<KB>    one workgroup per tile: wave-level multisplit of the
//                        tile's keys into per-bucket counts
//   k_route_scan         one workgroup: exclusive scan of the count matrix in
//                        place, and d_offsets
//   k_route_scatter<KB>  one workgroup per tile: re-reads the tile's keys, ranks
//                        every packet inside its bucket, sorts the tile's
//                        indices through LDS and writes them as contiguous runs
// KB is the number of key bits (1, 2, 4, 8).  Buckets that fit two bits are
// split with one ballot per bucket value and wave-uniform counters; wider keys
// build each lane's peer mask (the lanes holding the same key) from KB
// ballots, and the lowest lane of a peer group does the group's one LDS update.
//
// Position order inside a tile is (wave, round, lane): position
// wave * 512 + round * 64 + lane, so every load instruction of a wave reads 64
// consecutive keys and ascending position is ascending packet index.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <string>

#include "devutil.hpp"
#include "nffacl.h"
#include "route.hpp"

namespace nffacl {
namespace dev {

constexpr uint32_t kWaves = kRouteBlock / 64;

__device__ __forceinline__ uint32_t rank_below(uint64_t m) {  // set bits of m below this lane
    return __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0u));
}

// The wave's buckets of its 8 rounds of tile `tile`; bit r of `live` says
// round r's packet exists (index < n).  Dead rounds get bucket 0 and take no
// part in any count.
__device__ __forceinline__ void load_buckets(const uint32_t *__restrict__ port, uint32_t n, uint32_t first,
                                             uint32_t sep, uint32_t n_out, uint32_t (&k)[kRouteRounds],
                                             uint32_t &live) {
    uint32_t p[kRouteRounds];
    live = 0;
#pragma unroll
    for (uint32_t r = 0; r < kRouteRounds; ++r) {
        const uint32_t i = first + 64u * r;
        const bool ok = i < n;
        p[r] = ok ? port[i] : 0u;
        live |= uint32_t(ok) << r;
    }
#pragma unroll
    for (uint32_t r = 0; r < kRouteRounds; ++r) {
        const uint32_t b = sep ? uint32_t(p[r] != 0u) : min(p[r], n_out);
        k[r] = (live >> r) & 1u ? b : 0u;
    }
}

// The live lanes of the wave holding this lane's key.
template <int KB>
__device__ __forceinline__ uint64_t peers(uint32_t k, bool ok) {
    uint64_t m = ballot(ok);
#pragma unroll
    for (int b = 0; b < KB; ++b) {
        const bool bit = (k >> b) & 1u;
        const uint64_t s = ballot(bit);
        m &= bit ? s : ~s;
    }
    return m;
}

// Per-bucket counts of the wave's 8 rounds, wave-uniform (KB <= 2).
template <uint32_t KN>
__device__ __forceinline__ void ballot_counts(const uint32_t (&k)[kRouteRounds], uint32_t live, uint32_t (&c)[KN]) {
#pragma unroll
    for (uint32_t v = 0; v < KN; ++v) c[v] = 0;
#pragma unroll
    for (uint32_t r = 0; r < kRouteRounds; ++r)
#pragma unroll
        for (uint32_t v = 0; v < KN; ++v) c[v] += __popcll(ballot(((live >> r) & 1u) && k[r] == v));
}

template <int KB>
__global__ __launch_bounds__(kRouteBlock) void k_route_count(const uint32_t *__restrict__ port, uint32_t n,
                                                             uint32_t sep, uint32_t n_out, uint32_t tiles,
                                                             uint32_t *__restrict__ counts) {
    constexpr uint32_t KN = 1u << KB;
    const uint32_t lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t tile = blockIdx.x;
    uint32_t k[kRouteRounds], live;
    load_buckets(port, n, tile * kRouteTile + wave * (64u * kRouteRounds) + lane, sep, n_out, k, live);
    if constexpr (KB <= 2) {
        __shared__ uint32_t wcnt[kWaves][KN];
        uint32_t c[KN];
        ballot_counts<KN>(k, live, c);
#pragma unroll
        for (uint32_t v = 0; v < KN; ++v)
            if (lane == v) wcnt[wave][v] = c[v];
        __syncthreads();
        if (threadIdx.x <= n_out) {
            uint32_t s = 0;
#pragma unroll
            for (uint32_t w = 0; w < kWaves; ++w) s += wcnt[w][threadIdx.x];
            counts[threadIdx.x * tiles + tile] = s;
        }
    } else {
        __shared__ uint32_t hist[KN];
        if (threadIdx.x < KN) hist[threadIdx.x] = 0;
        __syncthreads();
#pragma unroll
        for (uint32_t r = 0; r < kRouteRounds; ++r) {
            const bool ok = (live >> r) & 1u;
            const uint64_t m = peers<KB>(k[r], ok);
            if (ok && rank_below(m) == 0) atomicAdd(&hist[k[r]], static_cast<uint32_t>(__popcll(m)));
        }
        __syncthreads();
        if (threadIdx.x <= n_out) counts[threadIdx.x * tiles + tile] = hist[threadIdx.x];
    }
}

// Exclusive scan of counts[0, buckets * tiles) in place, one workgroup: every
// thread sums its own chunk, the chunk sums are scanned (DPP inside a wave,
// LDS across the 16 waves), every thread rewrites its chunk.  offsets[b] is
// the scanned value at bucket b's first tile; offsets[buckets] = n.
__global__ __launch_bounds__(kRouteBlock) void k_route_scan(uint32_t *counts, uint32_t tiles, uint32_t buckets,
                                                            uint32_t n, uint32_t *__restrict__ offsets) {
    __shared__ uint32_t wsum[kWaves];
    const uint32_t tid = threadIdx.x, lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t total = tiles * buckets;  // <= 2^18 * 256
    const uint32_t chunk = (total + kRouteBlock - 1) / kRouteBlock;
    const uint32_t lo = min(tid * chunk, total), hi = min(lo + chunk, total);
    uint32_t sum = 0;
    for (uint32_t i = lo; i < hi; ++i) sum += counts[i];
    const uint32_t incl = wave_scan_incl(sum);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t run = incl - sum;
    for (uint32_t w = 0; w < wave; ++w) run += wsum[w];
    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t c = counts[i];
        counts[i] = run;
        run += c;
    }
    __syncthreads();
    if (tid <= buckets) offsets[tid] = (tid < buckets && tiles) ? counts[tid * tiles] : n;
}

template <int KB>
__global__ __launch_bounds__(kRouteBlock) void k_route_scatter(const uint32_t *__restrict__ port, uint32_t n,
                                                               uint32_t sep, uint32_t n_out, uint32_t tiles,
                                                               const uint32_t *__restrict__ starts,
                                                               uint32_t *__restrict__ index) {
    constexpr uint32_t KN = 1u << KB;
    __shared__ uint32_t cnt[kWaves][KN];   // A: (wave, key) counts; after B: the (wave, key)'s tile-local start
    __shared__ uint32_t kstart[KN];        // key totals, then the key's tile-local start
    __shared__ uint32_t goff[KN];          // the key's first position in d_index for this tile, minus kstart
    __shared__ uint32_t stage[kRouteTile]; // sorted tile: key << 16 | position
    const uint32_t tid = threadIdx.x, lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t tile = blockIdx.x;
    const uint32_t pos0 = wave * (64u * kRouteRounds) + lane;
    uint32_t k[kRouteRounds], live;
    load_buckets(port, n, tile * kRouteTile + pos0, sep, n_out, k, live);

    // A: counts per (wave, key), and every packet's rank among the wave's
    // packets of its key (in position order); a wave touches its own row only
    uint32_t posw[kRouteRounds];
    if constexpr (KB <= 2) {
        uint32_t c[KN];
#pragma unroll
        for (uint32_t v = 0; v < KN; ++v) c[v] = 0;
#pragma unroll
        for (uint32_t r = 0; r < kRouteRounds; ++r) {
            posw[r] = 0;
#pragma unroll
            for (uint32_t v = 0; v < KN; ++v) {
                const uint64_t m = ballot(((live >> r) & 1u) && k[r] == v);
                if (k[r] == v) posw[r] = c[v] + rank_below(m);
                c[v] += __popcll(m);
            }
        }
#pragma unroll
        for (uint32_t v = 0; v < KN; ++v)
            if (lane == v) cnt[wave][v] = c[v];
    } else {
        // (volatile: lanes of the wave read what other lanes of it stored, in program order)
        volatile uint32_t *row = cnt[wave];
        for (uint32_t i = lane; i < KN; i += 64) row[i] = 0;
#pragma unroll
        for (uint32_t r = 0; r < kRouteRounds; ++r) {
            const bool ok = (live >> r) & 1u;
            const uint64_t m = peers<KB>(k[r], ok);
            const uint32_t rank = rank_below(m);
            const uint32_t before = row[k[r]];  // the whole peer group reads one address
            if (ok && rank == 0) row[k[r]] = before + static_cast<uint32_t>(__popcll(m));
            posw[r] = before + rank;
        }
    }
    __syncthreads();

    // B: key totals, their exclusive scan (wave 0), then every column's scan across the waves
    if (tid < KN) {
        uint32_t s = 0;
#pragma unroll
        for (uint32_t w = 0; w < kWaves; ++w) s += cnt[w][tid];
        kstart[tid] = s;
    }
    __syncthreads();
    if (wave == 0) {
        constexpr uint32_t PER = KN > 64 ? KN / 64 : 1;
        uint32_t v[PER], s = 0;
#pragma unroll
        for (uint32_t i = 0; i < PER; ++i) {
            const uint32_t key = lane * PER + i;
            v[i] = key < KN ? kstart[key] : 0u;
            s += v[i];
        }
        uint32_t run = wave_scan_incl(s) - s;
#pragma unroll
        for (uint32_t i = 0; i < PER; ++i) {
            const uint32_t key = lane * PER + i;
            if (key < KN) kstart[key] = run;
            run += v[i];
        }
    }
    __syncthreads();
    if (tid < KN) {
        uint32_t run = kstart[tid];
        goff[tid] = (tid <= n_out ? starts[tid * tiles + tile] : 0u) - run;
#pragma unroll
        for (uint32_t w = 0; w < kWaves; ++w) {
            const uint32_t c = cnt[w][tid];
            cnt[w][tid] = run;
            run += c;
        }
    }
    __syncthreads();

    // C: a packet's tile-local sorted position = its (wave, key)'s start + its rank from A
#pragma unroll
    for (uint32_t r = 0; r < kRouteRounds; ++r)
        if ((live >> r) & 1u) stage[cnt[wave][k[r]] + posw[r]] = k[r] << 16 | (pos0 + 64u * r);
    __syncthreads();

    // D: sorted position j goes out; consecutive j of one key are consecutive in d_index
    const uint32_t tile_n = min(kRouteTile, n - tile * kRouteTile);
#pragma unroll
    for (uint32_t i = 0; i < kRouteRounds; ++i) {
        const uint32_t j = tid + i * kRouteBlock;
        if (j < tile_n) {
            const uint32_t e = stage[j];
            const uint32_t dst = goff[e >> 16] + j;
            if (dst < n) index[dst] = tile * kRouteTile + (e & 0xffffu);  // (always; never a store past d_index)
        }
    }
}

// Output slot j = slot index[j]: stride / 16 lanes per packet, 16 bytes each;
// the gathered side is read once (nontemporal), the dense side is lane g.
__global__ __launch_bounds__(256) void k_route_gather(const u32x4 *__restrict__ slots, uint32_t lpp, int shift,
                                                      const uint32_t *__restrict__ index, uint64_t lanes,
                                                      u32x4 *__restrict__ out) {
    for (uint64_t g = uint64_t(blockIdx.x) * 256 + threadIdx.x; g < lanes; g += uint64_t(gridDim.x) * 256) {
        const uint64_t pkt = shift >= 0 ? g >> shift : g / lpp;
        const uint32_t c = static_cast<uint32_t>(g - pkt * lpp);
        out[g] = __builtin_nontemporal_load(slots + uint64_t(index[pkt]) * lpp + c);
    }
}

}  // namespace dev

namespace {

template <int KB>
void launch_tiles(const nffacl_router *r, const uint32_t *d_port, uint32_t n, uint32_t tiles, uint32_t *d_index,
                  uint32_t *d_offsets, hipStream_t s) {
    const uint32_t sep = r->mode == NFFACL_ROUTE_SEPARATE;
    if (tiles)
        hipLaunchKernelGGL(dev::k_route_count<KB>, dim3(tiles), dim3(kRouteBlock), 0, s, d_port, n, sep, r->n_out, tiles,
                           r->d_counts);
    hipLaunchKernelGGL(dev::k_route_scan, dim3(1), dim3(kRouteBlock), 0, s, r->d_counts, tiles, r->n_out + 1, n,
                       d_offsets);
    if (tiles)
        hipLaunchKernelGGL(dev::k_route_scatter<KB>, dim3(tiles), dim3(kRouteBlock), 0, s, d_port, n, sep, r->n_out,
                           tiles, r->d_counts, d_index);
}

}  // namespace
}  // namespace nffacl

using namespace nffacl;

extern "C" {

int nffacl_route_plan(uint64_t n, uint32_t n_out, uint64_t *tiles, uint64_t *scratch_bytes) {
    if (!tiles || !scratch_bytes || n > kRouteMaxN || n_out < 1 || n_out > kRouteMaxOut) return NFFACL_ERR_INVALID_ARG;
    *tiles = (n + kRouteTile - 1) / kRouteTile;
    *scratch_bytes = *tiles * (n_out + 1) * sizeof(uint32_t);
    return NFFACL_OK;
}

int nffacl_router_create(int hip_device, uint32_t mode, uint32_t n_out, uint64_t max_n, nffacl_router **out) {
    if (!out) return NFFACL_ERR_INVALID_ARG;
    *out = nullptr;
    if (mode != NFFACL_ROUTE_SEPARATE && mode != NFFACL_ROUTE_SPLIT) return NFFACL_ERR_INVALID_ARG;
    if (mode == NFFACL_ROUTE_SEPARATE && n_out != 2) return NFFACL_ERR_INVALID_ARG;
    uint64_t tiles = 0, bytes = 0, ftiles = 0, fbytes = 0;
    if (nffacl_route_plan(max_n, n_out, &tiles, &bytes) != NFFACL_OK) return NFFACL_ERR_INVALID_ARG;
    if (nffacl_route_frames_plan(max_n, &ftiles, &fbytes) != NFFACL_OK) return NFFACL_ERR_INVALID_ARG;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        (void)hipGetLastError();
        set_last_error("no HIP device visible");
        return NFFACL_ERR_NO_DEVICE;
    }
    if (hip_device < 0 || hip_device >= count) return NFFACL_ERR_INVALID_ARG;
    HIP_TRY(hipSetDevice(hip_device));
    nffacl_router *r = new (std::nothrow) nffacl_router();
    if (!r) return NFFACL_ERR_NOMEM;
    r->device = hip_device;
    r->mode = mode;
    r->n_out = n_out;
    r->max_n = max_n;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&r->d_counts), std::max<uint64_t>(bytes, sizeof(uint32_t)));
    if (e == hipSuccess)
        e = hipMalloc(reinterpret_cast<void **>(&r->d_fsums), std::max<uint64_t>(fbytes, sizeof(uint64_t)));
    if (e == hipSuccess) e = hipEventCreateWithFlags(&r->last, hipEventDisableTiming);
    if (e != hipSuccess) {
        set_last_error(std::string("router scratch: ") + hipGetErrorString(e));
        nffacl_router_destroy(r);
        return e == hipErrorOutOfMemory ? NFFACL_ERR_NOMEM : NFFACL_ERR_HIP;
    }
    *out = r;
    return NFFACL_OK;
}

int nffacl_route_device(nffacl_router *r, const uint32_t *d_port, uint64_t n, uint32_t *d_index, uint32_t *d_offsets,
                        void *stream) {
    if (!r || !d_index || !d_offsets || (!d_port && n) || n > r->max_n) return NFFACL_ERR_INVALID_ARG;
    HIP_TRY(hipSetDevice(r->device));
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const uint32_t n32 = static_cast<uint32_t>(n);  // max_n <= 2^31
    const uint32_t tiles = (n32 + kRouteTile - 1) / kRouteTile;
    switch (route_key_bits(r->n_out)) {
    case 1: launch_tiles<1>(r, d_port, n32, tiles, d_index, d_offsets, s); break;
    case 2: launch_tiles<2>(r, d_port, n32, tiles, d_index, d_offsets, s); break;
    case 4: launch_tiles<4>(r, d_port, n32, tiles, d_index, d_offsets, s); break;
    default: launch_tiles<8>(r, d_port, n32, tiles, d_index, d_offsets, s); break;
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(r->last, s));
    r->used = true;
    return NFFACL_OK;
}

int nffacl_route_gather_device(const uint8_t *d_slots, uint32_t stride, const uint32_t *d_index, uint64_t m,
                               uint8_t *d_out, void *stream) {
    if (stride < 64 || (stride % 16) != 0 || m > kRouteMaxN) return NFFACL_ERR_INVALID_ARG;
    if (m == 0) return NFFACL_OK;
    if (!d_slots || !d_index || !d_out || (reinterpret_cast<uintptr_t>(d_slots) % 16) != 0 ||
        (reinterpret_cast<uintptr_t>(d_out) % 16) != 0)
        return NFFACL_ERR_INVALID_ARG;
    const uint32_t lpp = stride / 16;
    const int shift = (lpp & (lpp - 1)) == 0 ? __builtin_ctz(lpp) : -1;
    const uint64_t lanes = m * lpp;
    const uint32_t grid = static_cast<uint32_t>(std::min<uint64_t>((lanes + 255) / 256, uint64_t(1) << 20));
    hipLaunchKernelGGL(dev::k_route_gather, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const dev::u32x4 *>(d_slots), lpp, shift, d_index, lanes,
                       reinterpret_cast<dev::u32x4 *>(d_out));
    HIP_TRY(hipGetLastError());
    return NFFACL_OK;
}

void nffacl_router_destroy(nffacl_router *r) {
    if (!r) return;
    (void)hipSetDevice(r->device);
    // the scratch is freed behind the last launch that used it, and behind nothing else
    if (r->last) {
        if (r->used) (void)hipEventSynchronize(r->last);
        (void)hipEventDestroy(r->last);
    }
    if (r->d_counts) (void)hipFree(r->d_counts);
    if (r->d_fsums) (void)hipFree(r->d_fsums);
    (void)hipGetLastError();
    delete r;
}

}  // extern "C"
