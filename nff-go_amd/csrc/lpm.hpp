// lpm.hpp — longest-prefix-match route tables (internal; lpm.cpp, lpm.hip).
//
// The reference's LPM (packet/packet.go:857-912) is DPDK's DIR-24-8: a 64 MB
// tbl24 and tbl8 groups, one scattered HBM sector per address whatever the
// table holds.  The device table here is 16-8-8 with its top level in LDS:
//
//   L0    65 536 u16, indexed by address bits 31..16.  0: miss.  1..H: a leaf,
//         answer word hops[e].  > H: level-1 group e - H - 1.
//   hops  H + 1 answer words (kLpmHit | next hop; hops[0] = 0, the miss), padded
//         to a multiple of 4 dwords.  H <= kLpmMaxHops.  L0 and hops are
//         contiguous: the image a workgroup stages into LDS.
//   L1    groups of 256 u32 indexed by bits 15..8, in ascending /16 order.
//   L2    groups of 256 u32 indexed by bits 7..0, in the order the L1 entries
//         that point at them appear.
// An L1 / L2 word: kLpmHit | 24-bit next hop, kLpmExt | level-2 group number
// (L1 only), or 0 (miss).  A /16 block whose next hop got no code (more than
// kLpmMaxHops distinct hops among the L0 leaves) is expanded into an L1 group
// of leaves, so the walk has one leaf form.
//
// Blob, in dwords: [0] kLpmMagic  [1] H  [2] L1 groups  [3] L2 groups
// [4] off_l0 (= kLpmHeaderDwords)  [5] off_hops  [6] off_l1  [7] off_l2;
// every offset a multiple of 4.
#pragma once

#include <cstdint>
#include <map>
#include <mutex>
#include <vector>

namespace nffacl {

constexpr uint32_t kLpmMagic = 0x314D504Cu;  // "LPM1"
constexpr uint32_t kLpmHeaderDwords = 8;
constexpr uint32_t kLpmL0Dwords = 65536 / 2;
constexpr uint32_t kLpmMaxHops = 4095;
constexpr uint32_t kLpmHit = 1u << 31;
constexpr uint32_t kLpmExt = 1u << 30;
constexpr uint32_t kLpmValue = 0x00FFFFFFu;

// A tile is kLpmTile consecutive addresses, kLpmPerLane per thread of a
// kLpmBlock workgroup.
constexpr uint32_t kLpmBlock = 1024;
constexpr uint32_t kLpmPerLane = 4;
constexpr uint32_t kLpmTile = kLpmBlock * kLpmPerLane;

struct LpmLayout {
    uint32_t hops = 0, n_l1 = 0, n_l2 = 0;
    uint32_t off_l0 = 0, off_hops = 0, off_l1 = 0, off_l2 = 0;
    uint32_t stage_dwords = 0;  // L0 + hops
    uint64_t blob_dwords = 0;
};

// Rules keyed by depth << 32 | masked ip (ascending depth) -> next hop.
using LpmRules = std::map<uint64_t, uint32_t>;

// The device table of `rules` (expansion, longest depth wins).
// NFFACL_ERR_NOMEM when the level-1 groups do not fit the u16 code space.
int lpm_compile(const LpmRules &rules, std::vector<uint32_t> &blob, LpmLayout &lay);

struct LpmDevice;  // lpm.hip: the committed table and its home
void lpm_device_destroy(LpmDevice *d);

}  // namespace nffacl

struct nffacl_lpm {
    std::mutex mu;
    uint32_t max_rules = 0, number_tbl8 = 0;
    nffacl::LpmRules rules;
    std::map<uint32_t, uint32_t> deep;  // /24 block -> its prefixes longer than 24
    nffacl::LpmDevice *dev = nullptr;
};
