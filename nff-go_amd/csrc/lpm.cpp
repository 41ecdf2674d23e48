// lpm.cpp — the host side of the LPM route table (nffacl.h, nffacl_lpm_*):
// the rule list with the reference's statuses, and the compiler from that
// list to the 16-8-8 device table (lpm.hpp).  No device code: the commit and
// the lookups are lpm.hip.
#include "lpm.hpp"

#include <array>
#include <cstring>
#include <new>
#include <string>

#include "nffacl.h"

namespace nffacl {

void set_last_error(const std::string &s);

namespace {

using Group = std::array<uint32_t, 256>;

uint32_t depth_mask(uint32_t depth) { return depth >= 32 ? 0xFFFFFFFFu : ~(0xFFFFFFFFu >> depth); }

}  // namespace

// Rules come in ascending depth, so a fill never meets a deeper rule's work:
// it overwrites what shorter prefixes left, and a group opened by a longer
// prefix is seeded with the entry that covered it.
int lpm_compile(const LpmRules &rules, std::vector<uint32_t> &blob, LpmLayout &lay) {
    std::vector<uint32_t> top(65536, 0u);  // answer words; kLpmExt | creation number of the block's L1 group
    std::vector<Group> l1, l2;             // in creation order; renumbered on the way out
    auto open_l1 = [&](uint32_t b) -> Group & {
        if (!(top[b] & kLpmExt)) {
            Group g;
            g.fill(top[b]);
            l1.push_back(g);
            top[b] = kLpmExt | static_cast<uint32_t>(l1.size() - 1);
        }
        return l1[top[b] & kLpmValue];
    };
    for (const auto &kv : rules) {
        const uint32_t depth = static_cast<uint32_t>(kv.first >> 32), ip = static_cast<uint32_t>(kv.first);
        const uint32_t leaf = kLpmHit | (kv.second & kLpmValue);
        if (depth <= 16) {
            const uint32_t b = ip >> 16, cnt = 1u << (16 - depth);
            for (uint32_t k = 0; k < cnt; ++k) top[b + k] = leaf;
        } else if (depth <= 24) {
            Group &g = open_l1(ip >> 16);
            const uint32_t i = (ip >> 8) & 0xFFu, cnt = 1u << (24 - depth);
            for (uint32_t k = 0; k < cnt; ++k) g[i + k] = leaf;
        } else {
            uint32_t &e = open_l1(ip >> 16)[(ip >> 8) & 0xFFu];
            if (!(e & kLpmExt)) {
                if (l2.size() > kLpmValue) return NFFACL_ERR_NOMEM;
                Group g;
                g.fill(e);
                l2.push_back(g);
                e = kLpmExt | static_cast<uint32_t>(l2.size() - 1);
            }
            Group &g = l2[e & kLpmValue];
            const uint32_t i = ip & 0xFFu, cnt = 1u << (32 - depth);
            for (uint32_t k = 0; k < cnt; ++k) g[i + k] = leaf;
        }
    }
    // hop codes in order of first appearance among the L0 leaves; a leaf
    // whose hop gets none becomes a group of leaves
    std::map<uint32_t, uint32_t> code;
    std::vector<uint32_t> hops{0u};
    for (uint32_t b = 0; b < 65536; ++b) {
        const uint32_t e = top[b];
        if (!(e & kLpmHit) || code.count(e)) continue;
        if (hops.size() > kLpmMaxHops) {
            open_l1(b);
            continue;
        }
        code[e] = static_cast<uint32_t>(hops.size());
        hops.push_back(e);
    }
    const uint32_t H = static_cast<uint32_t>(hops.size() - 1);
    if (l1.size() > 65535u - H) {
        set_last_error("LPM table needs " + std::to_string(l1.size()) + " level-1 groups beside " +
                       std::to_string(H) + " coded next hops: over 65535 together");
        return NFFACL_ERR_NOMEM;
    }
    while (hops.size() % 4) hops.push_back(0u);

    lay = LpmLayout{};
    lay.hops = H, lay.n_l1 = static_cast<uint32_t>(l1.size()), lay.n_l2 = static_cast<uint32_t>(l2.size());
    lay.off_l0 = kLpmHeaderDwords;
    lay.off_hops = lay.off_l0 + kLpmL0Dwords;
    lay.stage_dwords = kLpmL0Dwords + static_cast<uint32_t>(hops.size());
    lay.off_l1 = lay.off_hops + static_cast<uint32_t>(hops.size());
    const uint64_t off_l2 = uint64_t(lay.off_l1) + 256ull * lay.n_l1;
    lay.blob_dwords = off_l2 + 256ull * lay.n_l2;
    if (lay.blob_dwords >> 32) return NFFACL_ERR_NOMEM;
    lay.off_l2 = static_cast<uint32_t>(off_l2);

    blob.assign(lay.blob_dwords, 0u);
    const uint32_t head[kLpmHeaderDwords] = {kLpmMagic, H, lay.n_l1, lay.n_l2, lay.off_l0, lay.off_hops,
                                             lay.off_l1, lay.off_l2};
    std::memcpy(blob.data(), head, sizeof(head));
    std::memcpy(blob.data() + lay.off_hops, hops.data(), hops.size() * sizeof(uint32_t));
    uint16_t *l0 = reinterpret_cast<uint16_t *>(blob.data() + lay.off_l0);
    uint32_t g1 = 0, g2 = 0;  // groups leave in ascending address order
    for (uint32_t b = 0; b < 65536; ++b) {
        const uint32_t e = top[b];
        if (e & kLpmHit) {
            l0[b] = static_cast<uint16_t>(code[e]);
        } else if (e & kLpmExt) {
            l0[b] = static_cast<uint16_t>(H + 1 + g1);
            uint32_t *dst = blob.data() + lay.off_l1 + 256ull * g1++;
            const Group &g = l1[e & kLpmValue];
            for (uint32_t i = 0; i < 256; ++i) {
                dst[i] = g[i];
                if (g[i] & kLpmExt) {
                    dst[i] = kLpmExt | g2;
                    std::memcpy(blob.data() + lay.off_l2 + 256ull * g2++, l2[g[i] & kLpmValue].data(), sizeof(Group));
                }
            }
        }
    }
    return NFFACL_OK;
}

}  // namespace nffacl

using namespace nffacl;

extern "C" {

int nffacl_lpm_create(uint32_t max_rules, uint32_t number_tbl8, nffacl_lpm **out) {
    if (!out) return NFFACL_ERR_INVALID_ARG;
    *out = nullptr;
    if (max_rules == 0) return NFFACL_ERR_INVALID_ARG;
    nffacl_lpm *lpm = new (std::nothrow) nffacl_lpm();
    if (!lpm) return NFFACL_ERR_NOMEM;
    lpm->max_rules = max_rules;
    lpm->number_tbl8 = number_tbl8;
    *out = lpm;
    return NFFACL_OK;
}

int nffacl_lpm_add(nffacl_lpm *lpm, uint32_t ip, uint32_t depth, uint32_t next_hop) {
    if (!lpm || depth < 1 || depth > 32) return NFFACL_ERR_INVALID_ARG;
    const uint32_t masked = ip & depth_mask(depth);
    const uint64_t key = uint64_t(depth) << 32 | masked;
    std::lock_guard<std::mutex> g(lpm->mu);
    auto it = lpm->rules.find(key);
    if (it != lpm->rules.end()) {
        it->second = next_hop & kLpmValue;
        return NFFACL_OK;
    }
    if (lpm->rules.size() >= lpm->max_rules) return NFFACL_ERR_NOMEM;
    if (depth > 24) {
        auto blk = lpm->deep.find(masked >> 8);
        if (blk == lpm->deep.end()) {
            if (lpm->deep.size() >= lpm->number_tbl8) return NFFACL_ERR_NOMEM;
            lpm->deep[masked >> 8] = 1;
        } else {
            ++blk->second;
        }
    }
    lpm->rules[key] = next_hop & kLpmValue;
    return NFFACL_OK;
}

int nffacl_lpm_delete(nffacl_lpm *lpm, uint32_t ip, uint32_t depth) {
    if (!lpm || depth < 1 || depth > 32) return NFFACL_ERR_INVALID_ARG;
    const uint32_t masked = ip & depth_mask(depth);
    std::lock_guard<std::mutex> g(lpm->mu);
    auto it = lpm->rules.find(uint64_t(depth) << 32 | masked);
    if (it == lpm->rules.end()) return NFFACL_ERR_INVALID_ARG;
    lpm->rules.erase(it);
    if (depth > 24) {
        auto blk = lpm->deep.find(masked >> 8);
        if (blk != lpm->deep.end() && --blk->second == 0) lpm->deep.erase(blk);
    }
    return NFFACL_OK;
}

int nffacl_lpm_count(const nffacl_lpm *lpm, uint64_t *rules) {
    if (!lpm || !rules) return NFFACL_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(const_cast<nffacl_lpm *>(lpm)->mu);
    *rules = lpm->rules.size();
    return NFFACL_OK;
}

void nffacl_lpm_free(nffacl_lpm *lpm) {
    if (!lpm) return;
    if (lpm->dev) lpm_device_destroy(lpm->dev);
    delete lpm;
}

int nffacl_lpm_compile(const nffacl_lpm *lpm, uint32_t *blob, uint64_t cap_dwords, uint64_t *need_dwords) {
    if (!lpm || !need_dwords) return NFFACL_ERR_INVALID_ARG;
    std::vector<uint32_t> words;
    LpmLayout lay;
    int st;
    {
        std::lock_guard<std::mutex> g(const_cast<nffacl_lpm *>(lpm)->mu);
        st = lpm_compile(lpm->rules, words, lay);
    }
    if (st != NFFACL_OK) return st;
    *need_dwords = words.size();
    if (blob) {
        if (cap_dwords < words.size()) return NFFACL_ERR_INVALID_ARG;
        std::memcpy(blob, words.data(), words.size() * sizeof(uint32_t));
    }
    return NFFACL_OK;
}

}  // extern "C"
