// launch.hpp — how a compiled table is launched (internal): the kernel
// arguments, walk and launch shape engine.hip derives from a DevTable, shared
// with the key kernels (keys.hip), which walk the same tables.
#pragma once

#include <cstddef>
#include <cstdint>

#include "classify.hpp"
#include "engine.hpp"

namespace nffacl {

// LDS budget per workgroup for a staged table (gfx950: 160 KiB per CU).
constexpr size_t kLdsBytes = 160 * 1024;

struct IndexedLaunch {
    int tm;  // dev::TableMode
    int ns;
    uint32_t block, per_cu;
    size_t lds_bytes;
};

// All defined in engine.hip.
uint32_t grid_for(const nffacl_engine *eng, uint64_t n, uint32_t block, uint32_t per_cu);
dev::IndexedArgs indexed_args(const DevTable *t);
bool table_consistent(const DevTable *t);
IndexedLaunch indexed_launch(const nffacl_engine *eng, const DevTable *t);

}  // namespace nffacl
