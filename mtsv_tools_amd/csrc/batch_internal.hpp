// batch_internal.hpp -- what batch.hip and batch_pass.hip share and nobody else needs.
#pragma once
#include <algorithm>

#include "batch.hpp"

namespace mtsv {

// bytes (may be null): Batch::bytes, where the allocation counts towards it
template <class T>
void dev_alloc(T** p, uint64_t count, uint64_t* bytes = nullptr) {
    uint64_t b = std::max<uint64_t>(count, 1) * sizeof(T);
    HIP_CHECK(hipMalloc((void**)p, b));
    if (bytes) *bytes += b;
}

}  // namespace mtsv
