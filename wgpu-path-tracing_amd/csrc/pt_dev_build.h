// pt_dev_build.h — what the two device builders (gpu_tree.hip, own_tree_gpu.hip) share on the host: the scratch of one build, owned by
// scope (pt_dev_scratch.h), and the radix sort of their Morton keys.
#pragma once
#include "pt_dev_scratch.h"
#include <hipcub/hipcub.hpp>

#include <stdint.h>

// n 64-bit keys (30-bit Morton code << 32 | index: bits 62 and 63 are never set) sorted ascending on stream s, in -> out, in scratch the caller provides:
// at least pt_sort_keys_bytes of it. Nothing is allocated here, so the caller may size one buffer for this and its other hipCUB calls.
inline hipError_t pt_sort_keys_bytes(size_t &bytes, uint32_t n, hipStream_t s) {
    unsigned long long *none = nullptr;
    return hipcub::DeviceRadixSort::SortKeys(nullptr, bytes, none, none, (int)n, 0, 62, s);
}
inline hipError_t pt_sort_keys(void *tmp, size_t tmp_bytes, const unsigned long long *in, unsigned long long *out, uint32_t n, hipStream_t s) {
    return hipcub::DeviceRadixSort::SortKeys(tmp, tmp_bytes, in, out, (int)n, 0, 62, s);
}
