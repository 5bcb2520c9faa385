// pt_dev_build.h — what the two device builders (gpu_tree.hip, own_tree_gpu.hip) share on the host: the scratch of one build, owned by
// scope, and the radix sort of their Morton keys.
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <stdint.h>
#include <vector>

inline bool hip_ok(hipError_t e) { return e == hipSuccess; }

// Every hipMalloc of one build: all freed when it goes out of scope. The owner sees to it that nothing on the stream still uses them then.
struct DevScratch {
    std::vector<void *> owned;
    bool failed = false;                       // an allocation failed (its get() returned nullptr): checked once per group of them
    DevScratch() = default;
    DevScratch(const DevScratch &) = delete;
    DevScratch &operator=(const DevScratch &) = delete;
    ~DevScratch() { for (void *p : owned) (void)hipFree(p); }
    template <class T> T *get(size_t n) {
        void *p = nullptr;
        if (!hip_ok(hipMalloc(&p, n * sizeof(T)))) { failed = true; return nullptr; }
        owned.push_back(p);
        return static_cast<T *>(p);
    }
    template <class T> T *keep(T *p) {         // hand one out: it is no longer freed here
        owned.erase(std::remove(owned.begin(), owned.end(), static_cast<void *>(p)), owned.end());
        return p;
    }
    template <class... P> void drop(P *...p) { // free some early (lowers the peak); nullptr: nothing
        for (void *q : {static_cast<void *>(p)...}) if (q) (void)hipFree(keep(q));
    }
};

// n 64-bit keys (30-bit Morton code << 32 | index: bits 62 and 63 are never set) sorted ascending on stream s, in -> out, in scratch the caller provides:
// at least pt_sort_keys_bytes of it. Nothing is allocated here, so the caller may size one buffer for this and its other hipCUB calls.
inline hipError_t pt_sort_keys_bytes(size_t &bytes, uint32_t n, hipStream_t s) {
    unsigned long long *none = nullptr;
    return hipcub::DeviceRadixSort::SortKeys(nullptr, bytes, none, none, (int)n, 0, 62, s);
}
inline hipError_t pt_sort_keys(void *tmp, size_t tmp_bytes, const unsigned long long *in, unsigned long long *out, uint32_t n, hipStream_t s) {
    return hipcub::DeviceRadixSort::SortKeys(tmp, tmp_bytes, in, out, (int)n, 0, 62, s);
}
