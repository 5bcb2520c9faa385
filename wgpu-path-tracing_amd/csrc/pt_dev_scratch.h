// pt_dev_scratch.h — device allocations owned by scope: the scratch of one tree build (pt_dev_build.h), and the new buffers of a call that
// allocates and fills everything before it swaps (ptmi_set_triangle_groups, ptmi_set_skin). Host code; needs the HIP runtime and nothing else.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stddef.h>
#include <vector>

inline bool hip_ok(hipError_t e) { return e == hipSuccess; }

// Every hipMalloc of one build: all freed when it goes out of scope. The owner sees to it that nothing on the stream still uses them then.
struct DevScratch {
    std::vector<void *> owned;
    bool failed = false;                       // an allocation failed (its get() returned nullptr): checked once per group of them
    hipError_t error = hipSuccess;             // ... and what the first one that failed returned
    DevScratch() = default;
    DevScratch(const DevScratch &) = delete;
    DevScratch &operator=(const DevScratch &) = delete;
    ~DevScratch() { for (void *p : owned) (void)hipFree(p); }
    template <class T> T *get(size_t n) {
        void *p = nullptr;
        const hipError_t e = hipMalloc(&p, n * sizeof(T));
        if (!hip_ok(e)) { if (!failed) error = e; failed = true; return nullptr; }
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
