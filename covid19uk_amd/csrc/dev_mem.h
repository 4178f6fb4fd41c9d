// Who owns the library's device memory, and the policies that go with allocating it.  Host code only:
// no kernel and no kernel header.  seir_hip.hip includes it behind its g_err, fail() and HIP_TRY: a failure here is reported as
// every other of the library, an error code with the text behind seir_last_error().
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <utility>

// One hipMalloc'ed block and its only owner.  Nothing frees device memory by name: a block goes when its owner goes out of scope,
// is reset, or is assigned another (`x = DevBuf{}`, or a fresh struct that holds some).  Kernel arguments stay raw pointers
// (as<T>()): an owner never sits inside a struct that is passed to a kernel by value.
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept { *this = std::move(o); }
    DevBuf &operator=(DevBuf &&o) noexcept {         // what this one held goes with `o`
        std::swap(p, o.p);
        std::swap(bytes, o.bytes);
        return *this;
    }
    ~DevBuf() { reset(); }
    void reset() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    explicit operator bool() const { return p != nullptr; }
    template <typename T> T *as() const { return (T *)p; }
    // A fresh block of n bytes (at least 8), contents undefined; what was held before is freed first.
    int alloc(size_t n) {
        reset();
        HIP_TRY(hipMalloc(&p, n ? n : 8));
        bytes = n ? n : 8;
        return 0;
    }
    // A fresh block of zeros: the one way a new allocation is zeroed.  hipMemset may return before the device is done, and the
    // null stream is not ordered with the (non-blocking) streams the kernels run on: without the wait a kernel enqueued right
    // behind the allocation can find its output zeroed under it.  An allocation is never on the hot path, so the wait is free.
    // On failure the owner keeps what it held.
    int zeroed(size_t n) {
        DevBuf b;
        if (int rc = b.alloc(n)) return rc;
        HIP_TRY(hipMemset(b.p, 0, b.bytes));
        HIP_TRY(hipStreamSynchronize(nullptr));
        *this = std::move(b);
        return 0;
    }
    // A fresh block with a copy of n bytes of host memory in it (a blocking copy).  On failure the owner keeps what it held.
    int upload(const void *src, size_t n) {
        DevBuf b;
        if (int rc = b.alloc(n)) return rc;
        HIP_TRY(hipMemcpy(b.p, src, n, hipMemcpyHostToDevice));
        *this = std::move(b);
        return 0;
    }
};

// The same for page-locked host memory; it stays where it is.
struct PinnedBuf {
    void *p = nullptr;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    ~PinnedBuf() { reset(); }
    void reset() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
    }
    template <typename T> T *as() const { return (T *)p; }
};

// A product's buffers could not be made: its size and its name in front of what the failed step has just reported.
static int alloc_failed(unsigned long long bytes, const char *of_what) {
    char why[sizeof(g_err)];
    snprintf(why, sizeof(why), "%s", g_err);
    return fail(SEIR_ERR_DEVICE, "allocating %llu bytes of %s failed: %s", bytes, of_what, why);
}

// One product may take half of what is free on the device: the policy of a device that is shared, not a measurement.  The caller
// spells out its half of the refusal ("the group sums need N bytes (shape)"); the comparison, the free figure and the tail are here.
// Test hook: with SEIR_DEBUG_FREE_BYTES=<n> in the environment the free figure is min(the device's, n) -- for the products whose
// buffers are too small for any device to refuse (the verification's accumulators are 32 B per cell): their refusal is then
// exercised without a test that holds the memory of a device which others use.  Read at every call; absent, nothing changes.
__attribute__((format(printf, 2, 3))) static int refuse_above_half_free(unsigned long long bytes, const char *need_fmt, ...) {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (const char *cap = getenv("SEIR_DEBUG_FREE_BYTES")) {
        char *end = nullptr;
        const unsigned long long v = strtoull(cap, &end, 10);
        if (end != cap && *end == '\0' && v < (unsigned long long)free_b) free_b = (size_t)v;
    }
    if (bytes <= (unsigned long long)free_b / 2) return 0;
    char need[400];
    va_list ap;
    va_start(ap, need_fmt);
    vsnprintf(need, sizeof(need), need_fmt, ap);
    va_end(ap);
    return fail(SEIR_ERR_INVALID, "%s, more than half of the %llu bytes free on the device", need, (unsigned long long)free_b);
}

// Above 64 KiB of dynamic LDS a kernel needs the attribute.  The caller takes the kernel's address, since a kernel template is
// emitted where the host code first names it and the places of the kernels in the code object are pinned.
static hipError_t lds_attribute(const void *kernel, size_t lds) {
    return lds > 64 * 1024 ? hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) : hipSuccess;
}
