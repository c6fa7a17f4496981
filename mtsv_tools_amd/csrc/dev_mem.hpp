// dev_mem.hpp -- what the host files share (the batch workspace; fold, text, parse, lca, dedup; the index upload and the
// builder): a device array that grows, a page-locked host array, a stream, sets of events, the host clock, a tile size from
// the environment, the device check.  Host code.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "dev_index.hpp"

namespace mtsv {

// (tests) MTSV_ALLOC_REFUSE=<text>: a DevBuf allocation whose `what` contains <text> is refused as if the device had no memory
// for it, without a call to the runtime.  Read at the allocation: allocations are rare, and each stalls the device anyway.
inline bool alloc_refused(const char* what) {
    const char* e = getenv("MTSV_ALLOC_REFUSE");
    return e && *e && strstr(what, e) != nullptr;
}

// An array of device memory, freed with its owner (on the device that is current then: an owner that is bound to a device
// sets it in its destructor's body, which runs before its members are destroyed).  Move only.
template <class T>
struct DevBuf {
    T* p = nullptr;
    uint64_t cap = 0;  // elements

    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept { swap(o); }
    ~DevBuf() { release(); }
    void swap(DevBuf& o) {
        std::swap(p, o.p);
        std::swap(cap, o.cap);
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    // exactly n elements (what it held is lost); nothing changes when the allocation fails
    void alloc(uint64_t n, const char* what) {
        T* q = nullptr;
        const bool refused = alloc_refused(what);
        if (refused || hipMalloc((void**)&q, std::max<uint64_t>(n, 1) * sizeof(T)) != hipSuccess) {
            if (!refused) (void)hipGetLastError();
            throw std::runtime_error(std::string("device: no memory for ") + what + " (" + std::to_string(n * sizeof(T)) + " bytes)");
        }
        release();
        p = q;
        cap = n;
    }
    // the same with the old array released first, where the peak of a growth must not hold both: empty when the allocation fails
    void renew(uint64_t n, const char* what) {
        release();
        alloc(n, what);
    }
    // p[0 .. want) after whatever `stream` still does with the old array; it grows by an eighth over what is asked for
    void room(hipStream_t stream, uint64_t want, const char* what, uint64_t floor = 1024) {
        if (want <= cap && p) return;
        HIP_CHECK(hipStreamSynchronize(stream));
        alloc(std::max<uint64_t>(want + want / 8, floor), what);
    }
};

template <class... B>
void release_all(B&... b) {
    (b.release(), ...);
}

// An array of page-locked host memory (hipHostMalloc with `flags`), freed with its owner.  What it held is never kept: a new
// size releases the old array first, and the array is empty when the allocation fails.
template <class T>
struct HostBuf {
    T* p = nullptr;
    uint64_t cap = 0;  // elements

    HostBuf() = default;
    HostBuf(const HostBuf&) = delete;
    HostBuf& operator=(const HostBuf&) = delete;
    ~HostBuf() { release(); }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
    void renew(uint64_t n, unsigned flags = hipHostMallocDefault) {
        release();
        HIP_CHECK(hipHostMalloc((void**)&p, std::max<uint64_t>(n, 1) * sizeof(T), flags));
        cap = n;
    }
};

// A stream, destroyed with its owner (which waits for it first where work may be in flight).  An owner declares its streams
// before its arrays, so that they outlive them.
struct DevStream {
    hipStream_t s = nullptr;

    DevStream() = default;
    DevStream(const DevStream&) = delete;
    DevStream& operator=(const DevStream&) = delete;
    ~DevStream() {
        if (s) (void)hipStreamDestroy(s);
    }
    void create(unsigned flags) { HIP_CHECK(hipStreamCreateWithFlags(&s, flags)); }
    void create(unsigned flags, int priority) { HIP_CHECK(hipStreamCreateWithPriority(&s, flags, priority)); }
    operator hipStream_t() const { return s; }
};

// Created by create(), not by the constructor: a member is constructed before its owner's constructor has set the device.
template <int N>
struct DevEvents {
    hipEvent_t e[N] = {};

    DevEvents() = default;
    DevEvents(const DevEvents&) = delete;
    DevEvents& operator=(const DevEvents&) = delete;
    ~DevEvents() {
        for (auto& x : e)
            if (x) (void)hipEventDestroy(x);
    }
    void create() {
        for (auto& x : e)
            if (!x) HIP_CHECK(hipEventCreate(&x));
    }
    bool created() const { return e[N - 1] != nullptr; }  // (sets created at first use)
    hipEvent_t operator[](int k) const { return e[k]; }
};

// Events of one kind (`flags`), as many as have been asked for so far, kept between uses.
struct DevEventList {
    std::vector<hipEvent_t> e;

    DevEventList() = default;
    DevEventList(const DevEventList&) = delete;
    DevEventList& operator=(const DevEventList&) = delete;
    ~DevEventList() {
        for (auto& x : e) (void)hipEventDestroy(x);
    }
    hipEvent_t at(size_t k, unsigned flags) {
        while (e.size() <= k) {
            hipEvent_t x;
            HIP_CHECK(hipEventCreateWithFlags(&x, flags));
            e.push_back(x);
        }
        return e[k];
    }
    hipEvent_t operator[](size_t k) const { return e[k]; }
};

inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// a tile size from the environment (tests: tile edges within reach of small inputs): dflt when `name` is not set, else its
// value clamped to [lo, hi] and rounded down to lo times a power of two
inline uint32_t tile_from_env(const char* name, uint32_t dflt, uint32_t lo, uint32_t hi) {
    const char* e = getenv(name);
    if (!e) return dflt;
    const uint64_t want = std::min<uint64_t>(std::max<uint64_t>(strtoull(e, nullptr, 10), lo), hi);
    uint32_t tile = lo;
    while (tile * 2 <= want) tile *= 2;
    return tile;
}

inline void require_device(int device) {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess) {
        (void)hipGetLastError();
        n_dev = 0;
    }
    if (device < 0 || device >= n_dev) throw std::runtime_error("device: no HIP device " + std::to_string(device) + " (" + std::to_string(n_dev) + " visible)");
}

}  // namespace mtsv
