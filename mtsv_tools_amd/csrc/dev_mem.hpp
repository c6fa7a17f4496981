// dev_mem.hpp -- what the host files of the stages share (fold, text, parse, lca, dedup; the index upload and the builder):
// a device array that grows, a set of events, the host clock, a tile size from the environment, the device check.  Host code.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <stdexcept>
#include <string>

#include "dev_index.hpp"

namespace mtsv {

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
        if (hipMalloc((void**)&q, std::max<uint64_t>(n, 1) * sizeof(T)) != hipSuccess) {
            (void)hipGetLastError();
            throw std::runtime_error(std::string("device: no memory for ") + what + " (" + std::to_string(n * sizeof(T)) + " bytes)");
        }
        release();
        p = q;
        cap = n;
    }
    // p[0 .. want) after whatever `stream` still does with the old array; it grows by an eighth over what is asked for
    void room(hipStream_t stream, uint64_t want, const char* what, uint64_t floor = 1024) {
        if (want <= cap && p) return;
        HIP_CHECK(hipStreamSynchronize(stream));
        alloc(std::max<uint64_t>(want + want / 8, floor), what);
    }
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
        for (auto& x : e) HIP_CHECK(hipEventCreate(&x));
    }
    hipEvent_t operator[](int k) const { return e[k]; }
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
