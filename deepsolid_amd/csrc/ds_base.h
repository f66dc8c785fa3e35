// ds_base.h -- the part of the host code that needs no kernel header: the error slot of ds_last_error, HIP_OK, the dtype dispatch,
// the 3 x 3 inverse and the workspace arena.  ds_host.h builds on it; ds_hf.hip needs nothing more.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/deepsolid_hip.h"

namespace ds {

// the message slot of ds_last_error (one per thread, ds_api.hip)
void set_last_error(const char* msg);

namespace host {

// formats the message into that slot; returns 1
int fail(const char* fmt, ...);

#define HIP_OK(call)                                                              \
    do {                                                                          \
        hipError_t e_ = (call);                                                   \
        if (e_ != hipSuccess) return fail("%s: %s", #call, hipGetErrorString(e_)); \
    } while (0)

// f<double>(args) or f<float>(args) by the element type code of the C ABI (0: float64, else float32)
#define DS_BY_DTYPE(dtype, f, ...) ((dtype) == 0 ? f<double>(__VA_ARGS__) : f<float>(__VA_ARGS__))

inline void inv3(const double* a, double* o) {
    const double det = a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) +
                       a[2] * (a[3] * a[7] - a[4] * a[6]);
    o[0] = (a[4] * a[8] - a[5] * a[7]) / det; o[1] = (a[2] * a[7] - a[1] * a[8]) / det; o[2] = (a[1] * a[5] - a[2] * a[4]) / det;
    o[3] = (a[5] * a[6] - a[3] * a[8]) / det; o[4] = (a[0] * a[8] - a[2] * a[6]) / det; o[5] = (a[2] * a[3] - a[0] * a[5]) / det;
    o[6] = (a[3] * a[7] - a[4] * a[6]) / det; o[7] = (a[1] * a[6] - a[0] * a[7]) / det; o[8] = (a[0] * a[4] - a[1] * a[3]) / det;
}

template <typename I> inline I rup(I x, int m) { return (x + m - 1) / m * m; }

// A workspace as a stack of elements of T.  Every layout below is ONE function over an arena and serves both as the size of the
// layout and as its pointers: with a base, take(n) hands out the next n elements (carve mode); with a null base it only counts
// (measure mode: `used` is the extent).  An entry point checks `ok` after carving and before its first launch.
template <typename T> struct Arena {
    T* base = nullptr;
    size_t cap = SIZE_MAX, used = 0;
    bool ok = true;                                  // false once more was taken than `cap` -- here or in a part() of this arena
    T* take(size_t n) { T* p = base ? base + used : nullptr; used += n; ok = ok && used <= cap; return p; }
    void align(size_t k) { take((k - used % k) % k); }
    // a buffer of n elements already handed out, carved up again (buffers that live inside an idle one); its overrun counts here
    template <typename F> void part(T* buf, size_t n, F&& carve) { Arena a{buf, n}; carve(a); ok = ok && a.ok; }
};
template <typename T> Arena<T> arena_of(void* ws, int64_t ws_bytes) { return Arena<T>{(T*)ws, (size_t)std::max<int64_t>(ws_bytes, 0) / sizeof(T)}; }
// extent, in elements, of a layout function
template <typename F> size_t measure(F&& layout) { Arena<double> a; layout(a); return a.used; }

inline int carve_fail(const char* what) { return fail("internal: %s: workspace carve exceeds its size", what); }

}  // namespace host
}  // namespace ds
