// Host-side helpers shared by the C-ABI translation units; the argument checks, image grid and pose fill are the frame-side units'
// (their device-side rules: sobfu_frame.hpp).
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <type_traits>

#include "sobfu_hip.h"

#define SOBFU_CHECK_ARGS(cond)                \
    do {                                      \
        if (!(cond)) return SOBFU_E_BADARG;   \
    } while (0)

#define SOBFU_HIP_TRY(expr)                   \
    do {                                      \
        hipError_t _e = (expr);               \
        if (_e != hipSuccess) return (int) _e; \
    } while (0)

#define SOBFU_TRY(expr)                       \
    do {                                      \
        int _rc = (expr);                     \
        if (_rc != 0) return _rc;             \
    } while (0)

namespace sobfu_hip {

// What a C-ABI handle holds, as members that release it themselves: unique_ptr with stateless deleters (an empty member releases
// nothing; a handle's members go in the reverse order of their declaration).  hipEvent_t / hipStream_t are pointer types already.
struct DeviceFree {
    void operator()(void* p) const { (void) hipFree(p); }
};
struct PinnedFree {
    void operator()(void* p) const { (void) hipHostFree(p); }
};
struct EventDestroy {
    void operator()(hipEvent_t e) const { (void) hipEventDestroy(e); }
};
struct StreamDestroy {
    void operator()(hipStream_t s) const { (void) hipStreamDestroy(s); }
};
template <class T> using DevicePtr = std::unique_ptr<T, DeviceFree>;
template <class T> using PinnedPtr = std::unique_ptr<T, PinnedFree>;
using EventPtr  = std::unique_ptr<std::remove_pointer_t<hipEvent_t>, EventDestroy>;
using StreamPtr = std::unique_ptr<std::remove_pointer_t<hipStream_t>, StreamDestroy>;
// hipMalloc into an owner: what it held is released FIRST, so a failed allocation leaves it empty
template <class T> inline hipError_t device_alloc(DevicePtr<T>& out, size_t bytes) {
    out.reset();
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess) out.reset(static_cast<T*>(p));
    return e;
}
inline hipError_t event_create(EventPtr& out, unsigned flags) {
    hipEvent_t e = nullptr;
    const hipError_t rc = hipEventCreateWithFlags(&e, flags);
    if (rc == hipSuccess) out.reset(e);
    return rc;
}

// the pointer and the row size of its pitched image (bytes; 0 for a dense array) are multiples of `to`
inline bool aligned(const void* p, long long step, int to) { return ((uintptr_t) p % (uintptr_t) to) == 0 && step % to == 0; }
inline bool positive_finite(float x) { return std::isfinite(x) && x > 0.f; }
inline bool finite_all(const float* v, int n) {
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}
inline bool intr_ok(float fx, float fy, float cx, float cy) {
    return std::isfinite(fx) && std::isfinite(fy) && fx != 0.f && fy != 0.f && std::isfinite(cx) && std::isfinite(cy);
}
constexpr int kGridZ = 65535;  // volume_ok's max_z for a launch with one z-slice per blockIdx.z (voxel_grid); INT_MAX for a 1-D launch
inline bool volume_ok(int X, int Y, int Z, int max_z) { return X > 0 && Y > 0 && Z > 0 && Z <= max_z && (long long) X * Y * Z <= (1LL << 40); }
inline dim3 image_grid(int rows, int cols) { return dim3((unsigned) ((cols + 63) / 64), (unsigned) ((rows + 3) / 4)); }
// (R row-major, t) of the C ABI into a kernel's arguments: R, its transpose and t, each where the kernel wants it (NULL: not wanted)
inline void fill_pose(const float R[9], const float t[3], float* R_out, float* Rt_out, float* t_out) {
    for (int i = 0; i < 9; ++i) {
        if (R_out) R_out[i] = R[i];
        if (Rt_out) Rt_out[i] = R[3 * (i % 3) + i / 3];
    }
    for (int i = 0; i < 3 && t_out; ++i) t_out[i] = t[i];
}


// The max-norm rows pass B folds max ||u||^2 into (bit patterns of non-negative floats): the norm a row stands for, rounded as the
// device's gate rounds it (__fsqrt_rd)
constexpr int kSlots = 256;
inline float host_sqrt_rd(float s) {
    float r = std::sqrt(s);
    if (r > 0.f && (double) r * (double) r > (double) s) r = std::nextafterf(r, -INFINITY);
    return r;
}
inline float slots_to_norm(const uint32_t* s) {
    uint32_t m = 0;
    for (int i = 0; i < kSlots; ++i) m = s[i] > m ? s[i] : m;
    float f;
    std::memcpy(&f, &m, 4);
    return host_sqrt_rd(f);
}

}  // namespace sobfu_hip
