// Shared host-side helpers of libofd_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include "../../include/ofd.h"

namespace ofd {

void set_error(const char* fmt, ...);

#define OFD_CHECK_ARG(cond, ...)                                   \
    do {                                                           \
        if (!(cond)) {                                             \
            ::ofd::set_error(__VA_ARGS__);                         \
            return OFD_ERR_ARG;                                    \
        }                                                          \
    } while (0)

// a caller-provided workspace of `have` bytes where `need` are required: "<what>: workspace <have> < <need>"
#define OFD_CHECK_WORKSPACE(have, need, what)                                              \
    do {                                                                                   \
        const size_t have_ = (have), need_ = (need);                                       \
        if (have_ < need_) {                                                               \
            ::ofd::set_error(what ": workspace %zu < %zu", have_, need_);                  \
            return OFD_ERR_WORKSPACE;                                                      \
        }                                                                                  \
    } while (0)

#define OFD_HIP(call)                                                                     \
    do {                                                                                   \
        hipError_t e_ = (call);                                                            \
        if (e_ != hipSuccess) {                                                            \
            ::ofd::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return OFD_ERR_HIP;                                                            \
        }                                                                                  \
    } while (0)

#define OFD_LAUNCH_CHECK() OFD_HIP(hipGetLastError())

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// Integer value of an environment switch, `dflt` when unset.  Read on every call: the tests flip the reference switches (OFD_CONV_PC,
// OFD_GW_BAND, OFD_CONV1_NO_PL, OFD_CONV1_GRID, OFD_CONV7_PERSIST) inside one process to compare a fast kernel with its reference.
static inline int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}

typedef uint16_t bf16_t;   // raw bits

__device__ __forceinline__ float bf2f(bf16_t v) { return __uint_as_float(((uint32_t)v) << 16); }
// round-to-nearest-even, NaN stays NaN: the plain cast lowers to v_cvt_pk_bf16_f32 on gfx950
// (a hand-written integer rounding costs a divergent branch per value)
__device__ __forceinline__ bf16_t f2bf(float f) {
    const __bf16 h = (__bf16)f;
    return __builtin_bit_cast(bf16_t, h);
}
__device__ __forceinline__ uint32_t f2bf2(float lo, float hi) {
    typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
    typedef __attribute__((ext_vector_type(2))) float f32x2_t;
    const f32x2_t v = {lo, hi};
    const bf16x2_t h = __builtin_convertvector(v, bf16x2_t);
    return __builtin_bit_cast(uint32_t, h);
}

// a[0..7] += the eight bf16 of a 16-byte unit
__device__ __forceinline__ void bf16_octet_add(float (&a)[8], const uint4& v) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        a[2 * j] += bf2f((bf16_t)(w[j] & 0xffffu));
        a[2 * j + 1] += bf2f((bf16_t)(w[j] >> 16));
    }
}

// XCD-aware tile order: workgroup i runs on XCD i % 8, so dispatch index `tile` is mapped to a tile such that the workgroups of one XCD
// walk a contiguous run of tiles (what neighbouring tiles share -- halo rows, window overlap -- is then served by one L2)
__device__ __forceinline__ int xcd_tile_order(int tile, int ntiles) {
    if (ntiles >= 8) {
        const int q = ntiles / 8, r = ntiles % 8, xcd = tile % 8, idx = tile / 8;
        tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    return tile;
}

}  // namespace ofd
