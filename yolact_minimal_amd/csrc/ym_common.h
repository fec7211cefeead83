// Shared helpers for the gfx950 kernels of libyolact_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "yolact_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

void ym_set_error(const char* fmt, ...);
void ym_note_unordered_sum(void);      // an entry point enqueued a kernel whose sums end in floating-point atomics (elementwise.hip)

#define YM_REQUIRE(cond, ...)                \
    do {                                     \
        if (!(cond)) {                       \
            ym_set_error(__VA_ARGS__);       \
            return YM_EINVAL;                \
        }                                    \
    } while (0)

static inline int ym_check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        ym_set_error("%s: %s", what, hipGetErrorString(e));
        return YM_ELAUNCH;
    }
    return YM_OK;
}

static inline int ym_cdiv(int a, int b) { return (a + b - 1) / b; }

// A host table of per-image {img_h, img_w, offset} entries (ym_ragged_image) as it travels to a kernel: BY VALUE in the kernel
// arguments, indexed by a uniform block index (masks.hip "Where a launch set's output sizes come from").
struct YmRaggedTable { ym_ragged_image img[YM_RAGGED_MAX_IMAGES]; };

// Elements per row of one instance mask: img_w floats, or (packed) ceil(img_w / 64) 64-bit words.
__host__ __device__ inline size_t ym_mask_row(bool packed, int img_w) { return packed ? (size_t)((img_w + 63) >> 6) : (size_t)img_w; }

// The checks every such table gets: 1..YM_RAGGED_MAX_IMAGES entries, positive sizes, every block at a multiple of
// YM_RAGGED_ALIGN_BYTES bytes (`esz` = bytes per element of `offset`), no two blocks overlapping; `extent_of(b)` = elements of block b.
template <class ExtentOf>
static inline int ym_check_ragged_table_indexed(const char* what, const ym_ragged_image* images, int B, int64_t esz, ExtentOf extent_of) {
    YM_REQUIRE(images, "%s: null image table", what);
    YM_REQUIRE(B >= 1 && B <= YM_RAGGED_MAX_IMAGES, "%s: 1 .. %d images per call, got %d", what, YM_RAGGED_MAX_IMAGES, B);
    for (int b = 0; b < B; ++b) {
        const ym_ragged_image& im = images[b];
        YM_REQUIRE(im.img_h > 0 && im.img_w > 0, "%s: image %d is %d x %d", what, b, im.img_h, im.img_w);
        YM_REQUIRE(im.offset >= 0 && (im.offset * esz) % YM_RAGGED_ALIGN_BYTES == 0, "%s: image %d: block offset %lld is not a multiple of %d bytes",
                   what, b, (long long)im.offset, YM_RAGGED_ALIGN_BYTES);
    }
    for (int a = 0; a < B; ++a)          // (B <= 32: a few hundred compares)
        for (int b = a + 1; b < B; ++b)
            YM_REQUIRE(images[a].offset + extent_of(a) <= images[b].offset || images[b].offset + extent_of(b) <= images[a].offset,
                       "%s: the blocks of images %d and %d overlap", what, a, b);
    return YM_OK;
}

// ... with the extent as a function of the entry alone: `extent(entry)` = elements per block.
template <class Extent>
static inline int ym_check_ragged_table(const char* what, const ym_ragged_image* images, int B, int64_t esz, Extent extent) {
    return ym_check_ragged_table_indexed(what, images, B, esz, [&](int b) { return extent(images[b]); });
}

// hipFuncAttributeMaxDynamicSharedMemorySize belongs to ONE DEVICE's copy of a kernel: a process that drives a second GPU (nms_batch
// and the request pipeline accept tensors on a non-current device) must raise it there as well.  One slot per (call site, device),
// raised when a launch asks for more than was granted; a refusal is reported instead of surfacing as an opaque launch failure.
struct YmLdsAttr { size_t granted[32]; };
static inline int ym_ensure_dyn_lds(YmLdsAttr& a, const void* fn, size_t bytes, const char* what) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 32) {
        ym_set_error("%s: no current HIP device (or device index >= 32)", what);
        return YM_EINVAL;
    }
    if (bytes > a.granted[dev]) {
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) {
            ym_set_error("%s: %zu bytes of dynamic LDS refused on device %d: %s", what, bytes, dev, hipGetErrorString(e));
            return YM_EINVAL;
        }
        a.granted[dev] = bytes;
    }
    return YM_OK;
}

// Bijective XCD-aware remap (cdna guide T1): hardware places block b on XCD b % 8; give each XCD a
// contiguous chunk of the logical tile space so neighbouring tiles share one L2.
__device__ __forceinline__ int ym_xcd_remap(int bid, int nwg) {
    const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
    const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + (bid >> 3);
}

// The normalise + affine step of train-mode BN, in ONE fixed operation order (sub, mul, fused multiply-add): the forward pass and
// every backward kernel that re-derives the ReLU mask from y instead of reading `out` (train_ops.hip, the fused statistics of
// the data-gradient epilogue in conv_mfma.hip) must agree on the sign bit for bit.
__device__ __forceinline__ float bn_affine(float v, float mu, float is, float g, float b) {
    return __builtin_fmaf((v - mu) * is, g, b);
}

__device__ __forceinline__ float ym_apply_act(float v, int act) {
    if (act == YM_ACT_RELU) return v < 0.f ? 0.f : v;   // NaN stays NaN, like torch.relu
    if (act == YM_ACT_TANH) return tanhf(v);
    if (act == YM_ACT_GELU) return 0.5f * v * (1.f + erff(v * 0.70710678118654752440f));
    return v;
}
