// Mask assembly for gfx950.
//  k_mask_assemble : sigmoid(coef[n][32] x proto[P][32]^T) on the f32 MFMA pipe with the crop fused into the
//                    epilogue.  GEMM roles are chosen for the STORE side: MFMA "A" = coefficients (i = detection),
//                    "B" = prototypes (j = pixel), so D's column index (lane & 31) is the pixel and each accumulator
//                    register row is written as 32 consecutive pixels of one detection (128-B segments).
//                    Both operands are K-contiguous in HBM ([.][32] floats), so lane half h reads k = 8g+4h..+3
//                    as one 16-byte global load per group g — no LDS staging at all (K = 32 fits in registers).
//                    Algorithmic bytes: P*32*4 (proto, read once) + n*P*4 (masks, written once): HBM-bound.
//  k_mask_resize<PACKED> : bilinear (align_corners=False) to S x S, > 0.5, cropped to img_h x img_w; the dense output
//                    (n*img_h*img_w*4 B) dominates, written with 16-byte stores; PACKED: 1 bit per pixel (one ballot = one 64-pixel
//                    word).  A device count, when given, bounds the rows.
//  k_masks_fused<PACKED, Sizes> : after_nms in one launch (below), dense or bits, for one output size (UniformSizes) or one per image
//                    (RaggedSizes); after_nms_launches<PACKED, Sizes> is the launch set of the four ym_after_nms_* entries, with
//                    k_boxes_to_pixels_batch<Sizes> at its end.
//  k_pack_masks / k_unpack_masks : dense <-> bits.
//  Window mode (`Pv`, ym_after_nms_window[_packed]): the Hp x Wp prototype map is the top-left window of a VIRTUAL Pv x Pv map (the
//                    network ran on the top-left Hn x Wn of its square input, Pv = img_size / 4).  Pv = 0 is the reference's rule
//                    (the map is the whole extent, scaled per axis) and what every older entry passes; the rule for Pv > 0 is at
//                    `ProtoGeom` below.  One argument of the same kernels, not a second set.
#pragma clang fp contract(off)
#include "ym_common.h"
#include <algorithm>

namespace {

__device__ __forceinline__ void crop_span(float a, float b, float size, float& lo, float& hi) {
    // utils/box_utils.py:117-132 with padding = 1
    a = a * size;
    b = b * size;
    lo = fminf(a, b);
    hi = fmaxf(a, b);
    lo = lo - 1.f;
    lo = lo < 0.f ? 0.f : lo;
    hi = hi + 1.f;
    hi = hi > size ? size : hi;
}

// Where a 0..1 box lands on the prototype map and how an output pixel maps back to it.
//   Pv == 0: the map is the whole extent: boxes scale by (Wp, Hp), the resize by Hp / S and Wp / S, S = max(img_h, img_w).
//   Pv  > 0: the map is the top-left Hp x Wp of a virtual Pv x Pv map: boxes and the crop window scale by Pv on both axes, the resize
//            by Pv / S on both axes, and source indices clamp to the PHYSICAL Hp - 1 / Wp - 1 (src_coord's own clamp), so a row or
//            column past the window reads the window's last one, crop status included.
struct ProtoGeom {
    float ch, cw;       // crop extents (rows, columns)
    float sy, sx;       // resize scales
};
__device__ __forceinline__ ProtoGeom proto_geom(int Hp, int Wp, int Pv, int img_h, int img_w) {
    const int S = img_h > img_w ? img_h : img_w;
    const float eh = (float)(Pv > 0 ? Pv : Hp), ew = (float)(Pv > 0 ? Pv : Wp);
    return ProtoGeom{eh, ew, eh / (float)S, ew / (float)S};
}

__global__ __launch_bounds__(256) void k_mask_assemble(const float* __restrict__ proto, const float* __restrict__ coefs,
                                                        const float* __restrict__ boxes, int n, int Hp, int Wp, int Pv,
                                                        int do_crop, float* __restrict__ out) {
    const int P = Hp * Wp;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pix0 = (blockIdx.x * 4 + wave) * 32;
    if (pix0 >= P) return;
    const int pj = lane & 31, h = lane >> 5;
    const int pix = pix0 + pj;
    f32x4 pb[4];
#pragma unroll
    for (int g = 0; g < 4; ++g)
        pb[g] = pix < P ? *reinterpret_cast<const f32x4*>(proto + (size_t)pix * 32 + g * 8 + h * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    const int py = pix / Wp, px = pix - py * Wp;
    const float fx = (float)px, fy = (float)py;

    for (int d0 = 0; d0 < n; d0 += 32) {
        const int det = d0 + pj;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 ca = det < n ? *reinterpret_cast<const f32x4*>(coefs + (size_t)det * 32 + g * 8 + h * 4)
                                     : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ca[s], pb[g][s], acc, 0, 0, 0);
        }
        if (pix >= P) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int d = d0 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (d >= n) continue;
            float v = 1.f / (1.f + expf(-acc[r]));
            if (do_crop) {
                const f32x4 b = *reinterpret_cast<const f32x4*>(boxes + (size_t)d * 4);
                float x1, x2, y1, y2;
                crop_span(b[0], b[2], (float)(Pv > 0 ? Pv : Wp), x1, x2);
                crop_span(b[1], b[3], (float)(Pv > 0 ? Pv : Hp), y1, y2);
                const bool inside = fx >= x1 && fx < x2 && fy >= y1 && fy < y2;
                v = inside ? v : 0.f;
            }
            out[(size_t)d * P + pix] = v;
        }
    }
}

__device__ __forceinline__ void src_coord(int dst, float scale, int in_sz, int& i0, int& i1, float& l1) {
    float src = scale * ((float)dst + 0.5f) - 0.5f;
    if (src < 0.f) src = 0.f;
    i0 = (int)src;
    l1 = src - (float)i0;                      // (the fraction of the UNclamped index: a coordinate past the map blends its last
    if (i0 > in_sz - 1) i0 = in_sz - 1;        //  row with itself, like interpolation over a replicate-padded map; only window mode
    i1 = i0 + ((i0 < in_sz - 1) ? 1 : 0);      //  gets there, a map scaled to its own extent never exceeds in_sz - 1)
}

// Is the soft mask, interpolated between source rows r0 / r1 (weights 1 - ly / ly) at output column x, foreground?  THE expression of
// every resize below, dense or packed, from HBM or from the fused kernel's LDS patch: they agree bit for bit because it is written once.
__device__ __forceinline__ bool fg_at(const float* r0, const float* r1, float ly, int x, int img_w, float sx, int Wp) {
    int x0, x1; float lx;
    src_coord(x < img_w ? x : img_w - 1, sx, Wp, x0, x1, lx);
    const float hy = 1.f - ly, hx = 1.f - lx;
    const float v = hy * (hx * r0[x0] + lx * r0[x1]) + ly * (hx * r1[x0] + lx * r1[x1]);
    return v > 0.5f;
}

__device__ __forceinline__ int clamped_count(const int32_t* count, int max_det) {
    const int n = *count;
    return n < 0 ? 0 : (n > max_det ? max_det : n);
}

template <bool PACKED> struct mask_elem { typedef float type; };
template <> struct mask_elem<true> { typedef unsigned long long type; };

// The two-kernel path's resize of n soft masks.  An item is 4 consecutive pixels of a thread (dense: one 16-byte store) or the 64 of
// a wave (PACKED: lane = pixel, one ballot = one word), grid-strided.  `count` (nullable): the image's count on the device bounds n,
// so rows at or past it are not written.
template <bool PACKED>
__global__ __launch_bounds__(256) void k_mask_resize(const float* __restrict__ masks, const int32_t* __restrict__ count, int n, int Hp,
                                                      int Wp, int Pv, int img_h, int img_w,
                                                      typename mask_elem<PACKED>::type* __restrict__ out) {
    n = count ? clamped_count(count, n) : n;
    constexpr int LG = PACKED ? 6 : 2, PER_BLOCK = PACKED ? 4 : 256;
    const ProtoGeom g = proto_geom(Hp, Wp, Pv, img_h, img_w);
    const float sy = g.sy, sx = g.sx;
    const int wq = (img_w + (1 << LG) - 1) >> LG;
    const size_t total = (size_t)n * img_h * wq;
    const size_t first = (size_t)blockIdx.x * PER_BLOCK + (PACKED ? threadIdx.x >> 6 : threadIdx.x);
    for (size_t i = first; i < total; i += (size_t)gridDim.x * PER_BLOCK) {
        const int xq = (int)(i % wq);
        size_t t = i / wq;
        const int y = (int)(t % img_h);
        const int d = (int)(t / img_h);
        int y0, y1; float ly;
        src_coord(y, sy, Hp, y0, y1, ly);
        const float* r0 = masks + ((size_t)d * Hp + y0) * Wp;
        const float* r1 = masks + ((size_t)d * Hp + y1) * Wp;
        if constexpr (PACKED) {
            const int lane = threadIdx.x & 63, x = xq * 64 + lane;
            const bool fg = fg_at(r0, r1, ly, x, img_w, sx, Wp);
            const unsigned long long w = __ballot(x < img_w && fg);
            if (lane == 0) out[i] = w;
        } else {
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = fg_at(r0, r1, ly, xq * 4 + e, img_w, sx, Wp) ? 1.f : 0.f;
            float* dst = out + ((size_t)d * img_h + y) * img_w + xq * 4;
            if ((img_w & 3) == 0) {
                *reinterpret_cast<f32x4*>(dst) = f32x4{o[0], o[1], o[2], o[3]};
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (xq * 4 + e < img_w) dst[e] = o[e];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// after_nms in ONE launch for a batch of images: assemble (coef x prototype, sigmoid, crop) -> bilinear resize to S x S ->
// > 0.5 -> slice to img_h x img_w  (utils/output_utils.py:217-228), without the [n][Hp][Wp] soft masks ever reaching HBM.
//
// grid = (output tiles, detection slot, image); a workgroup owns a FT_H x FT_W output tile of one detection.  The cropped soft
// mask is exactly 0 outside the detection's window, and bilinear interpolation of zeros is +0 -> "> 0.5" is false: a tile whose
// source patch lies outside the window is a pure zero fill (16-byte stores, the HBM-bound bulk of the n*img_h*img_w*4 output
// bytes).  Active tiles first build their source patch of the soft mask in LDS (thread = prototype pixel: 32-float dot with
// the coefficients + sigmoid + crop test, the same fp32 formula as k_mask_assemble up to the summation order), then resize
// from LDS with ATen's source-index arithmetic.  Detection slots >= the image's count (read on the device) exit at once.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int FT_W = 256, FT_H = 16;          // output tile: 64 lanes x float4 wide, 4 waves x 4 rows high
constexpr int FP_W = 96, FP_H = 10;           // source patch capacity (floats): checked on the host against the scale

// One FT_H x FT_W output tile of ONE detection: the body of every instantiation of k_masks_fused.  `pimg` is the image's
// prototype map, `coef` / `box` the detection's 32 coefficients / 4 box floats, `obase` the detection's mask ([img_h][img_w] floats or
// [img_h][wq] words), `patch` / `cf` the workgroup's LDS.  PACKED only changes the lane -> pixel map and the store (below).
template <bool PACKED>
__device__ __forceinline__ void fused_tile(float* patch, float* cf, const float* __restrict__ pimg, const float* __restrict__ coef,
                                           const float* __restrict__ box, int tile, int Hp, int Wp, int Pv, int img_h, int img_w,
                                           int do_crop, typename mask_elem<PACKED>::type* __restrict__ obase) {
    static_assert(FT_W == 256 && FT_H == 16, "4 words x (4 waves x 4 rows) per tile");
    const int tiles_x = (img_w + FT_W - 1) / FT_W;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int oy0 = ty * FT_H, ox0 = tx * FT_W;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const ProtoGeom g = proto_geom(Hp, Wp, Pv, img_h, img_w);
    const float sy = g.sy, sx = g.sx;

    float x1 = 0.f, x2 = g.cw, y1 = 0.f, y2 = g.ch;
    if (do_crop) {
        const f32x4 bx = *reinterpret_cast<const f32x4*>(box);
        crop_span(bx[0], bx[2], g.cw, x1, x2);
        crop_span(bx[1], bx[3], g.ch, y1, y2);
    }
    // source patch of this tile (src_coord is monotonic in the destination index)
    int py0, py1, px0, px1, t0, t1; float l;
    const int oy_last = min(oy0 + FT_H, img_h) - 1, ox_last = min(ox0 + FT_W, img_w) - 1;
    src_coord(oy0, sy, Hp, py0, t1, l);
    src_coord(oy_last, sy, Hp, t0, py1, l);
    src_coord(ox0, sx, Wp, px0, t1, l);
    src_coord(ox_last, sx, Wp, t0, px1, l);
    const int ph = py1 - py0 + 1, pw = px1 - px0 + 1;
    // any source pixel of the patch inside the crop window [x1,x2) x [y1,y2)?  (float compares like the reference's crop)
    const bool active = (float)px1 >= x1 && (float)px0 < x2 && (float)py1 >= y1 && (float)py0 < y2;
    // dense: a lane owns 4 consecutive pixels of its wave's four rows
    const bool vec = (img_w & 3) == 0;
    const int x = ox0 + lane * 4;
    // packed: lane k < 16 stores word (k & 3) of row (k >> 2) of this wave's four rows
    const int wq = (img_w + 63) >> 6;
    const int my_y = oy0 + wave * (FT_H / 4) + (lane >> 2), my_j = (ox0 >> 6) + (lane & 3);
    const bool stores = lane < 16 && my_y < img_h && my_j < wq;
    if (!active) {
        if constexpr (PACKED) {
            if (stores) obase[(size_t)my_y * wq + my_j] = 0ull;
        } else {
#pragma unroll
            for (int r = 0; r < FT_H / 4; ++r) {
                const int y = oy0 + wave * (FT_H / 4) + r;
                if (y >= img_h || x >= img_w) continue;
                float* dst = obase + (size_t)y * img_w + x;
                if (vec) *reinterpret_cast<f32x4*>(dst) = f32x4{0.f, 0.f, 0.f, 0.f};
                else
                    for (int e = 0; e < 4 && x + e < img_w; ++e) dst[e] = 0.f;
            }
        }
        return;
    }
    if (tid < 32) cf[tid] = coef[tid];
    __syncthreads();
    for (int i = tid; i < ph * pw; i += 256) {
        const int r = i / pw, c = i - r * pw;
        const int py = py0 + r, px = px0 + c;
        const float fx = (float)px, fy = (float)py;
        float v = 0.f;
        if (fx >= x1 && fx < x2 && fy >= y1 && fy < y2) {
            const f32x4* pr = reinterpret_cast<const f32x4*>(pimg + ((size_t)py * Wp + px) * 32);
            float acc = 0.f;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const f32x4 pv = pr[q];
                const f32x4 cv = *reinterpret_cast<const f32x4*>(cf + q * 4);
                acc = __builtin_fmaf(cv[0], pv[0], acc);
                acc = __builtin_fmaf(cv[1], pv[1], acc);
                acc = __builtin_fmaf(cv[2], pv[2], acc);
                acc = __builtin_fmaf(cv[3], pv[3], acc);
            }
            v = 1.f / (1.f + expf(-acc));
        }
        patch[r * FP_W + c] = v;
    }
    __syncthreads();
    [[maybe_unused]] unsigned long long mine = 0ull;
#pragma unroll
    for (int r = 0; r < FT_H / 4; ++r) {
        const int y = oy0 + wave * (FT_H / 4) + r;
        if (y >= img_h) continue;                                // (wave-uniform: rows past the image own no patch rows)
        if (!PACKED && x >= img_w) continue;
        int y0, y1i; float ly;
        src_coord(y, sy, Hp, y0, y1i, ly);
        const float* r0 = patch + (y0 - py0) * FP_W - px0;
        const float* r1 = patch + (y1i - py0) * FP_W - px0;
        if constexpr (PACKED) {
            // a lane owns pixels ox0 + 64e + lane: one ballot per (row, e) IS one word, lane r * 4 + e keeps it
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (ox0 + 64 * e >= img_w) continue;             // (wave-uniform: this word does not exist)
                const int xe = ox0 + 64 * e + lane;
                const bool fg = fg_at(r0, r1, ly, xe, img_w, sx, Wp);
                const unsigned long long w = __ballot(xe < img_w && fg);
                mine = lane == r * 4 + e ? w : mine;
            }
        } else {
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = fg_at(r0, r1, ly, x + e, img_w, sx, Wp) ? 1.f : 0.f;
            float* dst = obase + (size_t)y * img_w + x;
            if (vec) *reinterpret_cast<f32x4*>(dst) = f32x4{o[0], o[1], o[2], o[3]};
            else
                for (int e = 0; e < 4 && x + e < img_w; ++e) dst[e] = o[e];
        }
    }
    if constexpr (PACKED) {
        if (stores) obase[(size_t)my_y * wq + my_j] = mine;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Where a launch set's output sizes come from: a small object that travels to the kernels BY VALUE in their arguments (no copy, no
// synchronisation per call) and is indexed by blockIdx.z, which is uniform, so its words come from the argument segment with scalar
// loads.  The host asks it the same questions: image b's size, the first element of slot d of its mask block (`base`), whether it takes
// the fused kernel.
//   UniformSizes: one img_h x img_w for every image, block b right behind block b - 1; any B up to the grid's 65535.
//   RaggedSizes : ym_after_nms_ragged's per-image {img_h, img_w, offset} table (B <= YM_RAGGED_MAX_IMAGES) and the images that fit the
//                 fused kernel (bit b of `fused_bits`).  grid.x is the largest tile count of the batch: an image that takes the
//                 two-kernel path, and tiles past an image's own count, have nothing to do.
// Bit-packed output (include/yolact_hip.h "bit-packed instance masks"): a row is wq = ceil(img_w / 64) uint64 instead of img_w floats.
// ---------------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline int fused_tiles(int img_h, int img_w) { return ((img_w + FT_W - 1) / FT_W) * ((img_h + FT_H - 1) / FT_H); }

// Does the fused kernel's LDS patch hold the source pixels of one output tile at this scale?  (Window mode scales both axes by Pv / S;
// the clamp to the physical map only ever shortens a patch.)
bool fused_fits(int Hp, int Wp, int Pv, int img_h, int img_w) {
    const int S = img_h > img_w ? img_h : img_w;
    const double sy = (double)(Pv > 0 ? Pv : Hp) / S, sx = (double)(Pv > 0 ? Pv : Wp) / S;
    return (int)(FT_H * sy) + 3 <= FP_H && (int)(FT_W * sx) + 3 <= FP_W;
}

struct UniformSizes {
    // (one vector, not two ints: the optimiser reads an 8-byte struct of two ints from the argument segment as ONE 64-bit integer and
    // then no longer sees two sign-extended 32-bit values, which costs the dense kernel ~60 instructions of 64-bit address multiplies)
    typedef int i32x2 __attribute__((ext_vector_type(2)));
    i32x2 hw;                                  // {img_h, img_w}
    __host__ __device__ int h(int) const { return hw[0]; }
    __host__ __device__ int w(int) const { return hw[1]; }
    template <bool PACKED> __host__ __device__ size_t base(int b, int max_det, int d = 0) const { return ((size_t)b * max_det + d) * (size_t)hw[0] * ym_mask_row(PACKED, hw[1]); }
    bool fused(int, int Hp, int Wp) const { return fused_fits(Hp, Wp, 0, hw[0], hw[1]); }
    __device__ bool nothing_to_do(int, int) const { return false; }
};

struct RaggedSizes {
    YmRaggedTable tab;
    unsigned fused_bits;
    __host__ __device__ int h(int b) const { return tab.img[b].img_h; }
    __host__ __device__ int w(int b) const { return tab.img[b].img_w; }
    template <bool PACKED> __host__ __device__ size_t base(int b, int, int d = 0) const { return (size_t)tab.img[b].offset + (size_t)d * h(b) * ym_mask_row(PACKED, w(b)); }
    __host__ __device__ bool fused(int b, int = 0, int = 0) const { return (fused_bits >> b) & 1u; }
    __device__ bool nothing_to_do(int b, int tile) const { return !fused(b) || tile >= fused_tiles(h(b), w(b)); }
};

// The same pixels as bits are the same kernel with another lane -> pixel map and another store (fused_tile<true>): the tile, the LDS
// patch and every floating-point expression are the dense kernel's, so a bit equals (dense value != 0).  A lane owns pixels ox0 + 64e +
// lane (e = 0..3) of its wave's four rows: one ballot per (row, e) IS one word, lane k < 16 keeps word k and the wave's 16 words leave
// as one 8-byte store per lane (four 32-byte row pieces).  A tile outside the crop window stores its 16 x 4 zero words (512 B) and
// exits; the dense [n][img_h][img_w] tensor exists nowhere.
template <bool PACKED, class Sizes>
__global__ __launch_bounds__(256) void k_masks_fused(const float* __restrict__ proto, const float* __restrict__ coefs,
                                                      const float* __restrict__ boxes, const int32_t* __restrict__ counts,
                                                      int max_det, int Hp, int Wp, int Pv, const Sizes sz, int do_crop,
                                                      typename mask_elem<PACKED>::type* __restrict__ out) {
    __shared__ float patch[FP_H * FP_W];
    __shared__ __attribute__((aligned(16))) float cf[32];
    const int b = blockIdx.z, d = blockIdx.y;
    if (sz.nothing_to_do(b, blockIdx.x)) return;
    const int img_h = sz.h(b), img_w = sz.w(b);
    const int n = counts ? counts[b] : max_det;
    if (d >= n) return;
    const size_t slot = (size_t)b * max_det + d;
    fused_tile<PACKED>(patch, cf, proto + (size_t)b * Hp * Wp * 32, coefs + slot * 32, boxes + slot * 4, blockIdx.x, Hp, Wp, Pv, img_h,
                       img_w, do_crop, out + sz.template base<PACKED>(b, max_det, d));
}

// dense {0, nonzero} rows -> words.  A wave takes PK consecutive words of the flat [rows][wq] output (PK row pieces of 64 pixels in
// flight per lane), lane u keeps word u: one 8 * PK byte store per wave.
constexpr int PK = 8;
// (workgroup `block` of the `nblocks` that share one [rows][W] tensor: k_pack_masks' whole grid, or one block's share of
// k_pack_masks_ragged's)
template <typename T>
__device__ __forceinline__ void pack_rows(const T* __restrict__ m, long long rows, int W, unsigned long long* __restrict__ out, int block,
                                          int nblocks) {
    const int wq = (W + 63) >> 6, lane = threadIdx.x & 63;
    const long long total = rows * wq;
    for (long long g = ((long long)block * 4 + (threadIdx.x >> 6)) * PK; g < total; g += (long long)nblocks * 4 * PK) {
        T v[PK];
#pragma unroll
        for (int u = 0; u < PK; ++u) {
            const long long w = g + u < total ? g + u : total - 1;
            const long long row = w / wq;
            const int x = (int)(w - row * wq) * 64 + lane;
            v[u] = x < W ? m[row * W + x] : (T)0;
        }
        unsigned long long mine = 0ull;
#pragma unroll
        for (int u = 0; u < PK; ++u) {
            const unsigned long long w = __ballot(v[u] != (T)0);
            mine = lane == u ? w : mine;
        }
        if (lane < PK && g + lane < total) out[g + lane] = mine;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_pack_masks(const T* __restrict__ m, long long rows, int W, unsigned long long* __restrict__ out) {
    pack_rows(m, rows, W, out, (int)blockIdx.x, (int)gridDim.x);
}

// The dense blocks of B images of different sizes in one launch: the sources and the table travel BY VALUE in the kernel arguments,
// a workgroup finds its image from the prefix of the images' workgroup counts and is then a workgroup of k_pack_masks for that block.
struct PackRaggedTable {
    const void* src[YM_RAGGED_MAX_IMAGES];
    long long rows[YM_RAGGED_MAX_IMAGES];          // rows_b * img_h_b
    long long out_off[YM_RAGGED_MAX_IMAGES];       // words from `bits` to the image's block
    int W[YM_RAGGED_MAX_IMAGES];
    int block_first[YM_RAGGED_MAX_IMAGES + 1];
};
template <typename T>
__global__ __launch_bounds__(256) void k_pack_masks_ragged(const PackRaggedTable t, int B, unsigned long long* __restrict__ out) {
    int b = 0;
    while (b + 1 < B && (int)blockIdx.x >= t.block_first[b + 1]) ++b;
    pack_rows(static_cast<const T*>(t.src[b]), t.rows[b], t.W[b], out + t.out_off[b], (int)blockIdx.x - t.block_first[b],
              t.block_first[b + 1] - t.block_first[b]);
}

// words -> the reference's float tensor (exactly 0.0f / 1.0f): a thread owns 4 consecutive pixels (never across a word boundary)
__global__ __launch_bounds__(256) void k_unpack_masks(const unsigned long long* __restrict__ bits, long long rows, int W, int vec,
                                                       float* __restrict__ out) {
    const int wq = (W + 63) >> 6, Q = (W + 3) >> 2;
    const long long total = rows * Q;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long row = i / Q;
        const int x0 = (int)(i - row * Q) * 4;
        const unsigned nib = (unsigned)(bits[row * wq + (x0 >> 6)] >> (x0 & 63)) & 15u;
        float* dst = out + row * W + x0;
        if (vec) {
            *reinterpret_cast<f32x4*>(dst) = f32x4{(float)(nib & 1u), (float)((nib >> 1) & 1u), (float)((nib >> 2) & 1u), (float)(nib >> 3)};
        } else {
            for (int e = 0; e < 4 && x0 + e < W; ++e) dst[e] = (float)((nib >> e) & 1u);
        }
    }
}

__global__ void k_boxes_to_pixels(float* boxes, int32_t* px, int count, float S) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) {
        const float v = boxes[i] * S;
        boxes[i] = v;
        px[i] = (int32_t)v;   // trunc toward zero, like Tensor.int()
    }
}

// the four after_nms entries: grid.y = image, scaled by its own S = max(img_h, img_w)
template <class Sizes>
__global__ void k_boxes_to_pixels_batch(float* boxes, int32_t* px, int per_image, const Sizes sz) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (i < per_image) {
        const int h = sz.h(b), w = sz.w(b);
        const size_t at = (size_t)b * per_image + i;
        const float v = boxes[at] * (float)(h > w ? h : w);
        boxes[at] = v;
        px[at] = (int32_t)v;
    }
}

}  // namespace

// n soft masks of one image; Pv as in proto_geom (ym_mask_assemble: 0)
static int mask_assemble(const float* proto, const float* coefs, const float* boxes, int n, int Hp, int Wp, int Pv, int K, int do_crop,
                         float* out, ym_stream_t s) {
    YM_REQUIRE(K == 32, "mask_assemble: coefficient dim must be 32, got %d", K);
    YM_REQUIRE(n >= 0 && Hp > 0 && Wp > 0, "mask_assemble: bad shape");
    if (n == 0) return YM_OK;
    YM_REQUIRE(proto && coefs && out && (boxes || !do_crop), "mask_assemble: null pointer");
    const int P = Hp * Wp;
    const int waves = ym_cdiv(P, 32);
    hipLaunchKernelGGL(k_mask_assemble, dim3(ym_cdiv(waves, 4)), dim3(256), 0, (hipStream_t)s, proto, coefs, boxes, n, Hp,
                       Wp, Pv, do_crop, out);
    return ym_check_launch("mask_assemble");
}

extern "C" int ym_mask_assemble(const float* proto, const float* coefs, const float* boxes, int n, int Hp, int Wp, int K,
                                int do_crop, float* out, ym_stream_t s) {
    return mask_assemble(proto, coefs, boxes, n, Hp, Wp, 0, K, do_crop, out, s);
}

// n soft masks (the device count, when given, bounds n) -> img_h x img_w binary masks, dense or packed
template <bool PACKED>
static void launch_resize(const float* masks, const int32_t* count, int n, int Hp, int Wp, int Pv, int img_h, int img_w,
                          typename mask_elem<PACKED>::type* out, hipStream_t st) {
    const size_t items = PACKED ? ((size_t)n * img_h * ym_cdiv(img_w, 64) + 3) / 4       // a wave per word
                                : ((size_t)n * img_h * ((img_w + 3) / 4) + 255) / 256;   // a thread per 4 pixels
    hipLaunchKernelGGL(k_mask_resize<PACKED>, dim3((int)(items > 16384 ? 16384 : items)), dim3(256), 0, st, masks, count, n, Hp, Wp,
                       Pv, img_h, img_w, out);
}

extern "C" int ym_mask_resize_binarize(const float* masks, int n, int Hp, int Wp, int img_h, int img_w, float* out,
                                       ym_stream_t s) {
    YM_REQUIRE(n >= 0 && Hp > 0 && Wp > 0 && img_h > 0 && img_w > 0, "mask_resize: bad shape");
    if (n == 0) return YM_OK;
    YM_REQUIRE(masks && out, "mask_resize: null pointer");
    launch_resize<false>(masks, nullptr, n, Hp, Wp, 0, img_h, img_w, out, (hipStream_t)s);
    return ym_check_launch("mask_resize");
}

extern "C" int ym_boxes_to_pixels(float* boxes_f, int32_t* boxes_px, int n, float S, ym_stream_t s) {
    YM_REQUIRE(n >= 0, "boxes_to_pixels: n < 0");
    if (n == 0) return YM_OK;
    YM_REQUIRE(boxes_f && boxes_px, "boxes_to_pixels: null pointer");
    hipLaunchKernelGGL(k_boxes_to_pixels, dim3(ym_cdiv(n * 4, 256)), dim3(256), 0, (hipStream_t)s, boxes_f, boxes_px, n * 4, S);
    return ym_check_launch("boxes_to_pixels");
}

// The launch set of the four after_nms entries (arguments checked by the caller; `what` names the entry in errors): ONE fused launch
// over every image whose scale fits it, then image by image the strongly down-scaled ones (image smaller than ~2.7x the prototype
// map) on the two-kernel path through a soft-mask scratch, then the box scaling.  Either way only the rows below counts[b] are
// written (all max_det without counts): the fused kernel's slots past the count exit, and the resize reads the count on the device.
template <bool PACKED, class Sizes>
static int after_nms_launches(const char* what, const float* proto, const float* coefs, float* boxes, const int32_t* counts, int B,
                              int max_det, int Hp, int Wp, int Pv, int K, const Sizes& sz, int do_crop,
                              typename mask_elem<PACKED>::type* masks, int32_t* boxes_px, void* workspace, size_t workspace_bytes,
                              ym_stream_t s) {
    hipStream_t st = (hipStream_t)s;
    int tiles = 0;
    for (int b = 0; b < B; ++b)
        if (sz.fused(b, Hp, Wp)) tiles = std::max(tiles, fused_tiles(sz.h(b), sz.w(b)));
    if (tiles)
        hipLaunchKernelGGL((k_masks_fused<PACKED, Sizes>), dim3(tiles, max_det, B), dim3(256), 0, st, proto, coefs, boxes, counts, max_det,
                           Hp, Wp, Pv, sz, do_crop, masks);
    for (int b = 0; b < B; ++b) {
        if (sz.fused(b, Hp, Wp)) continue;
        const size_t soft_bytes = (size_t)max_det * Hp * Wp * sizeof(float);
        if (!workspace || workspace_bytes < soft_bytes) { ym_set_error("%s: workspace %zu B < %zu B", what, workspace_bytes, soft_bytes); return YM_ENOSPC; }
        const size_t slot = (size_t)b * max_det;
        const int rc = mask_assemble(proto + (size_t)b * Hp * Wp * 32, coefs + slot * 32, boxes + slot * 4, max_det, Hp, Wp, Pv, K, do_crop,
                                     (float*)workspace, s);
        if (rc != YM_OK) return rc;
        launch_resize<PACKED>((const float*)workspace, counts ? counts + b : nullptr, max_det, Hp, Wp, Pv, sz.h(b), sz.w(b),
                              masks + sz.template base<PACKED>(b, max_det), st);
    }
    hipLaunchKernelGGL(k_boxes_to_pixels_batch<Sizes>, dim3(ym_cdiv(max_det * 4, 256), B), dim3(256), 0, st, boxes, boxes_px, max_det * 4, sz);
    return ym_check_launch(what);
}

extern "C" size_t ym_after_nms_batch_workspace_bytes(int max_det, int Hp, int Wp, int img_h, int img_w) {
    return fused_fits(Hp, Wp, 0, img_h, img_w) ? 0 : (size_t)max_det * Hp * Wp * sizeof(float);
}

extern "C" int ym_after_nms_batch(const float* proto, const float* coefs, float* boxes, const int32_t* counts, int B, int max_det,
                                  int Hp, int Wp, int K, int img_h, int img_w, int do_crop, float* masks, int32_t* boxes_px,
                                  void* workspace, size_t workspace_bytes, ym_stream_t s) {
    YM_REQUIRE(K == 32, "after_nms: coefficient dim must be 32, got %d", K);
    YM_REQUIRE(B >= 1 && B <= 65535 && max_det >= 1 && max_det <= 65535 && Hp > 0 && Wp > 0 && img_h > 0 && img_w > 0, "after_nms: bad shape");
    YM_REQUIRE(proto && coefs && boxes && masks && boxes_px, "after_nms: null pointer");
    return after_nms_launches<false>("after_nms", proto, coefs, boxes, counts, B, max_det, Hp, Wp, 0, K, UniformSizes{{img_h, img_w}}, do_crop, masks,
                                     boxes_px, workspace, workspace_bytes, s);
}

extern "C" int ym_after_nms_batch_packed(const float* proto, const float* coefs, float* boxes, const int32_t* counts, int B, int max_det,
                                         int Hp, int Wp, int K, int img_h, int img_w, int do_crop, uint64_t* mask_bits,
                                         int32_t* boxes_px, void* workspace, size_t workspace_bytes, ym_stream_t s) {
    YM_REQUIRE(K == 32, "after_nms_packed: coefficient dim must be 32, got %d", K);
    YM_REQUIRE(B >= 1 && B <= 65535 && max_det >= 1 && max_det <= 65535 && Hp > 0 && Wp > 0 && img_h > 0 && img_w > 0, "after_nms_packed: bad shape");
    YM_REQUIRE(proto && coefs && boxes && mask_bits && boxes_px, "after_nms_packed: null pointer");
    return after_nms_launches<true>("after_nms_packed", proto, coefs, boxes, counts, B, max_det, Hp, Wp, 0, K, UniformSizes{{img_h, img_w}}, do_crop,
                                    reinterpret_cast<unsigned long long*>(mask_bits), boxes_px, workspace, workspace_bytes, s);
}

// ---- batches whose images differ in size -----------------------------------------------------------------------------------------
// Checks the shape and the table; *fused = bit b set when image b takes the fused kernel.
static int ragged_check(const char* what, const ym_ragged_image* images, int B, int max_det, int Hp, int Wp, int Pv, bool packed,
                        unsigned* fused) {
    YM_REQUIRE(max_det >= 1 && max_det <= 65535 && Hp > 0 && Wp > 0, "%s: bad shape", what);
    YM_REQUIRE(Pv == 0 || (Pv >= Hp && Pv >= Wp), "%s: the %d x %d prototype map is not inside the virtual extent %d", what, Hp, Wp, Pv);
    const int rc = ym_check_ragged_table(what, images, B, packed ? 8 : 4, [=](const ym_ragged_image& im) {
        return (int64_t)max_det * im.img_h * (int64_t)ym_mask_row(packed, im.img_w);
    });
    if (rc != YM_OK) return rc;
    *fused = 0u;
    for (int b = 0; b < B; ++b)
        if (fused_fits(Hp, Wp, Pv, images[b].img_h, images[b].img_w)) *fused |= 1u << b;
    return YM_OK;
}

extern "C" size_t ym_after_nms_window_workspace_bytes(const ym_ragged_image* images, int B, int max_det, int Hp, int Wp, int Pv) {
    if (!images || B < 1 || B > YM_RAGGED_MAX_IMAGES || max_det < 1 || Hp <= 0 || Wp <= 0 || Pv < 0) return 0;
    for (int b = 0; b < B; ++b)
        if (images[b].img_h > 0 && images[b].img_w > 0 && !fused_fits(Hp, Wp, Pv, images[b].img_h, images[b].img_w))
            return (size_t)max_det * Hp * Wp * sizeof(float);
    return 0;
}

extern "C" size_t ym_after_nms_ragged_workspace_bytes(const ym_ragged_image* images, int B, int max_det, int Hp, int Wp) {
    return ym_after_nms_window_workspace_bytes(images, B, max_det, Hp, Wp, 0);
}

template <bool PACKED>
static int after_nms_ragged(const char* what, const float* proto, const float* coefs, float* boxes, const int32_t* counts, int B, int max_det,
                            int Hp, int Wp, int Pv, int K, const ym_ragged_image* images, int do_crop,
                            typename mask_elem<PACKED>::type* masks, int32_t* boxes_px, void* workspace, size_t workspace_bytes,
                            ym_stream_t s) {
    YM_REQUIRE(K == 32, "%s: coefficient dim must be 32, got %d", what, K);
    RaggedSizes sz = {};
    const int rc = ragged_check(what, images, B, max_det, Hp, Wp, Pv, PACKED, &sz.fused_bits);
    if (rc != YM_OK) return rc;
    YM_REQUIRE(proto && coefs && boxes && masks && boxes_px, "%s: null pointer", what);
    YM_REQUIRE(((uintptr_t)masks & 15) == 0, "%s: the mask buffer must be 16-byte aligned", what);
    std::copy(images, images + B, sz.tab.img);
    return after_nms_launches<PACKED>(what, proto, coefs, boxes, counts, B, max_det, Hp, Wp, Pv, K, sz, do_crop, masks, boxes_px, workspace,
                                      workspace_bytes, s);
}

extern "C" int ym_after_nms_ragged(const float* proto, const float* coefs, float* boxes, const int32_t* counts, int B, int max_det, int Hp,
                                   int Wp, int K, const ym_ragged_image* images, int do_crop, float* masks, int32_t* boxes_px,
                                   void* workspace, size_t workspace_bytes, ym_stream_t s) {
    return after_nms_ragged<false>("after_nms_ragged", proto, coefs, boxes, counts, B, max_det, Hp, Wp, 0, K, images, do_crop, masks, boxes_px,
                                   workspace, workspace_bytes, s);
}

extern "C" int ym_after_nms_ragged_packed(const float* proto, const float* coefs, float* boxes, const int32_t* counts, int B, int max_det,
                                          int Hp, int Wp, int K, const ym_ragged_image* images, int do_crop, uint64_t* mask_bits,
                                          int32_t* boxes_px, void* workspace, size_t workspace_bytes, ym_stream_t s) {
    return after_nms_ragged<true>("after_nms_ragged_packed", proto, coefs, boxes, counts, B, max_det, Hp, Wp, 0, K, images, do_crop,
                                  reinterpret_cast<unsigned long long*>(mask_bits), boxes_px, workspace, workspace_bytes, s);
}

// ---- window mode: the ragged entries with the virtual extent (one image size is the one-entry table) ---------------------------------
extern "C" int ym_after_nms_window(const float* proto, const float* coefs, float* boxes, const int32_t* counts, int B, int max_det, int Hp,
                                   int Wp, int K, const ym_ragged_image* images, int Pv, int do_crop, float* masks, int32_t* boxes_px,
                                   void* workspace, size_t workspace_bytes, ym_stream_t s) {
    YM_REQUIRE(Pv > 0, "after_nms_window: virtual prototype extent %d", Pv);
    return after_nms_ragged<false>("after_nms_window", proto, coefs, boxes, counts, B, max_det, Hp, Wp, Pv, K, images, do_crop, masks, boxes_px,
                                   workspace, workspace_bytes, s);
}

extern "C" int ym_after_nms_window_packed(const float* proto, const float* coefs, float* boxes, const int32_t* counts, int B, int max_det,
                                          int Hp, int Wp, int K, const ym_ragged_image* images, int Pv, int do_crop, uint64_t* mask_bits,
                                          int32_t* boxes_px, void* workspace, size_t workspace_bytes, ym_stream_t s) {
    YM_REQUIRE(Pv > 0, "after_nms_window_packed: virtual prototype extent %d", Pv);
    return after_nms_ragged<true>("after_nms_window_packed", proto, coefs, boxes, counts, B, max_det, Hp, Wp, Pv, K, images, do_crop,
                                  reinterpret_cast<unsigned long long*>(mask_bits), boxes_px, workspace, workspace_bytes, s);
}

extern "C" int ym_pack_masks(const void* masks, int is_u8, int n, int H, int W, uint64_t* bits, ym_stream_t s) {
    YM_REQUIRE(n >= 0 && H > 0 && W > 0, "pack_masks: bad shape");
    if (n == 0) return YM_OK;
    YM_REQUIRE(masks && bits, "pack_masks: null pointer");
    const long long rows = (long long)n * H, groups = (rows * ym_cdiv(W, 64) + PK - 1) / PK;
    const int grid = (int)((groups + 3) / 4 > 16384 ? 16384 : (groups + 3) / 4);
    unsigned long long* out = reinterpret_cast<unsigned long long*>(bits);
    if (is_u8) hipLaunchKernelGGL(k_pack_masks<uint8_t>, dim3(grid), dim3(256), 0, (hipStream_t)s, (const uint8_t*)masks, rows, W, out);
    else hipLaunchKernelGGL(k_pack_masks<float>, dim3(grid), dim3(256), 0, (hipStream_t)s, (const float*)masks, rows, W, out);
    return ym_check_launch("pack_masks");
}

extern "C" int ym_pack_masks_ragged(const void* const* src, int is_uint8, const int32_t* rows, const ym_ragged_image* images, int B,
                                    uint64_t* bits, ym_stream_t s) {
    const char* what = "pack_masks_ragged";
    YM_REQUIRE(B >= 1 && B <= YM_RAGGED_MAX_IMAGES, "%s: 1 .. %d images per call, got %d", what, YM_RAGGED_MAX_IMAGES, B);
    YM_REQUIRE(src && rows && images && bits, "%s: null pointer", what);
    for (int b = 0; b < B; ++b) YM_REQUIRE(rows[b] >= 0 && (rows[b] == 0 || src[b]), "%s: image %d: %d rows from %p", what, b, rows[b], src[b]);
    const int rc = ym_check_ragged_table(what, images, B, 8, [&](const ym_ragged_image& im) {
        return (int64_t)rows[&im - images] * im.img_h * (int64_t)ym_mask_row(true, im.img_w);
    });
    if (rc != YM_OK) return rc;
    PackRaggedTable t = {};
    for (int b = 0; b < B; ++b) {
        t.src[b] = src[b];
        t.rows[b] = (long long)rows[b] * images[b].img_h;
        t.out_off[b] = images[b].offset;
        t.W[b] = images[b].img_w;
        const long long groups = (t.rows[b] * ym_cdiv(images[b].img_w, 64) + PK - 1) / PK;     // (k_pack_masks' grid, per block)
        t.block_first[b + 1] = t.block_first[b] + (int)((groups + 3) / 4 > 16384 ? 16384 : (groups + 3) / 4);
    }
    if (t.block_first[B] == 0) return YM_OK;
    unsigned long long* out = reinterpret_cast<unsigned long long*>(bits);
    if (is_uint8) hipLaunchKernelGGL(k_pack_masks_ragged<uint8_t>, dim3((unsigned)t.block_first[B]), dim3(256), 0, (hipStream_t)s, t, B, out);
    else hipLaunchKernelGGL(k_pack_masks_ragged<float>, dim3((unsigned)t.block_first[B]), dim3(256), 0, (hipStream_t)s, t, B, out);
    return ym_check_launch(what);
}

extern "C" int ym_unpack_masks(const uint64_t* bits, int n, int H, int W, float* masks, ym_stream_t s) {
    YM_REQUIRE(n >= 0 && H > 0 && W > 0, "unpack_masks: bad shape");
    if (n == 0) return YM_OK;
    YM_REQUIRE(masks && bits, "unpack_masks: null pointer");
    const long long rows = (long long)n * H, total = rows * ((W + 3) / 4);
    const int grid = (int)((total + 255) / 256 > 16384 ? 16384 : (total + 255) / 256);
    const int vec = (W & 3) == 0 && ((uintptr_t)masks & 15) == 0;
    hipLaunchKernelGGL(k_unpack_masks, dim3(grid), dim3(256), 0, (hipStream_t)s, reinterpret_cast<const unsigned long long*>(bits), rows, W,
                       vec, masks);
    return ym_check_launch("unpack_masks");
}
