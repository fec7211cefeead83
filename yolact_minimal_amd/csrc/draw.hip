// Detection rendering for gfx950: draw_img (reference utils/output_utils.py:327-369) on the device.
//  k_draw_prep    : one wave per frame.  Reads counts / scores / ids / boxes ON THE DEVICE, drops rows past the count or under
//                   visual_thre (ballot + prefix popcount keeps the survivors in their original order, which is the draw order),
//                   formats "{name}: {score:.2f}" and writes one 96-byte record per survivor into the workspace.
//  k_draw_frame   : one pass over the output frame, a thread owns 4 consecutive pixels of a row.  Records, palette and the fps text
//                   are staged once per workgroup in LDS (uniform-address reads afterwards).  Per detection one 16-byte mask load
//                   (16 of them in flight per wave), integer class sum, palette blend (4c + 6v + 5) / 10, then boxes / plates /
//                   glyphs by walking the records upward until the first hit ("smallest i wins" == the reference's reversed draw loop), then the fps overlay;
//                   12 output bytes leave as three dword stores.  Bound by the n*H*W*4 mask bytes it reads.
//                   The <false> instance is the element-wise path for rows whose width is not a multiple of 4 (or unaligned bases).
//  k_cutout_object: per-detection matte (img where mask != 0 else 255), full frame; the caller slices the box window.
//  k_draw_frame<VEC, true> / k_cutout_object_packed: the mask term read from bit-packed masks (one 8-byte word serves 64 pixels
//                   of a detection), same bytes out.
//  k_draw_frame<VEC, PACKED, Sizes>: where frame b and its mask block lie comes from a small object in the kernel arguments, like
//                   k_masks_fused's (masks.hip): UniformSizes = one H x W, frame b right behind frame b - 1 (ym_draw_detections_batch);
//                   RaggedSizes = ym_draw_detections_ragged's two per-image tables.
//  Host side: the four ym_draw_detections_* entries check what is their own, build their Sizes and share ONE launch path,
//                   draw_launches<Sizes>, over their common arguments (DrawArgs).  It asks the Sizes which images take VEC = true and
//                   which VEC = false and launches each non-empty set once: a uniform batch is one set (any B up to 65535); a ragged
//                   batch decides per image (bit b of `set_bits` = image b belongs to this launch, B <= YM_RAGGED_MAX_IMAGES), grid.x
//                   is the set's largest tile count and workgroups past an image's own count return at once.
// All arithmetic is integer; results are exact (tests compare with tolerance 0).
#include <algorithm>
#include "ym_common.h"

namespace {

constexpr int ADV = YM_DRAW_FONT_ADVANCE, TH = YM_DRAW_FONT_HEIGHT;
constexpr int REC = 24;            // ints per record
constexpr int HDR = 16;            // ints per frame header: [0] survivors, [1] fps text length, [2..9] fps text
constexpr int PAL = 256;           // palette slots staged in LDS
constexpr int R_ID = 0, R_SRC = 1, R_X1 = 2, R_Y1 = 3, R_X2 = 4, R_Y2 = 5, R_TW = 6, R_LEN = 7, R_UX0 = 8, R_UX1 = 9, R_UY0 = 10,
              R_UY1 = 11, R_COL = 12, R_TEXT = 13;
constexpr int COORD_LIM = 1 << 24; // box corners are clamped here: far outside any frame, so clipping hides the clamp
constexpr int FRAME_THREADS = 128;

static_assert((REC - R_TEXT) * 4 == YM_DRAW_LABEL_MAX, "label bytes per record");
static_assert(REC % 4 == 0 && HDR % 4 == 0 && PAL % 4 == 0, "records are staged as 16-byte pieces");

__device__ __forceinline__ int clampi(long long v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : (int)v); }

__device__ __forceinline__ unsigned pack_bgr(const uint8_t* p) { return p[0] | (p[1] << 8) | (p[2] << 16); }

struct LabelWriter {
    char* t;
    int len;
    __device__ __forceinline__ void put(int c) {
        if (len < YM_DRAW_LABEL_MAX) t[len++] = (char)((c < 0x20 || c > 0x7E) ? '?' : c);
    }
};

// f'{score:.2f}': cents = rint(double(score) * 100) (the product is exact in double, rint is round-half-to-even), sign first.
__device__ void put_score(LabelWriter& w, float sc) {
    if (sc != sc) { w.put('n'); w.put('a'); w.put('n'); return; }
    if (__builtin_signbit(sc)) w.put('-');
    const double a = fabs((double)sc);
    if (a > 3.0e38) { w.put('i'); w.put('n'); w.put('f'); return; }
    double c = rint(a * 100.0);
    if (c > 1.0e17) c = 1.0e17;               // scores are probabilities; digits past 1e15 are not promised
    const unsigned long long u = (unsigned long long)c;
    const unsigned long long ip = u / 100;
    const int frac = (int)(u % 100);
    unsigned long long p = 1;
    while (ip / p >= 10) p *= 10;
    for (; p; p /= 10) w.put('0' + (int)((ip / p) % 10));
    w.put('.');
    w.put('0' + frac / 10);
    w.put('0' + frac % 10);
}

__global__ __launch_bounds__(64) void k_draw_prep(const int64_t* __restrict__ ids, const float* __restrict__ scores,
                                                  const int32_t* __restrict__ boxes, const int32_t* __restrict__ counts, int max_det,
                                                  const uint8_t* __restrict__ palette, int palette_n, const char* __restrict__ names,
                                                  int num_names, int flags, float thre, unsigned long long f0, unsigned long long f1,
                                                  unsigned long long f2, unsigned long long f3, int fps_len, int* __restrict__ ws) {
    __shared__ int name_lds[64][YM_DRAW_NAME_STRIDE / 4 + 1];      // a lane's class-name row (+1: rows on different banks)
    const int b = blockIdx.x, lane = threadIdx.x;
    int* hdr = ws + (size_t)b * (HDR + (size_t)max_det * REC);
    int* recs = hdr + HDR;
    int cnt = max_det;
    if (counts) cnt = clampi(counts[b], 0, max_det);
    int running = 0;
    for (int base = 0; base < cnt; base += 64) {
        const int i = base + lane;
        bool ok = i < cnt;
        const size_t row = (size_t)b * max_det + i;
        const float sc = (ok && scores) ? scores[row] : 0.f;
        if (ok && thre > 0.f && !(sc >= thre)) ok = false;      // after_nms: keep = class_p >= visual_thre (only when it is > 0)
        const unsigned long long m = __ballot(ok);
        if (ok) {
            int* r = recs + (size_t)(running + __popcll(m & ((1ull << lane) - 1ull))) * REC;
            const int id = clampi(ids[row], -COORD_LIM, COORD_LIM);
            const int x1 = clampi(boxes[row * 4 + 0], -COORD_LIM, COORD_LIM), y1 = clampi(boxes[row * 4 + 1], -COORD_LIM, COORD_LIM);
            const int x2 = clampi(boxes[row * 4 + 2], -COORD_LIM, COORD_LIM), y2 = clampi(boxes[row * 4 + 3], -COORD_LIM, COORD_LIM);
            LabelWriter w{reinterpret_cast<char*>(r + R_TEXT), 0};
            if (id >= 0 && id < num_names) {
                // the row comes in as 10 independent dword loads; the byte loop then reads LDS instead of paying a global
                // latency per character
                const int* nrow = reinterpret_cast<const int*>(names) + (size_t)id * (YM_DRAW_NAME_STRIDE / 4);
#pragma unroll
                for (int j = 0; j < YM_DRAW_NAME_STRIDE / 4; ++j) name_lds[lane][j] = nrow[j];
                const unsigned char* nm = reinterpret_cast<const unsigned char*>(name_lds[lane]);
                for (int j = 0; j < YM_DRAW_NAME_STRIDE - 1 && nm[j]; ++j) w.put(nm[j]);
            } else {
                w.put('?');
            }
            if (!(flags & YM_DRAW_HIDE_SCORE)) {
                w.put(':');
                w.put(' ');
                put_score(w, sc);
            }
            const int tw = w.len * ADV;
            int ci = (id + 1) % palette_n;
            if (ci < 0) ci += palette_n;
            r[R_ID] = id;
            r[R_SRC] = i;
            r[R_X1] = x1;
            r[R_Y1] = y1;
            r[R_X2] = x2;
            r[R_Y2] = y2;
            r[R_TW] = tw;
            r[R_LEN] = w.len;
            r[R_UX0] = min(x1, x2);
            r[R_UX1] = max(max(x1, x2), x1 + tw);
            r[R_UY0] = min(y1, y2);
            r[R_UY1] = max(max(y1, y2), y1 + TH + 5);
            r[R_COL] = (int)pack_bgr(palette + ci * 3);
        }
        running += __popcll(m);
    }
    if (lane == 0) {
        hdr[0] = running;
        hdr[1] = fps_len;
        hdr[2] = (int)(unsigned)f0; hdr[3] = (int)(unsigned)(f0 >> 32);
        hdr[4] = (int)(unsigned)f1; hdr[5] = (int)(unsigned)(f1 >> 32);
        hdr[6] = (int)(unsigned)f2; hdr[7] = (int)(unsigned)(f2 >> 32);
        hdr[8] = (int)(unsigned)f3; hdr[9] = (int)(unsigned)(f3 >> 32);
    }
}

// Is pixel (cx, row) of a text line set?  cx >= 0 counts from the line's left edge, row in [0, TH) from the cell's top.
// `text` holds the bytes packed little-endian in LDS words; every byte is in 0x20..0x7E (k_draw_prep / the host guarantee it).
__device__ __forceinline__ bool glyph_bit(const int* text, int len, int cx, int row, const uint16_t* __restrict__ font) {
    const int k = cx / ADV;
    if (k >= len) return false;
    const int ch = (text[k >> 2] >> ((k & 3) * 8)) & 0xff;
    const unsigned bits = font[(ch - 0x20) * TH + row];
    return (bits >> (cx - k * ADV)) & 1u;
}

__device__ __forceinline__ unsigned blend(unsigned c, unsigned v) {
    unsigned o = 0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const unsigned cc = (c >> (8 * ch)) & 0xff, vv = (v >> (8 * ch)) & 0xff;
        o |= ((4 * cc + 6 * vv + 5) / 10) << (8 * ch);
    }
    return o;
}

__device__ __forceinline__ unsigned shade(unsigned v) {
    unsigned o = 0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) o |= ((3 * ((v >> (8 * ch)) & 0xff)) / 5) << (8 * ch);
    return o;
}

template <bool VEC>
__device__ __forceinline__ void load_px(const uint8_t* p, int npx, unsigned (&px)[4]) {
    if (VEC) {
        const unsigned* d = reinterpret_cast<const unsigned*>(p);
        const unsigned d0 = d[0], d1 = d[1], d2 = d[2];
        px[0] = d0 & 0xffffffu;
        px[1] = (d0 >> 24) | ((d1 & 0xffffu) << 8);
        px[2] = (d1 >> 16) | ((d2 & 0xffu) << 16);
        px[3] = d2 >> 8;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) px[k] = k < npx ? pack_bgr(p + 3 * k) : 0u;
    }
}

template <bool VEC>
__device__ __forceinline__ void store_px(uint8_t* p, int npx, const unsigned (&px)[4]) {
    if (VEC) {
        unsigned* d = reinterpret_cast<unsigned*>(p);
        d[0] = px[0] | (px[1] << 24);
        d[1] = (px[1] >> 8) | (px[2] << 16);
        d[2] = (px[2] >> 16) | (px[3] << 8);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < npx) {
                p[3 * k + 0] = (uint8_t)px[k];
                p[3 * k + 1] = (uint8_t)(px[k] >> 8);
                p[3 * k + 2] = (uint8_t)(px[k] >> 16);
            }
    }
}

// U detections' 16-byte mask loads issued back to back, then the class sum: written out as two loops because the compiler otherwise
// waits for each load before it issues the next (one load in flight per wave, and a wave owns only 256 pixels).
template <int U>
__device__ __forceinline__ void mask_batch(const int* recs, const float* mp, size_t HW, int (&s)[4]) {
    f32x4 m[U];
    int w[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        w[u] = recs[u * REC + R_ID] + 1;
        m[u] = *reinterpret_cast<const f32x4*>(mp + (size_t)recs[u * REC + R_SRC] * HW);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] += (int)m[u][k] * w[u];
}

// The same for bit-packed masks (include/yolact_hip.h "bit-packed instance masks"): `bp` points at the word of detection slot 0 that
// holds this thread's 4 pixels (4 | 64: never two words), `sh` is their bit offset.  A wave's 256 pixels lie in at most 5 words
// per detection, so these are broadcast loads.
template <int U>
__device__ __forceinline__ void bits_batch(const int* recs, const unsigned long long* bp, size_t HWq, int sh, int (&s)[4]) {
    unsigned long long m[U];
    int w[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        w[u] = recs[u * REC + R_ID] + 1;
        m[u] = bp[(size_t)recs[u * REC + R_SRC] * HWq];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const unsigned nib = (unsigned)(m[u] >> sh);
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] += (int)((nib >> k) & 1u) * w[u];
    }
}

__host__ __device__ inline int frame_tiles(int H, int W) { return (H * ((W + 3) >> 2) + FRAME_THREADS - 1) / FRAME_THREADS; }

// What the four ym_draw_detections_* entries share: their arguments as one plain host struct (`masks`: float [max_det][H][W] per
// image, or -- `packed` -- the bit rows uint64 [max_det][H][ceil(W / 64)]; `cutout_total`: the uniform entries only).
struct DrawArgs {
    const uint8_t* img; const void* masks; bool packed; const int64_t* ids; const float* scores; const int32_t* boxes_px;
    const int32_t* counts; int B, max_det; const uint8_t* palette; int palette_n, num_classes; const char* names; int num_names;
    const uint16_t* font; int flags; float visual_thre; const char* fps_text; uint8_t* out; uint8_t* cutout_total; void* workspace;
    size_t workspace_bytes; ym_stream_t s;
    bool reads_masks() const { return !(flags & YM_DRAW_HIDE_MASK) && max_det > 0; }
    // may a W pixels wide frame `at` bytes into img / out, its mask block `block` elements into masks, take k_draw_frame<true>?
    bool vec_ok(int W, size_t at, size_t block) const {
        const uintptr_t m = (uintptr_t)masks + block * (packed ? 8 : 4);
        return W % 4 == 0 && ((uintptr_t)img + at) % 4 == 0 && ((uintptr_t)out + at) % 4 == 0 && (uintptr_t)cutout_total % 4 == 0 &&
               (!reads_masks() || m % 16 == 0 || (packed && m % 8 == 0));
    }
};

// first_byte(b, y, x): where pixel (y, x) of frame b starts in img / out / cut_total; masks(b): first element (float, or word when
// packed) of its mask block.  The host asks select(vec, a): the largest tile count among the images that take k_draw_frame<vec>
// (0 = no launch).
struct UniformSizes {
    typedef int i32x2 __attribute__((ext_vector_type(2)));      // (one vector, not two ints: see masks.hip's UniformSizes)
    i32x2 hw;                                                   // {H, W}
    __host__ __device__ int h(int) const { return hw[0]; }
    __host__ __device__ int w(int) const { return hw[1]; }
    __device__ size_t first_byte(int b, int y, int x) const { return (((size_t)b * hw[0] + y) * hw[1] + x) * 3; }
    __device__ size_t masks(int b, int max_det, bool packed) const { return (size_t)b * max_det * hw[0] * ym_mask_row(packed, hw[1]); }
    __device__ bool nothing_to_do(int, int) const { return false; }
    // all images or none: image 0's answer holds for every image, since with W % 4 == 0 every frame stride H * W * 3 is a multiple of
    // 4, every dense mask stride one of 16 bytes and every packed one of 8
    int select(bool vec, const DrawArgs& a) const { return vec == a.vec_ok(hw[1], 0, 0) ? frame_tiles(hw[0], hw[1]) : 0; }
};

struct RaggedSizes {
    YmRaggedTable frames, blocks;
    unsigned set_bits;
    __host__ __device__ int h(int b) const { return frames.img[b].img_h; }
    __host__ __device__ int w(int b) const { return frames.img[b].img_w; }
    __device__ size_t first_byte(int b, int y, int x) const { return (size_t)frames.img[b].offset + ((size_t)y * w(b) + x) * 3; }
    __device__ size_t masks(int b, int, bool) const { return (size_t)blocks.img[b].offset; }
    __device__ bool nothing_to_do(int b, int tile) const { return !((set_bits >> b) & 1u) || tile >= frame_tiles(h(b), w(b)); }
    // image by image (a.B <= YM_RAGGED_MAX_IMAGES = the bits of `set_bits`), which it records for the kernel
    int select(bool vec, const DrawArgs& a) {
        int tiles = 0;
        set_bits = 0u;
        for (int b = 0; b < a.B; ++b)
            if (vec == a.vec_ok(w(b), frames.img[b].offset, blocks.img[b].offset)) {
                set_bits |= 1u << b;
                tiles = std::max(tiles, frame_tiles(h(b), w(b)));
            }
        return tiles;
    }
};

// (`sz` BEFORE `max_det`: UniformSizes' two ints then lie where `H, W` always lay and come in with the first scalar load; behind
// `max_det` the 8-byte aligned struct leaves a hole, and the frame size is fetched by a load of its own in front of the barrier)
template <bool VEC, bool PACKED, class Sizes>
__global__ __launch_bounds__(FRAME_THREADS) void k_draw_frame(const uint8_t* __restrict__ img, const void* __restrict__ masks_v,
                                                              const int* __restrict__ ws, const Sizes sz, int max_det,
                                                              const uint8_t* __restrict__ palette, int palette_n, int modulus,
                                                              const uint16_t* __restrict__ font, int flags, uint8_t* out,
                                                              uint8_t* cut_total) {
    extern __shared__ int lds[];
    int* pal = lds;                 // [PAL] packed BGR
    int* hdr = lds + PAL;           // [HDR]
    int* recs = hdr + HDR;          // [n][REC]
    const int b = blockIdx.y, tid = threadIdx.x;
    if (sz.nothing_to_do(b, blockIdx.x)) return;            // (uniform over the workgroup: nobody is left at the barrier)
    const int H = sz.h(b), W = sz.w(b);
    const int* wsb = ws + (size_t)b * (HDR + (size_t)max_det * REC);
    const int n = max(0, min(wsb[0], max_det));
    for (int j = tid; j < palette_n; j += FRAME_THREADS) pal[j] = (int)pack_bgr(palette + j * 3);
    {   // header + records as 16-byte pieces, 4 loads per thread issued before the first LDS write
        const int4* src = reinterpret_cast<const int4*>(wsb);
        int4* dst = reinterpret_cast<int4*>(hdr);
        const int total4 = (HDR + n * REC) / 4;
        for (int j0 = 0; j0 < total4; j0 += 4 * FRAME_THREADS) {
            int4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + u * FRAME_THREADS + tid;
                v[u] = src[min(j, total4 - 1)];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + u * FRAME_THREADS + tid;
                if (j < total4) dst[j] = v[u];
            }
        }
    }
    __syncthreads();

    const int Q = (W + 3) >> 2;
    const int q = blockIdx.x * FRAME_THREADS + tid;
    if (q >= H * Q) return;
    const int y = q / Q, x0 = (q - y * Q) * 4;
    const int npx = min(4, W - x0);
    const size_t pix = sz.first_byte(b, y, x0);                         // first byte of this thread's pixels
    unsigned px[4];
    load_px<VEC>(img + pix, npx, px);
    if (n == 0) {                                            // no detection: the frame comes back unchanged (draw_img's early return)
        store_px<VEC>(out + pix, npx, px);
        if (cut_total) {
            const unsigned white[4] = {0xffffffu, 0xffffffu, 0xffffffu, 0xffffffu};
            store_px<VEC>(cut_total + pix, npx, white);
        }
        return;
    }

    if (!(flags & YM_DRAW_HIDE_MASK)) {
        int s[4] = {0, 0, 0, 0};
        int i = 0;
        if (PACKED) {
            const int wq = (W + 63) >> 6, sh = x0 & 63;
            const size_t HWq = (size_t)H * wq;
            const unsigned long long* bp = static_cast<const unsigned long long*>(masks_v) + sz.masks(b, max_det, true) + (size_t)y * wq + (x0 >> 6);
            for (; i + 16 <= n; i += 16) bits_batch<16>(recs + i * REC, bp, HWq, sh, s);
            for (; i + 4 <= n; i += 4) bits_batch<4>(recs + i * REC, bp, HWq, sh, s);
            for (; i < n; ++i) bits_batch<1>(recs + i * REC, bp, HWq, sh, s);
        }
        const size_t HW = (size_t)H * W;
        const float* mp = static_cast<const float*>(masks_v) + (PACKED ? 0 : sz.masks(b, max_det, false)) + (size_t)y * W + x0;
        if (VEC && !PACKED) {
            for (; i + 16 <= n; i += 16) mask_batch<16>(recs + i * REC, mp, HW, s);
            for (; i + 4 <= n; i += 4) mask_batch<4>(recs + i * REC, mp, HW, s);
        }
        for (; i < n; ++i) {
            const int idp1 = recs[i * REC + R_ID] + 1;
            const float* mi = mp + (size_t)recs[i * REC + R_SRC] * HW;
            if (VEC) {
                const f32x4 m = *reinterpret_cast<const f32x4*>(mi);
#pragma unroll
                for (int k = 0; k < 4; ++k) s[k] += (int)m[k] * idp1;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < npx) s[k] += (int)mi[k] * idp1;
            }
        }
        unsigned cut[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int sm = s[k] % modulus;
            if (sm < 0) sm += modulus;
            cut[k] = sm != 0 ? px[k] : 0xffffffu;
            px[k] = blend((unsigned)pal[sm], px[k]);
        }
        if (cut_total) store_px<VEC>(cut_total + pix, npx, cut);
    }

    if (!(flags & YM_DRAW_HIDE_BBOX)) {
        unsigned pending = (1u << npx) - 1u;
        for (int i = 0; i < n && pending; ++i) {
            const int* r = recs + i * REC;
            if (y < r[R_UY0] || y > r[R_UY1] || x0 + 3 < r[R_UX0] || x0 > r[R_UX1]) continue;
            const int x1 = r[R_X1], y1 = r[R_Y1], x2 = r[R_X2], y2 = r[R_Y2];
            const int bx0 = min(x1, x2), bx1 = max(x1, x2), by0 = min(y1, y2), by1 = max(y1, y2);
            const bool on_h = y == y1 || y == y2, in_y = y >= by0 && y <= by1;
            const bool plate_y = y >= y1 && y <= y1 + TH + 5;
            const int row = y - (y1 + 15 - (TH - 1));
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!((pending >> k) & 1u)) continue;
                const int x = x0 + k;
                const bool outline = (on_h && x >= bx0 && x <= bx1) || (in_y && (x == x1 || x == x2));
                const bool plate = plate_y && x >= x1 && x <= x1 + r[R_TW];
                if (!(outline || plate)) continue;
                unsigned c = (unsigned)r[R_COL];
                if (plate && row >= 0 && row < TH && glyph_bit(r + R_TEXT, r[R_LEN], x - x1, row, font)) c = 0xffffffu;
                px[k] = c;
                pending &= ~(1u << k);
            }
        }
    }

    if ((flags & YM_DRAW_REAL_TIME) && y < TH + 8) {
        const int flen = hdr[1];
        const int row = y - 3;                              // baseline at y = TH + 2
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int x = x0 + k;
            if (k < npx && x < flen * ADV + 8) {
                px[k] = shade(px[k]);
                if (row >= 0 && row < TH && glyph_bit(hdr + 2, flen, x, row, font)) px[k] = 0xffffffu;
            }
        }
    }
    store_px<VEC>(out + pix, npx, px);
}

__global__ __launch_bounds__(256) void k_cutout_object(const uint8_t* __restrict__ img, const float* __restrict__ masks, int HW,
                                                       uint8_t* __restrict__ out) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const size_t o = (size_t)blockIdx.y * HW + p;
    const bool in = masks[o] != 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[o * 3 + c] = in ? img[(size_t)p * 3 + c] : (uint8_t)255;
}

__global__ __launch_bounds__(256) void k_cutout_object_packed(const uint8_t* __restrict__ img, const unsigned long long* __restrict__ bits,
                                                              int H, int W, uint8_t* __restrict__ out) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= H * W) return;
    const int y = p / W, x = p - y * W, wq = (W + 63) >> 6;
    const size_t o = (size_t)blockIdx.y * H * W + p;
    const bool in = (bits[((size_t)blockIdx.y * H + y) * wq + (x >> 6)] >> (x & 63)) & 1ull;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[o * 3 + c] = in ? img[(size_t)p * 3 + c] : (uint8_t)255;
}

bool frame_dims_ok(int H, int W) { return H >= 1 && W >= 1 && H <= 16384 && W <= 16384; }

}  // namespace

extern "C" size_t ym_draw_workspace_bytes(int B, int max_det) {
    if (B < 1 || max_det < 0 || max_det > YM_DRAW_MAX_DET) {
        ym_set_error("ym_draw_workspace_bytes: B >= 1 and 0 <= max_det <= %d required (B=%d max_det=%d)", YM_DRAW_MAX_DET, B, max_det);
        return 0;
    }
    return (size_t)B * (HDR + (size_t)max_det * REC) * sizeof(int);
}

// What every draw entry checks besides its frame sizes (`what` names the entry in errors).
static int draw_check(const char* what, const DrawArgs& a, int max_B) {
    YM_REQUIRE(a.B >= 1 && a.B <= max_B && a.max_det >= 0 && a.max_det <= YM_DRAW_MAX_DET, "%s: 1 <= B <= %d and 0 <= max_det <= %d required (B=%d max_det=%d)",
               what, max_B, YM_DRAW_MAX_DET, a.B, a.max_det);
    YM_REQUIRE(a.img && a.out && a.palette && a.font && a.workspace, "%s: null img / out / palette / font / workspace", what);
    YM_REQUIRE(a.max_det == 0 || (a.ids && a.boxes_px && a.names), "%s: null ids / boxes_px / names", what);
    YM_REQUIRE(((uintptr_t)a.names & 3) == 0, "%s: the class-name table must be 4-byte aligned", what);
    YM_REQUIRE(!a.reads_masks() || a.masks, "%s: masks are needed unless YM_DRAW_HIDE_MASK is set", what);
    YM_REQUIRE(!a.cutout_total || !(a.flags & YM_DRAW_HIDE_MASK), "%s: the cutout matte needs the masks (YM_DRAW_HIDE_MASK is set)", what);
    YM_REQUIRE(a.scores || ((a.flags & YM_DRAW_HIDE_SCORE) && !(a.visual_thre > 0.f)) || a.max_det == 0,
               "%s: scores are needed for the labels and for visual_thre", what);
    YM_REQUIRE(a.num_classes >= 2 && a.palette_n >= 1 && a.palette_n <= PAL && a.num_classes - 1 <= a.palette_n && a.num_names >= 0,
               "%s: num_classes=%d needs a palette of at least num_classes-1 (<= %d) colours, got %d", what, a.num_classes, PAL, a.palette_n);
    const size_t need = ym_draw_workspace_bytes(a.B, a.max_det);
    YM_REQUIRE(a.workspace_bytes >= need && ((uintptr_t)a.workspace & 15) == 0, "%s: workspace of %zu bytes (16-byte aligned) needed, got %zu",
               what, need, a.workspace_bytes);
    YM_REQUIRE(!a.packed || (uintptr_t)a.masks % 8 == 0, "%s: the mask words must be 8-byte aligned", what);
    YM_REQUIRE(a.fps_text || !(a.flags & YM_DRAW_REAL_TIME), "%s: YM_DRAW_REAL_TIME needs the fps text", what);
    return YM_OK;
}

// The launch set of the four entries (arguments checked by the caller): the prep launch, then k_draw_frame<true> over the images that
// take the 16-byte instance and k_draw_frame<false> over the others; an empty set is not launched.
template <class Sizes>
static int draw_launches(const DrawArgs& a, Sizes sz) {
    unsigned long long f[4] = {0, 0, 0, 0};                  // the fps text packed for k_draw_prep
    int fps_len = 0;
    if (a.flags & YM_DRAW_REAL_TIME)
        for (; fps_len < 32 && a.fps_text[fps_len]; ++fps_len) {
            const unsigned char c = (unsigned char)a.fps_text[fps_len];
            f[fps_len >> 3] |= (unsigned long long)((c < 0x20 || c > 0x7E) ? '?' : c) << ((fps_len & 7) * 8);
        }
    hipStream_t st = (hipStream_t)a.s;
    k_draw_prep<<<a.B, 64, 0, st>>>(a.ids, a.scores, a.boxes_px, a.counts, a.max_det, a.palette, a.palette_n, a.names, a.num_names, a.flags,
                                    a.visual_thre, f[0], f[1], f[2], f[3], fps_len, (int*)a.workspace);
    const int rc = ym_check_launch("k_draw_prep");
    if (rc != YM_OK) return rc;
    const size_t lds = (size_t)(PAL + HDR + a.max_det * REC) * sizeof(int);
#define YM_DRAW_FRAME(V, P)                                                                                                         \
    k_draw_frame<V, P, Sizes><<<grid, FRAME_THREADS, lds, st>>>(a.img, a.masks, (const int*)a.workspace, sz, a.max_det, a.palette,  \
                                                                a.palette_n, a.num_classes - 1, a.font, a.flags, a.out, a.cutout_total)
    for (int vec = 1; vec >= 0; --vec) {
        const int tiles = sz.select(vec, a);
        if (!tiles) continue;
        const dim3 grid(tiles, a.B);
        if (a.packed) { if (vec) YM_DRAW_FRAME(true, true); else YM_DRAW_FRAME(false, true); }
        else { if (vec) YM_DRAW_FRAME(true, false); else YM_DRAW_FRAME(false, false); }
    }
#undef YM_DRAW_FRAME
    return ym_check_launch("k_draw_frame");
}

// One H x W for every frame, frame b right behind frame b - 1; any B up to the grid's 65535.
static int draw_uniform(const char* what, const DrawArgs& a, int H, int W) {
    YM_REQUIRE(frame_dims_ok(H, W), "%s: frame %dx%d out of range (1..16384)", what, H, W);
    const int rc = draw_check(what, a, 65535);
    if (rc != YM_OK) return rc;
    return draw_launches(a, UniformSizes{{H, W}});
}

// `frames`: frame b's size and its first byte in img AND out; `mask_blocks`: ym_after_nms_ragged[_packed]'s table (NULL with
// YM_DRAW_HIDE_MASK: the masks are not read)
static int draw_ragged(const char* what, const DrawArgs& a, const ym_ragged_image* frames, const ym_ragged_image* mask_blocks) {
    const int B = a.B, max_det = a.max_det;
    const bool packed = a.packed;
    int rc = ym_check_ragged_table(what, frames, B, 1, [](const ym_ragged_image& im) { return (int64_t)im.img_h * im.img_w * 3; });
    if (rc != YM_OK) return rc;
    for (int b = 0; b < B; ++b)
        YM_REQUIRE(frame_dims_ok(frames[b].img_h, frames[b].img_w), "%s: frame %d is %dx%d, out of range (1..16384)", what, b,
                   frames[b].img_h, frames[b].img_w);
    rc = draw_check(what, a, YM_RAGGED_MAX_IMAGES);
    if (rc != YM_OK) return rc;
    const bool read_masks = a.reads_masks();
    YM_REQUIRE(mask_blocks || !read_masks, "%s: the mask block table is needed unless YM_DRAW_HIDE_MASK is set", what);
    RaggedSizes sz = {};
    std::copy(frames, frames + B, sz.frames.img);
    if (read_masks) {
        rc = ym_check_ragged_table(what, mask_blocks, B, packed ? 8 : 4, [=](const ym_ragged_image& im) {
            return (int64_t)max_det * im.img_h * (int64_t)ym_mask_row(packed, im.img_w);
        });
        if (rc != YM_OK) return rc;
        for (int b = 0; b < B; ++b)
            YM_REQUIRE(mask_blocks[b].img_h == frames[b].img_h && mask_blocks[b].img_w == frames[b].img_w,
                       "%s: image %d: masks of %d x %d for a frame of %d x %d", what, b, mask_blocks[b].img_h, mask_blocks[b].img_w,
                       frames[b].img_h, frames[b].img_w);
        std::copy(mask_blocks, mask_blocks + B, sz.blocks.img);
    }
    return draw_launches(a, sz);
}

extern "C" int ym_draw_detections_batch(const uint8_t* img, const float* masks, const int64_t* ids, const float* scores,
                                        const int32_t* boxes_px, const int32_t* counts, int B, int max_det, int H, int W,
                                        const uint8_t* palette, int palette_n, int num_classes, const char* names, int num_names,
                                        const uint16_t* font, int flags, float visual_thre, const char* fps_text, uint8_t* out,
                                        uint8_t* cutout_total, void* workspace, size_t workspace_bytes, ym_stream_t s) {
    return draw_uniform("ym_draw_detections_batch", {img, masks, false, ids, scores, boxes_px, counts, B, max_det, palette, palette_n, num_classes,
                        names, num_names, font, flags, visual_thre, fps_text, out, cutout_total, workspace, workspace_bytes, s}, H, W);
}

extern "C" int ym_draw_detections_batch_packed(const uint8_t* img, const uint64_t* mask_bits, const int64_t* ids, const float* scores,
                                               const int32_t* boxes_px, const int32_t* counts, int B, int max_det, int H, int W,
                                               const uint8_t* palette, int palette_n, int num_classes, const char* names, int num_names,
                                               const uint16_t* font, int flags, float visual_thre, const char* fps_text, uint8_t* out,
                                               uint8_t* cutout_total, void* workspace, size_t workspace_bytes, ym_stream_t s) {
    return draw_uniform("ym_draw_detections_batch_packed", {img, mask_bits, true, ids, scores, boxes_px, counts, B, max_det, palette, palette_n,
                        num_classes, names, num_names, font, flags, visual_thre, fps_text, out, cutout_total, workspace, workspace_bytes, s}, H, W);
}

extern "C" int ym_draw_detections_ragged(const uint8_t* img, const float* masks, const int64_t* ids, const float* scores,
                                         const int32_t* boxes_px, const int32_t* counts, int B, int max_det,
                                         const ym_ragged_image* frames, const ym_ragged_image* mask_blocks, const uint8_t* palette,
                                         int palette_n, int num_classes, const char* names, int num_names, const uint16_t* font,
                                         int flags, float visual_thre, const char* fps_text, uint8_t* out, void* workspace,
                                         size_t workspace_bytes, ym_stream_t s) {
    return draw_ragged("ym_draw_detections_ragged", {img, masks, false, ids, scores, boxes_px, counts, B, max_det, palette, palette_n, num_classes,
                       names, num_names, font, flags, visual_thre, fps_text, out, nullptr, workspace, workspace_bytes, s}, frames, mask_blocks);
}

extern "C" int ym_draw_detections_ragged_packed(const uint8_t* img, const uint64_t* mask_bits, const int64_t* ids, const float* scores,
                                                const int32_t* boxes_px, const int32_t* counts, int B, int max_det,
                                                const ym_ragged_image* frames, const ym_ragged_image* mask_blocks,
                                                const uint8_t* palette, int palette_n, int num_classes, const char* names,
                                                int num_names, const uint16_t* font, int flags, float visual_thre,
                                                const char* fps_text, uint8_t* out, void* workspace, size_t workspace_bytes,
                                                ym_stream_t s) {
    return draw_ragged("ym_draw_detections_ragged_packed", {img, mask_bits, true, ids, scores, boxes_px, counts, B, max_det, palette, palette_n,
                       num_classes, names, num_names, font, flags, visual_thre, fps_text, out, nullptr, workspace, workspace_bytes, s}, frames,
                       mask_blocks);
}

extern "C" int ym_draw_cutout_objects(const uint8_t* img, const float* masks, int n, int H, int W, uint8_t* out, ym_stream_t s) {
    YM_REQUIRE(n >= 1 && n <= 65535 && frame_dims_ok(H, W), "ym_draw_cutout_objects: 1 <= n <= 65535 and a frame of 1..16384 per side required (n=%d %dx%d)", n, H, W);
    YM_REQUIRE(img && masks && out, "ym_draw_cutout_objects: null pointer");
    k_cutout_object<<<dim3(ym_cdiv(H * W, 256), n), 256, 0, (hipStream_t)s>>>(img, masks, H * W, out);
    return ym_check_launch("k_cutout_object");
}

extern "C" int ym_draw_cutout_objects_packed(const uint8_t* img, const uint64_t* mask_bits, int n, int H, int W, uint8_t* out, ym_stream_t s) {
    YM_REQUIRE(n >= 1 && n <= 65535 && frame_dims_ok(H, W), "ym_draw_cutout_objects_packed: 1 <= n <= 65535 and a frame of 1..16384 per side required (n=%d %dx%d)", n, H, W);
    YM_REQUIRE(img && mask_bits && out, "ym_draw_cutout_objects_packed: null pointer");
    k_cutout_object_packed<<<dim3(ym_cdiv(H * W, 256), n), 256, 0, (hipStream_t)s>>>(img, reinterpret_cast<const unsigned long long*>(mask_bits), H, W, out);
    return ym_check_launch("k_cutout_object_packed");
}
