// COCO annotation -> dense instance mask on the device (the reader's `self.coco.annToMask(aa)`,
// utils/coco.py:96): pycocotools annToRLE (frPyObjects on the polygon list, merge = union) + decode.  Algorithm = cocoapi
// common/maskApi.c rleFrPoly / rleDecode, restated in oracle/coco_ref.py.  Only the polygon vertices (a few hundred bytes) cross
// PCIe; the dense [n, H, W] uint8 masks are born in HBM where train_aug / the loss consume them.
//
// One workgroup per annotation.  The run-length code of a polygon is a sorted list of toggle positions in the column-major pixel
// order, so no sort is needed: every boundary point XORs one bit of a column-major bitmap (LDS when 2 bitmaps fit, else the
// caller's workspace), a prefix-XOR down each column plus a parity carry across the columns turns toggles into the fill, and
// the polygons of one annotation are OR-ed.  Each wave walks whole edges (lane = step along the edge); the doubles follow the C
// expression order without contraction (__dmul_rn / __dadd_rn / __ddiv_rn).
//
// One kernel template serves every entry: ym_ann_to_mask_ragged rasterises the annotations of up to YM_RAGGED_MAX_IMAGES images of different
// sizes, polygon lists and run lengths mixed, in one launch (the batched loader); ym_poly_to_mask / ym_runs_to_mask are its
// one-image instances.
#include <algorithm>
#include "ym_common.h"

namespace {

constexpr int NT = 512;
constexpr int NW = NT / 64;
constexpr int MAXW = 4096;
constexpr size_t LDS_BUDGET = 160 * 1024 - MAXW - 256;     // static: one parity byte per column + scan scratch

struct Pt { int u, v; };

__device__ __forceinline__ int scaled5(double c) { return (int)__dadd_rn(__dmul_rn(5.0, c), 0.5); }

// d-th point of the walk from (xs, ys) to (xe, ye) on the 5x grid (rleFrPoly's edge loop; `flip` keeps the walk monotone in t
// while the points still come out in start -> end order)
__device__ __forceinline__ Pt edge_point(int xs, int ys, int xe, int ye, int d) {
    const int dx = abs(xe - xs), dy = abs(ys - ye);
    const bool flip = (dx >= dy && xs > xe) || (dx < dy && ys > ye);
    if (flip) { int t = xs; xs = xe; xe = t; t = ys; ys = ye; ye = t; }
    Pt p;
    if (dx >= dy) {
        const int t = flip ? dx - d : d;
        p.u = t + xs;
        if (dx == 0) p.v = ys;                                   // repeated vertex: C has 0/0 here; u never changes, v unused
        else {
            const double s = __ddiv_rn((double)(ye - ys), (double)dx);
            p.v = (int)__dadd_rn(__dadd_rn((double)ys, __dmul_rn(s, (double)t)), 0.5);
        }
    } else {
        const int t = flip ? dy - d : d;
        p.v = t + ys;
        const double s = __ddiv_rn((double)(xe - xs), (double)dy);
        p.u = (int)__dadd_rn(__dadd_rn((double)xs, __dmul_rn(s, (double)t)), 0.5);
    }
    return p;
}

__device__ __forceinline__ void toggle(uint32_t* tog, int HWS, int H, int W, int x, int y) {
    if (y >= H) { x += 1; y = 0; }                               // position x*H + H is the first pixel of the next column
    if (x >= W) return;                                          // ... or the end of the image
    atomicXor(&tog[(size_t)x * HWS + (y >> 5)], 1u << (y & 31));
}

// boundary points of one polygon (k vertices at v[0 .. 2k)) -> toggles
__device__ void polygon_toggles(const double* __restrict__ v, int k, int H, int W, int HWS, uint32_t* tog) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int j = wave; j < k; j += NW) {
        const int jn = j + 1 == k ? 0 : j + 1;
        const int xs = scaled5(v[2 * j]), ys = scaled5(v[2 * j + 1]), xe = scaled5(v[2 * jn]), ye = scaled5(v[2 * jn + 1]);
        const int L = max(abs(xe - xs), abs(ye - ys)) + 1;
        for (int d = lane; d < L; d += 64) {
            const Pt cur = edge_point(xs, ys, xe, ye, d);
            Pt prev;
            if (d > 0) prev = edge_point(xs, ys, xe, ye, d - 1);
            else if (j > 0) {                                    // the point before is the last one of the previous edge
                const int xp = scaled5(v[2 * j - 2]), yp = scaled5(v[2 * j - 1]);
                prev = edge_point(xp, yp, xs, ys, max(abs(xs - xp), abs(ys - yp)));
            } else continue;
            if (cur.u == prev.u) continue;
            double xd = (double)(cur.u < prev.u ? cur.u : cur.u - 1);
            xd = __dadd_rn(__ddiv_rn(__dadd_rn(xd, 0.5), 5.0), -0.5);
            if (floor(xd) != xd || xd < 0 || xd > (double)(W - 1)) continue;
            double yd = (double)(cur.v < prev.v ? cur.v : prev.v);
            yd = __dadd_rn(__ddiv_rn(__dadd_rn(yd, 0.5), 5.0), -0.5);
            if (yd < 0) yd = 0; else if (yd > (double)H) yd = (double)H;
            toggle(tog, HWS, H, W, (int)xd, (int)ceil(yd));
        }
    }
}

// run lengths (column-major, starting with zeros) -> toggles at every run boundary
__device__ void runs_toggles(const uint32_t* __restrict__ cnt, int R, int H, int W, int HWS, uint32_t* tog, uint32_t* s_scan) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (int j0 = 0; j0 < R; j0 += NT) {
        const int j = j0 + threadIdx.x;
        const uint32_t c = j < R ? cnt[j] : 0u;
        uint32_t inc = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t t = __shfl_up(inc, o);
            if (lane >= o) inc += t;
        }
        __syncthreads();
        if (lane == 63) s_scan[wave] = inc;
        __syncthreads();
        uint32_t before = carry;
        for (int w2 = 0; w2 < wave; ++w2) before += s_scan[w2];
        uint32_t total = 0;
        for (int w2 = 0; w2 < NW; ++w2) total += s_scan[w2];
        const uint32_t end = before + inc;                       // first pixel after run j
        if (j < R - 1 && end < (uint32_t)H * (uint32_t)W) toggle(tog, HWS, H, W, (int)(end / (uint32_t)H), (int)(end % (uint32_t)H));
        carry += total;
    }
}

// What a launch knows about its images, BY VALUE in the kernel arguments (ym_common.h YmRaggedTable): image b is img[b].img_h x
// img[b].img_w, its block of masks starts img[b].offset bytes from `masks` and holds the annotations [first[b], first[b + 1]).
// ws[b] = the first word of its annotations' bitmap slices in the workspace, or -1: the bitmaps of that image live in the LDS.
template <int N>
struct AnnTable {
    ym_ragged_image img[N];
    int64_t ws[N];
    int32_t first[N + 1];
    int32_t B;
};

// One workgroup per annotation `a` of the launch (global over its images).  Its image is the last table entry that starts at or
// before it (an image without annotations shares its `first` with the next one): at most 31 uniform compares, scalar loads at a
// uniform index.  H, W, the column stride and the output pointer follow from that entry.
//   SRC 0: polygon lists, annotation a owns the items [ann_off[a], ann_off[a + 1]) of one shared prefix array (ym_poly_to_mask);
//   SRC 1: run lengths, annotation a is item a (ym_runs_to_mask);
//   SRC 2: the kind is ann_kind[a], a branch that is uniform per workgroup, and every annotation ends its own list of item starts
//          with a closing end, because the two kinds index different arrays (ym_ann_to_mask_ragged).
// N = the table's capacity: the one-image entries instantiate N = 1, where the scan is gone and the table is 40 bytes.
template <int SRC, int N>
__global__ __launch_bounds__(NT) void k_ann_to_mask(const double* __restrict__ xy, const uint32_t* __restrict__ runs,
                                                    const int32_t* __restrict__ item_off, const int32_t* __restrict__ ann_off,
                                                    const int32_t* __restrict__ ann_kind, const AnnTable<N> tab,
                                                    uint8_t* __restrict__ masks, uint32_t* __restrict__ gws) {
    extern __shared__ uint32_t smem[];
    __shared__ uint8_t s_par[MAXW];
    __shared__ uint32_t s_scan[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int a = blockIdx.x;
    int b = 0;
    for (int i = 1; i < N && i < tab.B; ++i)
        if (tab.first[i] <= a) b = i;
    const int H = tab.img[b].img_h, W = tab.img[b].img_w, local = a - tab.first[b];
    const int HW32 = (H + 31) >> 5, HWS = HW32 | 1, nwords = W * HWS;
    uint32_t* tog = tab.ws[b] >= 0 ? gws + tab.ws[b] + (size_t)local * 2 * nwords : smem;
    uint32_t* acc = tog + nwords;
    for (int i = tid; i < nwords; i += NT) acc[i] = 0;

    const int kind = SRC == 2 ? ann_kind[a] : SRC;
    const int p0 = SRC == 1 ? a : ann_off[a], p1 = SRC == 1 ? a + 1 : ann_off[a + 1] - (SRC == 2);
    for (int p = p0; p < p1; ++p) {
        for (int i = tid; i < nwords; i += NT) tog[i] = 0;
        __syncthreads();
        const int f = item_off[p], k = item_off[p + 1] - f;
        if (kind == 0) polygon_toggles(xy + 2 * (size_t)f, k, H, W, HWS, tog);
        else runs_toggles(runs + f, k, H, W, HWS, tog, s_scan);
        __syncthreads();
        // inclusive prefix-XOR down every column; s_par[x] = parity of the whole column
        for (int x = tid; x < W; x += NT) {
            uint32_t par = 0;
            uint32_t* col = tog + (size_t)x * HWS;
            for (int i = 0; i < HW32; ++i) {
                uint32_t w = col[i];
                w ^= w << 1; w ^= w << 2; w ^= w << 4; w ^= w << 8; w ^= w << 16;
                if (par) w = ~w;
                col[i] = w;
                par = w >> 31;
            }
            s_par[x] = (uint8_t)par;
        }
        __syncthreads();
        // the run-length order continues from one column into the next: carry[x] = parity of all the columns before x
        uint32_t carry = 0;
        for (int x0 = 0; x0 < W; x0 += NT) {
            const int x = x0 + tid;
            const uint32_t mine = x < W ? s_par[x] : 0u;
            uint32_t inc = mine;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t t = __shfl_up(inc, o);
                if (lane >= o) inc ^= t;
            }
            if (lane == 63) s_scan[wave] = inc;
            __syncthreads();
            uint32_t before = carry, total = 0;
            for (int w2 = 0; w2 < NW; ++w2) {
                if (w2 < wave) before ^= s_scan[w2];
                total ^= s_scan[w2];
            }
            if (x < W) {
                const uint32_t flipm = (before ^ inc ^ mine) ? ~0u : 0u;      // exclusive parity
                const uint32_t* col = tog + (size_t)x * HWS;
                uint32_t* ac = acc + (size_t)x * HWS;
                for (int i = 0; i < HW32; ++i) ac[i] |= col[i] ^ flipm;
            }
            carry ^= total;
            __syncthreads();
        }
    }
    __syncthreads();
    // row-major uint8 output, four pixels per store when the mask size allows aligned words (a block starts at a multiple of
    // YM_RAGGED_ALIGN_BYTES from the 4-byte aligned `masks`)
    const unsigned P = (unsigned)H * (unsigned)W;
    uint8_t* out = masks + tab.img[b].offset + (size_t)local * P;
    if ((P & 3u) == 0) {
        for (unsigned g = tid; g < P / 4; g += NT) {
            unsigned y = (4 * g) / (unsigned)W, x = 4 * g - y * (unsigned)W;
            uint32_t pack = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                pack |= ((acc[(size_t)x * HWS + (y >> 5)] >> (y & 31)) & 1u) << (8 * c);
                if (++x == (unsigned)W) { x = 0; ++y; }
            }
            reinterpret_cast<uint32_t*>(out)[g] = pack;
        }
    } else {
        for (unsigned i = tid; i < P; i += NT) {
            const unsigned y = i / (unsigned)W, x = i - y * (unsigned)W;
            out[i] = (uint8_t)((acc[(size_t)x * HWS + (y >> 5)] >> (y & 31)) & 1u);
        }
    }
}

inline int col_stride(int H) { return ((H + 31) >> 5) | 1; }     // words per bitmap column, odd (LDS banks)
inline size_t bitmap_bytes(int H, int W) { return (size_t)2 * W * col_stride(H) * 4; }

// The one launch path: `tab` holds the sizes, blocks and annotation ranges (tab.ws still unset).  Images whose bitmap pair fits
// LDS_BUDGET share the launch's dynamic LDS, sized for the largest of them; the others get one workspace slice per annotation.
// A small image in a launch with a large one inherits the large LDS request and so leaves fewer workgroups resident per CU: the
// grid is one workgroup per annotation, at most a few hundred on 256 CUs, so residency is not what bounds it and the launch is
// not split by size.
template <int SRC, int N>
int launch(const char* what, const double* xy, const uint32_t* runs, const int32_t* item_off, const int32_t* ann_off,
           const int32_t* ann_kind, AnnTable<N>& tab, uint8_t* masks, void* workspace, size_t workspace_bytes, ym_stream_t s) {
    size_t lds = 0, need = 0;
    for (int b = 0; b < tab.B; ++b) {
        const size_t n = (size_t)(tab.first[b + 1] - tab.first[b]), bm = bitmap_bytes(tab.img[b].img_h, tab.img[b].img_w);
        tab.ws[b] = -1;
        if (n == 0) continue;
        if (bm <= LDS_BUDGET) { lds = bm > lds ? bm : lds; continue; }
        tab.ws[b] = (int64_t)(need / 4);
        need += n * bm;
    }
    if (need && (!workspace || workspace_bytes < need)) { ym_set_error("%s: workspace < %zu bytes", what, need); return YM_ENOSPC; }
    static YmLdsAttr attr = {};                                   // (one per instantiation of this function template)
    if (int rc = ym_ensure_dyn_lds(attr, reinterpret_cast<const void*>(k_ann_to_mask<SRC, N>), LDS_BUDGET, what)) return rc;
    hipLaunchKernelGGL((k_ann_to_mask<SRC, N>), dim3(tab.first[tab.B]), dim3(NT), lds, (hipStream_t)s, xy, runs, item_off, ann_off, ann_kind,
                       tab, masks, (uint32_t*)workspace);
    return ym_check_launch(what);
}

// ym_poly_to_mask / ym_runs_to_mask: the one-image instances of the launch above
template <int SRC>
int launch_single(const char* what, const double* xy, const uint32_t* runs, const int32_t* item_off, const int32_t* ann_off, int n, int H,
                  int W, uint8_t* masks, void* workspace, size_t workspace_bytes, ym_stream_t s) {
    YM_REQUIRE(item_off && masks && (SRC == 1 || ann_off), "%s: null pointer", what);
    YM_REQUIRE(n > 0 && H > 0 && W > 0 && W <= MAXW && (long long)H * W < (1ll << 31), "%s: need n > 0, 0 < W <= %d, H*W < 2^31", what, MAXW);
    YM_REQUIRE(((uintptr_t)masks & 3) == 0, "%s: masks must be 4-byte aligned", what);
    AnnTable<1> tab = {};
    tab.B = 1;
    tab.img[0] = ym_ragged_image{H, W, 0};
    tab.first[1] = n;
    return launch<SRC>(what, xy, runs, item_off, ann_off, nullptr, tab, masks, workspace, workspace_bytes, s);
}

// The refusals of the ragged entry and of its size function: tables, sizes, annotation ranges, blocks.
int check_ragged(const char* what, const ym_ragged_image* images, const int32_t* ann_first, int B) {
    YM_REQUIRE(images && ann_first, "%s: null %s table", what, images ? "ann_first" : "image");
    YM_REQUIRE(B >= 1 && B <= YM_RAGGED_MAX_IMAGES, "%s: 1 .. %d images per call, got %d", what, YM_RAGGED_MAX_IMAGES, B);
    YM_REQUIRE(ann_first[0] == 0, "%s: ann_first[0] = %d, not 0", what, ann_first[0]);
    for (int b = 0; b < B; ++b) {
        YM_REQUIRE(ann_first[b + 1] >= ann_first[b], "%s: ann_first decreases at image %d (%d after %d)", what, b, ann_first[b + 1],
                   ann_first[b]);
        const ym_ragged_image& im = images[b];
        YM_REQUIRE(im.img_h > 0 && im.img_w > 0 && im.img_w <= MAXW && (long long)im.img_h * im.img_w < (1ll << 31),
                   "%s: image %d is %d x %d: need 0 < W <= %d, H*W < 2^31", what, b, im.img_h, im.img_w, MAXW);
    }
    return ym_check_ragged_table(what, images, B, 1, [=](const ym_ragged_image& im) {
        const long b = &im - images;
        return (int64_t)(ann_first[b + 1] - ann_first[b]) * im.img_h * im.img_w;
    });
}

}  // namespace

extern "C" size_t ym_ann_to_mask_workspace_bytes(int n, int H, int W) {
    if (n <= 0 || H <= 0 || W <= 0) return 0;
    const size_t bm = bitmap_bytes(H, W);
    return bm > LDS_BUDGET ? (size_t)n * bm : 0;
}

extern "C" int ym_poly_to_mask(const double* xy, const int32_t* poly_off, const int32_t* ann_off, int n, int H, int W, uint8_t* masks,
                               void* workspace, size_t workspace_bytes, ym_stream_t s) {
    YM_REQUIRE(xy, "poly_to_mask: null pointer");
    return launch_single<0>("poly_to_mask", xy, nullptr, poly_off, ann_off, n, H, W, masks, workspace, workspace_bytes, s);
}

extern "C" int ym_runs_to_mask(const uint32_t* counts, const int32_t* run_off, int n, int H, int W, uint8_t* masks, void* workspace,
                               size_t workspace_bytes, ym_stream_t s) {
    YM_REQUIRE(counts, "runs_to_mask: null pointer");
    return launch_single<1>("runs_to_mask", nullptr, counts, run_off, nullptr, n, H, W, masks, workspace, workspace_bytes, s);
}

extern "C" size_t ym_ann_to_mask_ragged_workspace_bytes(const ym_ragged_image* images, const int32_t* ann_first, int B) {
    if (check_ragged("ann_to_mask_ragged_workspace_bytes", images, ann_first, B) != YM_OK) return 0;
    size_t need = 0;
    for (int b = 0; b < B; ++b) need += ym_ann_to_mask_workspace_bytes(ann_first[b + 1] - ann_first[b], images[b].img_h, images[b].img_w);
    return need;
}

extern "C" int ym_ann_to_mask_ragged(const double* xy, const uint32_t* counts, const int32_t* item_off, const int32_t* ann_off,
                                     const int32_t* ann_kind, const ym_ragged_image* images, const int32_t* ann_first, int B,
                                     uint8_t* masks, void* workspace, size_t workspace_bytes, ym_stream_t s) {
    const char* what = "ann_to_mask_ragged";
    int rc = check_ragged(what, images, ann_first, B);
    if (rc != YM_OK) return rc;
    YM_REQUIRE(((uintptr_t)masks & 3) == 0, "%s: masks must be 4-byte aligned", what);
    const int n = ann_first[B];
    if (n == 0) return YM_OK;
    YM_REQUIRE(item_off && ann_off && ann_kind && masks, "%s: %d annotations with a null item_off, ann_off, ann_kind or masks pointer", what, n);
    AnnTable<YM_RAGGED_MAX_IMAGES> tab = {};
    tab.B = B;
    std::copy(images, images + B, tab.img);
    std::copy(ann_first, ann_first + B + 1, tab.first);
    return launch<2>(what, xy, counts, item_off, ann_off, ann_kind, tab, masks, workspace, workspace_bytes, s);
}
