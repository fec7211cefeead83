// Evaluation inner products right after after_nms: mask IoU of the predicted binary masks against the
// ground-truth masks (reference utils/box_utils.py:189-200: a [n,HW]x[HW,g] fp32 matmul on {0,1} masks), pixel-box IoU
// (utils/box_utils.py:8-37) and the greedy per-class matching of prep_metrics (utils/common_utils.py:174-216).
// The masks are {0,1}, so the matmul is a popcount of ANDed bit rows: HBM-bound (every mask read exactly once, 123 MB for 100
// masks at 480x640), exact in integers -> the IoU is bit-identical to the reference's fp32 result (counts < 2^24).
// ym_mask_iou_packed takes masks that already ARE bit rows (utils/packed_masks.py): 3.84 MB instead of 123 MB, same counts.
#pragma clang fp contract(off)
#include "ym_common.h"

namespace {

// pixels per workgroup pass = SEGS x 256 (4 x SEGS 64-bit words per mask row; 2 x 128 rows of them in LDS).  The host picks SEGS so
// that the chunks of a row fill the 256 CUs in whole rounds (pick_segs): 480x640 masks = 300 chunks of 1024 pixels were 1.17 rounds
// (31.4 us for 100 + 15 masks), 240 chunks of 1280 are one (26.2 us).
#include "packed_inter.h"          // MAXR, PWORDS and inter_packed_chunk: the pair loop on bit rows, shared with coco_eval.hip
constexpr int RPI = 4;                 // rows a wave has in flight per iteration of the packing pass

// Bits of a mask-row chunk: lane l of a 256-pixel segment holds pixels 4l..4l+3, one ballot per component = four 64-bit
// words.  The bit order inside a chunk is a fixed permutation of the pixel order, the same for both operands, so
// popcount(a & b) is unchanged.
// grid: (pixel chunks, groups of 128 gt rows).  Every workgroup writes its own partial counts inter[chunk][n][g], area_a[chunk][n],
// area_b[chunk][g] with plain stores (global atomics were the bottleneck: 1500 per workgroup); the finalize kernel sums the chunks.
template <int SEGS>
__global__ __launch_bounds__(512) void k_mask_inter(const float* __restrict__ A, int n, const float* __restrict__ Bm, int g, long long P,
                                                    int* __restrict__ inter, int* __restrict__ area_a, int* __restrict__ area_b) {
    constexpr int CHUNK = SEGS * 256, WORDS = SEGS * 4;
    __shared__ unsigned long long sa[MAXR][WORDS + 1];
    __shared__ unsigned long long sb[MAXR][WORDS + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    const long long p0 = (long long)blockIdx.x * CHUNK;
    const int g0 = blockIdx.y * MAXR, gn = min(MAXR, g - g0);
    const bool fast = (P & 3) == 0 && p0 + CHUNK <= P;     // float4 loads need 16-byte aligned rows and a whole chunk
    inter += (size_t)blockIdx.x * n * g;
    area_a += (size_t)blockIdx.x * n;
    area_b += (size_t)blockIdx.x * g;
    for (int a0 = 0; a0 < n; a0 += MAXR) {
        const int an = min(MAXR, n - a0);
        __syncthreads();
        // pack rows: one wave takes a whole row chunk.  The pass is HBM-latency bound, so on the fast path (16-byte aligned rows,
        // a whole chunk inside the row: every chunk of a 480x640 mask) a wave requests RPI rows -- CHUNK/256 float4 loads per lane
        // and row -- before it turns the first one into ballots; lane q < WORDS keeps word q, one LDS store per row.
        const int rows = an + (a0 == 0 ? gn : 0);
        if (fast) {
            for (int r = wave; r < rows; r += RPI * nw) {
                f32x4 v[RPI][SEGS];
#pragma unroll
                for (int u = 0; u < RPI; ++u) {
                    const int rr = min(r + u * nw, rows - 1);       // (past the end: the last row again, not used)
                    const float* row = (rr < an ? A + (size_t)(a0 + rr) * P : Bm + (size_t)(g0 + rr - an) * P) + p0 + 4 * lane;
#pragma unroll
                    for (int sg = 0; sg < SEGS; ++sg) v[u][sg] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(row + sg * 256));
                }
#pragma unroll
                for (int u = 0; u < RPI; ++u) {
                    const int rr = r + u * nw;
                    if (rr < rows) {
                        unsigned long long mine = 0;
                        int c = 0;
#pragma unroll
                        for (int sg = 0; sg < SEGS; ++sg)
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const unsigned long long w = __ballot(v[u][sg][e] != 0.f);
                                mine = lane == sg * 4 + e ? w : mine;
                                c += __popcll(w);
                            }
                        const bool is_a = rr < an;
                        if (lane < WORDS) (is_a ? sa[rr] : sb[rr - an])[lane] = mine;
                        // areas (once per row: a rows only from the first gt group, gt rows only from the first a pass)
                        if (lane == 0) {
                            if (is_a) { if (blockIdx.y == 0) area_a[a0 + rr] = c; }
                            else area_b[g0 + rr - an] = c;
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);    // (row by row: the ballots of a row are wave-uniform SGPR pairs)
                }
            }
        } else {
            // the last, partial chunk of a row / rows that are not 16-byte aligned: pixel by pixel, one row per wave and iteration
            for (int rr = wave; rr < rows; rr += nw) {
                const bool is_a = rr < an;
                const float* row = is_a ? A + (size_t)(a0 + rr) * P : Bm + (size_t)(g0 + rr - an) * P;
                unsigned long long mine = 0;
                int c = 0;
                for (int q = 0; q < WORDS; ++q) {
                    const long long p = p0 + q * 64 + lane;
                    const unsigned long long w = __ballot(p < P && row[p] != 0.f);
                    mine = lane == q ? w : mine;
                    c += __popcll(w);
                }
                if (lane < WORDS) (is_a ? sa[rr] : sb[rr - an])[lane] = mine;
                if (lane == 0) {
                    if (is_a) { if (blockIdx.y == 0) area_a[a0 + rr] = c; }
                    else area_b[g0 + rr - an] = c;
                }
            }
        }
        __syncthreads();
        for (int pr = tid; pr < an * gn; pr += blockDim.x) {
            const int i = pr / gn, j = pr - i * gn;
            int c = 0;
#pragma unroll 8
            for (int w = 0; w < WORDS; ++w) c += __popcll(sa[i][w] & sb[j][w]);
            inter[(size_t)(a0 + i) * g + g0 + j] = c;
        }
    }
}

__global__ __launch_bounds__(512) void k_mask_inter_packed(const unsigned long long* __restrict__ A, int n,
                                                           const unsigned long long* __restrict__ Bm, int g, long long Pw,
                                                           int* __restrict__ inter, int* __restrict__ area_a, int* __restrict__ area_b) {
    inter_packed_chunk(A, n, n, Bm, g, Pw, blockIdx.x, blockIdx.y, inter, area_a, area_b);
}

// sum the per-chunk partials (exact integers) and apply the reference's formula; 64 pairs x FSL chunk slices per workgroup (the
// slices' loads are independent: 4 slices took 16.5 us for 300 chunks -- a serial chain of 75 L2 round trips per thread)
constexpr int FSL = 16;
// Pair (i, j) of one 64-pair workgroup: the chunk sums of its three counts, split over the FSL slices and joined in LDS (every
// thread of the workgroup calls it; `live` = the pair exists).  The result is the reference's quotient, valid in slice 0.  `nstride`
// = the row count the partials are laid out for (inter_packed_chunk).  The ONE statement of the mask IoU's finalize step.
__device__ __forceinline__ float mask_iou_from_partials(const int* __restrict__ inter, const int* __restrict__ area_a,
                                                        const int* __restrict__ area_b, int chunks, int nstride, int g, int i, int j,
                                                        bool live) {
    __shared__ int s_i[FSL][64], s_a[FSL][64], s_b[FSL][64];
    const int lane = threadIdx.x & 63, sl = threadIdx.x >> 6;
    int it = 0, aa = 0, ab = 0;
    if (live) {
#pragma unroll 4
        for (int c = sl; c < chunks; c += FSL) {
            it += inter[((size_t)c * nstride + i) * g + j];
            aa += area_a[(size_t)c * nstride + i];
            ab += area_b[(size_t)c * g + j];
        }
    }
    s_i[sl][lane] = it; s_a[sl][lane] = aa; s_b[sl][lane] = ab;
    __syncthreads();
    int ti = 0, ta = 0, tb = 0;
    if (sl == 0) {
#pragma unroll
        for (int q = 0; q < FSL; ++q) { ti += s_i[q][lane]; ta += s_a[q][lane]; tb += s_b[q][lane]; }
    }
    const float fi = (float)ti, fa = (float)ta, fb = (float)tb;
    return __fdiv_rn(fi, (fa + fb) - fi);                // inter / ((area1.t() + area2) - inter); 0/0 -> NaN like the reference
}

__global__ __launch_bounds__(64 * FSL) void k_mask_iou_finalize(const int* __restrict__ inter, const int* __restrict__ area_a,
                                                                const int* __restrict__ area_b, int chunks, int n, int g, float* __restrict__ iou) {
    const int e = blockIdx.x * 64 + (threadIdx.x & 63);
    const bool live = e < n * g;
    const int i = live ? e / g : 0, j = live ? e - i * g : 0;
    const float v = mask_iou_from_partials(inter, area_a, area_b, chunks, n, g, i, j, live);
    if (threadIdx.x < 64 && live) iou[e] = v;
}

// Pixel-box IoU of p = [x1 y1 x2 y2] and q (utils/box_utils.py:8-37).  The ONE statement of the formula.
__device__ __forceinline__ float box_iou_pair(const float* p, const float* q) {
    float w = fminf(p[2], q[2]) - fmaxf(p[0], q[0]);
    float h = fminf(p[3], q[3]) - fmaxf(p[1], q[1]);
    w = w < 0.f ? 0.f : w;
    h = h < 0.f ? 0.f : h;
    const float inter = w * h;
    const float aa = (p[2] - p[0]) * (p[3] - p[1]), ab = (q[2] - q[0]) * (q[3] - q[1]);
    return __fdiv_rn(inter, (aa + ab) - inter);
}

__global__ void k_box_iou(const float* __restrict__ a, const float* __restrict__ b, int n, int g, float* __restrict__ iou) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * g) return;
    const int i = e / g, j = e - i * g;
    iou[e] = box_iou_pair(a + (size_t)i * 4, b + (size_t)j * 4);
}

// prep_metrics' matching (utils/common_utils.py:186-216): block = (iou type, threshold), thread = class.  Predictions are
// visited in their given order; each takes the unused same-class gt with the largest IoU strictly above the running maximum
// (which starts AT the threshold; python compares float32->double IoUs with the double threshold).
constexpr int MAXG = 512;
// One (IoU type, threshold, class) matching: `emit(i, hit)` for every prediction i < n of class c, in row order.  The ONE statement
// of the rule: k_match_detections and the accumulator's k_eval_match_log both call it.
template <class Emit>
__device__ __forceinline__ void match_class(const float* __restrict__ iou, const int* pred_cls, const int* gt_cls, int n, int g,
                                            double th, int c, Emit emit) {
    unsigned used[MAXG / 32];
#pragma unroll
    for (int w = 0; w < MAXG / 32; ++w) used[w] = 0u;
    for (int i = 0; i < n; ++i) {
        if (pred_cls[i] != c) continue;
        double best = th;
        int bj = -1;
        for (int j = 0; j < g; ++j) {
            if (gt_cls[j] != c || ((used[j >> 5] >> (j & 31)) & 1u)) continue;
            const double v = (double)iou[(size_t)i * g + j];
            if (v > best) { best = v; bj = j; }
        }
        if (bj >= 0) used[bj >> 5] |= 1u << (bj & 31);
        emit(i, bj >= 0);
    }
}

__global__ __launch_bounds__(128) void k_match_detections(const float* __restrict__ iou_box, const float* __restrict__ iou_mask,
                                                          const int* __restrict__ pred_cls, const int* __restrict__ gt_cls, int n, int g,
                                                          const double* __restrict__ thr, int T, int num_classes,
                                                          uint8_t* __restrict__ matched) {
    const int type = blockIdx.x / T, k = blockIdx.x - type * T;
    const float* iou = type == 0 ? iou_box : iou_mask;
    uint8_t* out = matched + ((size_t)type * T + k) * n;
    const double th = thr[k];
    for (int c = threadIdx.x; c < num_classes; c += blockDim.x)
        match_class(iou, pred_cls, gt_cls, n, g, th, c, [&](int i, bool hit) { out[i] = hit ? 1 : 0; });
}

// ---- device-resident mAP accumulator (include/yolact_hip.h "device-resident mAP accumulator") ---------------------------------
// prep_metrics for one image on its padded rows: the classes are staged in LDS once (int64 ids / the float gt column -> int), every
// (cell = type * T + k, class) pair is one work item of match_class, a hit sets bit `cell` of the row's flag word (LDS integer
// atomic: the cells of a row are spread over threads), then the rows go to the log.  One workgroup of 16 waves.  The items of a
// class are NEIGHBOURING lanes: a wave executes the gt loop of a prediction whenever one of its lanes owns that prediction's class,
// so with 2T lanes per class a wave holds ~3 classes (T = 10) and walks only their predictions.
constexpr int EVAL_THREADS = 1024;
// (the body of one image's workgroup: k_eval_match_log runs it for its one image, k_eval_match_log_ragged for image blockIdx.x)
__device__ __forceinline__ void eval_match_log_image(const long long* __restrict__ ids, const float* __restrict__ scores,
                                                     const int* __restrict__ count, int n, const float* __restrict__ iou_box,
                                                     const float* __restrict__ iou_mask, const float* __restrict__ gt, int g,
                                                     const double* __restrict__ thr, int T, int num_classes,
                                                     float* __restrict__ log_score, int* __restrict__ log_class,
                                                     unsigned* __restrict__ log_flags, unsigned long long* __restrict__ gt_count,
                                                     int* __restrict__ class_rows) {
    __shared__ int s_pred[YM_EVAL_MAX_DET];
    __shared__ unsigned s_flags[YM_EVAL_MAX_DET];
    __shared__ int s_gt[MAXG];
    const int tid = threadIdx.x;
    const int valid = count ? min(max(*count, 0), n) : n;
    for (int i = tid; i < n; i += EVAL_THREADS) {
        const long long id = ids[i];
        s_pred[i] = (i < valid && id >= 0 && id < num_classes) ? (int)id : -1;
        s_flags[i] = 0u;
    }
    for (int j = tid; j < g; j += EVAL_THREADS) {
        const float v = gt[(size_t)j * 5 + 4];              // .int(): truncation toward zero
        const int c = (v > -1.f && v < (float)num_classes) ? (int)v : -1;
        s_gt[j] = c;
        if (valid > 0 && c >= 0) atomicAdd(&gt_count[c], 1ull);    // an image without detections never reaches prep_metrics
    }
    __syncthreads();
    if (valid > 0 && g > 0)
        for (int item = tid; item < 2 * T * num_classes; item += EVAL_THREADS) {
            const int c = item / (2 * T), cell = item - c * 2 * T;     // (neighbouring lanes: one class, its 2T cells -- see above)
            const int type = cell / T, k = cell - type * T;
            match_class(type == 0 ? iou_box : iou_mask, s_pred, s_gt, valid, g, thr[k], c,
                        [&](int i, bool hit) { if (hit) atomicOr(&s_flags[i], 1u << cell); });
        }
    __syncthreads();
    for (int i = tid; i < n; i += EVAL_THREADS) {
        const int c = s_pred[i];
        log_class[i] = c;
        log_score[i] = c >= 0 ? scores[i] : 0.f;
        log_flags[i] = s_flags[i];
        if (c >= 0) atomicAdd(&class_rows[c], 1);
    }
}

__global__ __launch_bounds__(EVAL_THREADS) void k_eval_match_log(const long long* __restrict__ ids, const float* __restrict__ scores,
                                                                 const int* __restrict__ count, int n, const float* __restrict__ iou_box,
                                                                 const float* __restrict__ iou_mask, const float* __restrict__ gt, int g,
                                                                 const double* __restrict__ thr, int T, int num_classes,
                                                                 float* __restrict__ log_score, int* __restrict__ log_class,
                                                                 unsigned* __restrict__ log_flags, unsigned long long* __restrict__ gt_count,
                                                                 int* __restrict__ class_rows) {
    eval_match_log_image(ids, scores, count, n, iou_box, iou_mask, gt, g, thr, T, num_classes, log_score, log_class, log_flags, gt_count,
                         class_rows);
}

// ---- the metric stage of a whole request (include/yolact_hip.h "ym_eval_add_ragged_packed") ------------------------------------
// What the three launches know about their images, BY VALUE in the kernel arguments (like YmRaggedTable).  Image b's partial counts
// are inter [chunks_b][max_det][g_b], area_a [chunks_b][max_det], area_b [chunks_b][g_b] ints at part_off[b] of the workspace
// (chunks_b = chunk_first[b + 1] - chunk_first[b]); its IoUs are box [max_det][g_b], then mask [max_det][g_b] floats at iou_off[b].
// An image that is padding, or has no ground truth, owns no chunk.
struct EvalRaggedTable {
    int chunk_first[YM_RAGGED_MAX_IMAGES + 1];   // prefix sum of ceil(words_b / PWORDS): which image a workgroup of the first launch serves
    int gt_first[YM_RAGGED_MAX_IMAGES + 1];      // first row of image b in `gt` (and g_b as the difference)
    int words[YM_RAGGED_MAX_IMAGES];             // img_h_b * ceil(img_w_b / 64)
    int img_h[YM_RAGGED_MAX_IMAGES], img_w[YM_RAGGED_MAX_IMAGES];
    long long det_off[YM_RAGGED_MAX_IMAGES], gt_off[YM_RAGGED_MAX_IMAGES];   // words from det_bits / gt_bits to the image's block
    long long part_off[YM_RAGGED_MAX_IMAGES], iou_off[YM_RAGGED_MAX_IMAGES];
    long long log_row[YM_RAGGED_MAX_IMAGES];     // image_index * max_det; < 0 = padding
};

__device__ __forceinline__ int eval_ragged_count(const int* __restrict__ counts, int b, int max_det) { return min(max(counts[b], 0), max_det); }

// grid: (all chunks of all images, the largest number of gt groups of an image).  Rows at or past the image's count are not loaded.
__global__ __launch_bounds__(512) void k_eval_inter_ragged(const unsigned long long* __restrict__ det_bits,
                                                           const unsigned long long* __restrict__ gt_bits, const int* __restrict__ counts,
                                                           int B, int max_det, const EvalRaggedTable t, int* __restrict__ part) {
    int b = 0;
    while (b + 1 < B && (int)blockIdx.x >= t.chunk_first[b + 1]) ++b;
    const int g = t.gt_first[b + 1] - t.gt_first[b];
    if ((int)blockIdx.y * MAXR >= g) return;
    const int n = eval_ragged_count(counts, b, max_det);
    if (n == 0) return;
    const int chunks = t.chunk_first[b + 1] - t.chunk_first[b];
    int* inter = part + t.part_off[b];
    int* area_a = inter + (size_t)chunks * max_det * g;
    int* area_b = area_a + (size_t)chunks * max_det;
    inter_packed_chunk(det_bits + t.det_off[b], n, max_det, gt_bits + t.gt_off[b], g, (long long)t.words[b], (int)blockIdx.x - t.chunk_first[b],
                       (int)blockIdx.y, inter, area_a, area_b);
}

// grid: (groups of 64 pairs of the largest image, B).  Pair e = i * g_b + j, i below the image's count: slice 0 writes the mask IoU
// from the partial counts, slice 1 the box IoU of (float)boxes_px against the gt box scaled in fp32 (one rounding per product: what
// the in-place `gt_boxes[:, 0::2] *= width` of DeviceAPData.add leaves; this file is compiled without contraction).
__global__ __launch_bounds__(64 * FSL) void k_eval_iou_ragged(const int* __restrict__ boxes_px, const float* __restrict__ gt,
                                                              const int* __restrict__ counts, int max_det, const EvalRaggedTable t,
                                                              const int* __restrict__ part, float* __restrict__ iou) {
    const int b = blockIdx.y;
    const int g = t.gt_first[b + 1] - t.gt_first[b];
    if (t.log_row[b] < 0 || g == 0) return;
    const int n = eval_ragged_count(counts, b, max_det);
    if ((int)blockIdx.x * 64 >= n * g) return;              // (n == 0 as well)
    const int e = blockIdx.x * 64 + (threadIdx.x & 63), sl = threadIdx.x >> 6;
    const bool live = e < n * g;
    const int i = live ? e / g : 0, j = live ? e - i * g : 0;
    const int chunks = t.chunk_first[b + 1] - t.chunk_first[b];
    const int* inter = part + t.part_off[b];
    const int* area_a = inter + (size_t)chunks * max_det * g;
    const int* area_b = area_a + (size_t)chunks * max_det;
    float* iou_box = iou + t.iou_off[b];
    float* iou_mask = iou_box + (size_t)max_det * g;
    const float v = mask_iou_from_partials(inter, area_a, area_b, chunks, max_det, g, i, j, live);
    if (sl == 0 && live) iou_mask[e] = v;
    if (sl == 1 && live) {
        const int* pb = boxes_px + ((size_t)b * max_det + i) * 4;
        const float* qb = gt + (size_t)(t.gt_first[b] + j) * 5;
        const float fw = (float)t.img_w[b], fh = (float)t.img_h[b];
        const float p[4] = {(float)pb[0], (float)pb[1], (float)pb[2], (float)pb[3]};
        const float q[4] = {qb[0] * fw, qb[1] * fh, qb[2] * fw, qb[3] * fh};
        iou_box[e] = box_iou_pair(p, q);
    }
}

// grid: B.  Workgroup b is k_eval_match_log's workgroup for image b: its max_det padded rows, its count, its rows of `gt`, its
// IoUs from the launch before, its log rows.  A padding entry exits at once.
__global__ __launch_bounds__(EVAL_THREADS) void k_eval_match_log_ragged(const long long* __restrict__ ids, const float* __restrict__ scores,
                                                                        const int* __restrict__ counts, int max_det,
                                                                        const EvalRaggedTable t, const float* __restrict__ iou,
                                                                        const float* __restrict__ gt, const double* __restrict__ thr, int T,
                                                                        int num_classes, float* __restrict__ log_score,
                                                                        int* __restrict__ log_class, unsigned* __restrict__ log_flags,
                                                                        unsigned long long* __restrict__ gt_count, int* __restrict__ class_rows) {
    const int b = blockIdx.x;
    const long long row = t.log_row[b];
    if (row < 0) return;
    const int g = t.gt_first[b + 1] - t.gt_first[b];
    const float* iou_box = iou + t.iou_off[b];
    eval_match_log_image(ids + (size_t)b * max_det, scores + (size_t)b * max_det, counts + b, max_det, iou_box, iou_box + (size_t)max_det * g,
                         gt + (size_t)t.gt_first[b] * 5, g, thr, T, num_classes, log_score + row, log_class + row, log_flags + row,
                         gt_count, class_rows);
}

// The flags in sorted order, once: the 2T workgroups of a class then read consecutive words.
__global__ void k_eval_gather(const unsigned* __restrict__ flags, const long long* __restrict__ order, long long rows,
                              unsigned* __restrict__ sorted) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const long long p = order[r];
    sorted[r] = (p >= 0 && p < rows) ? flags[p] : 0u;
}

__device__ __forceinline__ int wave_inclusive_sum(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    return v;
}

__device__ __forceinline__ double wave_suffix_max(double v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double o = __shfl_down(v, d);
        if (lane + d < 64) v = fmax(v, o);
    }
    return v;
}

// APDataObject.get_ap of one (class, cell): workgroup (class, cell) walks the class's sorted rows twice.  Pass A counts the true
// positives.  Pass B goes BACKWARDS in chunks of YM_EVAL_AP_ROWS_PER_PASS rows carrying (true positives before the chunk, envelope
// of everything behind it): tp of a row = tp before the chunk + an integer scan, precision = tp / (rank + 1), envelope = suffix
// maximum (max is exact: any association gives the reference's value).  recall = tp / num_gt depends on tp alone and grows with it, so the
// first rank that reaches grid value k is the first rank whose tp reaches t_k = the smallest t with (double)t / num_gt >= k / 100.0
// (found with those very quotients); it lies in the one chunk with tp_before < t_k <= tp_after (t_k = 0: rank 0), where a binary
// search over the chunk's tp finds it and the envelope there is the sample.  Thread 0 adds the 101 samples left to right.
constexpr int AP_THREADS = 256, AP_RPT = YM_EVAL_AP_ROWS_PER_PASS / AP_THREADS, AP_GRID = 101;
static_assert(AP_THREADS * AP_RPT == YM_EVAL_AP_ROWS_PER_PASS && AP_THREADS >= AP_GRID, "one pass = AP_RPT rows per thread");
__global__ __launch_bounds__(AP_THREADS) void k_eval_ap(const unsigned* __restrict__ flags, long long rows, const long long* __restrict__ seg,
                                                        const long long* __restrict__ gt_count, int num_classes, double* __restrict__ ap,
                                                        uint8_t* __restrict__ empty) {
    __shared__ long long s_t[AP_GRID];
    __shared__ double s_sample[AP_GRID];
    __shared__ int s_tp[YM_EVAL_AP_ROWS_PER_PASS];           // tp of each row of the chunk, minus the tp before the chunk
    __shared__ double s_env[YM_EVAL_AP_ROWS_PER_PASS];
    __shared__ int s_wsum[AP_THREADS / 64];
    __shared__ double s_wmax[AP_THREADS / 64];
    __shared__ long long s_total;
    const int c = blockIdx.x, cell = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long beg = min(max(seg[c], 0ll), rows), end = min(max(seg[c + 1], 0ll), rows);
    if (end < beg) end = beg;
    const long long m = end - beg, G = gt_count[c];
    if (cell == 0 && tid == 0) empty[c] = (m == 0 && G == 0) ? 1 : 0;
    double* out = ap + (size_t)cell * num_classes + c;
    if (G <= 0 || m == 0) {                                    // (uniform over the workgroup)
        if (tid == 0) *out = 0.0;
        return;
    }
    const unsigned* f = flags + beg;
    const double Gd = (double)G;
    if (tid < AP_GRID) {
        const double x = (double)tid / 100.0;
        long long t = (long long)(x * Gd);
        t = min(max(t, 0ll), G);
        while (t > 0 && (double)(t - 1) / Gd >= x) --t;
        while (t < G && (double)t / Gd < x) ++t;               // (G / G = 1 >= every grid value)
        s_t[tid] = t;
        s_sample[tid] = 0.0;
    }
    // pass A: true positives of the whole class
    long long mine = 0;
    for (long long r = tid; r < m; r += AP_THREADS) mine += (f[r] >> cell) & 1u;
    if (tid == 0) s_total = 0;
    __syncthreads();
    atomicAdd((unsigned long long*)&s_total, (unsigned long long)mine);      // (integers: any order gives the same sum)
    __syncthreads();
    long long remaining = s_total;                              // true positives at or before the end of the current chunk
    double carry = -1.0;                                        // envelope of the rows behind the current chunk (precision >= 0)
    const long long chunks = (m + YM_EVAL_AP_ROWS_PER_PASS - 1) / YM_EVAL_AP_ROWS_PER_PASS;
    for (long long ch = chunks - 1; ch >= 0; --ch) {
        const long long r0 = ch * YM_EVAL_AP_ROWS_PER_PASS;
        const int cn = (int)min((long long)YM_EVAL_AP_ROWS_PER_PASS, m - r0);
        int b[AP_RPT], local = 0;
#pragma unroll
        for (int e = 0; e < AP_RPT; ++e) {
            const int q = tid * AP_RPT + e;
            b[e] = q < cn ? (int)((f[r0 + q] >> cell) & 1u) : 0;
            local += b[e];
        }
        const int incl = wave_inclusive_sum(local, lane);
        if (lane == 63) s_wsum[wave] = incl;
        __syncthreads();
        int before = incl - local, chunk_tp = 0;
#pragma unroll
        for (int w = 0; w < AP_THREADS / 64; ++w) {
            before += w < wave ? s_wsum[w] : 0;
            chunk_tp += s_wsum[w];
        }
        const long long tp_in = remaining - chunk_tp;
        double p[AP_RPT];
        int run = before;
#pragma unroll
        for (int e = 0; e < AP_RPT; ++e) {
            const int q = tid * AP_RPT + e;
            run += b[e];
            s_tp[q] = run;
            p[e] = q < cn ? (double)(tp_in + run) / (double)(r0 + q + 1) : -1.0;
        }
#pragma unroll
        for (int e = AP_RPT - 2; e >= 0; --e) p[e] = fmax(p[e], p[e + 1]);
        const double sfx = wave_suffix_max(p[0], lane);         // max over this thread's rows and the later lanes'
        if (lane == 0) s_wmax[wave] = sfx;
        __syncthreads();
        double behind = carry;                                  // everything after this thread's rows
#pragma unroll
        for (int w = 0; w < AP_THREADS / 64; ++w) behind = w > wave ? fmax(behind, s_wmax[w]) : behind;
        const double next_lane = __shfl_down(sfx, 1);
        if (lane < 63) behind = fmax(behind, next_lane);
#pragma unroll
        for (int e = 0; e < AP_RPT; ++e) s_env[tid * AP_RPT + e] = fmax(p[e], behind);
        __syncthreads();
        if (tid < AP_GRID) {
            const long long t = s_t[tid];
            const bool here = t == 0 ? ch == 0 : (tp_in < t && t <= tp_in + chunk_tp);
            if (here) {
                const int want = (int)(t - tp_in);              // first row of the chunk with s_tp >= want
                int lo = 0, hi = cn - 1;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (s_tp[mid] >= want) hi = mid; else lo = mid + 1;
                }
                s_sample[tid] = s_env[lo];
            }
        }
        carry = s_env[0];
        remaining = tp_in;
        __syncthreads();
    }
    if (tid == 0) {
        double sum = 0.0;
        for (int k = 0; k < AP_GRID; ++k) sum += s_sample[k];
        *out = sum / 101.0;
    }
}

}  // namespace

// 256-pixel segments per chunk: the choice with the fewest (rounds over 256 CUs) x (work per chunk); ties go to the larger chunk
// (fewer partial counts for the finalize pass)
static int pick_segs(long long P) {
    int best = 4;
    long long best_cost = -1;
    for (int sg = 3; sg <= 5; ++sg) {
        const long long chunks = (P + sg * 256 - 1) / (sg * 256);
        const long long cost = ((chunks + 255) / 256) * sg;
        if (best_cost < 0 || cost <= best_cost) { best = sg; best_cost = cost; }
    }
    return best;
}

extern "C" size_t ym_mask_iou_workspace_bytes(int n, int g, int64_t P) {
    const int chunk = pick_segs(P) * 256;
    const size_t chunks = (size_t)((P + chunk - 1) / chunk);
    return chunks * ((size_t)n * g + n + g) * sizeof(int) + 256;
}

extern "C" int ym_mask_iou(const float* masks_a, int n, const float* masks_b, int g, int64_t P, float* iou, void* workspace,
                           size_t workspace_bytes, ym_stream_t s) {
    YM_REQUIRE(masks_a && masks_b && iou && workspace, "mask_iou: null pointer");
    YM_REQUIRE(n > 0 && g > 0 && P > 0 && P < (1ll << 24), "mask_iou: n, g > 0 and 0 < P < 2^24 (exact fp32 counts)");
    YM_REQUIRE((long long)n * g < (1ll << 24), "mask_iou: n*g too large");
    if (workspace_bytes < ym_mask_iou_workspace_bytes(n, g, P)) { ym_set_error("mask_iou: workspace too small"); return YM_ENOSPC; }
    hipStream_t st = (hipStream_t)s;
    const int segs = pick_segs(P), chunk = segs * 256;
    const int chunks = (int)((P + chunk - 1) / chunk);
    int* inter = (int*)workspace;
    int* area_a = inter + (size_t)chunks * n * g;
    int* area_b = area_a + (size_t)chunks * n;
    const dim3 grid((unsigned)chunks, (unsigned)((g + MAXR - 1) / MAXR));
    if (segs == 3) hipLaunchKernelGGL(k_mask_inter<3>, grid, dim3(512), 0, st, masks_a, n, masks_b, g, (long long)P, inter, area_a, area_b);
    else if (segs == 4) hipLaunchKernelGGL(k_mask_inter<4>, grid, dim3(512), 0, st, masks_a, n, masks_b, g, (long long)P, inter, area_a, area_b);
    else hipLaunchKernelGGL(k_mask_inter<5>, grid, dim3(512), 0, st, masks_a, n, masks_b, g, (long long)P, inter, area_a, area_b);
    hipLaunchKernelGGL(k_mask_iou_finalize, dim3((n * g + 63) / 64), dim3(64 * FSL), 0, st, inter, area_a, area_b, chunks, n, g, iou);
    return ym_check_launch("mask_iou");
}

extern "C" size_t ym_mask_iou_packed_workspace_bytes(int n, int g, int64_t words) {
    const size_t chunks = (size_t)((words + PWORDS - 1) / PWORDS);
    return chunks * ((size_t)n * g + n + g) * sizeof(int) + 256;
}

extern "C" int ym_mask_iou_packed(const uint64_t* bits_a, int n, const uint64_t* bits_b, int g, int64_t words, float* iou, void* workspace,
                                  size_t workspace_bytes, ym_stream_t s) {
    YM_REQUIRE(bits_a && bits_b && iou && workspace, "mask_iou_packed: null pointer");
    YM_REQUIRE(n > 0 && g > 0 && words > 0 && words < (1ll << 18), "mask_iou_packed: n, g > 0 and 0 < words < 2^18 (exact fp32 counts)");
    YM_REQUIRE((long long)n * g < (1ll << 24), "mask_iou_packed: n*g too large");
    if (workspace_bytes < ym_mask_iou_packed_workspace_bytes(n, g, words)) { ym_set_error("mask_iou_packed: workspace too small"); return YM_ENOSPC; }
    hipStream_t st = (hipStream_t)s;
    const int chunks = (int)((words + PWORDS - 1) / PWORDS);
    int* inter = (int*)workspace;
    int* area_a = inter + (size_t)chunks * n * g;
    int* area_b = area_a + (size_t)chunks * n;
    const dim3 grid((unsigned)chunks, (unsigned)((g + MAXR - 1) / MAXR));
    hipLaunchKernelGGL(k_mask_inter_packed, grid, dim3(512), 0, st, reinterpret_cast<const unsigned long long*>(bits_a), n,
                       reinterpret_cast<const unsigned long long*>(bits_b), g, (long long)words, inter, area_a, area_b);
    hipLaunchKernelGGL(k_mask_iou_finalize, dim3((n * g + 63) / 64), dim3(64 * FSL), 0, st, inter, area_a, area_b, chunks, n, g, iou);
    return ym_check_launch("mask_iou_packed");
}

extern "C" int ym_box_iou(const float* boxes_a, int n, const float* boxes_b, int g, float* iou, ym_stream_t s) {
    YM_REQUIRE(boxes_a && boxes_b && iou && n > 0 && g > 0, "box_iou: bad args");
    hipLaunchKernelGGL(k_box_iou, dim3((n * g + 255) / 256), dim3(256), 0, (hipStream_t)s, boxes_a, boxes_b, n, g, iou);
    return ym_check_launch("box_iou");
}

extern "C" int ym_match_detections(const float* iou_box, const float* iou_mask, const int32_t* pred_cls, const int32_t* gt_cls, int n,
                                   int g, const double* thresholds, int T, int num_classes, uint8_t* matched, ym_stream_t s) {
    YM_REQUIRE(iou_box && iou_mask && pred_cls && gt_cls && thresholds && matched, "match_detections: null pointer");
    YM_REQUIRE(n > 0 && g > 0 && g <= MAXG && T > 0 && num_classes > 0, "match_detections: need 0 < g <= %d", MAXG);
    hipLaunchKernelGGL(k_match_detections, dim3(2 * T), dim3(128), 0, (hipStream_t)s, iou_box, iou_mask, pred_cls, gt_cls, n, g,
                       thresholds, T, num_classes, matched);
    return ym_check_launch("match_detections");
}

extern "C" int ym_eval_match_log(const int64_t* ids, const float* scores, const int32_t* count, int n, const float* iou_box,
                                 const float* iou_mask, const float* gt, int g, const double* thresholds, int T, int num_classes,
                                 float* log_score, int32_t* log_class, uint32_t* log_flags, int64_t log_offset, int64_t* gt_count,
                                 int32_t* class_rows, ym_stream_t s) {
    YM_REQUIRE(ids && scores && thresholds && log_score && log_class && log_flags && gt_count && class_rows, "eval_match_log: null pointer");
    YM_REQUIRE(g == 0 || (iou_box && iou_mask && gt), "eval_match_log: null pointer");
    YM_REQUIRE(n > 0 && n <= YM_EVAL_MAX_DET && log_offset >= 0, "eval_match_log: need 0 < n <= %d rows and a log offset >= 0", YM_EVAL_MAX_DET);
    YM_REQUIRE(g >= 0 && g <= MAXG && T > 0 && num_classes > 0, "eval_match_log: need 0 <= g <= %d", MAXG);
    YM_REQUIRE(T <= YM_EVAL_MAX_THRESHOLDS, "eval_match_log: at most %d thresholds (2T flag bits per row)", YM_EVAL_MAX_THRESHOLDS);
    hipLaunchKernelGGL(k_eval_match_log, dim3(1), dim3(EVAL_THREADS), 0, (hipStream_t)s, reinterpret_cast<const long long*>(ids), scores,
                       count, n, iou_box, iou_mask, gt, g, thresholds, T, num_classes, log_score + log_offset, log_class + log_offset,
                       log_flags + log_offset, reinterpret_cast<unsigned long long*>(gt_count), class_rows);
    return ym_check_launch("eval_match_log");
}

// Where image b's partial counts (ints) and IoUs (floats, behind all the partials) lie in the workspace of ym_eval_add_ragged_packed:
// a function of the sizes alone, so a padding entry keeps its (unused) room and the workspace query needs no image_index.
// false for arguments the entry refuses.
static bool eval_ragged_layout(const ym_ragged_image* det_blocks, const int32_t* gt_first, int B, int max_det, long long* part_off,
                               long long* iou_off, size_t* part_ints, size_t* iou_floats) {
    if (!det_blocks || !gt_first || B < 1 || B > YM_RAGGED_MAX_IMAGES || max_det < 1 || max_det > YM_EVAL_MAX_DET) return false;
    size_t parts = 0, ious = 0;
    for (int b = 0; b < B; ++b) {
        const long long g = (long long)gt_first[b + 1] - gt_first[b];
        if (g < 0 || g > MAXG || det_blocks[b].img_h <= 0 || det_blocks[b].img_w <= 0) return false;
        const long long words = (long long)det_blocks[b].img_h * (long long)ym_mask_row(true, det_blocks[b].img_w);
        if (words >= (1ll << 18)) return false;
        const size_t chunks = (size_t)((words + PWORDS - 1) / PWORDS);
        if (part_off) part_off[b] = (long long)parts;
        if (iou_off) iou_off[b] = (long long)ious;
        if (g > 0) {
            parts += chunks * ((size_t)max_det * g + max_det + g);
            ious += 2 * (size_t)max_det * g;
        }
    }
    *part_ints = parts;
    *iou_floats = ious;
    return true;
}

extern "C" size_t ym_eval_add_ragged_workspace_bytes(const ym_ragged_image* det_blocks, const int32_t* gt_first, int B, int max_det) {
    size_t parts = 0, ious = 0;
    if (!eval_ragged_layout(det_blocks, gt_first, B, max_det, nullptr, nullptr, &parts, &ious)) return 0;
    return (parts + ious) * sizeof(int) + 256;
}

extern "C" int ym_eval_add_ragged_packed(const int64_t* ids, const float* scores, const int32_t* boxes_px, const int32_t* counts, int B,
                                         int max_det, const uint64_t* det_bits, const ym_ragged_image* det_blocks, const float* gt,
                                         const int32_t* gt_first, const uint64_t* gt_bits, const ym_ragged_image* gt_blocks,
                                         const int64_t* image_index, const double* thresholds, int T, int num_classes, float* log_score,
                                         int32_t* log_class, uint32_t* log_flags, int64_t log_rows, int64_t* gt_count, int32_t* class_rows,
                                         void* workspace, size_t workspace_bytes, ym_stream_t s) {
    const char* what = "eval_add_ragged_packed";
    YM_REQUIRE(B >= 1 && B <= YM_RAGGED_MAX_IMAGES, "%s: 1 .. %d images per call, got %d", what, YM_RAGGED_MAX_IMAGES, B);
    YM_REQUIRE(max_det >= 1 && max_det <= YM_EVAL_MAX_DET, "%s: need 0 < max_det <= %d, got %d", what, YM_EVAL_MAX_DET, max_det);
    YM_REQUIRE(T >= 1 && T <= YM_EVAL_MAX_THRESHOLDS, "%s: 1 .. %d thresholds (2T flag bits per row), got %d", what,
               YM_EVAL_MAX_THRESHOLDS, T);
    YM_REQUIRE(num_classes > 0, "%s: num_classes = %d", what, num_classes);
    YM_REQUIRE(ids && scores && boxes_px && counts && det_bits && det_blocks && gt_first && gt_blocks && image_index && thresholds &&
                   log_score && log_class && log_flags && gt_count && class_rows && workspace,
               "%s: null pointer", what);
    YM_REQUIRE(gt_first[0] >= 0, "%s: gt_first[0] = %d", what, gt_first[0]);
    for (int b = 0; b < B; ++b) {
        const long long g = (long long)gt_first[b + 1] - gt_first[b];
        YM_REQUIRE(g >= 0, "%s: gt_first is not ascending at image %d", what, b);
        YM_REQUIRE(g <= MAXG, "%s: image %d has %lld gt instances, at most %d are matched", what, b, g, MAXG);
    }
    YM_REQUIRE(gt_first[B] == 0 || (gt && gt_bits), "%s: null pointer", what);
    const int rc_det = ym_check_ragged_table(what, det_blocks, B, 8, [&](const ym_ragged_image& im) {
        return (int64_t)max_det * im.img_h * (int64_t)ym_mask_row(true, im.img_w);
    });
    if (rc_det != YM_OK) return rc_det;
    const int rc_gt = ym_check_ragged_table(what, gt_blocks, B, 8, [&](const ym_ragged_image& im) {
        const int64_t b = &im - gt_blocks;
        return (int64_t)(gt_first[b + 1] - gt_first[b]) * im.img_h * (int64_t)ym_mask_row(true, im.img_w);
    });
    if (rc_gt != YM_OK) return rc_gt;
    bool any = false, any_gt = false;
    for (int b = 0; b < B; ++b) {
        YM_REQUIRE(gt_blocks[b].img_h == det_blocks[b].img_h && gt_blocks[b].img_w == det_blocks[b].img_w,
                   "%s: image %d: gt masks of %d x %d for detection masks of %d x %d", what, b, gt_blocks[b].img_h, gt_blocks[b].img_w,
                   det_blocks[b].img_h, det_blocks[b].img_w);
        YM_REQUIRE((long long)det_blocks[b].img_h * (long long)ym_mask_row(true, det_blocks[b].img_w) < (1ll << 18),
                   "%s: image %d: need img_h * ceil(img_w / 64) < 2^18 words (exact fp32 counts)", what, b);
        if (image_index[b] < 0) continue;
        YM_REQUIRE(image_index[b] < log_rows && (image_index[b] + 1) * max_det <= log_rows,
                   "%s: image index %lld: its %d rows end past the %lld rows of the log", what, (long long)image_index[b], max_det,
                   (long long)log_rows);
        for (int a = 0; a < b; ++a)
            YM_REQUIRE(image_index[a] != image_index[b], "%s: image index %lld twice in one call", what, (long long)image_index[b]);
        any = true;
        any_gt = any_gt || gt_first[b + 1] > gt_first[b];
    }
    EvalRaggedTable t = {};
    size_t parts = 0, ious = 0;
    YM_REQUIRE(eval_ragged_layout(det_blocks, gt_first, B, max_det, t.part_off, t.iou_off, &parts, &ious), "%s: bad sizes", what);
    if (workspace_bytes < (parts + ious) * sizeof(int) + 256) { ym_set_error("%s: workspace too small", what); return YM_ENOSPC; }
    if (!any) return YM_OK;                                  // (padding only)
    int max_groups = 1, max_pairs = 0;
    for (int b = 0; b < B; ++b) {
        const int g = gt_first[b + 1] - gt_first[b];
        const bool live = image_index[b] >= 0;
        t.gt_first[b] = gt_first[b];
        t.img_h[b] = det_blocks[b].img_h;
        t.img_w[b] = det_blocks[b].img_w;
        t.words[b] = det_blocks[b].img_h * (int)ym_mask_row(true, det_blocks[b].img_w);
        t.det_off[b] = det_blocks[b].offset;
        t.gt_off[b] = gt_blocks[b].offset;
        t.log_row[b] = live ? image_index[b] * max_det : -1;
        t.chunk_first[b + 1] = t.chunk_first[b] + (live && g > 0 ? ym_cdiv(t.words[b], PWORDS) : 0);
        if (live && g > 0) {
            max_groups = max_groups > ym_cdiv(g, MAXR) ? max_groups : ym_cdiv(g, MAXR);
            max_pairs = max_pairs > max_det * g ? max_pairs : max_det * g;
        }
    }
    t.gt_first[B] = gt_first[B];
    for (int b = B; b < YM_RAGGED_MAX_IMAGES; ++b) { t.chunk_first[b + 1] = t.chunk_first[B]; t.gt_first[b + 1] = gt_first[B]; t.log_row[b] = -1; }
    hipStream_t st = (hipStream_t)s;
    int* part = (int*)workspace;
    float* iou = (float*)workspace + parts;
    if (any_gt) {
        hipLaunchKernelGGL(k_eval_inter_ragged, dim3((unsigned)t.chunk_first[B], (unsigned)max_groups), dim3(512), 0, st,
                           reinterpret_cast<const unsigned long long*>(det_bits), reinterpret_cast<const unsigned long long*>(gt_bits), counts, B,
                           max_det, t, part);
        hipLaunchKernelGGL(k_eval_iou_ragged, dim3((unsigned)ym_cdiv(max_pairs, 64), (unsigned)B), dim3(64 * FSL), 0, st, boxes_px, gt, counts,
                           max_det, t, (const int*)part, iou);
    }
    hipLaunchKernelGGL(k_eval_match_log_ragged, dim3((unsigned)B), dim3(EVAL_THREADS), 0, st, reinterpret_cast<const long long*>(ids), scores,
                       counts, max_det, t, (const float*)iou, gt, thresholds, T, num_classes, log_score, log_class, log_flags,
                       reinterpret_cast<unsigned long long*>(gt_count), class_rows);
    return ym_check_launch(what);
}

extern "C" size_t ym_eval_ap_workspace_bytes(int64_t rows) { return rows > 0 ? (size_t)rows * sizeof(uint32_t) : 0; }

extern "C" int ym_eval_ap(const uint32_t* log_flags, const int64_t* order, int64_t rows, const int64_t* seg, const int64_t* gt_count, int T,
                          int num_classes, double* ap, uint8_t* empty, void* workspace, size_t workspace_bytes, ym_stream_t s) {
    YM_REQUIRE(log_flags && seg && gt_count && ap && empty, "eval_ap: null pointer");
    YM_REQUIRE(rows > 0 && T > 0 && T <= YM_EVAL_MAX_THRESHOLDS && num_classes > 0 && num_classes <= 65535,
               "eval_ap: need rows > 0, 0 < T <= %d, 0 < num_classes <= 65535", YM_EVAL_MAX_THRESHOLDS);
    hipStream_t st = (hipStream_t)s;
    const unsigned* sorted = log_flags;
    if (order) {
        if (!workspace || workspace_bytes < ym_eval_ap_workspace_bytes(rows)) { ym_set_error("eval_ap: workspace too small"); return YM_ENOSPC; }
        hipLaunchKernelGGL(k_eval_gather, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, log_flags,
                           reinterpret_cast<const long long*>(order), (long long)rows, (unsigned*)workspace);
        sorted = (const unsigned*)workspace;
    }
    hipLaunchKernelGGL(k_eval_ap, dim3((unsigned)num_classes, (unsigned)(2 * T)), dim3(AP_THREADS), 0, st, sorted, (long long)rows,
                       reinterpret_cast<const long long*>(seg), reinterpret_cast<const long long*>(gt_count), num_classes, ap, empty);
    return ym_check_launch("eval_ap");
}
