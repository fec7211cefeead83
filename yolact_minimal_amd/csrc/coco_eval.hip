// COCO-protocol evaluation on the device (include/yolact_hip.h "device-resident COCO evaluator"): what `eval.py --coco_api` gets
// from pycocotools.cocoeval.COCOeval after the dump (eval.py:90-104), restated from the published cocoapi algorithm:
//   maskApi.c  bbIou / rleIou                     -> k_coco_iou_box, k_coco_iou_mask
//   cocoeval.py computeIoU / evaluateImg          -> k_coco_match_log (one image, every category, area range, threshold, IoU type)
//   the three of them for a whole request       -> k_coco_inter_ragged, k_coco_iou_ragged, k_coco_match_log_ragged
//   cocoeval.py accumulate                        -> k_coco_gather + k_coco_accumulate (precision / recall grids)
// `summarize` is host numpy on the one downloaded grid (utils/coco_eval.py).  Everything floating-point is fp64 without contraction,
// sums are integer counts, the only atomics are integer ones: the grids repeat bit for bit.
#pragma clang fp contract(off)
#include "ym_common.h"

namespace {

constexpr int MAXG = YM_COCO_MAX_GT;
constexpr int AREAS = YM_COCO_AREAS;
constexpr int WORDS_PER_ROW = 2 * AREAS;          // flag words of a log row: [IoU type][area range]
#include "packed_inter.h"                         // MAXR, PWORDS and inter_packed_chunk: the pair loop on bit rows, shared with metrics.hip

// ---- maskApi.c bbIou: boxes are [x, y, w, h] doubles -------------------------------------------------------------------------
// (the ONE statement of bbIou's formula: k_coco_iou_box and k_coco_iou_ragged both call it)
__device__ __forceinline__ double coco_bb_iou(const double* D, const double* G, bool crowd) {
    const double da = D[2] * D[3], ga = G[2] * G[3];
    double o = 0.0;
    const double w = fmin(D[2] + D[0], G[2] + G[0]) - fmax(D[0], G[0]);
    if (w > 0.0) {
        const double h = fmin(D[3] + D[1], G[3] + G[1]) - fmax(D[1], G[1]);
        if (h > 0.0) {
            const double in = w * h;
            const double u = crowd ? da : da + ga - in;
            o = in / u;
        }
    }
    return o;
}

__global__ void k_coco_iou_box(const double* __restrict__ dt, int n, const double* __restrict__ gt, int g,
                               const uint8_t* __restrict__ crowd, double* __restrict__ iou) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * g) return;
    const int i = e / g, j = e - i * g;
    iou[e] = coco_bb_iou(dt + (size_t)i * 4, gt + (size_t)j * 4, crowd[j] != 0);
}

// ---- maskApi.c rleIou on bit rows: i = |d & g|, 0 when i == 0, else i / (crowd ? |d| : |d| + |g| - i) --------------------------
// grid (detection, group of IM_GJ gts): a thread walks its words of the detection row once and ANDs them with the group's rows;
// the counts meet in LDS integers.  The detection's popcount (its segm area) is written by the first group.
constexpr int IM_GJ = 8, IM_THREADS = 256;
__global__ __launch_bounds__(IM_THREADS) void k_coco_iou_mask(const unsigned long long* __restrict__ A, int n,
                                                              const unsigned long long* __restrict__ B, int g, long long words,
                                                              const uint8_t* __restrict__ crowd, double* __restrict__ iou,
                                                              int* __restrict__ area_d) {
    __shared__ int s_cnt[2 * IM_GJ + 1];
    const int tid = threadIdx.x, i = blockIdx.x, j0 = blockIdx.y * IM_GJ, gn = min(IM_GJ, g - j0);
    if (tid < 2 * IM_GJ + 1) s_cnt[tid] = 0;
    __syncthreads();
    int inter[IM_GJ], ga[IM_GJ], da = 0;
#pragma unroll
    for (int q = 0; q < IM_GJ; ++q) inter[q] = ga[q] = 0;
    const unsigned long long* a = A + (size_t)i * words;
    for (long long w = tid; w < words; w += IM_THREADS) {
        const unsigned long long av = a[w];
        da += __popcll(av);
#pragma unroll
        for (int q = 0; q < IM_GJ; ++q)
            if (q < gn) {
                const unsigned long long bv = B[(size_t)(j0 + q) * words + w];
                inter[q] += __popcll(av & bv);
                ga[q] += __popcll(bv);
            }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        da += __shfl_xor(da, d);
#pragma unroll
        for (int q = 0; q < IM_GJ; ++q) {
            inter[q] += __shfl_xor(inter[q], d);
            ga[q] += __shfl_xor(ga[q], d);
        }
    }
    if ((tid & 63) == 0) {
        atomicAdd(&s_cnt[2 * IM_GJ], da);
#pragma unroll
        for (int q = 0; q < IM_GJ; ++q) {
            atomicAdd(&s_cnt[q], inter[q]);
            atomicAdd(&s_cnt[IM_GJ + q], ga[q]);
        }
    }
    __syncthreads();
    const int area = s_cnt[2 * IM_GJ];
    if (tid == 0 && blockIdx.y == 0) area_d[i] = area;
    if (tid < gn) {
        const int in = s_cnt[tid];
        double o = 0.0;
        if (in != 0) {
            const long long u = crowd[j0 + tid] ? (long long)area : (long long)area + s_cnt[IM_GJ + tid] - in;
            o = (double)in / (double)u;
        }
        iou[(size_t)i * g + j0 + tid] = o;
    }
}

// ---- cocoeval.py computeIoU's ordering + evaluateImg for one image -----------------------------------------------------------
// One workgroup.  (1) the valid rows get their class; (2) every valid row counts the rows ahead of it in (class ascending, score
// descending, row ascending) order: that is its slot in s_order, and the rows of its own class ahead of it are its in-(image,
// category) rank = cocoapi's stable argsort of -score; the row of rank 0 registers its category as a "head"; (3) the gts are
// ordered per area range by (class, ignored, index) = cocoapi's stable argsort of _ignore inside a category; (4) every
// (head, IoU type, area range, threshold) is one greedy chain of evaluateImg, one lane each, neighbouring lanes in one category; its
// matched-gt bitmap lives in LDS ([word][lane]: no bank conflicts); the result is OR-ed into the row's flag word.
constexpr int MATCH_THREADS = 512, USED_WORDS = MAXG / 32;
// (the body of one image's workgroup: k_coco_match_log runs it for its one image, k_coco_match_log_ragged for image blockIdx.x)
__device__ __forceinline__ void coco_match_log_image(
        const long long* __restrict__ ids, const float* __restrict__ scores, const int* __restrict__ count, int n,
        const int* __restrict__ boxes_px, const double* __restrict__ iou_box, const double* __restrict__ iou_mask,
        const double* __restrict__ area_box, const int* __restrict__ area_mask, const int* __restrict__ gt_cls,
        const uint8_t* __restrict__ gt_crowd, const double* __restrict__ gt_area, int g, const double* __restrict__ thr, int T,
        const double* __restrict__ area_rng, int num_classes, int max_rank, float* __restrict__ log_score, int* __restrict__ log_class,
        int* __restrict__ log_rank, unsigned* __restrict__ log_flags, unsigned long long* __restrict__ npig, int* __restrict__ class_rows) {
    __shared__ int s_cls[YM_EVAL_MAX_DET];
    __shared__ int s_rank[YM_EVAL_MAX_DET];
    __shared__ unsigned short s_order[YM_EVAL_MAX_DET];
    __shared__ unsigned short s_head[YM_EVAL_MAX_DET], s_hn[YM_EVAL_MAX_DET], s_hg0[YM_EVAL_MAX_DET], s_hgn[YM_EVAL_MAX_DET];
    __shared__ int s_gcls[MAXG];
    __shared__ unsigned char s_gflag[MAXG];                 // bit a = ignored in area range a, bit 7 = crowd
    __shared__ unsigned short s_gorder[AREAS][MAXG];
    __shared__ unsigned s_used[USED_WORDS][MATCH_THREADS];
    __shared__ int s_nheads;
    const int tid = threadIdx.x;
    const int below = count ? min(max(*count, 0), n) : n;
    if (tid == 0) s_nheads = 0;
    for (int i = tid; i < n; i += MATCH_THREADS) {
        bool ok = i < below;
        if (ok && boxes_px) {                               // eval.py:65: rows whose pixel box is empty never reach the JSON
            const int* b = boxes_px + (size_t)i * 4;
            ok = (long long)(b[2] - b[0]) * (long long)(b[3] - b[1]) > 0;
        }
        const long long id = ok ? ids[i] : -1;
        s_cls[i] = (id >= 0 && id < num_classes) ? (int)id : -1;
        for (int w = 0; w < WORDS_PER_ROW; ++w) log_flags[(size_t)i * WORDS_PER_ROW + w] = 0u;
    }
    for (int j = tid; j < g; j += MATCH_THREADS) {
        const int c = gt_cls[j];
        const bool ok = c >= 0 && c < num_classes;
        const bool crowd = gt_crowd[j] != 0;
        const double area = gt_area[j];
        unsigned f = crowd ? 0x80u : 0u;
        for (int a = 0; a < AREAS; ++a) {
            const bool ign = crowd || area < area_rng[2 * a] || area > area_rng[2 * a + 1];
            f |= ign ? 1u << a : 0u;
            if (ok && !ign) atomicAdd(&npig[(size_t)a * num_classes + c], 1ull);
        }
        s_gcls[j] = ok ? c : -1;
        s_gflag[j] = (unsigned char)f;
    }
    __syncthreads();
    for (int i = tid; i < n; i += MATCH_THREADS) {
        const int c = s_cls[i];
        if (c < 0) { s_rank[i] = 0; continue; }
        const float sc = scores[i];
        int lower = 0, rank = 0, same = 0;
        for (int j = 0; j < n; ++j) {
            const int cj = s_cls[j];
            if (cj < 0) continue;
            if (cj < c) { ++lower; continue; }
            if (cj != c) continue;
            ++same;
            const float sj = scores[j];
            rank += (sj > sc || (sj == sc && j < i)) ? 1 : 0;
        }
        s_rank[i] = rank;
        s_order[lower + rank] = (unsigned short)i;
        if (rank == 0) {
            const int h = atomicAdd(&s_nheads, 1);
            s_head[h] = (unsigned short)lower;
            s_hn[h] = (unsigned short)min(same, max_rank);
        }
    }
    for (int item = tid; item < AREAS * g; item += MATCH_THREADS) {
        const int a = item / g, j = item - a * g, c = s_gcls[j];
        if (c < 0) continue;
        const int ig = (s_gflag[j] >> a) & 1;
        int pos = 0;
        for (int q = 0; q < g; ++q) {
            const int cq = s_gcls[q];
            if (cq < 0) continue;
            const int iq = (s_gflag[q] >> a) & 1;
            pos += (cq < c || (cq == c && (iq < ig || (iq == ig && q < j)))) ? 1 : 0;
        }
        s_gorder[a][pos] = (unsigned short)j;
    }
    __syncthreads();
    const int nheads = s_nheads;
    for (int h = tid; h < nheads; h += MATCH_THREADS) {
        const int c = s_cls[s_order[s_head[h]]];
        int lower = 0, same = 0;
        for (int q = 0; q < g; ++q) {
            const int cq = s_gcls[q];
            lower += (cq >= 0 && cq < c) ? 1 : 0;
            same += cq == c ? 1 : 0;
        }
        s_hg0[h] = (unsigned short)lower;
        s_hgn[h] = (unsigned short)same;
    }
    __syncthreads();                                          // (also orders the zeroed flag words before the ORs below)
    const int chains = 2 * AREAS * T;
    for (int item = tid; item < nheads * chains; item += MATCH_THREADS) {
        const int h = item / chains, chain = item - h * chains;
        const int tw = chain / T, k = chain - tw * T, type = tw / AREAS, a = tw - type * AREAS;
        const double* iou = type == 0 ? iou_box : iou_mask;
        if ((type == 0 ? (const void*)area_box : (const void*)area_mask) == nullptr) continue;      // this IoU type is not evaluated
        const int p0 = s_head[h], nd = s_hn[h], g0 = s_hg0[h], gn = s_hgn[h];
        const double t = thr[k], lo = area_rng[2 * a], hi = area_rng[2 * a + 1];
#pragma unroll
        for (int w = 0; w < USED_WORDS; ++w) s_used[w][tid] = 0u;
        for (int d = 0; d < nd; ++d) {
            const int i = s_order[p0 + d];
            double best = fmin(t, 1.0 - 1e-10);
            int m = -1, m_ig = 0;
            for (int q = 0; q < gn; ++q) {
                const int j = s_gorder[a][g0 + q];
                const unsigned f = s_gflag[j];
                const int ig = (f >> a) & 1;
                // a gt already matched at this threshold is taken again only when it is a crowd
                if (((s_used[q >> 5][tid] >> (q & 31)) & 1u) && !(f & 0x80u)) continue;
                // the best match so far is a regular gt and the ignored gts begin here: stop
                if (m >= 0 && m_ig == 0 && ig == 1) break;
                const double v = iou[(size_t)i * g + j];
                if (v < best) continue;
                best = v;
                m = q;
                m_ig = ig;
            }
            unsigned bits;
            if (m >= 0) {
                s_used[m >> 5][tid] |= 1u << (m & 31);
                bits = (1u << k) | (m_ig ? 1u << (16 + k) : 0u);
            } else {
                const double ar = type == 0 ? area_box[i] : (double)area_mask[i];
                bits = (ar < lo || ar > hi) ? 1u << (16 + k) : 0u;
            }
            if (bits) atomicOr(&log_flags[(size_t)i * WORDS_PER_ROW + tw], bits);
        }
    }
    for (int i = tid; i < n; i += MATCH_THREADS) {
        const int c = (s_cls[i] >= 0 && s_rank[i] < max_rank) ? s_cls[i] : -1;
        log_class[i] = c;
        log_rank[i] = c >= 0 ? s_rank[i] : 0;
        log_score[i] = c >= 0 ? scores[i] : 0.f;
        if (c >= 0) atomicAdd(&class_rows[c], 1);
    }
}

__global__ __launch_bounds__(MATCH_THREADS) void k_coco_match_log(
        const long long* __restrict__ ids, const float* __restrict__ scores, const int* __restrict__ count, int n,
        const int* __restrict__ boxes_px, const double* __restrict__ iou_box, const double* __restrict__ iou_mask,
        const double* __restrict__ area_box, const int* __restrict__ area_mask, const int* __restrict__ gt_cls,
        const uint8_t* __restrict__ gt_crowd, const double* __restrict__ gt_area, int g, const double* __restrict__ thr, int T,
        const double* __restrict__ area_rng, int num_classes, int max_rank, float* __restrict__ log_score, int* __restrict__ log_class,
        int* __restrict__ log_rank, unsigned* __restrict__ log_flags, unsigned long long* __restrict__ npig, int* __restrict__ class_rows) {
    coco_match_log_image(ids, scores, count, n, boxes_px, iou_box, iou_mask, area_box, area_mask, gt_cls, gt_crowd, gt_area, g, thr, T,
                         area_rng, num_classes, max_rank, log_score, log_class, log_rank, log_flags, npig, class_rows);
}

// ---- evaluateImg for a whole request (include/yolact_hip.h "ym_eval_coco_add_ragged_packed") -----------------------------------
// What the three launches know about their images, BY VALUE in the kernel arguments (like EvalRaggedTable of metrics.hip).  The
// workspace is a region of doubles and, behind it, a region of ints.  Image b's doubles at dbl_off[b]: iou_box [max_det][g_b] and
// area_box [max_det] (bbox), then iou_mask [max_det][g_b] (segm).  Its ints at int_off[b] (segm only): the partial counts inter
// [chunks_b][max_det][g_b], area_a [chunks_b][max_det], area_b [chunks_b][g_b] (chunks_b = ceil(words_b / PWORDS), also for g_b = 0),
// then area_mask [max_det].  An image that is padding owns no chunk of the first launch.
struct CocoRaggedTable {
    int chunk_first[YM_RAGGED_MAX_IMAGES + 1];   // prefix sum of the chunks: which image a workgroup of the first launch serves
    int gt_first[YM_RAGGED_MAX_IMAGES + 1];      // first gt of image b in the gt arrays (and g_b as the difference)
    int words[YM_RAGGED_MAX_IMAGES];             // img_h_b * ceil(img_w_b / 64)
    long long det_off[YM_RAGGED_MAX_IMAGES], gt_off[YM_RAGGED_MAX_IMAGES];   // words from det_bits / gt_bits to the image's block
    long long dbl_off[YM_RAGGED_MAX_IMAGES], int_off[YM_RAGGED_MAX_IMAGES];
    long long log_row[YM_RAGGED_MAX_IMAGES];     // image_index * max_det; < 0 = padding
};

__device__ __forceinline__ int coco_ragged_count(const int* __restrict__ counts, int b, int max_det) { return min(max(counts[b], 0), max_det); }

// The chunks of image b's masks: what the table's prefix says for an image of the first launch, the same number recomputed for the
// finalize step (0 when segm is off: `words` stays 0).
__device__ __forceinline__ int coco_ragged_chunks(const CocoRaggedTable& t, int b) { return (t.words[b] + PWORDS - 1) / PWORDS; }

// grid: (all chunks of all live images, the largest number of gt groups of an image).  Rows at or past the image's count are not
// loaded.  An image without ground truth keeps its chunks: its detections' popcounts (area_a) decide their ignore bits.
__global__ __launch_bounds__(512) void k_coco_inter_ragged(const unsigned long long* __restrict__ det_bits,
                                                           const unsigned long long* __restrict__ gt_bits, const int* __restrict__ counts,
                                                           int B, int max_det, const CocoRaggedTable t, int* __restrict__ part) {
    int b = 0;
    while (b + 1 < B && (int)blockIdx.x >= t.chunk_first[b + 1]) ++b;
    const int g = t.gt_first[b + 1] - t.gt_first[b];
    if (blockIdx.y > 0 && (int)blockIdx.y * MAXR >= g) return;
    const int n = coco_ragged_count(counts, b, max_det);
    if (n == 0) return;
    const int chunks = t.chunk_first[b + 1] - t.chunk_first[b];
    int* inter = part + t.int_off[b];
    int* area_a = inter + (size_t)chunks * max_det * g;
    int* area_b = area_a + (size_t)chunks * max_det;
    inter_packed_chunk(det_bits + t.det_off[b], n, max_det, gt_bits + t.gt_off[b], g, (long long)t.words[b], (int)blockIdx.x - t.chunk_first[b],
                       (int)blockIdx.y, inter, area_a, area_b);
}

// grid: (groups of 64 items of the largest image, B).  The items of an image with n rows below its count: the n * g_b pairs
// e = i * g_b + j, then the n rows.  The chunk sums of an item are split over FSL slices and joined in LDS (exact integers).  Slice 0
// writes the mask side: a pair's rleIou quotient (k_coco_iou_mask's), a row's area_mask.  Slice 1 writes the box side: bbIou on
// (x1, y1, x2 - x1, y2 - y1) of the int32 pixel box in fp64 (exact), a row's area_box = w * h.
constexpr int FSL = 16;
__global__ __launch_bounds__(64 * FSL) void k_coco_iou_ragged(const int* __restrict__ boxes_px, const double* __restrict__ gt_xywh,
                                                              const uint8_t* __restrict__ gt_crowd, const int* __restrict__ counts,
                                                              int max_det, int kinds, const CocoRaggedTable t, int* __restrict__ part,
                                                              double* __restrict__ dbl) {
    __shared__ int s_i[FSL][64], s_a[FSL][64], s_b[FSL][64];
    const int b = blockIdx.y;
    if (t.log_row[b] < 0) return;
    const int g = t.gt_first[b + 1] - t.gt_first[b];
    const int n = coco_ragged_count(counts, b, max_det);
    const int pairs = n * g, items = pairs + n;
    if ((int)blockIdx.x * 64 >= items) return;              // (uniform; n == 0 as well)
    const int lane = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const int e = blockIdx.x * 64 + lane;
    const bool live = e < items, pair = e < pairs;
    const int i = pair ? e / g : (live ? e - pairs : 0), j = pair ? e - i * g : 0;
    const bool bbox = (kinds & 1) != 0, segm = (kinds & 2) != 0;
    const int chunks = segm ? coco_ragged_chunks(t, b) : 0;
    int* inter = part + t.int_off[b];
    int* area_a = inter + (size_t)chunks * max_det * g;
    int* area_b = area_a + (size_t)chunks * max_det;
    int* area_mask = area_b + (size_t)chunks * g;
    double* iou_box = dbl + t.dbl_off[b];
    double* area_box = iou_box + (size_t)max_det * g;
    double* iou_mask = bbox ? area_box + max_det : iou_box;
    int it = 0, aa = 0, ab = 0;
    if (live) {
#pragma unroll 4
        for (int c = sl; c < chunks; c += FSL) {
            aa += area_a[(size_t)c * max_det + i];
            if (pair) {
                it += inter[((size_t)c * max_det + i) * g + j];
                ab += area_b[(size_t)c * g + j];
            }
        }
    }
    s_i[sl][lane] = it; s_a[sl][lane] = aa; s_b[sl][lane] = ab;
    __syncthreads();
    if (!live) return;
    if (sl == 0 && segm) {
        int in = 0, da = 0, ga = 0;
#pragma unroll
        for (int q = 0; q < FSL; ++q) { in += s_i[q][lane]; da += s_a[q][lane]; ga += s_b[q][lane]; }
        if (pair) {
            double o = 0.0;
            if (in != 0) {
                const long long u = gt_crowd[t.gt_first[b] + j] ? (long long)da : (long long)da + ga - in;
                o = (double)in / (double)u;
            }
            iou_mask[e] = o;
        } else {
            area_mask[i] = da;
        }
    }
    if (sl == 1 && bbox) {
        const int* pb = boxes_px + ((size_t)b * max_det + i) * 4;
        const double x1 = (double)pb[0], y1 = (double)pb[1];
        const double D[4] = {x1, y1, (double)pb[2] - x1, (double)pb[3] - y1};
        if (pair) iou_box[e] = coco_bb_iou(D, gt_xywh + (size_t)(t.gt_first[b] + j) * 4, gt_crowd[t.gt_first[b] + j] != 0);
        else area_box[i] = D[2] * D[3];
    }
}

// grid: B.  Workgroup b is k_coco_match_log's workgroup for image b: its max_det padded rows, its count, its gts, its IoUs and
// areas from the launch before, its log rows.  A padding entry exits at once.
__global__ __launch_bounds__(MATCH_THREADS) void k_coco_match_log_ragged(
        const long long* __restrict__ ids, const float* __restrict__ scores, const int* __restrict__ counts, int max_det,
        const int* __restrict__ boxes_px, int kinds, const CocoRaggedTable t, const int* __restrict__ part, const double* __restrict__ dbl,
        const int* __restrict__ gt_cls, const uint8_t* __restrict__ gt_crowd, const double* __restrict__ gt_area,
        const double* __restrict__ thr, int T, const double* __restrict__ area_rng, int num_classes, int max_rank,
        float* __restrict__ log_score, int* __restrict__ log_class, int* __restrict__ log_rank, unsigned* __restrict__ log_flags,
        unsigned long long* __restrict__ npig, int* __restrict__ class_rows) {
    const int b = blockIdx.x;
    const long long row = t.log_row[b];
    if (row < 0) return;
    const int g = t.gt_first[b + 1] - t.gt_first[b], g0 = t.gt_first[b];
    const bool bbox = (kinds & 1) != 0, segm = (kinds & 2) != 0;
    const int chunks = segm ? coco_ragged_chunks(t, b) : 0;
    const double* iou_box = dbl + t.dbl_off[b];
    const double* area_box = iou_box + (size_t)max_det * g;
    const double* iou_mask = bbox ? area_box + max_det : iou_box;
    const int* area_mask = part + t.int_off[b] + (size_t)chunks * ((size_t)max_det * g + max_det + g);
    coco_match_log_image(ids + (size_t)b * max_det, scores + (size_t)b * max_det, counts + b, max_det,
                         boxes_px ? boxes_px + (size_t)b * max_det * 4 : nullptr, bbox ? iou_box : nullptr, segm ? iou_mask : nullptr,
                         bbox ? area_box : nullptr, segm ? area_mask : nullptr, gt_cls + g0, gt_crowd + g0, gt_area + g0, g, thr, T,
                         area_rng, num_classes, max_rank, log_score + row, log_class + row, log_rank + row,
                         log_flags + row * WORDS_PER_ROW, npig, class_rows);
}

// ---- cocoeval.py accumulate ---------------------------------------------------------------------------------------------------
// The flag words and ranks in sorted order, once ([word][row]: the workgroups of a class read consecutive words).
__global__ void k_coco_gather(const unsigned* __restrict__ flags, const int* __restrict__ rank, const long long* __restrict__ order,
                              long long rows, unsigned* __restrict__ sorted, int* __restrict__ sorted_rank) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const long long p = order[r];
    const bool ok = p >= 0 && p < rows;
    for (int w = 0; w < WORDS_PER_ROW; ++w) sorted[(size_t)w * rows + r] = ok ? flags[(size_t)p * WORDS_PER_ROW + w] : 0u;
    sorted_rank[r] = ok ? rank[p] : 0x7fffffff;
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

// One (category, IoU type, area range, threshold, maxDet) cell per workgroup.  A sorted row of the category is a true positive
// (rank < maxDet, matched, not ignored), a false positive (rank < maxDet, unmatched, not ignored) or neither; rows that are neither
// change no count, so precision there equals the row's before and the envelope / the searchsorted samples are those of cocoapi's
// list without them.  Pass A counts both kinds.  Pass B goes BACKWARDS in chunks of YM_COCO_ROWS_PER_PASS rows carrying (tp and fp
// before the chunk, envelope of everything behind it): pr = tp / ((fp + tp) + eps), envelope = suffix maximum (exact in any order).
// rc = tp / npig grows with tp alone, so np.searchsorted(rc, recThrs[r], 'left') is the first row whose tp reaches t_r = the smallest
// t with (double)t / npig >= recThrs[r] (found with those very quotients; none -> the sample stays 0, cocoapi's IndexError exit).
constexpr int ACC_THREADS = 256, ACC_RPT = YM_COCO_ROWS_PER_PASS / ACC_THREADS;
static_assert(ACC_THREADS * ACC_RPT == YM_COCO_ROWS_PER_PASS && YM_COCO_ROWS_PER_PASS < 65536, "tp and fp of a pass share one scan word");
__global__ __launch_bounds__(ACC_THREADS) void k_coco_accumulate(const unsigned* __restrict__ sorted, const int* __restrict__ sorted_rank,
                                                                 long long rows, const long long* __restrict__ seg,
                                                                 const long long* __restrict__ npig, const double* __restrict__ rec_thr,
                                                                 int R, const int* __restrict__ max_dets, int M, int T, int K, double eps,
                                                                 int kinds, double* __restrict__ precision, double* __restrict__ recall) {
    __shared__ long long s_t[ACC_THREADS];
    __shared__ double s_sample[ACC_THREADS];
    __shared__ int s_tp[YM_COCO_ROWS_PER_PASS];
    __shared__ double s_env[YM_COCO_ROWS_PER_PASS];
    __shared__ int s_wsum[ACC_THREADS / 64];
    __shared__ double s_wmax[ACC_THREADS / 64];
    __shared__ unsigned long long s_total[2];
    const int c = blockIdx.x, cell = blockIdx.y, mi = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tw = cell / T, k = cell - tw * T, type = tw / AREAS, a = tw - type * AREAS;
    if (!((kinds >> type) & 1)) return;
    const long long G = npig[(size_t)a * K + c];
    if (G <= 0) return;                                         // (uniform) the cell keeps -1
    long long beg = min(max(seg[c], 0ll), rows), end = min(max(seg[c + 1], 0ll), rows);
    if (end < beg) end = beg;
    const long long m = end - beg;
    const int md = max_dets[mi];
    const unsigned* f = sorted + (size_t)tw * rows + beg;
    const int* rk = sorted_rank + beg;
    const double Gd = (double)G;
    double* pout = precision + (size_t)type * T * R * K * AREAS * M;
    double* rout = recall + (size_t)type * T * K * AREAS * M + (((size_t)k * K + c) * AREAS + a) * M + mi;
    if (tid < R) {
        const double x = rec_thr[tid];
        long long t = (long long)(x * Gd);
        t = min(max(t, 0ll), G);
        while (t > 0 && (double)(t - 1) / Gd >= x) --t;
        while (t < G && (double)t / Gd < x) ++t;
        if ((double)t / Gd < x) t = G + 1;                      // recall never gets there
        s_t[tid] = t;
        s_sample[tid] = 0.0;
    }
    // row -> 1 (true positive) | 65536 (false positive) | 0
    auto kind_of = [&](long long r) -> int {
        const unsigned w = f[r];
        const bool live = rk[r] < md && !((w >> (16 + k)) & 1u);
        return !live ? 0 : (((w >> k) & 1u) ? 1 : 65536);
    };
    unsigned long long my_tp = 0, my_fp = 0;
    for (long long r = tid; r < m; r += ACC_THREADS) {
        const int b = kind_of(r);
        my_tp += b & 1;
        my_fp += b >> 16;
    }
    if (tid < 2) s_total[tid] = 0;
    __syncthreads();
    atomicAdd(&s_total[0], my_tp);                              // (integers: any order gives the same sums)
    atomicAdd(&s_total[1], my_fp);
    __syncthreads();
    long long rem_tp = (long long)s_total[0], rem_fp = (long long)s_total[1];
    if (tid == 0) *rout = (double)rem_tp / Gd;                  // rc[-1], 0 without rows
    double carry = -1.0;
    const long long chunks = (m + YM_COCO_ROWS_PER_PASS - 1) / YM_COCO_ROWS_PER_PASS;
    for (long long ch = chunks - 1; ch >= 0; --ch) {
        const long long r0 = ch * YM_COCO_ROWS_PER_PASS;
        const int cn = (int)min((long long)YM_COCO_ROWS_PER_PASS, m - r0);
        int b[ACC_RPT], local = 0;
#pragma unroll
        for (int e = 0; e < ACC_RPT; ++e) {
            const int q = tid * ACC_RPT + e;
            b[e] = q < cn ? kind_of(r0 + q) : 0;
            local += b[e];
        }
        const int incl = wave_inclusive_sum(local, lane);
        if (lane == 63) s_wsum[wave] = incl;
        __syncthreads();
        int before = incl - local, chunk = 0;
#pragma unroll
        for (int w = 0; w < ACC_THREADS / 64; ++w) {
            before += w < wave ? s_wsum[w] : 0;
            chunk += s_wsum[w];
        }
        const int chunk_tp = chunk & 0xffff, chunk_fp = chunk >> 16;
        const long long tp_in = rem_tp - chunk_tp, fp_in = rem_fp - chunk_fp;
        double p[ACC_RPT];
        int run = before;
#pragma unroll
        for (int e = 0; e < ACC_RPT; ++e) {
            const int q = tid * ACC_RPT + e;
            run += b[e];
            const int rtp = run & 0xffff, rfp = run >> 16;
            s_tp[q] = rtp;
            const double tp = (double)(tp_in + rtp), fp = (double)(fp_in + rfp);
            p[e] = q < cn ? tp / ((fp + tp) + eps) : -1.0;
        }
#pragma unroll
        for (int e = ACC_RPT - 2; e >= 0; --e) p[e] = fmax(p[e], p[e + 1]);
        const double sfx = wave_suffix_max(p[0], lane);
        if (lane == 0) s_wmax[wave] = sfx;
        __syncthreads();
        double behind = carry;
#pragma unroll
        for (int w = 0; w < ACC_THREADS / 64; ++w) behind = w > wave ? fmax(behind, s_wmax[w]) : behind;
        const double next_lane = __shfl_down(sfx, 1);
        if (lane < 63) behind = fmax(behind, next_lane);
#pragma unroll
        for (int e = 0; e < ACC_RPT; ++e) s_env[tid * ACC_RPT + e] = fmax(p[e], behind);
        __syncthreads();
        if (tid < R) {
            const long long t = s_t[tid];
            const bool here = t == 0 ? ch == 0 : (tp_in < t && t <= tp_in + chunk_tp);
            if (here) {
                const int want = (int)(t - tp_in);
                int lo = 0, hi = cn - 1;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (s_tp[mid] >= want) hi = mid; else lo = mid + 1;
                }
                s_sample[tid] = s_env[lo];
            }
        }
        carry = s_env[0];
        rem_tp = tp_in;
        rem_fp = fp_in;
        __syncthreads();
    }
    __syncthreads();
    if (tid < R) pout[((((size_t)k * R + tid) * K + c) * AREAS + a) * M + mi] = s_sample[tid];
}

}  // namespace

extern "C" int ym_coco_iou_box(const double* dt_xywh, int n, const double* gt_xywh, int g, const uint8_t* iscrowd, double* iou, ym_stream_t s) {
    YM_REQUIRE(dt_xywh && gt_xywh && iscrowd && iou && n > 0 && g > 0, "coco_iou_box: null pointer or n, g <= 0");
    YM_REQUIRE((long long)n * g < (1ll << 30), "coco_iou_box: n*g too large");
    hipLaunchKernelGGL(k_coco_iou_box, dim3((n * g + 255) / 256), dim3(256), 0, (hipStream_t)s, dt_xywh, n, gt_xywh, g, iscrowd, iou);
    return ym_check_launch("coco_iou_box");
}

extern "C" int ym_coco_iou_mask_packed(const uint64_t* bits_d, int n, const uint64_t* bits_g, int g, int64_t words, const uint8_t* iscrowd,
                                       double* iou, int32_t* area_d, ym_stream_t s) {
    YM_REQUIRE(bits_d && bits_g && iscrowd && iou && area_d, "coco_iou_mask_packed: null pointer");
    YM_REQUIRE(n > 0 && n <= 65535 && g > 0 && g <= MAXG && words > 0 && words < (1ll << 24),
               "coco_iou_mask_packed: need 0 < n <= 65535, 0 < g <= %d and 0 < words < 2^24", MAXG);
    hipLaunchKernelGGL(k_coco_iou_mask, dim3((unsigned)n, (unsigned)((g + IM_GJ - 1) / IM_GJ)), dim3(IM_THREADS), 0, (hipStream_t)s,
                       reinterpret_cast<const unsigned long long*>(bits_d), n, reinterpret_cast<const unsigned long long*>(bits_g), g,
                       (long long)words, iscrowd, iou, area_d);
    return ym_check_launch("coco_iou_mask_packed");
}

extern "C" int ym_coco_match_log(const int64_t* ids, const float* scores, const int32_t* count, int n, const int32_t* boxes_px,
                                 const double* iou_box, const double* iou_mask, const double* area_box, const int32_t* area_mask,
                                 const int32_t* gt_class, const uint8_t* gt_iscrowd, const double* gt_area, int g,
                                 const double* thresholds, int T, const double* area_rng, int num_classes, int max_rank,
                                 float* log_score, int32_t* log_class, int32_t* log_rank, uint32_t* log_flags, int64_t log_offset,
                                 int64_t* npig, int32_t* class_rows, ym_stream_t s) {
    YM_REQUIRE(thresholds && area_rng && log_score && log_class && log_rank && log_flags && npig && class_rows, "coco_match_log: null pointer");
    YM_REQUIRE(n >= 0 && n <= YM_EVAL_MAX_DET && log_offset >= 0, "coco_match_log: need 0 <= n <= %d rows and a log offset >= 0", YM_EVAL_MAX_DET);
    YM_REQUIRE(n == 0 || (ids && scores), "coco_match_log: null pointer");
    YM_REQUIRE(g >= 0 && g <= MAXG, "coco_match_log: need 0 <= g <= %d ground-truth annotations per image, got %d", MAXG, g);
    YM_REQUIRE(g == 0 || (gt_class && gt_iscrowd && gt_area), "coco_match_log: null pointer");
    YM_REQUIRE(T > 0 && T <= YM_EVAL_MAX_THRESHOLDS && num_classes > 0 && max_rank > 0,
               "coco_match_log: need 0 < T <= %d, num_classes > 0, max_rank > 0", YM_EVAL_MAX_THRESHOLDS);
    YM_REQUIRE(n == 0 || area_box || area_mask, "coco_match_log: no IoU type to evaluate");
    YM_REQUIRE(n == 0 || g == 0 || ((!area_box || iou_box) && (!area_mask || iou_mask)), "coco_match_log: an IoU type without its IoU matrix");
    hipLaunchKernelGGL(k_coco_match_log, dim3(1), dim3(MATCH_THREADS), 0, (hipStream_t)s, reinterpret_cast<const long long*>(ids), scores,
                       count, n, boxes_px, iou_box, iou_mask, area_box, area_mask, gt_class, gt_iscrowd, gt_area, g, thresholds, T, area_rng,
                       num_classes, max_rank, log_score + log_offset, log_class + log_offset, log_rank + log_offset,
                       log_flags + log_offset * WORDS_PER_ROW, reinterpret_cast<unsigned long long*>(npig), class_rows);
    return ym_check_launch("coco_match_log");
}

extern "C" size_t ym_coco_accumulate_workspace_bytes(int64_t rows) {
    return rows > 0 ? (size_t)rows * (WORDS_PER_ROW + 1) * sizeof(uint32_t) : 0;
}

extern "C" int ym_coco_accumulate(const uint32_t* log_flags, const int32_t* log_rank, const int64_t* order, int64_t rows, const int64_t* seg,
                                  const int64_t* npig, const double* rec_thrs, int R, const int32_t* max_dets, int M, int T,
                                  int num_classes, double eps, int kinds, double* precision, double* recall, void* workspace,
                                  size_t workspace_bytes, ym_stream_t s) {
    YM_REQUIRE(log_flags && log_rank && order && seg && npig && rec_thrs && max_dets && precision && recall, "coco_accumulate: null pointer");
    YM_REQUIRE(rows > 0 && T > 0 && T <= YM_EVAL_MAX_THRESHOLDS && num_classes > 0 && num_classes <= 65535 && M > 0 && M <= 64,
               "coco_accumulate: need rows > 0, 0 < T <= %d, 0 < num_classes <= 65535, 0 < M <= 64", YM_EVAL_MAX_THRESHOLDS);
    YM_REQUIRE(R > 0 && R <= ACC_THREADS, "coco_accumulate: 1 .. %d recall thresholds", ACC_THREADS);
    YM_REQUIRE(kinds > 0 && kinds < 4, "coco_accumulate: kinds is a mask of bbox (1) and segm (2)");
    if (!workspace || workspace_bytes < ym_coco_accumulate_workspace_bytes(rows)) { ym_set_error("coco_accumulate: workspace too small"); return YM_ENOSPC; }
    hipStream_t st = (hipStream_t)s;
    unsigned* sorted = (unsigned*)workspace;
    int* sorted_rank = (int*)(sorted + (size_t)rows * WORDS_PER_ROW);
    hipLaunchKernelGGL(k_coco_gather, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, log_flags, log_rank,
                       reinterpret_cast<const long long*>(order), (long long)rows, sorted, sorted_rank);
    hipLaunchKernelGGL(k_coco_accumulate, dim3((unsigned)num_classes, (unsigned)(2 * AREAS * T), (unsigned)M), dim3(ACC_THREADS), 0, st, sorted,
                       sorted_rank, (long long)rows, reinterpret_cast<const long long*>(seg), reinterpret_cast<const long long*>(npig), rec_thrs,
                       R, max_dets, M, T, num_classes, eps, kinds, precision, recall);
    return ym_check_launch("coco_accumulate");
}

// Where image b's doubles and ints lie in the workspace of ym_eval_coco_add_ragged_packed (CocoRaggedTable): a function of the sizes
// alone, so a padding entry keeps its (unused) room and the workspace query needs no image_index.  false for arguments the entry refuses.
static bool coco_ragged_layout(const ym_ragged_image* det_blocks, const int32_t* gt_first, int B, int max_det, int kinds, long long* dbl_off,
                               long long* int_off, size_t* doubles, size_t* ints) {
    if (!gt_first || B < 1 || B > YM_RAGGED_MAX_IMAGES || max_det < 1 || max_det > YM_EVAL_MAX_DET || kinds < 1 || kinds > 3) return false;
    const bool bbox = (kinds & 1) != 0, segm = (kinds & 2) != 0;
    if (segm && !det_blocks) return false;
    size_t nd = 0, ni = 0;
    for (int b = 0; b < B; ++b) {
        const long long g = (long long)gt_first[b + 1] - gt_first[b];
        if (g < 0 || g > MAXG) return false;
        if (dbl_off) dbl_off[b] = (long long)nd;
        if (int_off) int_off[b] = (long long)ni;
        if (bbox) nd += (size_t)max_det * g + max_det;
        if (segm) {
            if (det_blocks[b].img_h <= 0 || det_blocks[b].img_w <= 0) return false;
            const long long words = (long long)det_blocks[b].img_h * (long long)ym_mask_row(true, det_blocks[b].img_w);
            if (words >= (1ll << 24)) return false;
            const size_t chunks = (size_t)((words + PWORDS - 1) / PWORDS);
            nd += (size_t)max_det * g;
            ni += chunks * ((size_t)max_det * g + max_det + g) + max_det;
        }
    }
    *doubles = nd;
    *ints = ni;
    return true;
}

extern "C" size_t ym_eval_coco_add_ragged_workspace_bytes(const ym_ragged_image* det_blocks, const int32_t* gt_first, int B, int max_det,
                                                          int kinds) {
    size_t nd = 0, ni = 0;
    if (!coco_ragged_layout(det_blocks, gt_first, B, max_det, kinds, nullptr, nullptr, &nd, &ni)) return 0;
    return nd * sizeof(double) + ni * sizeof(int) + 256;
}

extern "C" int ym_eval_coco_add_ragged_packed(const int64_t* ids, const float* scores, const int32_t* boxes_px, const int32_t* counts, int B,
                                              int max_det, const uint64_t* det_bits, const ym_ragged_image* det_blocks,
                                              const int32_t* gt_class, const uint8_t* gt_iscrowd, const double* gt_area,
                                              const double* gt_xywh, const int32_t* gt_first, const uint64_t* gt_bits,
                                              const ym_ragged_image* gt_blocks, const int64_t* image_index, const double* thresholds, int T,
                                              const double* area_rng, int num_classes, int max_rank, int kinds, float* log_score,
                                              int32_t* log_class, int32_t* log_rank, uint32_t* log_flags, int64_t log_rows, int64_t* npig,
                                              int32_t* class_rows, void* workspace, size_t workspace_bytes, ym_stream_t s) {
    const char* what = "eval_coco_add_ragged_packed";
    YM_REQUIRE(B >= 1 && B <= YM_RAGGED_MAX_IMAGES, "%s: 1 .. %d images per call, got %d", what, YM_RAGGED_MAX_IMAGES, B);
    YM_REQUIRE(max_det >= 1 && max_det <= YM_EVAL_MAX_DET, "%s: need 0 < max_det <= %d, got %d", what, YM_EVAL_MAX_DET, max_det);
    YM_REQUIRE(T >= 1 && T <= YM_EVAL_MAX_THRESHOLDS, "%s: 1 .. %d thresholds (16 flag bits per word), got %d", what,
               YM_EVAL_MAX_THRESHOLDS, T);
    YM_REQUIRE(num_classes > 0 && max_rank > 0, "%s: num_classes = %d, max_rank = %d", what, num_classes, max_rank);
    YM_REQUIRE(kinds >= 1 && kinds <= 3, "%s: kinds is a mask of bbox (1) and segm (2), got %d", what, kinds);
    const bool bbox = (kinds & 1) != 0, segm = (kinds & 2) != 0;
    YM_REQUIRE(ids && scores && counts && gt_first && image_index && thresholds && area_rng && log_score && log_class && log_rank &&
                   log_flags && npig && class_rows && workspace,
               "%s: null pointer", what);
    YM_REQUIRE(!bbox || boxes_px, "%s: null pointer (bbox needs boxes_px)", what);
    YM_REQUIRE(!segm || (det_bits && det_blocks && gt_blocks), "%s: null pointer (segm needs det_bits and both tables)", what);
    YM_REQUIRE(gt_first[0] >= 0, "%s: gt_first[0] = %d", what, gt_first[0]);
    for (int b = 0; b < B; ++b) {
        const long long g = (long long)gt_first[b + 1] - gt_first[b];
        YM_REQUIRE(g >= 0, "%s: gt_first is not ascending at image %d", what, b);
        YM_REQUIRE(g <= MAXG, "%s: image %d has %lld gt annotations, at most %d are matched", what, b, g, MAXG);
    }
    YM_REQUIRE(gt_first[B] == 0 || (gt_class && gt_iscrowd && gt_area), "%s: null pointer", what);
    YM_REQUIRE(gt_first[B] == 0 || !bbox || gt_xywh, "%s: null pointer (bbox needs gt_xywh)", what);
    YM_REQUIRE(gt_first[B] == 0 || !segm || gt_bits, "%s: null pointer (segm needs gt_bits)", what);
    if (segm) {
        const int rc_det = ym_check_ragged_table(what, det_blocks, B, 8, [&](const ym_ragged_image& im) {
            return (int64_t)max_det * im.img_h * (int64_t)ym_mask_row(true, im.img_w);
        });
        if (rc_det != YM_OK) return rc_det;
        const int rc_gt = ym_check_ragged_table_indexed(what, gt_blocks, B, 8, [&](int b) {
            return (int64_t)(gt_first[b + 1] - gt_first[b]) * gt_blocks[b].img_h * (int64_t)ym_mask_row(true, gt_blocks[b].img_w);
        });
        if (rc_gt != YM_OK) return rc_gt;
        for (int b = 0; b < B; ++b) {
            YM_REQUIRE(gt_blocks[b].img_h == det_blocks[b].img_h && gt_blocks[b].img_w == det_blocks[b].img_w,
                       "%s: image %d: gt masks of %d x %d for detection masks of %d x %d", what, b, gt_blocks[b].img_h, gt_blocks[b].img_w,
                       det_blocks[b].img_h, det_blocks[b].img_w);
            YM_REQUIRE((long long)det_blocks[b].img_h * (long long)ym_mask_row(true, det_blocks[b].img_w) < (1ll << 24),
                       "%s: image %d: need img_h * ceil(img_w / 64) < 2^24 words (exact int32 counts)", what, b);
        }
    }
    bool any = false;
    for (int b = 0; b < B; ++b) {
        if (image_index[b] < 0) continue;
        YM_REQUIRE(image_index[b] < log_rows && (image_index[b] + 1) * max_det <= log_rows,
                   "%s: image index %lld: its %d rows end past the %lld rows of the log", what, (long long)image_index[b], max_det,
                   (long long)log_rows);
        for (int a = 0; a < b; ++a)
            YM_REQUIRE(image_index[a] != image_index[b], "%s: image index %lld twice in one call", what, (long long)image_index[b]);
        any = true;
    }
    CocoRaggedTable t = {};
    size_t nd = 0, ni = 0;
    YM_REQUIRE(coco_ragged_layout(det_blocks, gt_first, B, max_det, kinds, t.dbl_off, t.int_off, &nd, &ni), "%s: bad sizes", what);
    if (workspace_bytes < nd * sizeof(double) + ni * sizeof(int) + 256) { ym_set_error("%s: workspace too small", what); return YM_ENOSPC; }
    if (!any) return YM_OK;                                  // (padding only)
    int max_groups = 1, max_items = 0;
    for (int b = 0; b < B; ++b) {
        const int g = gt_first[b + 1] - gt_first[b];
        const bool live = image_index[b] >= 0;
        t.gt_first[b] = gt_first[b];
        t.log_row[b] = live ? image_index[b] * max_det : -1;
        if (segm) {
            t.words[b] = det_blocks[b].img_h * (int)ym_mask_row(true, det_blocks[b].img_w);
            t.det_off[b] = det_blocks[b].offset;
            t.gt_off[b] = gt_blocks[b].offset;
        }
        t.chunk_first[b + 1] = t.chunk_first[b] + (live && segm ? ym_cdiv(t.words[b], PWORDS) : 0);
        if (live) {
            max_groups = max_groups > ym_cdiv(g, MAXR) ? max_groups : ym_cdiv(g, MAXR);
            max_items = max_items > max_det * (g + 1) ? max_items : max_det * (g + 1);
        }
    }
    t.gt_first[B] = gt_first[B];
    for (int b = B; b < YM_RAGGED_MAX_IMAGES; ++b) { t.chunk_first[b + 1] = t.chunk_first[B]; t.gt_first[b + 1] = gt_first[B]; t.log_row[b] = -1; }
    hipStream_t st = (hipStream_t)s;
    double* dbl = (double*)workspace;
    int* part = (int*)(dbl + nd);
    if (segm)
        hipLaunchKernelGGL(k_coco_inter_ragged, dim3((unsigned)t.chunk_first[B], (unsigned)max_groups), dim3(512), 0, st,
                           reinterpret_cast<const unsigned long long*>(det_bits), reinterpret_cast<const unsigned long long*>(gt_bits), counts, B,
                           max_det, t, part);
    hipLaunchKernelGGL(k_coco_iou_ragged, dim3((unsigned)ym_cdiv(max_items, 64), (unsigned)B), dim3(64 * FSL), 0, st, boxes_px, gt_xywh,
                       gt_iscrowd, counts, max_det, kinds, t, part, dbl);
    hipLaunchKernelGGL(k_coco_match_log_ragged, dim3((unsigned)B), dim3(MATCH_THREADS), 0, st, reinterpret_cast<const long long*>(ids), scores,
                       counts, max_det, boxes_px, kinds, t, (const int*)part, (const double*)dbl, gt_class, gt_iscrowd, gt_area, thresholds, T,
                       area_rng, num_classes, max_rank, log_score, log_class, log_rank, log_flags, reinterpret_cast<unsigned long long*>(npig),
                       class_rows);
    return ym_check_launch(what);
}
