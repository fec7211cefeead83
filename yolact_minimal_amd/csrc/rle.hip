// COCO run-length encoding of the binary detection masks on the device: what
// `pycocotools.mask.encode(np.asfortranarray(mask))` + `.decode('ascii')` produce in the reference's MakeJson.add_mask
// (utils/common_utils.py:88-96, eval.py:64-67).  Algorithm = cocoapi common/maskApi.c rleEncode + rleToString:
// runs over the COLUMN-major pixel order, alternating 0/1 starting with zeros (first count may be 0); each count (from the 4th
// on: its difference to the count two places back) is written as little-endian 5-bit groups + continuation bit, +48.
// One workgroup per mask, one thread per image column (row-major rows are read coalesced across the columns), two passes over
// the mask (count transitions, then place them) = 2*H*W*4 bytes of HBM reads; the result is a few hundred bytes per mask
// instead of a 1.2 MB dense D2H copy.  ym_rle_encode_packed is the same kernel reading bit-packed masks (BitSrc below).
#include "ym_common.h"

namespace {

constexpr int NT = 1024;
constexpr int MAXW = 4096;
constexpr int UNR = 16;

// exclusive prefix sum of one value per thread over the workgroup; returns the prefix, *total = sum of all
__device__ __forceinline__ int block_exscan(int v, int* total, int* s_wave /*[NT/64 + 1]*/) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    __syncthreads();
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int w = 0; w < NT / 64; ++w) { const int t = s_wave[w]; s_wave[w] = run; run += t; }
        s_wave[NT / 64] = run;
    }
    __syncthreads();
    *total = s_wave[NT / 64];
    return s_wave[wave] + inc - v;
}

// Where a pixel comes from: the dense fp32 mask, or the bit rows of include/yolact_hip.h "bit-packed instance masks".  The dense
// walk is a chain of H / UNR dependent load batches per pass (latency bound).  The 64 columns of a wave are ONE word per row, so
// the packed walk loads 64 ROWS at once (lane = row) and turns the 64 x 64 bit block around with 64 ballots (lane k keeps the
// ballot of bit k = its column's 64 rows): H / 64 loads per pass, and the transitions of 64 rows are one xor + popcount.
struct DenseSrc {
    typedef float T;
    static constexpr bool kBits = false;
    const float* m;
    int W;
    __device__ __forceinline__ DenseSrc(const void* base, int mask, int H, int W_) : m((const float*)base + (size_t)mask * H * W_), W(W_) {}
    __device__ __forceinline__ T load(int y, int x) const { return m[(size_t)y * W + x]; }
    __device__ __forceinline__ static bool on(T v, int) { return v != 0.f; }
};
struct BitSrc {
    typedef unsigned long long T;
    static constexpr bool kBits = true;
    const unsigned long long* m;
    int wq;
    __device__ __forceinline__ BitSrc(const void* base, int mask, int H, int W_)
        : m((const unsigned long long*)base + (size_t)mask * H * ((W_ + 63) >> 6)), wq((W_ + 63) >> 6) {}
    __device__ __forceinline__ T load(int y, int x) const { return m[(size_t)y * wq + (x >> 6)]; }
    __device__ __forceinline__ static bool on(T v, int x) { return (v >> (x & 63)) & 1ull; }
    // rows y0 .. y0+63 of column 64 j + lane as bits 0 .. 63 (rows past H: 0).  Every lane of the wave must call it.
    __device__ __forceinline__ unsigned long long column_block(int y0, int j, int H, int lane) const {
        const int y = y0 + lane;
        const unsigned long long w = y < H ? m[(size_t)y * wq + j] : 0ull;
        const unsigned lo = (unsigned)w, hi = (unsigned)(w >> 32);
        unsigned long long mine = 0ull;
#pragma unroll
        for (int k = 0; k < 64; ++k) {
            const unsigned long long b = __ballot(((k < 32 ? lo : hi) >> (k & 31)) & 1u);
            mine = lane == k ? b : mine;
        }
        return mine;
    }
};

// transitions inside a block of nv <= 64 rows of one column (bit r set: row r differs from the row before it; `prev` = the pixel
// before row 0); updates `prev` to the block's last row
__device__ __forceinline__ unsigned long long block_transitions(unsigned long long col, int nv, bool& prev) {
    unsigned long long t = col ^ ((col << 1) | (prev ? 1ull : 0ull));
    if (nv < 64) t &= (1ull << nv) - 1ull;
    prev = (col >> (nv - 1)) & 1ull;
    return t;
}

// One mask by one workgroup of NT threads (every thread calls it): maskApi.c rleEncode + rleToString.  `pos` [cap] receives the
// positions of the transitions, `out` [cap_str] the string.  Returns the number of runs R; *len = the string's bytes, or -1 when
// R > cap or the string is longer than cap_str ("buffers too small": nothing is written past either).  Both values are uniform.
// kCounts: the run lengths are also an OUTPUT (`cnt` [cap], ym_rle_encode's `counts`) and the string reads them back; without it
// `cnt` is unused and a count is the difference of two positions (cnt[j] - cnt[j-2] follows from four).
template <class Src, bool kCounts>
__device__ __forceinline__ int rle_encode_mask(const Src& m, int H, int W, uint32_t* __restrict__ pos, uint32_t* __restrict__ cnt, int cap,
                                               uint8_t* __restrict__ out, int cap_str, int* s_col /*[MAXW]*/, int* s_wave /*[NT/64 + 1]*/,
                                               int* len_out) {
    typedef typename Src::T Px;
    const int tid = threadIdx.x;
    const unsigned P = (unsigned)H * (unsigned)W;

    // pass 1: transitions per column (the pixel before (0, x) in column-major order is (H-1, x-1); before (0,0): background)
    if constexpr (Src::kBits) {
        const int lane = tid & 63;
        for (int xb = tid - lane; xb < W; xb += NT) {            // (wave-uniform: the block transpose needs all 64 lanes)
            const int x = xb + lane;
            bool prev = x > 0 && x < W && Src::on(m.load(H - 1, x - 1), x - 1);
            int c = 0;
            for (int y0 = 0; y0 < H; y0 += 64) {
                const unsigned long long col = m.column_block(y0, xb >> 6, H, lane);
                c += __popcll(block_transitions(col, min(64, H - y0), prev));
            }
            if (x < W) s_col[x] = c;
        }
    } else
    for (int x = tid; x < W; x += NT) {
        bool prev = x > 0 && Src::on(m.load(H - 1, x - 1), x - 1);
        int c = 0, y = 0;
        for (; y + UNR <= H; y += UNR) {          // UNR independent row loads in flight per lane (the walk is latency bound)
            Px v[UNR];
#pragma unroll
            for (int u = 0; u < UNR; ++u) v[u] = m.load(y + u, x);
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const bool cur = Src::on(v[u], x);
                c += cur != prev;
                prev = cur;
            }
        }
        for (; y < H; ++y) {
            const bool cur = Src::on(m.load(y, x), x);
            c += cur != prev;
            prev = cur;
        }
        s_col[x] = c;
    }
    __syncthreads();
    // exclusive scan over the columns (chunks of NT with a running carry)
    int carry = 0;
    for (int x0 = 0; x0 < W; x0 += NT) {
        const int x = x0 + tid;
        const int v = x < W ? s_col[x] : 0;
        int total;
        const int pre = block_exscan(v, &total, s_wave);
        if (x < W) s_col[x] = carry + pre;
        carry += total;
        __syncthreads();
    }
    const int T = carry;                 // transitions; runs = T + 1 (the last run ends at P)
    const int R = T + 1;
    if (R > cap) {                       // caller's buffers are too small: report the size needed, encode nothing
        *len_out = -1;
        return R;
    }
    // pass 2: positions of the transitions, in column-major order
    if constexpr (Src::kBits) {
        const int lane = tid & 63;
        for (int xb = tid - lane; xb < W; xb += NT) {
            const int x = xb + lane;
            bool prev = x > 0 && x < W && Src::on(m.load(H - 1, x - 1), x - 1);
            int o = x < W ? s_col[x] : 0;
            for (int y0 = 0; y0 < H; y0 += 64) {
                const unsigned long long col = m.column_block(y0, xb >> 6, H, lane);
                unsigned long long t = block_transitions(col, min(64, H - y0), prev);
                if (x >= W) t = 0ull;
                while (t) {
                    pos[o++] = (unsigned)x * (unsigned)H + (unsigned)(y0 + __builtin_ctzll(t));
                    t &= t - 1ull;
                }
            }
        }
    } else
    for (int x = tid; x < W; x += NT) {
        bool prev = x > 0 && Src::on(m.load(H - 1, x - 1), x - 1);
        int o = s_col[x], y = 0;
        for (; y + UNR <= H; y += UNR) {
            Px v[UNR];
#pragma unroll
            for (int u = 0; u < UNR; ++u) v[u] = m.load(y + u, x);
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const bool cur = Src::on(v[u], x);
                if (cur != prev) pos[o++] = (unsigned)x * (unsigned)H + (unsigned)(y + u);
                prev = cur;
            }
        }
        for (; y < H; ++y) {
            const bool cur = Src::on(m.load(y, x), x);
            if (cur != prev) pos[o++] = (unsigned)x * (unsigned)H + (unsigned)y;
            prev = cur;
        }
    }
    __threadfence_block();
    __syncthreads();
    // counts[j] = pos[j] - pos[j-1]  (pos[-1] = 0, pos[T] = P)
    const auto count_at = [&](int j) -> unsigned { return (j < T ? pos[j] : P) - (j > 0 ? pos[j - 1] : 0u); };
    if constexpr (kCounts) {
        for (int j = tid; j < R; j += NT) cnt[j] = count_at(j);
        __threadfence_block();
        __syncthreads();
    }
    // rleToString: x = cnts[j] (j > 2: minus cnts[j-2]); 5 bits per char, bit 5 = "more", sign-aware termination, +48
    int scarry = 0;
    for (int j0 = 0; j0 < R; j0 += NT) {
        const int j = j0 + tid;
        long long x = 0;
        int len = 0;
        uint8_t ch[8];
        if (j < R) {
            if constexpr (kCounts) {
                x = (long long)cnt[j];
                if (j > 2) x -= (long long)cnt[j - 2];
            } else {
                x = (long long)count_at(j);
                if (j > 2) x -= (long long)count_at(j - 2);
            }
            bool more = true;
            while (more) {
                int c = (int)(x & 0x1f);
                x >>= 5;
                more = (c & 0x10) ? x != -1 : x != 0;
                if (more) c |= 0x20;
                ch[len++] = (uint8_t)(c + 48);
            }
        }
        int total;
        const int pre = block_exscan(len, &total, s_wave);
        const int o = scarry + pre;
        if (o + len <= cap_str)
            for (int k = 0; k < len; ++k) out[o + k] = ch[k];
        scarry += total;
        __syncthreads();
    }
    *len_out = scarry <= cap_str ? scarry : -1;
    return R;
}

template <class Src>
__global__ __launch_bounds__(NT) void k_rle_encode(const void* __restrict__ masks, int H, int W, uint32_t* __restrict__ pos_ws,
                                                   uint32_t* __restrict__ counts, int cap, int32_t* __restrict__ nruns,
                                                   uint8_t* __restrict__ str, int cap_str, int32_t* __restrict__ str_len) {
    __shared__ int s_col[MAXW];
    __shared__ int s_wave[NT / 64 + 1];
    const Src m(masks, blockIdx.x, H, W);
    int len;
    const int R = rle_encode_mask<Src, true>(m, H, W, pos_ws + (size_t)blockIdx.x * cap, counts + (size_t)blockIdx.x * cap, cap,
                                             str + (size_t)blockIdx.x * cap_str, cap_str, s_col, s_wave, &len);
    if (threadIdx.x == 0) {
        nruns[blockIdx.x] = R;
        str_len[blockIdx.x] = len;
    }
}

// ---- the detection rows of a whole request (include/yolact_hip.h "ym_rle_encode_ragged_packed") -------------------------------------
// What the encode launch knows about its images, BY VALUE in the kernel arguments (like CocoRaggedTable of coco_eval.hip).
struct RleRaggedTable {
    int img_h[YM_RAGGED_MAX_IMAGES], img_w[YM_RAGGED_MAX_IMAGES];
    long long off[YM_RAGGED_MAX_IMAGES];         // words from det_bits to the image's block
    unsigned live;                               // bit b: image b is no padding
};

constexpr int RLE_SLAB_PER_RUN = 4;              // bytes of a mask's string slab per run of cap_runs (rle_encode's cap_str)
constexpr int GATHER_THREADS = 256;

// grid: B * max_det, workgroup g = row g % max_det of image g / max_det.  A row that is no record writes state 0 and leaves before the
// first barrier without touching its mask words; a record's string goes to its slab, its length and run count to the record.
__global__ __launch_bounds__(NT) void k_rle_encode_ragged(const long long* __restrict__ ids, const float* __restrict__ scores,
                                                          const int* __restrict__ boxes_px, const int* __restrict__ counts, int max_det,
                                                          const unsigned long long* __restrict__ det_bits, const RleRaggedTable t, int cap,
                                                          uint32_t* __restrict__ pos_ws, uint8_t* __restrict__ slabs,
                                                          ym_rle_record* __restrict__ records) {
    __shared__ int s_col[MAXW];
    __shared__ int s_wave[NT / 64 + 1];
    const int g = blockIdx.x, b = g / max_det, r = g - b * max_det;
    ym_rle_record rec = {};
    bool is_record = ((t.live >> b) & 1u) != 0 && r < counts[b];
    if (is_record) {
        const int* pb = boxes_px + (size_t)g * 4;
        rec.class_id = (int32_t)ids[g];
        rec.score = scores[g];
        for (int k = 0; k < 4; ++k) rec.box[k] = pb[k];
        is_record = ((long long)pb[3] - pb[1]) * ((long long)pb[2] - pb[0]) > 0;     // eval.py:65
    }
    if (!is_record) {                                        // (uniform: a function of the block index and of counts[b] alone)
        if (threadIdx.x == 0) records[g] = ym_rle_record{};
        return;
    }
    const int H = t.img_h[b], W = t.img_w[b];
    const BitSrc m(det_bits + t.off[b], r, H, W);
    const int cap_str = cap * RLE_SLAB_PER_RUN;
    int len;
    rec.nruns = rle_encode_mask<BitSrc, false>(m, H, W, pos_ws + (size_t)g * cap, nullptr, cap, slabs + (size_t)g * cap_str, cap_str, s_col,
                                               s_wave, &len);
    rec.state = len >= 0 ? 1 : 2;
    rec.str_len = len >= 0 ? len : 0;
    if (threadIdx.x == 0) records[g] = rec;
}

// one workgroup: str_off = the exclusive sum of str_len over the rows in (image, row) order, and the header.  Integer sums in a
// fixed order: the layout is a function of the lengths alone.
__global__ __launch_bounds__(NT) void k_rle_scan_records(ym_rle_record* __restrict__ records, int rows, int32_t* __restrict__ header) {
    __shared__ int s_wave[NT / 64 + 1];
    int bytes = 0, recs = 0, over = 0;
    for (int r0 = 0; r0 < rows; r0 += NT) {
        const int i = r0 + threadIdx.x;
        const int state = i < rows ? records[i].state : 0;
        const int len = state == 1 ? records[i].str_len : 0;
        int total;
        const int pre = block_exscan(len, &total, s_wave);
        if (i < rows) records[i].str_off = bytes + pre;
        bytes += total;
        block_exscan(state != 0, &total, s_wave);
        recs += total;
        block_exscan(state == 2, &total, s_wave);
        over += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) { header[0] = bytes; header[1] = recs; header[2] = over; header[3] = 0; }
}

// grid: B * max_det.  The string of an encoded row moves from its slab to its place in the request's compact buffer.
__global__ __launch_bounds__(GATHER_THREADS) void k_rle_gather_strings(const ym_rle_record* __restrict__ records,
                                                                       const uint8_t* __restrict__ slabs, int slab,
                                                                       uint8_t* __restrict__ strings, long long strings_bytes) {
    const ym_rle_record rec = records[blockIdx.x];
    if (rec.state != 1 || rec.str_len > slab || (long long)rec.str_off + rec.str_len > strings_bytes) return;
    const uint8_t* src = slabs + (size_t)blockIdx.x * slab;
    uint8_t* dst = strings + rec.str_off;
    for (int k = threadIdx.x; k < rec.str_len; k += GATHER_THREADS) dst[k] = src[k];
}

}  // namespace

template <class Src>
static int rle_encode_launch(const char* what, const void* masks, int n, int H, int W, uint32_t* counts, int cap_runs, int32_t* nruns,
                             uint8_t* str, int cap_str, int32_t* str_len, void* workspace, size_t workspace_bytes, ym_stream_t s) {
    YM_REQUIRE(masks && counts && nruns && str && str_len && workspace, "%s: null pointer", what);
    YM_REQUIRE(n > 0 && H > 0 && W > 0 && W <= MAXW && cap_runs > 0 && cap_str > 0, "%s: need 0 < W <= %d", what, MAXW);
    YM_REQUIRE((long long)H * W < (1ll << 31), "%s: mask too large", what);
    if (workspace_bytes < (size_t)n * cap_runs * 4) { ym_set_error("%s: workspace < n*cap_runs*4 bytes", what); return YM_ENOSPC; }
    hipLaunchKernelGGL(k_rle_encode<Src>, dim3(n), dim3(NT), 0, (hipStream_t)s, masks, H, W, (uint32_t*)workspace, counts, cap_runs, nruns,
                       str, cap_str, str_len);
    return ym_check_launch(what);
}

extern "C" int ym_rle_encode(const float* masks, int n, int H, int W, uint32_t* counts, int cap_runs, int32_t* nruns, uint8_t* str,
                             int cap_str, int32_t* str_len, void* workspace, size_t workspace_bytes, ym_stream_t s) {
    return rle_encode_launch<DenseSrc>("rle_encode", masks, n, H, W, counts, cap_runs, nruns, str, cap_str, str_len, workspace,
                                       workspace_bytes, s);
}

extern "C" int ym_rle_encode_packed(const uint64_t* bits, int n, int H, int W, uint32_t* counts, int cap_runs, int32_t* nruns, uint8_t* str,
                                    int cap_str, int32_t* str_len, void* workspace, size_t workspace_bytes, ym_stream_t s) {
    return rle_encode_launch<BitSrc>("rle_encode_packed", bits, n, H, W, counts, cap_runs, nruns, str, cap_str, str_len, workspace,
                                     workspace_bytes, s);
}

// ---- ym_rle_encode_ragged_packed: validation and layout are host code that runs before the first HIP call ------------------------------
// The checks of the sizes, shared with the workspace query.  Workspace: positions [rows][cap_runs] uint32, then the string slabs
// [rows][slab = 4 * cap_runs] bytes; rows = B * max_det.
static int rle_ragged_check(const char* what, const ym_ragged_image* det_blocks, int B, int max_det, int cap_runs, size_t* rows,
                            size_t* slab) {
    YM_REQUIRE(B >= 1 && B <= YM_RAGGED_MAX_IMAGES, "%s: 1 .. %d images per call, got %d", what, YM_RAGGED_MAX_IMAGES, B);
    YM_REQUIRE(max_det >= 1 && cap_runs >= 1, "%s: need max_det >= 1 and cap_runs >= 1, got %d and %d", what, max_det, cap_runs);
    YM_REQUIRE(det_blocks, "%s: null image table", what);
    for (int b = 0; b < B; ++b) {
        const ym_ragged_image& im = det_blocks[b];
        YM_REQUIRE(im.img_h > 0 && im.img_w > 0 && im.img_w <= MAXW, "%s: image %d is %d x %d, need 0 < W <= %d", what, b, im.img_h, im.img_w,
                   MAXW);
        YM_REQUIRE((long long)im.img_h * im.img_w < (1ll << 31), "%s: image %d: mask too large", what, b);
    }
    // (a reader of whole words: the offsets count words, so every block is 8-byte aligned when det_bits is -- esz = the alignment
    //  unit makes the shared check's 256-byte rule, which the writers need, vacuous; sizes, offsets >= 0 and overlaps are checked)
    const int rc = ym_check_ragged_table(what, det_blocks, B, YM_RAGGED_ALIGN_BYTES, [&](const ym_ragged_image& im) {
        return (int64_t)max_det * im.img_h * (int64_t)ym_mask_row(true, im.img_w);
    });
    if (rc != YM_OK) return rc;
    const long long n = (long long)B * max_det, sl = (long long)cap_runs * RLE_SLAB_PER_RUN;
    YM_REQUIRE(n * sl < (1ll << 31), "%s: B * max_det * slab = %d * %d * %lld bytes: need < 2^31", what, B, max_det, sl);
    *rows = (size_t)n;
    *slab = (size_t)sl;
    return YM_OK;
}

extern "C" size_t ym_sizeof_rle_record(void) { return sizeof(ym_rle_record); }

extern "C" size_t ym_rle_encode_ragged_workspace_bytes(const ym_ragged_image* det_blocks, int B, int max_det, int cap_runs) {
    size_t rows = 0, slab = 0;
    if (rle_ragged_check("rle_encode_ragged_workspace_bytes", det_blocks, B, max_det, cap_runs, &rows, &slab) != YM_OK) return 0;
    return rows * (size_t)cap_runs * sizeof(uint32_t) + rows * slab;
}

extern "C" int ym_rle_encode_ragged_packed(const int64_t* ids, const float* scores, const int32_t* boxes_px, const int32_t* counts, int B,
                                           int max_det, const uint64_t* det_bits, const ym_ragged_image* det_blocks, const uint8_t* live,
                                           int cap_runs, ym_rle_record* records, uint8_t* strings, int64_t strings_bytes, int32_t* header,
                                           void* workspace, size_t workspace_bytes, ym_stream_t s) {
    const char* what = "rle_encode_ragged_packed";
    static_assert(sizeof(ym_rle_record) == 40, "ym_rle_record is 40 bytes");
    YM_REQUIRE(ids && scores && boxes_px && counts && det_bits && det_blocks && live && records && strings && header && workspace,
               "%s: null pointer", what);
    YM_REQUIRE(((uintptr_t)det_bits & 7) == 0 && ((uintptr_t)records & 3) == 0 && ((uintptr_t)header & 3) == 0 && ((uintptr_t)workspace & 3) == 0,
               "%s: det_bits must be 8-byte aligned; records, header and workspace 4-byte aligned", what);
    size_t rows = 0, slab = 0;
    const int rc = rle_ragged_check(what, det_blocks, B, max_det, cap_runs, &rows, &slab);
    if (rc != YM_OK) return rc;
    const size_t need = rows * (size_t)cap_runs * sizeof(uint32_t) + rows * slab;
    if (workspace_bytes < need) { ym_set_error("%s: workspace of %zu bytes, %zu needed", what, workspace_bytes, need); return YM_ENOSPC; }
    if (strings_bytes < (int64_t)(rows * slab)) {
        ym_set_error("%s: strings of %lld bytes, the worst case B * max_det * 4 * cap_runs = %zu is needed", what, (long long)strings_bytes,
                     rows * slab);
        return YM_ENOSPC;
    }
    RleRaggedTable t = {};
    for (int b = 0; b < B; ++b) {
        t.img_h[b] = det_blocks[b].img_h;
        t.img_w[b] = det_blocks[b].img_w;
        t.off[b] = det_blocks[b].offset;
        if (live[b]) t.live |= 1u << b;
    }
    hipStream_t st = (hipStream_t)s;
    uint32_t* pos_ws = (uint32_t*)workspace;
    uint8_t* slabs = (uint8_t*)(pos_ws + rows * (size_t)cap_runs);
    hipLaunchKernelGGL(k_rle_encode_ragged, dim3((unsigned)rows), dim3(NT), 0, st, reinterpret_cast<const long long*>(ids), scores, boxes_px,
                       counts, max_det, reinterpret_cast<const unsigned long long*>(det_bits), t, cap_runs, pos_ws, slabs, records);
    hipLaunchKernelGGL(k_rle_scan_records, dim3(1), dim3(NT), 0, st, records, (int)rows, header);
    hipLaunchKernelGGL(k_rle_gather_strings, dim3((unsigned)rows), dim3(GATHER_THREADS), 0, st, records, slabs, (int)slab, strings,
                       (long long)strings_bytes);
    return ym_check_launch(what);
}
