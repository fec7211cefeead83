// The pair loop on bit rows that every packed mask IoU of the library runs (metrics.hip: k_mask_inter_packed, k_eval_inter_ragged;
// coco_eval.hip: k_coco_inter_ragged).  Include it inside the file's anonymous namespace, after ym_common.h.
#pragma once

constexpr int MAXR = 128;              // rows of each side held in LDS at once

// Both operands already are bit rows (include/yolact_hip.h "bit-packed instance masks": [.][Pw] words, Pw = H * ceil(W / 64), pad
// bits zero): the ballot pass of k_mask_inter disappears, words go from HBM straight into the same LDS arrays and the same pair
// loop.  PWORDS words per chunk: 480x640 masks = 4800 words = 240 chunks, one round over the 256 CUs.  Same partial-count layout,
// same finalize kernel, no global atomics.
constexpr int PWORDS = 20;
// One workgroup's share: chunk `chunk` of the rows, gt group `gy`.  `n` rows of A are loaded and paired (the ragged stages pass an
// image's count here); `nstride` >= n is the row count the partial arrays are laid out for.  The ONE pair loop on bit rows.  The
// workgroup has 512 threads.  g = 0 is allowed: the rows of A are still counted into area_a.
__device__ __forceinline__ void inter_packed_chunk(const unsigned long long* __restrict__ A, int n, int nstride,
                                                   const unsigned long long* __restrict__ Bm, int g, long long Pw, int chunk, int gy,
                                                   int* __restrict__ inter, int* __restrict__ area_a, int* __restrict__ area_b) {
    __shared__ unsigned long long sa[MAXR][PWORDS + 1];
    __shared__ unsigned long long sb[MAXR][PWORDS + 1];
    const int tid = threadIdx.x;
    const long long w0 = (long long)chunk * PWORDS;
    const int nwd = (int)min((long long)PWORDS, Pw - w0);
    const int g0 = gy * MAXR, gn = min(MAXR, g - g0);
    inter += (size_t)chunk * nstride * g;
    area_a += (size_t)chunk * nstride;
    area_b += (size_t)chunk * g;
    for (int a0 = 0; a0 < n; a0 += MAXR) {
        const int an = min(MAXR, n - a0);
        __syncthreads();
        const int rows = an + (a0 == 0 ? gn : 0);          // (the gt rows stay in LDS for the later passes over A)
        for (int idx = tid; idx < rows * PWORDS; idx += 512) {
            const int rr = idx / PWORDS, q = idx - rr * PWORDS;
            const bool is_a = rr < an;
            const unsigned long long* row = is_a ? A + (size_t)(a0 + rr) * Pw : Bm + (size_t)(g0 + rr - an) * Pw;
            const unsigned long long v = q < nwd ? __builtin_nontemporal_load(row + w0 + q) : 0ull;
            (is_a ? sa[rr] : sb[rr - an])[q] = v;
        }
        __syncthreads();
        for (int rr = tid; rr < rows; rr += 512) {
            const bool is_a = rr < an;
            const unsigned long long* w = is_a ? sa[rr] : sb[rr - an];
            int c = 0;
#pragma unroll
            for (int q = 0; q < PWORDS; ++q) c += __popcll(w[q]);
            if (is_a) { if (gy == 0) area_a[a0 + rr] = c; }
            else area_b[g0 + rr - an] = c;
        }
        for (int pr = tid; pr < an * gn; pr += 512) {
            const int i = pr / gn, j = pr - i * gn;
            int c = 0;
#pragma unroll
            for (int w = 0; w < PWORDS; ++w) c += __popcll(sa[i][w] & sb[j][w]);
            inter[(size_t)(a0 + i) * g + g0 + j] = c;
        }
    }
}
