// Launch planner of the fused convolution: everything ym_conv2d_fwd decides before it launches (kernel family and variant, tile,
// K split, tail, epilogue, BatchNorm sums) is decided HERE, from the descriptor and the workspace alignment alone, and read back by
// the launch, the five queries and ym_conv2d_effective_plan (conv_mfma.hip).  Host only: this file holds no kernel and needs no
// device (the CU count falls back to 256).
#include <stdlib.h>
#include "conv_common.h"

using namespace ymk;

int ym_cu_count() {
    static int cus = 0;
    if (cus == 0) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cus = n;
    }
    return cus;
}

namespace {

// Can the output be written by the vectorised row-major epilogue (one plain NHWC tensor, 16-byte aligned operands)?  The K-slice
// exchange of the fused split-K finish / tail split lives in that epilogue.
bool vec_epilogue(const ym_conv_desc* d) {
    const ym_conv_seg& g = d->seg[0];
    const bool aligned = (((uintptr_t)g.out | (uintptr_t)d->residual | (uintptr_t)d->scale | (uintptr_t)d->shift) & 15) == 0;
    const bool rows_in_order = d->nlevels ? g.batch_stride == 0      // pyramid: the plain output keeps the input's row order
                                          : g.batch_stride == (int64_t)d->Ho * d->Wo * d->Cout;
    return d->nseg == 1 && g.n_begin == 0 && g.n_end == d->Cout && g.pitch == d->Cout && rows_in_order && d->Cout % 4 == 0 && aligned;
}

// Validation, tile, K split and tail; of the kernel family what the tile depends on (wave kernels, weight-stationary or not).
int plan_tiles(const ym_conv_desc* d, Plan* pl, bool allow_cls) {
    YM_REQUIRE(d && d->in && d->weight, "conv: null descriptor / pointer");
    YM_REQUIRE(d->B > 0 && d->H > 0 && d->W > 0 && d->Cout > 0, "conv: bad shape");
    YM_REQUIRE(d->Cin == 4 || d->Cin % 32 == 0, "conv: Cin must be 4 (stem) or a multiple of 32, got %d", d->Cin);
    YM_REQUIRE(d->k_pad % BK == 0 && d->k_pad >= d->KH * d->KW * d->Cin, "conv: k_pad %d invalid", d->k_pad);
    if (d->transposed) {
        YM_REQUIRE(d->stride == 1 || d->stride == 2, "conv(dgrad): stride must be 1 or 2");
        YM_REQUIRE(d->Cin % 32 == 0 && d->kwaves == 0, "conv(dgrad): dy channels must be padded to a multiple of 32; workgroup kernel only");
        YM_REQUIRE(d->H == (d->Ho + 2 * d->pad - d->KH) / d->stride + 1 && d->W == (d->Wo + 2 * d->pad - d->KW) / d->stride + 1,
                   "conv(dgrad): H/W (dy) inconsistent with Ho/Wo (dx)");
    } else if (d->nlevels == 0) {
        YM_REQUIRE(d->Ho == (d->H + 2 * d->pad - d->KH) / d->stride + 1 && d->Wo == (d->W + 2 * d->pad - d->KW) / d->stride + 1,
                   "conv: Ho/Wo inconsistent with H/W/K/stride/pad");
    }
    long long M_levels = 0;
    if (d->nlevels != 0) {
        YM_REQUIRE(d->nlevels >= 1 && d->nlevels <= 5, "conv: nlevels must be 0..5");
        YM_REQUIRE(!d->transposed && d->kwaves == 0 && d->Cin % 32 == 0 && d->stride == 1 && d->KH == d->KW && (d->KH & 1) &&
                   d->pad == d->KH / 2, "conv(pyramid): stride 1, odd square filter, pad = K/2, Cin %% 32 == 0, workgroup kernel");
        for (int l = 0; l < d->nlevels; ++l) {
            YM_REQUIRE(d->level_h[l] > 0 && d->level_w[l] > 0, "conv(pyramid): bad level %d", l);
            M_levels += (long long)d->B * d->level_h[l] * d->level_w[l];
        }
    }
    YM_REQUIRE(d->nseg >= 1 && d->nseg <= 3, "conv: nseg must be 1..3");
    for (int s = 0; s < d->nseg; ++s)
        YM_REQUIRE(d->seg[s].out && d->seg[s].n_end > d->seg[s].n_begin && d->seg[s].n_end <= d->Cout,
                   "conv: bad segment %d", s);
    const long long M = d->nlevels ? M_levels : (long long)d->B * d->Ho * d->Wo;
    YM_REQUIRE(M * (long long)d->Cout < (1ll << 31) && (d->nlevels ? M : (long long)d->B * d->H * d->W) * d->Cin < (1ll << 31) * 1ll,
               "conv: tensor too large for 32-bit indexing");
    pl->M = (int)M;
    pl->M_pix = (int)M;
    pl->cls = 0;
    pl->nkt = d->k_pad / BK;
    pl->tail_tiles = 0; pl->tail_split = 0; pl->tail_ktps = 0;
    int bm = d->tile_m, bn = d->tile_n;
    if (bm == 0 || bn == 0) {
        // largest tile that still gives every CU at least ~2 workgroups
        const int cand[3][2] = {{128, 128}, {128, 64}, {64, 64}};
        bm = 64; bn = 64;
        for (int c = 0; c < 3; ++c) {
            const long long wgs = (long long)ym_cdiv(pl->M, cand[c][0]) * ym_cdiv(d->Cout, cand[c][1]);
            if (wgs >= 512) { bm = cand[c][0]; bn = cand[c][1]; break; }
        }
        if (d->Cin == 4) { bm = 128; bn = 64; }
    }
    pl->family = CONV_IGEMM;
    if (d->stages >= 52 && d->stages <= 54) {
        // weight-stationary 1x1 kernel (conv_ws.hip): a plain GEMM with the filter slice resident in LDS.  What it does not cover
        // (a filter with taps, a stride, BatchNorm-backward sums, too much filter for the LDS) runs as a 64x64 direct-to-LDS launch.
        const bool shape_ok = (bm == 64 && bn == 256) || (bm == 128 && bn == 128) || (bm == 256 && bn == 64);
        const int act = d->seg[0].act;
        const bool ok = shape_ok && d->KH == 1 && d->KW == 1 && d->stride == 1 && d->pad == 0 && d->Cin % 32 == 0 && d->k_pad == d->Cin &&
                        d->nlevels == 0 && d->kwaves == 0 && d->mma == 0 && d->bnb_y == nullptr && vec_epilogue(d) &&
                        (act == YM_ACT_NONE || act == YM_ACT_RELU) && (size_t)bn * d->Cin * 4 <= (64u << 10) &&
                        ym_conv_ws_lds_bytes(bm, bn, pl->nkt, d->stages - 50) <= (160u << 10) && (unsigned long long)M * d->Cout * 4ull < 0xFFFFFFF0ull &&
                        (unsigned long long)M * d->Cin * 4ull < 0xFFFFFFF0ull;      // (conv_ws.hip forms A and C offsets in 32 bits)
        if (ok) {
            pl->bm = bm; pl->bn = bn; pl->tiles_m = ym_cdiv(pl->M, bm); pl->tiles_n = ym_cdiv(d->Cout, bn);
            pl->ksplit = 1; pl->kt_per_split = pl->nkt;
            pl->family = CONV_WS; pl->ring = d->stages - 50;
            return YM_OK;
        }
        bm = 64; bn = 64;
    }
    if (d->kwaves > 0) {
        YM_REQUIRE(d->Cin != 4, "conv: the wave-private kernel does not support the stem (Cin == 4)");
        YM_REQUIRE((bm == 32 || bm == 64) && (bn == 32 || bn == 64), "conv(wave): tile must be 32/64, got %dx%d", bm, bn);
        const bool dma = d->stages >= 22 && d->stages <= 24;
        pl->family = dma ? CONV_WAVE_DMA : CONV_WAVE;
        pl->ring = dma ? d->stages - 20 : 0;
        pl->bm = bm; pl->bn = bn; pl->tiles_m = ym_cdiv(pl->M, bm); pl->tiles_n = ym_cdiv(d->Cout, bn);
        pl->ksplit = 1; pl->kt_per_split = pl->nkt;
        // tail split of the wave-private DMA-ring kernel (conv_wave.hip): 32x32 tile with four K waves, plain NHWC output, counters
        if (d->tail_tiles > 0 && d->tail_ksplit > 1 && dma && bm == 32 && bn == 32 && d->kwaves == 4 &&
            (d->grid_wgs == 0 || d->grid_wgs == 4) && d->tile_counters && vec_epilogue(d)) {
            YM_REQUIRE(d->tail_tiles <= pl->tiles_m * pl->tiles_n, "conv(wave): tail_tiles %d > %d output tiles", d->tail_tiles, pl->tiles_m * pl->tiles_n);
            int ts = d->tail_ksplit > pl->nkt ? pl->nkt : d->tail_ksplit;
            if (ts > 8) ts = 8;                                    // (the last arriver gathers up to 8 slices at once)
            pl->tail_ktps = ym_cdiv(pl->nkt, ts);
            pl->tail_split = ym_cdiv(pl->nkt, pl->tail_ktps);
            pl->tail_tiles = pl->tail_split > 1 ? d->tail_tiles : 0;
        }
        return YM_OK;
    }
    YM_REQUIRE((bm == 128 || bm == 64) && (bn == 128 || bn == 64), "conv: tile must be 64/128");
    YM_REQUIRE(d->Cin != 4 || (bm == 128 && bn == 64), "conv: stem mode supports the 128x64 tile only");
    pl->bm = bm; pl->bn = bn;
    {
        // Stride-2 data gradient: rows ordered by output-pixel parity class, every class padded to whole M tiles, and only the
        // class's filter taps in its K range (ConvP::cls).  YM_DGRAD_CLASSES=0: the gather over all taps of rounds 1-3 (A/B).
        static int on = -1;
        if (on < 0) { const char* e = getenv("YM_DGRAD_CLASSES"); on = e ? atoi(e) : 1; }
        if (on && allow_cls && d->transposed && d->stride == 2 && d->nlevels == 0 && vec_epilogue(d)) {
            int t0 = 0, nkt_max = 0, nt_max = 0;
            for (int c = 0; c < 4; ++c) {
                const int ph = c >> 1, pw = c & 1;
                const int hc = (d->Ho - ph + 1) / 2, wc = (d->Wo - pw + 1) / 2;          // dx rows / columns of this parity
                const int kh0 = (ph + d->pad) & 1, kw0 = (pw + d->pad) & 1;
                const int nkh = kh0 < d->KH ? (d->KH - kh0 + 1) / 2 : 0, nkw = kw0 < d->KW ? (d->KW - kw0 + 1) / 2 : 0;
                pl->cls_tile0[c] = t0;
                pl->cls_rows[c] = d->B * hc * wc;
                pl->cls_w[c] = wc > 0 ? wc : 1;
                pl->cls_hw[c] = hc * wc > 0 ? hc * wc : 1;
                pl->cls_kh0[c] = kh0; pl->cls_kw0[c] = kw0; pl->cls_nkw[c] = nkw > 0 ? nkw : 1;
                pl->cls_nkt[c] = nkh * nkw * (d->Cin / BK);
                if (pl->cls_nkt[c] > nkt_max) nkt_max = pl->cls_nkt[c];
                t0 += ym_cdiv(pl->cls_rows[c], bm);
                if (ym_cdiv(pl->cls_rows[c], bm) > nt_max) nt_max = ym_cdiv(pl->cls_rows[c], bm);
            }
            pl->cls_tile0[4] = t0;
            pl->cls = 1;
            pl->M = 4 * nt_max * bm;                       // M tile t belongs to class t & 3 (its tile t >> 2): see the kernel
            pl->nkt = nkt_max > 0 ? nkt_max : 1;
        }
    }
    pl->tiles_m = ym_cdiv(pl->M, bm);
    pl->tiles_n = ym_cdiv(d->Cout, bn);
    int ks = d->ksplit;
    if (ks <= 0) {
        ks = 1;
        const int wgs = pl->tiles_m * pl->tiles_n;
        if (wgs < 256) {
            ks = ym_cdiv(512, wgs);
            const int max_ks = pl->nkt / 4 > 0 ? pl->nkt / 4 : 1;   // keep >= 4 K tiles per slice
            if (ks > max_ks) ks = max_ks;
            if (ks > 16) ks = 16;
        }
    }
    if (ks > pl->nkt) ks = pl->nkt;
    if (ks < 1) ks = 1;
    pl->kt_per_split = ym_cdiv(pl->nkt, ks);
    pl->ksplit = ym_cdiv(pl->nkt, pl->kt_per_split);
    if (d->tail_tiles > 0 && d->tail_ksplit > 1 && vec_epilogue(d)) {   // (a segmented / unaligned output ignores the tail knobs)
        YM_REQUIRE(d->tile_counters && pl->ksplit == 1 && d->Cin != 4, "conv: tail_tiles needs tile_counters, ksplit <= 1 and Cin %% 32 == 0");
        YM_REQUIRE(d->tail_tiles <= pl->tiles_m * pl->tiles_n, "conv: tail_tiles %d > %d output tiles", d->tail_tiles, pl->tiles_m * pl->tiles_n);
        int ts = d->tail_ksplit > pl->nkt ? pl->nkt : d->tail_ksplit;
        pl->tail_ktps = ym_cdiv(pl->nkt, ts);
        pl->tail_split = ym_cdiv(pl->nkt, pl->tail_ktps);
        pl->tail_tiles = pl->tail_split > 1 ? d->tail_tiles : 0;
    }
    // The class-ordered rows exist only inside the launch: K slices of such a plan must meet in the fused finish (arrival counters),
    // which maps a tile row back to its dx pixel.  `conv_splitk_reduce` reads the slabs as plain [M][Cout] rows, so without counters
    // (none given, or a workspace past the 32-bit exchange offsets) the plan falls back to the gather over all taps.
    if (pl->cls && pl->slots() > 1 && (!d->tile_counters || pl->ws_bytes(d->Cout) >= 0xFFFFFFF0ull)) return plan_tiles(d, pl, false);
    return YM_OK;
}

// The igemm-family kernel behind `stages` (after the two fall-back rules): the persistent walker, or the conv_igemm_f32 variant.
void plan_variant(const ym_conv_desc* d, Plan* pl) {
    const bool t64 = pl->bm == 64 && pl->bn == 64;
    const int act = d->seg[0].act;
    int stages = d->stages;
    if (stages >= 52 && stages <= 54) stages = 22;       // (a weight-stationary request the kernel does not cover: see plan_tiles)
    if (stages >= 42 && stages <= 48) {
        // persistent direct-to-LDS kernel (conv_persist.hip); what it does not cover runs on the non-persistent ring of the same depth
        const int ns = stages - 40;
        if (pl->vec && t64 && d->Cin % 32 == 0 && d->nlevels == 0 && d->mma == 0 && !pl->cls && (act == YM_ACT_NONE || act == YM_ACT_RELU) &&
            (pl->slots() == 1 || pl->counters) && d->bn_sum == nullptr && (ns == 2 || ns == 3 || ns == 4 || ns == 6 || ns == 8)) {
            static int defer = -1;                            // YM_PERS_DEFER=0: the synchronous epilogue (A/B experiments)
            if (defer < 0) { const char* e = getenv("YM_PERS_DEFER"); defer = e ? atoi(e) : 1; }
            int per_cu = (int)((160u << 10) / ym_conv_pers_lds_bytes(64, 64, ns, defer != 0));
            if (per_cu > 4) per_cu = 4;                       // 128 VGPRs: four waves per SIMD
            if (per_cu < 1) per_cu = 1;
            int g = d->grid_wgs > 0 ? d->grid_wgs : ym_cu_count() * per_cu;
            if (g > pl->grid()) g = pl->grid();
            if (g >= 8 && g < pl->grid()) g &= ~7;            // a workgroup's items then all lie in its own XCD's chunk of the tile space
            pl->family = CONV_PERS; pl->ring = ns; pl->pers_grid = g; pl->pers_defer = defer != 0;
            pl->mode = d->transposed ? 2 : 0;
            return;
        }
        stages = ns >= 4 && t64 && !d->transposed ? 24 : (ns == 2 ? 22 : 23);
    }
    // conv_igemm_f32<bm, bn, mode, ring, dl, pf, pyramid, spl>: 22 / 23 direct-to-LDS ring of 2 / 3; 24 / 33 / 34 (ring of 4, rings of
    // 3 / 4 with software-pipelined fragments) for the 64x64 forward tile; 3 the register ring where it is built (forward: not for
    // 128x128; data gradient: 64x64 only; split bf16: two register sets, every tile); everything else the register double buffer,
    // which is also all the pyramid, the stem and (but for 3) the split-bf16 products have.
    pl->mode = d->transposed ? 2 : (d->Cin == 4 ? 1 : 0);
    pl->pyramid = d->nlevels > 0;
    if (d->mma != 0) {                                   // split-bf16 products; tensors stay fp32 (the launch checks mma and the input)
        pl->spl = d->mma == 3 ? 2 : 3;
        pl->ring = stages == 3 ? 3 : 2;
    } else if (!pl->pyramid && pl->mode != 1) {
        const bool has3 = pl->mode == 0 ? !(pl->bm == 128 && pl->bn == 128) : t64;
        if (pl->mode == 0 && t64 && (stages == 24 || stages == 33 || stages == 34)) { pl->dl = true; pl->pf = stages > 30; pl->ring = stages % 10; }
        else if (stages == 22 || stages == 23) { pl->dl = true; pl->ring = stages - 20; }
        else if (stages == 3 && has3) pl->ring = 3;
    }
}

}  // namespace

int ym_conv_plan(const ym_conv_desc* d, bool ws_aligned, Plan* pl) {
    *pl = Plan{};
    if (int rc = plan_tiles(d, pl, true)) return rc;
    pl->kwaves = d->kwaves;
    pl->vec = vec_epilogue(d) && ws_aligned;
    pl->counters = pl->vec && pl->slots() > 1 && (d->kwaves == 0 || pl->tail_tiles > 0) && pl->ws_bytes(d->Cout) < 0xFFFFFFF0ull && d->tile_counters;
    pl->fuses_bn = pl->vec && (pl->slots() == 1 || pl->counters) && d->kwaves == 0;
    if (pl->family == CONV_IGEMM) plan_variant(d, pl);
    // what of the descriptor's grid_wgs the chosen kernel reads: walkers (weight-stationary, persistent), waves per workgroup (wave DMA)
    pl->grid_wgs = pl->family == CONV_IGEMM || pl->family == CONV_WAVE ? 0 : d->grid_wgs;
    // rows of the ordered BatchNorm partials: one per M tile (a stride-2 data gradient: the class-padded tiles), or per (walker, wave row)
    pl->bn_rows = !pl->fuses_bn ? 0 : pl->family != CONV_WS ? pl->tiles_m
                : ym_conv_ws_partial_rows(pl->M, d->Cout, pl->bm, pl->bn, pl->nkt, pl->ring, d->grid_wgs);
    return YM_OK;
}
