"""Set-up of a convolution launch: the descriptor's shape fields and the plan a tuned-table row resolves to.  Host-only: integer and
string logic plus ctypes field writes; no library call, no tensor, no file, and the tuned table is an argument.  engine.py,
train_engine.py and the tests all come here, so the policy is pinned on the CPU (tests/test_engine_table.py)."""
import math
import os

from . import plan_transfer
from .conv_plan import ConvPlan, WgradPlan, from_entry
from .hip import ConvDesc


def conv_desc(b, h, w, cin, cout, kh, kw, stride, pad, ho, wo, k_pad, segs, levels=None, transposed=False):
    """A ConvDesc with its geometry and the output segments `segs` = [(n_begin, n_end, ptr, batch_stride, pitch, act)].  `levels`
    [(h, w)]: a pyramid input (ym_conv_desc.nlevels); `transposed`: a data gradient.  Operand pointers, plan, arrival counters and
    BatchNorm sums are the caller's."""
    d = ConvDesc()
    d.B, d.H, d.W, d.Cin, d.Cout = b, h, w, cin, cout
    d.KH, d.KW, d.stride, d.pad, d.Ho, d.Wo, d.k_pad = kh, kw, stride, pad, ho, wo, k_pad
    d.transposed, d.nlevels, d.nseg = int(transposed), len(levels or ()), len(segs)
    for l, (lh, lw) in enumerate(levels or ()):
        d.level_h[l], d.level_w[l] = lh, lw
    for i, (n0, n1, ptr, bstride, pitch, act) in enumerate(segs):
        d.seg[i].n_begin, d.seg[i].n_end, d.seg[i].out = n0, n1, ptr
        d.seg[i].batch_stride, d.seg[i].pitch, d.seg[i].act = bstride, pitch, act
    return d


def entry(table, key, shape=(0, 0, 0, 1), mode='latency'):
    """(row, source) of a forward shape.  'latency' (one request at a time) reads `key`; 'throughput' (the slots of a
    RequestPipeline with several requests in flight) reads `key + '_tp'` first: choices that spread a launch over every CU (tail
    splits, one-wave workgroups) shorten a lone request and cost throughput when other requests want those CUs
    (tools/tune_forward.py --inflight N measures them on the pipeline's own img/s).  A shape without a row takes the row of the
    nearest tuned shape of its family, re-derived for `shape` = (M, N, K tiles, segments) (plan_transfer.py); source = 'table' /
    'nearest:<key>' / 'heuristic'."""
    if mode == 'throughput' and plan_transfer.mode() != 'only' and table.get(key + '_tp') is not None:
        return table[key + '_tp'], 'table'
    if shape[0] > 0:
        return plan_transfer.lookup(table, key, *shape)
    hit = table.get(key)
    return hit, ('heuristic' if hit is None else 'table')


def infer_plan(table, key, shape, mode, mma, eligible, preset=ConvPlan(), no_tuned=False, pyramid=False, bound=None):
    """(plan, mma, source, hit) of an inference launch.  `mma`: the requested matrix pipe (ym_conv_desc.mma), granted where
    `eligible` (not the stem, Cin % 32 == 0, no pyramid input: the split-bf16 workgroup kernel); `preset`: the plan the conv holds;
    `no_tuned`: YM_NO_TUNED=1.  `bound` = (hit, source) of an earlier resolution skips the table read (InferEngine.set_mma)."""
    if bound is not None:
        hit, source = bound
    else:
        row, source = entry(table, key, shape, mode)
        hit = from_entry(row)
        if pyramid:                             # (tile, K split and tail; the pyramid launch ignores the stages)
            return (preset if hit is None else hit._replace(kwaves=0, stages=0, grid_wgs=0)), 0, source, hit
        if hit is not None and preset.tile_m == preset.tile_n == preset.ksplit == preset.kwaves == 0:
            preset = hit
    mma = mma if mma in (3, 6) and eligible else 0
    plan = None
    if mma and not no_tuned:                    # this pipe's own row: exact, or the nearest tuned shape's
        plan = from_entry(plan_transfer.lookup(table, key + f'_mma{mma}', *shape)[0])
    if plan is None:
        plan = hit                              # (no entry for this pipe: the f32 choice, incl. its wave kernel for tiny layers)
        # (not the weight-stationary kernel, whose tiles this pipe lacks; nor a TRANSFERRED wave-kernel row: not measured on it)
        if mma and plan is not None and (plan.weight_stationary or (source != 'table' and plan.wave)):
            plan = ConvPlan()
    if plan is None or no_tuned:                # (each matrix pipe has its own measured choice)
        plan = preset
    elif plan.wave:                             # the tuner may prefer the f32 wave kernel for a tiny layer
        mma = 0
    if mma:
        # split modes stage through registers: 0/2 = one register set (fewer VGPRs: two workgroups per CU on the big tiles),
        # 3 = two sets (the tile being converted arrived an iteration earlier: wins where occupancy is one wave per SIMD anyway)
        plan = plan._replace(stages=3 if plan.stages == 3 else 0)
    return plan, mma, source, hit


def train_plan(table, key, shape, stats=False, tuning=False):
    """The plan of a training forward / data-gradient launch, or None (the caller sweeps, or leaves the planner's heuristic).
    `stats`: the launch carries fused BatchNorm sums, which the persistent kernel does not do: `<key>_st` holds the choice measured
    for such launches where the plain entry (shared with inference) selects the persistent kernel."""
    md = plan_transfer.mode()
    plan = None
    if md != 'only':
        plan = from_entry((table.get(key + '_st') if stats else None) or table.get(key))
    if plan is None and not tuning and md != 'off':
        # another --img_size / batch: the row of the nearest tuned shape of the family, re-derived for this M (plan_transfer.py);
        # with fused statistics the `_st` family competes with the plain one, the donor nearer in M wins
        donors = [(abs(math.log2(nb[1] / shape[0])), i, k) for i, k in enumerate(([key + '_st'] if stats else []) + [key])
                  for nb in [plan_transfer.nearest(table, k, md == 'only')] if nb is not None]
        if donors:
            k = min(donors)[2]
            plan = from_entry(plan_transfer.lookup(table, k, *shape)[0])
            if plan is not None and stats and k == key:
                plan = plan.with_bn_sums()
    return plan


def train_overrides(plan, table, key, mma, eligible):
    """(plan, mma) after YM_FORCE_STAGES / YM_FORCE_GRID (experiments / tests: e.g. 43 = every conv the persistent kernel covers
    runs on it) and the opt-in fast mode `mma` (YM_TRAIN_MMA=3): forward and data-gradient convs on the bf16 MFMA (split-bf16
    products, ym_conv_desc.mma) where `eligible` (Cin % 32 == 0, no pyramid).  NOT the parity mode: per-product error ~2^-17 (at most
    3 * 2^-16) instead of 2^-24, which the ill-conditioned backward of a random-init net amplifies beyond the fp32 reference's own noise."""
    force = os.environ.get('YM_FORCE_STAGES')
    if force:
        plan = plan._replace(tile_m=64, tile_n=64, kwaves=0, stages=int(force), grid_wgs=int(os.environ.get('YM_FORCE_GRID', '0')))
        if plan.tail_tiles and plan.ksplit > 1:
            plan = plan._replace(tail_tiles=0, tail_ksplit=0)
    if not (mma and eligible):
        return plan, 0
    row = from_entry(table.get(key + f'_mma{mma}'))
    if row is not None:                         # (tile, K split, K waves and tail: the staging and grid of the f32 choice stay)
        plan = row._replace(stages=plan.stages, grid_wgs=plan.grid_wgs)
    return (plan._replace(stages=0), mma) if plan.kwaves == 0 else (plan, 0)


def wgrad_plan(table, key, tuning=False):
    """The WgradPlan of a weight-gradient launch, or None."""
    plan = from_entry(table.get(key), WgradPlan) if plan_transfer.mode() != 'only' else None
    f = plan_transfer.parse_key(key)
    if plan is None and not tuning and f:
        plan = from_entry(plan_transfer.lookup(table, key, f.M, f.N, 0)[0], WgradPlan)
    return plan
