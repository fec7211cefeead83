"""Layer geometry of a forward key of the tuned table, and the plan the library runs for its row (host only; no GPU).

A key `M.._N.._C.._k.._s.._seg.._r..(_L5)(_st|_tp|_mma3)` names M = B * Ho * Wo output pixels, not B, Ho, Wo; a 3x3 filter's halo
addressing depends on them.  The table is measured on real layers, so every key must be a layer of some model at some image size:

* image sizes: the multiples of 32 from 128 to 864 (the reference accepts every multiple of 32);
* sides of a size s: the ResNet chain s, ceil(s/2), ceil(ceil(s/2)/2), ... (8 entries: image, stem, C2 ... C5 = P5, P6, P7) and the
  Swin chain s/4 followed by three more halvings;
* batches 1, 2, 4, 8, 16.

A plain key resolves to the (batch, size, side) with batch * side^2 = M, a `_L5` key to batch * (sum of side^2 over the FPN levels
P3 ... P7 of a size).  Among several matches: batch 1, then 8, then 2, 4, 16; then the smallest size (which of the matches is taken
changes the image size a side came from, never the launch's own M).  The input side of a strided key comes from the chain."""
from typing import NamedTuple, Optional, Tuple

from yolact_minimal_amd import plan_transfer

SIZES = tuple(range(128, 865, 32))
BATCHES = (1, 8, 2, 4, 16)          # order of preference


def _half(v):
    return (v + 1) // 2


def resnet_chain(size):
    out = [size]
    for _ in range(7):
        out.append(_half(out[-1]))
    return out


def swin_chain(size):
    out = [size // 4]
    for _ in range(3):
        out.append(_half(out[-1]))
    return out


def fpn_levels(size):
    """Sides of P3 ... P7."""
    return resnet_chain(size)[3:8]


class Geometry(NamedTuple):
    key: str
    M: int
    N: int
    C: int
    k: int
    stride: int
    pad: int
    nseg: int
    residual: bool
    suffix: str                       # '', '_st', '_tp', '_mma3'
    batch: int
    size: int                         # image size the layer was found in
    h: int                            # input side (0 for a pyramid key)
    ho: int                           # output side (0 for a pyramid key)
    levels: Optional[Tuple[int, ...]]   # sides of the five pyramid levels of a `_L5` key

    def describe(self):
        where = f'levels {self.levels}' if self.levels else f'{self.h}x{self.h} -> {self.ho}x{self.ho}'
        return f'{self.key}: batch {self.batch}, image {self.size}, {where}, pad {self.pad}'


def is_forward_key(key):
    f = plan_transfer.parse_key(key)
    return f is not None and f.prefix == ''


def forward_keys(table):
    return sorted(k for k in table if is_forward_key(k))


def _input_side(size, ho, k, stride, cin):
    """Input side of an output side `ho` found in `size`'s chains, or None if no layer of that filter produces it there."""
    if stride == 1:
        return ho, k // 2
    if k == stride:                   # Swin's patch embedding: 4x4 / 4 on the image, no padding
        return (size, 0) if cin == 4 and ho * stride == size else None
    chain = resnet_chain(size)
    pad = k // 2
    for i in range(1, len(chain)):
        if chain[i] == ho and (chain[i - 1] + 2 * pad - k) // stride + 1 == ho:
            if cin == 4 and i != 1:   # the stem reads the image itself
                continue
            return chain[i - 1], pad
    return None


def resolve(key):
    """Geometry of a forward key, or None when no layer of any model / size / batch matches it."""
    if not is_forward_key(key):
        return None
    _, M, N, C, k, stride, nseg, residual, lev, suffix = plan_transfer.parse_key(key)
    for batch in BATCHES:
        if M % batch:
            continue
        for size in SIZES:
            if lev:
                if lev != 5 or stride != 1:
                    return None
                levels = tuple(fpn_levels(size))
                if batch * sum(s * s for s in levels) == M:
                    return Geometry(key, M, N, C, k, stride, k // 2, nseg, residual, suffix, batch, size, 0, 0, levels)
                continue
            for ho in sorted(set(resnet_chain(size) + swin_chain(size))):
                if batch * ho * ho != M:
                    continue
                got = _input_side(size, ho, k, stride, C)
                if got is not None:
                    h, pad = got
                    assert (h + 2 * pad - k) // stride + 1 == ho, key
                    return Geometry(key, M, N, C, k, stride, pad, nseg, residual, suffix, batch, size, h, ho, None)
    return None


def launch_plan(g, row):
    """(ConvPlan, mma) that reach the descriptor of the launch a row is read for: the engines' own resolution (conv_launch.py: the
    inference policy, for an `_st` row the training one) over a table that holds this row alone."""
    from yolact_minimal_amd import conv_launch as CL
    assert plan_transfer.mode() != 'only'                         # (the row itself is meant, not a neighbour's)
    base, table = g.key[:len(g.key) - len(g.suffix)], {g.key: row}
    shape = (g.M, g.N, -(-(g.k * g.k * g.C) // 32), g.nseg)
    eligible = g.C % 32 == 0 and not g.levels
    if g.suffix == '_st':
        return CL.train_overrides(CL.train_plan(table, base, shape, stats=True), table, base, 0, eligible)
    mma = int(g.suffix[4:]) if g.suffix.startswith('_mma') else 0
    return CL.infer_plan(table, base, shape, 'throughput' if g.suffix == '_tp' else 'latency', mma, eligible, pyramid=bool(g.levels))[:2]


def family(g, effective, mma):
    """Kernel family of the plan that runs (hip.conv_effective_plan)."""
    if g.levels:
        return 'pyramid'
    if mma:
        return 'split-bf16'
    if effective.wave:
        return 'wave-DMA' if effective.wave_dma else 'wave'
    if effective.persistent:
        return 'persistent'
    if effective.weight_stationary:
        return 'weight-stationary'
    return 'LDS ring' if effective.stages >= 22 else 'register'


# Rows of the table that ym_conv2d_fwd does NOT run as written: key -> the row it runs instead.  Exact in both directions (a listed
# row resolves to precisely this, no other row differs from its request); retuning a listed shape removes its entry.
KNOWN_FALLBACKS = {
    # 8 * 64 * 32 + 4 * 256 * 32 floats = 192 KB of LDS for the filter slice + ring of 4: over the weight-stationary kernel's 160 KB
    'M147968_N128_C256_k1_s1_seg1_r0': [64, 64, 1, 0, 22, 0, 0],
}


def canonical_stages(g, plan, mma):
    """`stages` of a request in ym_conv2d_effective_plan's canonical values (include/yolact_hip.h): 0 and 2 both name the register
    double buffer, which is all a pyramid or stem launch has and, besides 3, all a split-bf16 one; a wave launch without DMA is 0."""
    if plan.wave:
        return plan.stages if plan.wave_dma else 0
    if g.levels or g.C == 4 or (mma and plan.stages != 3) or plan.stages == 0:
        return 2
    return plan.stages


def fallback(g, plan, mma, effective):
    """How the plan the library runs (`effective`) departs from the requested one, or None.  `ksplit` is the planner's to normalise
    (cdiv(nkt, cdiv(nkt, ksplit))) and is not compared; a tile of 0 leaves the tile to the planner."""
    diffs = []
    if plan.tile_m and plan.tile_n and (plan.tile_m, plan.tile_n) != (effective.tile_m, effective.tile_n):
        diffs.append(f'tile {plan.tile_m}x{plan.tile_n} runs as {effective.tile_m}x{effective.tile_n}')
    if plan.kwaves != effective.kwaves:
        diffs.append(f'kwaves {plan.kwaves} runs as {effective.kwaves}')
    if canonical_stages(g, plan, mma) != effective.stages:
        diffs.append(f'stages {plan.stages} runs as {effective.stages}')
    if plan.tail_tiles > 0 and plan.tail_ksplit > 1 and plan.tail_tiles != effective.tail_tiles:
        diffs.append(f'tail of {plan.tail_tiles} tiles runs as {effective.tail_tiles}')
    return '; '.join(diffs) or None


def check_effective(g, row, plan, mma, desc):
    """Ask the library which plan it runs for `desc` (the launch of `row`) and hold it to the request, or to KNOWN_FALLBACKS;
    returns the effective ConvPlan."""
    from yolact_minimal_amd import hip
    effective = hip.conv_effective_plan(desc)
    why = fallback(g, plan, mma, effective)
    if g.key in KNOWN_FALLBACKS:
        assert why is not None and effective.to_row() == KNOWN_FALLBACKS[g.key], (g.describe(), row, effective.to_row(), why)
    else:
        assert why is None, f'{g.describe()} row {row} runs as {effective.to_row()}: {why}'
    return effective
