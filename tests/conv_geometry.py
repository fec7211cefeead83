"""Layer geometry of a forward key of the tuned table (host only; no GPU, no library).

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


KNOWN_STAGES = (0, 2, 3, 22, 23, 24, 33, 34, 42, 43, 44, 46, 48, 52, 53, 54)


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


def family(g, plan, mma):
    if g.levels:
        return 'pyramid'
    if mma:
        return 'split-bf16'
    if plan.wave:
        return 'wave-DMA' if plan.wave_dma else 'wave'
    if plan.persistent:
        return 'persistent'
    if plan.weight_stationary:
        return 'weight-stationary'
    if plan.tile_m == 0:
        return 'heuristic'
    return 'LDS ring' if plan.stages >= 22 else 'register'


def silent_fallback(g, plan, mma):
    """Why ym_conv2d_fwd would run this launch on ANOTHER kernel than the row names without saying so, or None.  The library has no
    query for the kernel it picked; these are the conditions include/yolact_hip.h documents for the variants that fall back."""
    tile = (plan.tile_m, plan.tile_n)
    plain = g.nseg == 1 and g.N % 4 == 0           # one NHWC tensor the vector epilogue can write
    if plan.stages not in KNOWN_STAGES:
        return f'stages {plan.stages} names no kernel'
    if g.levels or mma or plan.wave:
        if (plan.tail_tiles or plan.tail_ksplit) and not plain:
            return 'a tail split needs one plain NHWC output'
        return None                                # (stages ignored / rejected loudly)
    if plan.persistent and not (tile == (64, 64) and plain and g.C % 32 == 0 and g.suffix != '_st'):
        return 'the persistent walker covers 64x64 tiles of a plain NHWC output without BatchNorm sums'
    if plan.weight_stationary and not (tile in ((64, 256), (128, 128), (256, 64)) and g.k == 1 and g.stride == 1 and plain and
                                       g.C % 32 == 0 and plan.tile_n * g.C * 4 <= (64 << 10)):
        return 'the weight-stationary kernel covers 1x1 / 1 filters whose slice fits the LDS, plain NHWC output'
    if plan.stages in (24, 33, 34) and tile != (64, 64):
        return f'stages {plan.stages} exists for the 64x64 tile only'
    if plan.stages == 3 and tile == (128, 128):
        return 'the register ring of 3 exists for 64-wide tiles only'
    if (plan.tail_tiles or plan.tail_ksplit) and not plain:
        return 'a tail split needs one plain NHWC output'
    return None
