"""Host model of the split-bf16 products (ym_conv_desc.mma = 3 / 6, conv_mfma.hip SPL = 2 / 3) and the small convolutions the
split-bf16 tests run.  Plain torch on whatever device the operands live on: no GPU is needed, the library is not called.

The kernel splits every fp32 operand, while it stages it into LDS, into bf16 planes p0 = bf16(x), p1 = bf16(x - p0), p2 = ...
(round to nearest even, residuals exact in fp32: `planes`) and sums the plane products of `kept_terms` in an fp32 accumulator.

Per-product error of the kept terms, relative to |x y| (u = 2^-8, the bound of one bf16 rounding: |r1| <= u |x|, |r2| <= u^2 |x|,
|r3| <= u^3 |x|, and |p_i| <= |r_i|(1 + u)):
  bf16x3 keeps p0 q0 + p0 q1 + p1 q0 = x y - (r2x y + x r2y - r2x r2y) - p1x p1y: at most 2 u^2 + u^2 (1 + u)^2 + u^4 < 3 * 2^-16 + 2^-23;
         the typical value is ~2^-17 (a rounding residual is uniform in its half ulp, and the three terms rarely align);
  bf16x6 adds p0 q2 + p2 q0 + p1 q1 and leaves r3x y + x r3y + p1 q2 + p2 q1 + p2 q2: at most 2 u^3 + 2 u^3 (1 + u)^2 + .. < 5 * 2^-24.

Exact operands.  `ints16`, `ints20` and `two_plane` build integers whose planes are known exactly, together with int64 twins; when
`check_exact_range` holds (sum |a b| < 2^24 for every output), every partial sum of plane products, in any order and over any slice
of K, is an integer that fp32 holds exactly, so the device result has exactly one correct value and is compared with torch.equal.
"""
from typing import NamedTuple

import torch

EXACT_LIMIT = 1 << 24


def planes(x, n):
    """[p0 .. p(n-1)] as fp32 tensors: p_i = bf16(r_i) (round to nearest even), r_0 = x, r_(i+1) = r_i - p_i in fp32."""
    r = x.to(torch.float32)
    out = []
    for _ in range(n):
        p = r.to(torch.bfloat16).to(torch.float32)
        out.append(p)
        r = r - p
    return out


def kept_terms(mma):
    """(plane of the activation, plane of the weight) of every product the kernel sums; mma 0 is the f32 pipe (no planes)."""
    if mma == 3:
        return ((0, 0), (0, 1), (1, 0))
    if mma == 6:
        return ((0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1))
    raise ValueError(f'mma {mma}: 3 (bf16x3) or 6 (bf16x6)')


def nplanes(mma):
    return {3: 2, 6: 3}[mma]


# ---- operand builders: (fp32 tensor, int64 twin), both on the CPU ----------------------------------------------------------------

def _signs(shape, gen):
    return torch.randint(0, 2, shape, generator=gen, dtype=torch.int64) * 2 - 1


def ints16(shape, gen):
    """+-[2^8, 2^16): p0 + p1 = x exactly, p1 != 0 for ~98 % of the elements."""
    v = torch.randint(1 << 8, 1 << 16, shape, generator=gen, dtype=torch.int64) * _signs(shape, gen)
    return v.to(torch.float32), v


def ints20(shape, gen):
    """[2^16, 2^20): p0 + p1 + p2 = x exactly, p2 != 0 for ~53 % of the elements."""
    v = torch.randint(1 << 16, 1 << 20, shape, generator=gen, dtype=torch.int64)
    return v.to(torch.float32), v


def two_plane(shape, gen):
    """+-(256 a + b), a in [8, 15], b in [1, 7]: p0 = +-256 a, p1 = +-b exactly; a product of two such values is below 2^24."""
    a = torch.randint(8, 16, shape, generator=gen, dtype=torch.int64)
    b = torch.randint(1, 8, shape, generator=gen, dtype=torch.int64)
    v = (256 * a + b) * _signs(shape, gen)
    return v.to(torch.float32), v


def small_ints(shape, gen, top):
    """Uniform in {-top .. top} (zeros included): one bf16 plane."""
    v = torch.randint(-top, top + 1, shape, generator=gen, dtype=torch.int64)
    return v.to(torch.float32), v


def thin_weight(w, keep, gen):
    """Zero all but `keep` randomly placed entries of every OUTPUT column of the GEMM.  `w` is OIHW of the forward conv: a forward
    launch's output channel is O (its K runs over I, kh, kw), a data gradient's is I (its K runs over O, kh, kw).  Returns a mask
    [2] of int64 0 / 1 masks: (for the forward launch, for the data gradient)."""
    cout, cin, kh, kw = w.shape
    fwd = torch.zeros(cout, cin * kh * kw, dtype=torch.int64)
    idx = torch.rand(cout, cin * kh * kw, generator=gen).argsort(1)[:, :keep]
    fwd.scatter_(1, idx, 1)
    t = torch.zeros(cin, cout * kh * kw, dtype=torch.int64)
    idx = torch.rand(cin, cout * kh * kw, generator=gen).argsort(1)[:, :keep]
    t.scatter_(1, idx, 1)
    return fwd.view(cout, cin, kh, kw), t.view(cin, cout, kh, kw).permute(1, 0, 2, 3).contiguous()


def thin_activation(shape, channels, period, gen):
    """int64 0 / 1 mask [B][H][W][C]: `channels` randomly placed channels at the pixels of a lattice of period `period` (the filter
    size: every k x k window inside the map then holds exactly one such pixel), none elsewhere."""
    b, h, w, c = shape
    m = torch.zeros(b * h * w, c, dtype=torch.int64)
    idx = torch.rand(b * h * w, c, generator=gen).argsort(1)[:, :channels]
    m.scatter_(1, idx, 1)
    m = m.view(b, h, w, c)
    lattice = torch.zeros(h, w, dtype=torch.int64)
    lattice[period // 2::period, period // 2::period] = 1
    return m * lattice[None, :, :, None]


# ---- geometry and the host convolution ---------------------------------------------------------------------------------------------

class Geo(NamedTuple):
    """A forward conv x [b][side][side][cin] -> y [b][out][out][cout], or (transposed) its data gradient dz [b][out][out][cout] ->
    dx [b][side][side][cin]; square filter k, pad k // 2, weight OIHW [cout][cin][k][k] in both cases (cout: padded to 32)."""
    name: str
    transposed: bool
    b: int
    side: int
    cin: int
    cout: int
    k: int
    stride: int

    pad = property(lambda self: self.k // 2)
    out = property(lambda self: (self.side + 2 * (self.k // 2) - self.k) // self.stride + 1)
    # the launch's GEMM: M rows, N output channels, K reduction length; operand and output shapes (NHWC)
    M = property(lambda self: self.b * (self.side if self.transposed else self.out) ** 2)
    N = property(lambda self: self.cin if self.transposed else self.cout)
    K = property(lambda self: self.k * self.k * (self.cout if self.transposed else self.cin))
    in_shape = property(lambda self: (self.b, self.out, self.out, self.cout) if self.transposed else (self.b, self.side, self.side, self.cin))
    out_shape = property(lambda self: (self.b, self.side, self.side, self.cin) if self.transposed else (self.b, self.out, self.out, self.cout))
    w_shape = property(lambda self: (self.cout, self.cin, self.k, self.k))


def conv(a, w, geo):
    """The launch's result [M rows as NHWC] from NHWC `a` and OIHW `w`, one matrix product per filter tap, in the operands' own dtype
    (int64 on the CPU: exact; float64: the high-precision reference)."""
    b, k, s, pad, out = geo.b, geo.k, geo.stride, geo.pad, geo.out
    span = s * (out - 1) + 1
    if not geo.transposed:
        ap = torch.nn.functional.pad(a, (0, 0, pad, pad, pad, pad))
        y = torch.zeros(b * out * out, geo.cout, dtype=a.dtype, device=a.device)
        for kh in range(k):
            for kw in range(k):
                y += ap[:, kh:kh + span:s, kw:kw + span:s].reshape(-1, geo.cin) @ w[:, :, kh, kw].t()
        return y.view(b, out, out, geo.cout)
    full = geo.side + 2 * pad
    dx = torch.zeros(b, full, full, geo.cin, dtype=a.dtype, device=a.device)
    flat = a.reshape(-1, geo.cout)
    for kh in range(k):
        for kw in range(k):
            if kh + span > full or kw + span > full:          # (cannot happen for out = (side + 2 pad - k) // s + 1)
                raise ValueError(geo)
            dx[:, kh:kh + span:s, kw:kw + span:s] += (flat @ w[:, :, kh, kw]).view(b, out, out, geo.cin)
    return dx[:, pad:pad + geo.side, pad:pad + geo.side].contiguous()


def check_exact_range(a_int, w_int, geo):
    """max over the outputs of sum |a b| (int64); asserts it is below 2^24, the condition under which the device result is exact."""
    top = int(conv(a_int.abs(), w_int.abs(), geo).max())
    assert top < EXACT_LIMIT, f'{geo.name}: sum |a b| reaches {top} >= 2^24: the operands do not pin one exact result'
    return top


def emulate(a, w, geo, mma):
    """fp64 sum of the kept plane products of fp32 operands `a`, `w`: what the kernel computes but for its fp32 accumulation."""
    n = nplanes(mma)
    pa, pw = [p.double() for p in planes(a, n)], [p.double() for p in planes(w, n)]
    terms = kept_terms(mma)
    total = None
    for i in range(n):                                       # sum_j p_i q_j = p_i (sum_j q_j): the plane sums are exact in fp64
        js = [j for (ii, j) in terms if ii == i]
        if not js:
            continue
        y = conv(pa[i], sum(pw[j] for j in js), geo)
        total = y if total is None else total + y
    return total


# ---- the shapes and plans of tests/test_gpu_split_bf16.py (resolved on the host by tests/test_split_bf16_cpu.py) -------------------

D1 = Geo('D1', True, 2, 9, 96, 64, 3, 1)         # M 162 (partial M tile), N 96 (partial N tile for 64 and 128), 18 K tiles
D2 = Geo('D2', True, 1, 23, 64, 128, 3, 2)       # four parity classes of different sizes and K ranges
D3 = Geo('D3', True, 2, 12, 128, 256, 1, 2)      # parity classes with empty tap sets
D4 = Geo('D4', True, 2, 12, 256, 1024, 1, 1)     # 32 K tiles, plain GEMM
F1 = Geo('F1', False, 2, 9, 64, 96, 3, 1)        # forward statistics, partial tiles
F2 = Geo('F2', False, 2, 12, 1024, 256, 1, 1)    # 32 K tiles
SHAPES = (D1, D2, D3, D4, F1, F2)
TILES = ((64, 64), (128, 64), (64, 128), (128, 128))


class Case(NamedTuple):
    """One launch: the plan fields of the descriptor, whether it gets arrival counters, whether a residual `add` is summed."""
    geo: Geo
    tile: tuple
    stages: int = 0
    ksplit: int = 1
    counters: bool = True
    tail: tuple = (0, 0)
    add: bool = False

    @property
    def id(self):
        s = f'{self.geo.name}-{self.tile[0]}x{self.tile[1]}-st{self.stages}'
        if self.ksplit > 1:
            s += f'-ks{self.ksplit}' + ('' if self.counters else '-nocounters')
        if self.tail[0]:
            s += f'-tail{self.tail[0]}x{self.tail[1]}'
        return s + ('-add' if self.add else '')


def cases(shapes=SHAPES, every_tile=True):
    """The plan matrix: four tiles x stages 0 / 3 (one / two register sets); on 64x64 a K split of 3 with and without arrival counters;
    on D1 / F1 a tail split; on D1 / D2 a residual add."""
    out = []
    for g in shapes:
        for tile in (TILES if every_tile else TILES[:1]):
            for stages in (0, 3):
                out.append(Case(g, tile, stages))
        out.append(Case(g, (64, 64), 0, ksplit=3))
        out.append(Case(g, (64, 64), 3, ksplit=3, counters=False))
        if g.name in ('D1', 'F1'):
            out.append(Case(g, (64, 64), 0, tail=(2, 3)))
        if g.name in ('D1', 'D2'):
            out.append(Case(g, (128, 64), 3, add=True))
            out.append(Case(g, (64, 64), 0, ksplit=3, add=True))
    return out


def descriptor(case, mma, inp, weight, out, counters, add=None):
    """The ym_conv_desc of `case` under matrix pipe `mma`, built as the engines build theirs (conv_launch.conv_desc) from raw
    addresses (placeholders will do on the host: the planner looks at nullness and alignment only)."""
    from yolact_minimal_amd import conv_launch
    g = case.geo
    if g.transposed:       # input = dz [b][out][out][cout], output = dx [b][side][side][cin]
        d = conv_launch.conv_desc(g.b, g.out, g.out, g.cout, g.cin, g.k, g.k, g.stride, g.pad, g.side, g.side, g.K,
                                  [(0, g.cin, out, g.side * g.side * g.cin, g.cin, 0)], transposed=True)
    else:
        d = conv_launch.conv_desc(g.b, g.side, g.side, g.cin, g.cout, g.k, g.k, g.stride, g.pad, g.out, g.out, g.K,
                                  [(0, g.cout, out, g.out * g.out * g.cout, g.cout, 0)])
    d.inp, d.weight, d.residual = inp, weight, add
    d.tile_m, d.tile_n, d.ksplit, d.stages = case.tile[0], case.tile[1], case.ksplit, case.stages
    d.tail_tiles, d.tail_ksplit = case.tail
    d.tile_counters = counters if case.counters else None
    d.mma = mma
    return d
