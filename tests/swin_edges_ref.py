"""References, case tables and launch arithmetic for tests/test_gpu_swin_edges.py.  Plain torch on the CPU, dtype-generic: no GPU is
needed and the library is not called (except by `main` at the bottom, the child process of the YM_ATTN_BWD_SLOTS=2 test);
tests/test_swin_edges_cpu.py pins everything here against torch and oracle/yolact_ref.py and proves that every case reaches the
edge it is named for.

References.  Every reference takes the float32 inputs of a case and evaluates them in `dtype` (float64: the truth; float32: the
CPU's own rounding, the yardstick the GPU bounds are measured against), so the rounding of the inputs is never counted as error.
  `layernorm_ref`       two-pass LayerNorm as the kernels compute it ((x - mean) * rstd * gamma + beta) and its autograd gradients
  `patch_merge_ln_ref`  `R.swin_merge` with an identity reduction (PatchMerging up to its LayerNorm)
  `gelu_ref`            0.5 z (1 + erf(z / sqrt 2))
  `attention_ref`       pad / roll / `R.swin_windows` / the lines of `R.swin_attention` between its two Linears / `R.swin_shift_mask` /
                        `R.swin_unwindows` / un-roll / crop.  It takes qkv ITSELF: padded tokens carry exactly qkv_bias, as in the kernels, and the gradient through them
                        is the qkv_bias gradient returned here (the share `ym_swin_window_attention_bwd` writes to dqkv_bias_pad).

Launch facts mirror the host code of yolact_minimal_amd/csrc/swin_ops.hip and swin_train.hip; each function names what it mirrors.
What the code says where the first reading of it differed:
  * LayerNorm backward walks 16 (C <= 128: 8 half-wave slots x U = 2), 8 (C <= 256) or 4 (wider) rows per workgroup and iteration,
    so 2048 workgroups make a grid pass of 32768 / 16384 / 8192 rows; M = 32768 + 37 is 2, 3 and 5 iterations.
  * `k_ln_param_grad` with 2048 workgroups is 32 unrolled trips and NO remainder; 50 workgroups are one unrolled trip for slices 0, 1
    and three remainder trips for slices 2..15, 114 are one or two unrolled trips and three or no remainder trips.
  * DropPath with B = 3, per_sample = 1,400,004 has both sample boundaries in the FIRST grid pass (1048576 float4); per_sample =
    2,100,000 puts the second boundary at float4 1,050,000: inside the second pass and inside a workgroup (thread 144).
  * (3, 29 x 21, 24 heads) is 1080 forward units, a multiple of 4; the partial last forward workgroup is taken by the cases with
    1, 6 and 1089 units.
"""
import functools
import json
import math
import sys

import torch
import torch.nn.functional as F

from oracle import yolact_ref as R

WS = 7
EPS = 1e-5
TINY = 1e-30
FLOOR = 1e-6                 # a few float32 ulps of the tensor's scale
K_ROW, K_SUM = 4.0, 8.0      # per-row / per-element results; results that sum across rows or windows in another order than the CPU


# ---- error measure -----------------------------------------------------------------------------------------------------------
def rel_err(got, ref64):
    """max|got - ref64| / max(max|ref64|, tiny): the error in units of the tensor's scale."""
    got, ref64 = got.detach().double().cpu(), ref64.detach().double()
    return float((got - ref64).abs().max()) / max(float(ref64.abs().max()), TINY)


def bound(cpu_err, k):
    return max(FLOOR, k * cpu_err)


# ---- references --------------------------------------------------------------------------------------------------------------
def _leaf(t, dtype, grad):
    return t.detach().to(dtype).clone().requires_grad_(grad)


def layernorm_ref(x, g, b, eps, dtype, dy=None):
    """out [M, C], or (out, dx, dgamma, dbeta) when dy is given."""
    x_, g_, b_ = (_leaf(t, dtype, dy is not None) for t in (x, g, b))
    d = x_ - x_.mean(-1, keepdim=True)
    out = d * (1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + eps)) * g_ + b_
    if dy is None:
        return out.detach()
    out.backward(dy.to(dtype))
    return out.detach(), x_.grad, g_.grad, b_.grad


def patch_merge_ln_ref(x, g, b, dtype, dy=None):
    """x [B, H, W, C] -> out [B, ceil(H/2), ceil(W/2), 4C] (eps = 1e-5, the oracle's), or (out, dx, dgamma, dbeta)."""
    bsz, h, w, c = x.shape
    x_, g_, b_ = (_leaf(t, dtype, dy is not None) for t in (x, g, b))
    sd = {'m.norm.weight': g_, 'm.norm.bias': b_, 'm.reduction.weight': torch.eye(4 * c, dtype=dtype)}
    out = R.swin_merge(x_.reshape(bsz, h * w, c), h, w, sd, 'm').reshape(bsz, (h + 1) // 2, (w + 1) // 2, 4 * c)
    if dy is None:
        return out.detach()
    out.backward(dy.to(dtype))
    return out.detach(), x_.grad, g_.grad, b_.grad


def gelu_ref(z, dtype, dy=None):
    """out, or (out, dz) when dy is given."""
    z_ = _leaf(z, dtype, dy is not None)
    out = 0.5 * z_ * (1.0 + torch.erf(z_ * (1.0 / math.sqrt(2.0))))
    if dy is None:
        return out.detach()
    out.backward(dy.to(dtype))
    return out.detach(), z_.grad


def _padded_windows(qkv_, bias_, b, h, w, shift):
    """[B*nW, 49, 3C] windows of qkv [B, h, w, 3C] padded with qkv_bias to multiples of the window and rolled by -shift."""
    hp, wp = -(-h // WS) * WS, -(-w // WS) * WS
    real = torch.zeros(1, hp, wp, 1, dtype=torch.bool)
    real[:, :h, :w] = True
    y = torch.where(real, F.pad(qkv_.reshape(b, h, w, -1), (0, 0, 0, wp - w, 0, hp - h)), bias_)
    if shift:
        y = torch.roll(y, shifts=(-shift, -shift), dims=(1, 2))
        real = torch.roll(real, shifts=(-shift, -shift), dims=(1, 2))
    return R.swin_windows(y, WS), R.swin_windows(real.expand(b, hp, wp, 1).contiguous(), WS)[..., 0], hp, wp


def attention_ref(qkv, qkv_bias, table, b, h, w, heads, shift, dtype, dout=None):
    """out [B, h, w, C] of the shifted-window attention between the qkv and proj Linears, or (out, dqkv, dqkv_bias, dtable) when
    dout [B, h, w, C] is given; dqkv_bias is the gradient that reaches the bias through the padded tokens alone."""
    c = heads * 32
    grad = dout is not None
    qkv_, bias_, table_ = (_leaf(t, dtype, grad) for t in (qkv, qkv_bias, table))
    xw, _, hp, wp = _padded_windows(qkv_, bias_, b, h, w, shift)
    bw = xw.shape[0]
    # `R.swin_attention` after its qkv Linear, line by line (it derives C from its input's width, so it cannot be handed qkv
    # itself); tests/test_swin_edges_cpu.py pins this against R.swin_attention and R.swin_block
    q, k, v = xw.reshape(bw, 49, 3, heads, 32).permute(2, 0, 3, 1, 4)
    attn = (q * 32 ** -0.5) @ k.transpose(-2, -1)
    attn = attn + table_[R.swin_rel_index(WS).view(-1)].view(49, 49, heads).permute(2, 0, 1).contiguous().unsqueeze(0)
    if shift:
        mask = R.swin_shift_mask(hp, wp, WS, WS // 2).to(dtype)
        nw = mask.shape[0]
        attn = (attn.view(bw // nw, nw, heads, 49, 49) + mask.unsqueeze(1).unsqueeze(0)).view(-1, heads, 49, 49)
    y = R.swin_unwindows((F.softmax(attn, -1) @ v).transpose(1, 2).reshape(bw, 49, c), WS, hp, wp)
    if shift:
        y = torch.roll(y, shifts=(shift, shift), dims=(1, 2))
    out = y[:, :h, :w, :].contiguous()
    if not grad:
        return out.detach()
    out.backward(dout.to(dtype).reshape(b, h, w, c))
    return out.detach(), qkv_.grad, bias_.grad, table_.grad


def attention_logits(qkv, qkv_bias, table, b, h, w, heads, shift):
    """fp64 (logits before the mask [B*nW, heads, 49, 49], additive mask [B*nW, 1, 49, 49] (0 / -100), real-query flags [B*nW, 49]),
    written out by hand from the windows: what the saturated cases are judged by."""
    c = heads * 32
    xw, real, hp, wp = _padded_windows(qkv.double(), qkv_bias.double(), b, h, w, shift)
    bw = xw.shape[0]
    q, k, _ = xw.reshape(bw, 49, 3, heads, 32).permute(2, 0, 3, 1, 4)
    bias = table.double()[R.swin_rel_index(WS).view(-1)].view(49, 49, heads).permute(2, 0, 1)
    logits = (q * 32 ** -0.5) @ k.transpose(-2, -1) + bias.unsqueeze(0)
    mask = torch.zeros(bw, 1, 49, 49, dtype=torch.float64)
    if shift:
        mask = R.swin_shift_mask(hp, wp, WS, WS // 2).double().repeat(b, 1, 1).unsqueeze(1)
    return logits, mask, real


def logit_facts(case):
    """(max |logit|, number of real queries whose largest softmax weight sits on a masked key) in fp64."""
    logits, mask, real = attention_logits(case['qkv'], case['qkv_bias'], case['table'], *case['shape'])
    top = (logits + mask).argmax(-1, keepdim=True)                                   # [bw, heads, 49, 1]
    on_masked = (mask.expand_as(logits).gather(-1, top)[..., 0] < 0) & real.unsqueeze(1)
    return float(logits.abs().max()), int(on_masked.sum())


def saturation_facts(case):
    """`logit_facts` and whether the fp64 output is finite."""
    out = attention_ref(case['qkv'], case['qkv_bias'], case['table'], *case['shape'], torch.float64)
    return logit_facts(case) + (bool(torch.isfinite(out).all()),)


# ---- launch facts ------------------------------------------------------------------------------------------------------------
def ln_fwd_launch(m, c):
    """(workgroups, rows per grid pass) of `ym_layernorm` (swin_ops.hip: the `C <= 256` branch with U = 4 and rows_per_wg = 8 / 4 capped
    at 4096 workgroups, `k_layernorm<0>` with 4 rows per workgroup capped at 8192)."""
    if c <= 256:
        per_wg = (8 if c <= 128 else 4) * 4
        cap = 4096
    else:
        per_wg, cap = 4, 8192
    blocks = min(-(-m // per_wg), cap)
    return blocks, blocks * per_wg


def merge_fwd_launch(b, h, w):
    """(rows, workgroups, rows per grid pass) of `ym_patch_merge_layernorm` (swin_ops.hip: `k_layernorm<1>`, (M + 3) / 4 capped at 8192)."""
    m = b * ((h + 1) // 2) * ((w + 1) // 2)
    blocks = min(-(-m // 4), 8192)
    return m, blocks, blocks * 4


def ln_bwd_launch(m, c, merge=False):
    """(workgroups, rows per grid pass) of `ym_layernorm_bwd` / `ym_patch_merge_layernorm_bwd` (swin_train.hip: `ln_bwd_blocks` =
    ceil(M / 16) capped at LN_BWD_MAX_BLOCKS = 2048; `k_layernorm_bwd_small<2, 32>` has 8 row slots x U = 2 per workgroup,
    `<2, 64>` 4 x 2, `k_layernorm_bwd` one row per wave; the patch-merge launch always takes the last)."""
    blocks = min(max(-(-m // 16), 1), 2048)
    per_wg = 4 if merge or c > 256 else (16 if c <= 128 else 8)
    return blocks, blocks * per_wg


def ln_param_grad_trips(blocks):
    """[(unrolled trips, remainder trips)] of the 16 block slices of `k_ln_param_grad` (swin_train.hip: `for (; b + 48 < blocks;
    b += 64)` then `for (; b < blocks; b += 16)`), and the number of partial rows they read in all."""
    trips, read = [], 0
    for sl in range(16):
        b, u, r = sl, 0, 0
        while b + 48 < blocks:
            b, u, read = b + 64, u + 1, read + 4
        while b < blocks:
            b, r, read = b + 16, r + 1, read + 1
        trips.append((u, r))
    return trips, read


def elementwise_launch(units, cap=4096, threads=256):
    """(workgroups, units per grid pass) of the grid-stride launches of swin_train.hip: `ym_gelu_fwd` / `ym_gelu_bwd` (units = n / 4
    float4), `ym_drop_path_add` / `ym_drop_path_bwd` (units = B * per_sample / 4) and `ym_adamw_step` (units = n), each
    ceil(units / 256) workgroups capped at 4096."""
    blocks = min(-(-units // threads), cap)
    return blocks, blocks * threads


def attn_windows(b, h, w):
    return b * -(-h // WS) * -(-w // WS)


def attn_fwd_units(b, h, w, heads):
    """(window, head) units of `ym_swin_window_attention` (swin_ops.hip): 4 per workgroup, (units + 3) / 4 workgroups."""
    return attn_windows(b, h, w) * heads


def attn_bwd_launch(b, h, w, heads, slots=4):
    """(windows, windows per round = slots * nblk) of `ym_swin_window_attention_bwd` (swin_train.hip: nblk = (256 * (4 / slots)) /
    heads workgroups per head, at least 1, at most ceil(windows / slots); workgroup k walks windows slots * (k + i * nblk) + slot)."""
    nwin = attn_windows(b, h, w)
    nblk = min(max((256 * (4 // slots)) // heads, 1), -(-nwin // slots))
    return nwin, slots * nblk


# ---- case tables -------------------------------------------------------------------------------------------------------------
LN_CHANNELS = (4, 96, 128, 132, 192, 256, 260, 384, 1532, 1536)
LN_ROWS = (1, 5, 37)
LN_FWD_STRIDE = ((131072 + 37, 96), (65536 + 21, 192), (32768 + 5, 384))      # M just over one grid pass of each forward variant
LN_BWD_STRIDE = ((32768 + 37, 96), (32768 + 37, 192), (32768 + 37, 384))
LN_PARAM_GRAD = tuple((m, c) for m in (16 * 49 + 3, 16 * 113 + 3) for c in (96, 192, 384))   # 50 and 114 workgroups
LN_DEGENERATE = (96, 260, 384)
MERGE_SHAPES = ((1, 1, 1, 4), (2, 1, 5, 8), (1, 2, 2, 384), (2, 7, 9, 33 * 4), (1, 2, 3, 16), (1, 3, 2, 16))
MERGE_STRIDE = (1, 363, 363, 8)
GELU_STRIDE_N = 4096 * 256 * 4 + 12
DROP_PATH = (3, 2_100_000)                                                      # (B, per_sample)
ADAMW_N = 4096 * 256 + 3
ATTN_CASES = ((1, 1, 1, 1, 3), (1, 1, 9, 3, 3), (1, 7, 7, 1, 3), (1, 7, 7, 1, 0), (1, 6, 8, 3, 3), (1, 14, 7, 3, 3),
              (3, 29, 21, 24, 3), (3, 75, 73, 3, 3))                            # (B, h, w, heads, shift)
ATTN_SATURATED = ((1, 6, 8, 3, 3), (3, 29, 21, 24, 3))
SATURATION_SCALES = (3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 10.0, 12.0, 16.0)
ATTN_SLOTS2 = ((1, 6, 8, 3, 3), (3, 29, 21, 24, 3))


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _gamma(c, gen):
    """gamma with zeros and negative values."""
    g = torch.randn(c, generator=gen)
    g[0] = 0.0
    g[c // 2] = 0.0
    g[1] = -g[1].abs() - 0.25
    return g


@functools.lru_cache(maxsize=None)
def ln_case(m, c, degenerate=False):
    """x [m, c] = 3 randn + 1, gamma (zeros and negatives), beta, dy.  `degenerate`: m must be >= 12; rows 1, 7 are the constant 0.5
    (variance 0, rstd = 1 / sqrt(eps); the forward is beta bit for bit), rows 2, 8 all zero, rows 3, 9 are 1000 + 0.01 randn."""
    gen = _gen(1, m, c, degenerate)
    x = torch.randn(m, c, generator=gen) * 3 + 1
    if degenerate:
        x[[1, 7]] = 0.5
        x[[2, 8]] = 0.0
        x[[3, 9]] = 1000 + 0.01 * torch.randn(2, c, generator=gen)
    return dict(x=x, g=_gamma(c, gen), b=torch.randn(c, generator=gen), dy=torch.randn(m, c, generator=gen))


@functools.lru_cache(maxsize=None)
def ln_refs(m, c, degenerate=False):
    """((out, dx, dgamma, dbeta) in fp64, the same in fp32) of `ln_case`."""
    k = ln_case(m, c, degenerate)
    return tuple(layernorm_ref(k['x'], k['g'], k['b'], EPS, dt, k['dy']) for dt in (torch.float64, torch.float32))


@functools.lru_cache(maxsize=None)
def merge_case(b, h, w, c):
    gen = _gen(2, b, h, w, c)
    return dict(x=torch.randn(b, h, w, c, generator=gen) * 2 + 0.5, g=_gamma(4 * c, gen), b=torch.randn(4 * c, generator=gen),
                dy=torch.randn(b, (h + 1) // 2, (w + 1) // 2, 4 * c, generator=gen))


@functools.lru_cache(maxsize=None)
def merge_refs(b, h, w, c):
    k = merge_case(b, h, w, c)
    return tuple(patch_merge_ln_ref(k['x'], k['g'], k['b'], dt, k['dy']) for dt in (torch.float64, torch.float32))


def _f32(v):
    return torch.tensor(v, dtype=torch.float32)


def gelu_thresholds():
    """The float32 z nearest 0 at which 1 + erf(z / sqrt 2) evaluated in float32 is exactly 0 (z < 0) and exactly 2 (z > 0), by
    bisection over the float32 bit patterns (the sum is monotone in z), each with its two float32 neighbours."""
    def first(sign, target):
        lo, hi = _f32(sign * 1.0).view(torch.int32).item(), _f32(sign * 12.0).view(torch.int32).item()   # bit patterns grow with |z|
        while hi - lo > 1:
            mid = (lo + hi) // 2
            z = torch.tensor(mid, dtype=torch.int32).view(torch.float32)
            if float(1.0 + torch.erf(z * _f32(0.70710678118654752440))) == target:
                hi = mid
            else:
                lo = mid
        return [float(torch.tensor(v, dtype=torch.int32).view(torch.float32)) for v in (hi - 1, hi, hi + 1)]
    return first(-1.0, 0.0) + first(1.0, 2.0)


@functools.lru_cache(maxsize=None)
def gelu_grid():
    """z in [-12, 12] in steps of 1/256, +-0, +-1e-30, float32 denormals, the cancellation thresholds; padded with zeros to a multiple
    of 4.  dy = 1 everywhere, so dz is the derivative itself."""
    special = [0.0, -0.0, 1e-30, -1e-30, 1e-40, -1e-40, 2.0 ** -149, -2.0 ** -149, 2.0 ** -126, -2.0 ** -126] + gelu_thresholds()
    z = torch.cat([torch.arange(-12 * 256, 12 * 256 + 1, dtype=torch.float32) / 256, _f32(special)])
    z = torch.cat([z, torch.zeros(-z.numel() % 4)])
    return dict(z=z, dy=torch.ones_like(z))


@functools.lru_cache(maxsize=None)
def gelu_stride_case():
    gen = _gen(3)
    return dict(z=torch.randn(GELU_STRIDE_N, generator=gen) * 2, dy=torch.randn(GELU_STRIDE_N, generator=gen))


@functools.lru_cache(maxsize=None)
def gelu_refs(which):
    k = gelu_grid() if which == 'grid' else gelu_stride_case()
    return tuple(gelu_ref(k['z'], dt, k['dy']) for dt in (torch.float64, torch.float32))


@functools.lru_cache(maxsize=None)
def attn_case(b, h, w, heads, shift, saturated=False):
    """qkv [b*h*w, 3C] = randn, qkv_bias = 0.3 randn, table = 0.5 randn, dout = randn.  `saturated`: table = 5 randn, and q and k
    (their bias too) scaled by the smallest factor of the list below for which the fp64 logits exceed 40 and some real query's
    largest softmax weight sits on a masked key (a -100 key beats every unmasked one: a logit spread above 100 in one row)."""
    c = heads * 32
    gen = _gen(4, b, h, w, heads, shift)
    qkv = torch.randn(b * h * w, 3 * c, generator=gen)
    bias = torch.randn(3 * c, generator=gen) * 0.3
    table = torch.randn(169, heads, generator=gen) * (5.0 if saturated else 0.5)
    case = dict(qkv=qkv, qkv_bias=bias, table=table, dout=torch.randn(b * h * w, c, generator=gen), shape=(b, h, w, heads, shift))
    if saturated:
        for s in SATURATION_SCALES:
            case['qkv'], case['qkv_bias'] = qkv.clone(), bias.clone()
            case['qkv'][:, :2 * c] *= s
            case['qkv_bias'][:2 * c] *= s
            peak, on_masked = logit_facts(case)
            if peak > 40 and on_masked > 0:
                break
        case['qk_scale'] = s
    return case


@functools.lru_cache(maxsize=None)
def attn_refs(b, h, w, heads, shift, saturated=False):
    """((out, dqkv, dqkv_bias, dtable) in fp64, the same in fp32) of `attn_case`."""
    k = attn_case(b, h, w, heads, shift, saturated)
    return tuple(attention_ref(k['qkv'], k['qkv_bias'], k['table'], b, h, w, heads, shift, dt, k['dout'])
                 for dt in (torch.float64, torch.float32))


# ---- the library's attention backward on a case (the GPU test and the child process below) -----------------------------------
ATTN_NAMES = ('out', 'dqkv', 'dqkv_bias', 'dtable')
ATTN_K = dict(out=K_ROW, dqkv=K_SUM, dqkv_bias=K_SUM, dtable=K_SUM)


def attn_errors(got, refs):
    """{name: (rel_err of `got`, rel_err of the fp32 CPU reference)} for the tensors of ATTN_NAMES present in `got`."""
    ref64, ref32 = refs
    return {n: (rel_err(got[n], ref64[i]), rel_err(ref32[i], ref64[i])) for i, n in enumerate(ATTN_NAMES) if n in got}


def run_attention_fn(case, dev):
    """WindowAttentionFn forward + backward on the device: {out, dqkv, dqkv_bias, dtable} on the CPU."""
    from yolact_minimal_amd.swin_train import WindowAttentionFn
    b, h, w, heads, shift = case['shape']
    c = heads * 32
    qkv = case['qkv'].to(dev).reshape(b, h, w, 3 * c).requires_grad_()
    bias, table = case['qkv_bias'].to(dev).requires_grad_(), case['table'].to(dev).requires_grad_()
    out = WindowAttentionFn.apply(qkv, bias, table, heads, WS, shift)
    out.backward(case['dout'].to(dev).reshape(b, h, w, c))
    return dict(out=out.detach().cpu().reshape(b, h, w, c), dqkv=qkv.grad.cpu().reshape(b * h * w, 3 * c), dqkv_bias=bias.grad.cpu(),
                dtable=table.grad.cpu())


def main(argv):
    """`python -m tests.swin_edges_ref attn-bwd`: the attention backward of ATTN_SLOTS2 through WindowAttentionFn in THIS process
    (whose environment decides the kernel variant: YM_ATTN_BWD_SLOTS is read once per process); one JSON line
    {case: {tensor: [rel_err, rel_err of the fp32 CPU reference], 'finite': bool}}."""
    assert argv == ['attn-bwd'], argv
    res = {}
    for shape in ATTN_SLOTS2:
        got = run_attention_fn(attn_case(*shape), 'cuda:0')
        res['x'.join(map(str, shape))] = dict(attn_errors(got, attn_refs(*shape)),
                                              finite=all(bool(torch.isfinite(t).all()) for t in got.values()))
    print(json.dumps(res))


if __name__ == '__main__':
    main(sys.argv[1:])
