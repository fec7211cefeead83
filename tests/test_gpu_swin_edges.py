"""The Swin-T kernels (csrc/swin_ops.hip, csrc/swin_train.hip) at their window, grid and saturation edges, each launch against the
plain float64 reference of the same operation (tests/swin_edges_ref.py, pinned to torch and the oracle and to the launch code by
tests/test_swin_edges_cpu.py).

  LayerNorm       every channel count at which the kernels change variant or mask a lane group, 1 / 5 / 37 rows, a ragged second grid
                  pass of each variant forward and backward, 50 and 114 workgroups through `k_ln_param_grad`, degenerate rows
  patch merge     maps of one pixel, odd and even sizes (each padded quadrant pattern), 33124 rows
  GELU            a grid over [-12, 12] with signed zeros, denormals and the values where 1 + erff cancels; a ragged second pass
  DropPath, AdamW a sample boundary inside the second grid pass; 4096 * 256 + 3 parameters, gradients with zeros and 1e-20
  attention       maps smaller than a window, one window, one head, partial last forward workgroup, a second round of the backward
                  (45 windows x 24 heads, 363 windows x 3 heads), saturated logits with masked keys on top, YM_ATTN_BWD_SLOTS=2

Rules.  Every output or gradient buffer is a NaN-filled view in the middle of a larger allocation with 256 sentinel floats on
each side: afterwards the view is finite and the strips are bit-unchanged.  Launches that claim a fixed order run twice and must
be bit-equal.  Accuracy: rel_err(GPU) <= max(1e-6, k * rel_err(fp32 CPU reference)), both against fp64 of the same inputs, k = 4 for
per-row / per-element results and 8 for sums across rows or windows; both figures are printed per case (table:
docs/experiments.md, "Swin-T kernels at their edges").
"""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import swin_edges_ref as E

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -12345.5
PAD = 256


# ---- guarded buffers ---------------------------------------------------------------------------------------------------------
class Guarded:
    """A float32 buffer of `shape` in the middle of a larger allocation: NaN inside (or `init`), SENTINEL in the strips."""

    def __init__(self, shape, init=None):
        n = 1
        for s in shape:
            n *= s
        self.whole = torch.full((n + 2 * PAD,), SENTINEL, device=DEV)
        self.t = self.whole[PAD:PAD + n].view(shape)
        if init is None:
            self.t.fill_(float('nan'))
        else:
            self.t.copy_(init)

    def check(self, what):
        """All finite inside, both strips bit-unchanged; returns the buffer on the CPU."""
        strips = torch.cat([self.whole[:PAD], self.whole[-PAD:]]).cpu()
        assert torch.equal(strips, torch.full((2 * PAD,), SENTINEL)), f'{what}: a write outside the buffer'
        got = self.t.cpu()
        bad = int((~torch.isfinite(got)).sum())
        assert bad == 0, f'{what}: {bad} of {got.numel()} elements unwritten or not finite'
        return got


def _lib():
    from yolact_minimal_amd import hip
    return hip, hip.lib()


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _report(what, names, got, refs, ks):
    """Print rel_err of the GPU and of the fp32 CPU reference per tensor, then assert the bound."""
    ref64, ref32 = refs
    rows = []
    for n, g, r64, r32, k in zip(names, got, ref64, ref32, ks):
        rows.append((n, E.rel_err(g, r64), E.rel_err(r32, r64), k))
    print(f'{what}: ' + ', '.join(f'{n} gpu {e:.2e} cpu32 {c:.2e}' for n, e, c, _ in rows))
    for n, e, c, k in rows:
        assert e <= E.bound(c, k), f'{what} {n}: rel_err {e:.3e} > max({E.FLOOR:g}, {k:g} x {c:.3e})'


# ---- launches ----------------------------------------------------------------------------------------------------------------
def _layernorm(k, merge=False):
    """Forward and backward through the raw entry points into guarded buffers, each twice: (out, dx, dgamma, dbeta) on the CPU."""
    from yolact_minimal_amd.swin_train import _ln_ws
    hip, lib = _lib()
    x, g, b, dy = (k[n].to(DEV) for n in ('x', 'g', 'b', 'dy'))
    c = g.numel()
    runs = []
    for _ in range(2):
        out, dx, dg, db = Guarded(tuple(dy.shape)), Guarded(tuple(x.shape)), Guarded((c,)), Guarded((c,))
        ws = _ln_ws(x.device, c)
        if merge:
            bsz, h, w, cs = x.shape
            hip.patch_merge_layernorm(x, g, b, E.EPS, out.t)
            hip.check(lib.ym_patch_merge_layernorm_bwd(hip.ptr(dy), hip.ptr(x), bsz, h, w, cs, hip.ptr(g), E.EPS, hip.ptr(dx.t),
                                                       hip.ptr(dg.t), hip.ptr(db.t), _vp(ws), ws.numel(), hip.stream_ptr()), 'merge bwd')
        else:
            hip.layernorm(x, g, b, E.EPS, out.t)
            hip.check(lib.ym_layernorm_bwd(hip.ptr(dy), hip.ptr(x), hip.ptr(g), E.EPS, x.numel() // c, c, hip.ptr(dx.t), hip.ptr(dg.t),
                                           hip.ptr(db.t), _vp(ws), ws.numel(), hip.stream_ptr()), 'layernorm bwd')
        runs.append(tuple(t.check(n) for t, n in zip((out, dx, dg, db), ('out', 'dx', 'dgamma', 'dbeta'))))
    for a, r, n in zip(runs[0], runs[1], ('out', 'dx', 'dgamma', 'dbeta')):
        assert torch.equal(a, r), f'{n} differs between two launches'
    return runs[0]


LN_NAMES, LN_KS = ('out', 'dx', 'dgamma', 'dbeta'), (E.K_ROW, E.K_ROW, E.K_SUM, E.K_SUM)


# ---- 1. LayerNorm ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', E.LN_CHANNELS)
def test_layernorm_channel_counts(c):
    """C at the first and last value of each kernel variant (<= 128 half wave, <= 256 one wave, wider: 6 lane groups) and with a
    ragged last lane group (132, 260, 1532); 1, 5 and 37 rows (a lone row, idle row slots, more than one workgroup)."""
    for m in E.LN_ROWS:
        _report(f'layernorm {m} x {c}', LN_NAMES, _layernorm(E.ln_case(m, c)), E.ln_refs(m, c), LN_KS)


@pytest.mark.parametrize('m,c', E.LN_FWD_STRIDE + E.LN_BWD_STRIDE + E.LN_PARAM_GRAD)
def test_layernorm_grid_stride_and_param_grad(m, c):
    """M just over one grid pass of the forward (4096 / 4096 / 8192 workgroups) or of the backward (2048 workgroups: 2, 3 and 5
    iterations, `k_ln_param_grad` 32 unrolled trips), and M = 16 * 49 + 3 / 16 * 113 + 3: 50 and 114 workgroups, both sides of
    `b + 48 < blocks` and the remainder loop."""
    _report(f'layernorm {m} x {c}', LN_NAMES, _layernorm(E.ln_case(m, c)), E.ln_refs(m, c), LN_KS)


@pytest.mark.parametrize('c', E.LN_DEGENERATE)
def test_layernorm_degenerate_rows(c):
    """Constant rows (variance 0): the forward is beta bit for bit and dx is finite; all-zero rows; rows of 1000 + 0.01 randn, whose
    float32 statistics lose most of their digits on any device -- the fp32 CPU reference measures how many."""
    k = E.ln_case(48, c, True)
    got = _layernorm(k)
    assert torch.equal(got[0][[1, 2, 7, 8]], k['b'].expand(4, c))
    _report(f'layernorm degenerate 48 x {c}', LN_NAMES, got, E.ln_refs(48, c, True), LN_KS)
    ordinary = [i for i in range(48) if i not in (3, 9)]                     # the other rows are not excused by the two hard ones
    ref64, ref32 = E.ln_refs(48, c, True)
    for i, n in ((0, 'out'), (1, 'dx')):
        e, cpu = E.rel_err(got[i][ordinary], ref64[i][ordinary]), E.rel_err(ref32[i][ordinary], ref64[i][ordinary])
        print(f'  rows without the large-mean ones: {n} gpu {e:.2e} cpu32 {cpu:.2e}')
        assert e <= E.bound(cpu, E.K_ROW)


# ---- 2. patch-merge LayerNorm ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', E.MERGE_SHAPES + (E.MERGE_STRIDE,))
def test_patch_merge_layernorm(shape):
    """The 2 x 2 gather with its zero-padded quadrants (odd H, odd W, both, neither; a map of one pixel) and its scatter of dx: every
    real pixel written (NaN pre-fill), nothing outside; (1, 363, 363, 8) is 33124 rows, past one grid pass both ways."""
    _report(f'patch merge {shape}', LN_NAMES, _layernorm(E.merge_case(*shape), merge=True), E.merge_refs(*shape), LN_KS)


# ---- 3. GELU -----------------------------------------------------------------------------------------------------------------
def _gelu(k):
    hip, lib = _lib()
    z, dy = k['z'].to(DEV), k['dy'].to(DEV)
    runs = []
    for _ in range(2):
        out, dz = Guarded((z.numel(),)), Guarded((z.numel(),))
        hip.check(lib.ym_gelu_fwd(hip.ptr(z), hip.ptr(out.t), z.numel(), hip.stream_ptr()), 'ym_gelu_fwd')
        hip.check(lib.ym_gelu_bwd(hip.ptr(dy), hip.ptr(z), hip.ptr(dz.t), z.numel(), hip.stream_ptr()), 'ym_gelu_bwd')
        runs.append((out.check('gelu out'), dz.check('gelu dz')))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    return runs[0]


@pytest.mark.parametrize('which', ['grid', 'stride'])
def test_gelu(which):
    """grid: z over [-12, 12] with +-0, +-1e-30, denormals and the float32 values where 1 + erff first rounds to 0 and to 2 (far
    tails are compared in absolute terms against the tensor's scale, as rel_err does); stride: 4096 * 256 * 4 + 12 elements."""
    k = E.gelu_grid() if which == 'grid' else E.gelu_stride_case()
    got = _gelu(k)
    _report(f'gelu {which}', ('out', 'dz'), got, E.gelu_refs(which), (E.K_ROW, E.K_ROW))
    if which == 'grid':
        z = k['z']
        assert bool((got[0][z == 0] == 0).all()) and bool((got[1][z == 0] == 0.5).all())
        assert bool((got[0][z <= -6].abs() <= 1e-8).all()) and torch.equal(got[0][z >= 6], z[z >= 6])


# ---- 4. DropPath-add and AdamW -----------------------------------------------------------------------------------------------
def test_drop_path_sample_boundary_in_the_second_grid_pass():
    """B = 3, per_sample = 2,100,000: the boundary between samples 1 and 2 is float4 1,050,000, in the second grid pass and inside a
    workgroup.  Forward and dy bit-equal to the reference expression on the CPU, kept and dropped samples both present."""
    hip, lib = _lib()
    b, per = E.DROP_PATH
    gen = torch.Generator().manual_seed(11)
    res, y, dout = (torch.randn(b, per, generator=gen) for _ in range(3))
    keep = 1 - 0.3
    rnd = torch.tensor([0.9, 0.1, 0.5])                                      # floor(keep + rnd) = 1, 0, 1
    mask = (keep + rnd.reshape(b, 1)).floor_()
    assert mask.flatten().tolist() == [1.0, 0.0, 1.0]
    yc = y.clone().requires_grad_()
    want = res + yc.div(keep) * mask
    want.backward(dout)
    want, want_dy = want.detach(), yc.grad
    rg, yg, dg, rn = res.to(DEV), y.to(DEV), dout.to(DEV), rnd.to(DEV)
    runs = []
    for _ in range(2):
        out, dy = Guarded((b, per)), Guarded((b, per))
        hip.check(lib.ym_drop_path_add(hip.ptr(rg), hip.ptr(yg), hip.ptr(rn), keep, hip.ptr(out.t), b, per, hip.stream_ptr()), 'add')
        hip.check(lib.ym_drop_path_bwd(hip.ptr(dg), hip.ptr(rn), keep, hip.ptr(dy.t), b, per, hip.stream_ptr()), 'bwd')
        runs.append((out.check('drop_path out'), dy.check('drop_path dy')))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][0], want)
    assert torch.equal(runs[0][1], want_dy)


def test_adamw_past_the_grid_cap():
    """One flat parameter of 4096 * 256 + 3 elements (3 in the second grid pass), 3 steps with weight decay, gradients with exact
    zeros and 1e-20 (g * g is a denormal): the parameter against torch.optim.AdamW on the device at the bar of
    test_adamw_kernel_matches_torch, exp_avg likewise.  exp_avg_sq has a bar of its own: `k_adamw` forms 1 - beta2 in float32,
    1.f - 0.999f = 0.00099998713 (0.999f is 0.99900001287), where torch rounds the double 0.001, so every g * g term carries the same
    factor 1 - 1.29e-5 and so does their sum (measured: 1.30e-5 at worst, 10 of 1048579 elements past 2e-6 + 2e-7); through
    sqrt(v) that is 6.5e-6 of an update of about lr = 5e-3, 3e-8 on the parameter, inside its atol."""
    hip, lib = _lib()
    n = E.ADAMW_N
    gen = torch.Generator().manual_seed(13)
    p0 = torch.randn(n, generator=gen)
    q = torch.nn.Parameter(p0.to(DEV))
    ref = torch.optim.AdamW([q], lr=5e-3, weight_decay=0.05)
    state = [[Guarded((n,), init=p0.to(DEV)), Guarded((n,), init=torch.zeros(n, device=DEV)), Guarded((n,), init=torch.zeros(n, device=DEV))]
             for _ in range(2)]
    for step in range(1, 4):
        gr = torch.randn(n, generator=gen)
        gr[::7] = 0.0
        gr[3::7] = 1e-20
        gr[-3:] = torch.tensor([0.0, 1e-20, 1.5])                           # the three elements of the second pass
        gd = gr.to(DEV)
        q.grad = gd.clone()
        ref.step()
        for p, m, v in state:
            hip.check(lib.ym_adamw_step(hip.ptr(p.t), hip.ptr(gd), hip.ptr(m.t), hip.ptr(v.t), n, 5e-3, 0.9, 0.999, 1e-8, 0.05, step,
                                        hip.stream_ptr()), 'ym_adamw_step')
        got = [[t.check(nm) for t, nm in zip(s, ('param', 'exp_avg', 'exp_avg_sq'))] for s in state]
        for a, r in zip(got[0], got[1]):
            assert torch.equal(a, r)
        torch.testing.assert_close(got[0][0], q.detach().cpu(), rtol=2e-6, atol=2e-7)
        st = ref.state[q]
        torch.testing.assert_close(got[0][1], st['exp_avg'].cpu(), rtol=2e-6, atol=2e-7)
        torch.testing.assert_close(got[0][2], st['exp_avg_sq'].cpu(), rtol=1.29e-5 + 2e-6, atol=1e-12)
    assert bool((got[0][0][-3:] != p0[-3:]).all())                           # the tail was stepped (weight decay alone moves it)


# ---- 5. window attention -----------------------------------------------------------------------------------------------------
def _attention(case):
    """`hip.swin_window_attention` and `ym_swin_window_attention_bwd` into guarded buffers: {out, dqkv, dqkv_bias, dtable} on the CPU.
    The forward twice (fixed order); the backward ends in fp32 atomics for dtable / dqkv_bias, so it is not compared run to run."""
    hip, lib = _lib()
    b, h, w, heads, shift = case['shape']
    c = heads * 32
    qkv, bias, table, dout = (case[n].to(DEV) for n in ('qkv', 'qkv_bias', 'table', 'dout'))
    outs = []
    for _ in range(2):
        out = Guarded((b * h * w, c))
        hip.swin_window_attention(qkv, bias, table, b, h, w, c, heads, E.WS, shift, out.t)
        outs.append(out.check('attention out'))
    assert torch.equal(outs[0], outs[1])
    dqkv = Guarded((b * h * w, 3 * c))
    dbias, dtable = Guarded((3 * c,), init=torch.zeros(3 * c, device=DEV)), Guarded((169, heads), init=torch.zeros(169, heads, device=DEV))
    hip.check(lib.ym_swin_window_attention_bwd(hip.ptr(qkv), hip.ptr(bias), hip.ptr(table), hip.ptr(dout), b, h, w, c, heads, E.WS,
                                               shift, hip.ptr(dqkv.t), hip.ptr(dbias.t), hip.ptr(dtable.t), hip.stream_ptr()), 'attention bwd')
    return dict(out=outs[0].reshape(b, h, w, c), dqkv=dqkv.check('dqkv'), dqkv_bias=dbias.check('dqkv_bias'), dtable=dtable.check('dtable'))


def _check_attention(what, got, refs):
    errs = E.attn_errors(got, refs)
    print(f'{what}: ' + ', '.join(f'{n} gpu {e:.2e} cpu32 {c:.2e}' for n, (e, c) in errs.items()))
    for n, (e, c) in errs.items():
        assert e <= E.bound(c, E.ATTN_K[n]), f'{what} {n}: rel_err {e:.3e} > max({E.FLOOR:g}, {E.ATTN_K[n]:g} x {c:.3e})'


@pytest.mark.parametrize('shape', E.ATTN_CASES)
def test_window_attention_forward_and_backward(shape):
    """Every token's output row and dqkv row, the table gradient and the qkv-bias gradient that arrives through the padded tokens
    (exactly zero where nothing is padded).  1 x 1 and 1 x 9: maps smaller than a window (mostly bias-only tokens); 7 x 7 with one
    head: a single unit, with and without shift; 1, 6 and 1089 forward units leave the last workgroup partly idle; 45 windows x 24
    heads and 363 windows x 3 heads make some backward workgroups walk a second set of windows and others not."""
    _check_attention(f'attention {shape}', _attention(E.attn_case(*shape)), E.attn_refs(*shape))


@pytest.mark.parametrize('shape', E.ATTN_SATURATED)
def test_window_attention_saturated(shape):
    """q and k scaled until the fp64 logits pass 200 and, for some real query, a masked key (-100) still carries the largest softmax
    weight (tests/test_swin_edges_cpu.py asserts both): the max subtraction of the forward, the recomputed row max of the backward
    and the ADDITIVE mask all matter here."""
    case = E.attn_case(*shape, True)
    _check_attention(f'attention saturated {shape} (q, k x {case["qk_scale"]})', _attention(case), E.attn_refs(*shape, True))


def test_autograd_functions_run_the_same_kernels():
    """LayerNormFn, PatchMergeLNFn, GeluFn and WindowAttentionFn against the raw launches above on one small case each: bit-equal
    where the order is fixed, within the attention bounds otherwise."""
    from yolact_minimal_amd.swin_train import GeluFn, LayerNormFn, PatchMergeLNFn
    for fn, k, merge in ((LayerNormFn, E.ln_case(37, 132), False), (PatchMergeLNFn, E.merge_case(2, 7, 9, 132), True)):
        x, g, b = (k[n].to(DEV).requires_grad_() for n in ('x', 'g', 'b'))
        out = fn.apply(x, g, b, E.EPS)
        out.backward(k['dy'].to(DEV))
        for a, r in zip((out.detach(), x.grad, g.grad, b.grad), _layernorm(k, merge)):
            assert torch.equal(a.cpu().reshape(r.shape), r)
    k = E.gelu_grid()
    z = k['z'].to(DEV).requires_grad_()
    out = GeluFn.apply(z)
    out.backward(k['dy'].to(DEV))
    raw = _gelu(k)
    assert torch.equal(out.detach().cpu(), raw[0]) and torch.equal(z.grad.cpu(), raw[1])
    shape = (1, 6, 8, 3, 3)
    got = E.run_attention_fn(E.attn_case(*shape), DEV)
    raw = _attention(E.attn_case(*shape))
    assert torch.equal(got['out'], raw['out']) and torch.equal(got['dqkv'], raw['dqkv'])
    _check_attention('WindowAttentionFn (1, 6, 8, 3, 3)', got, E.attn_refs(*shape))


# ---- 6. YM_ATTN_BWD_SLOTS=2 --------------------------------------------------------------------------------------------------
def test_attention_backward_with_two_slots_in_a_child_process():
    """The 256-thread / 72 KB instantiation of the attention backward: the setting is read once per process, so a fresh child
    (`python -m tests.swin_edges_ref attn-bwd`) runs (1, 6, 8, 3, 3) and (3, 29, 21, 24, 3) (45 windows > 42 per round) with
    YM_ATTN_BWD_SLOTS=2 and prints its rel_err figures; the bounds are those of the default build."""
    env = dict(os.environ, YM_ATTN_BWD_SLOTS='2')
    r = subprocess.run([sys.executable, '-m', 'tests.swin_edges_ref', 'attn-bwd'], cwd=REPO, env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert set(res) == {'x'.join(map(str, s)) for s in E.ATTN_SLOTS2}
    for name, errs in res.items():
        assert errs.pop('finite'), name
        print(f'2 slots {name}: ' + ', '.join(f'{n} gpu {e:.2e} cpu32 {c:.2e}' for n, (e, c) in errs.items()))
        assert set(errs) == set(E.ATTN_NAMES)
        for n, (e, c) in errs.items():
            assert e <= E.bound(c, E.ATTN_K[n]), f'2 slots {name} {n}: rel_err {e:.3e} > max({E.FLOOR:g}, {E.ATTN_K[n]:g} x {c:.3e})'
