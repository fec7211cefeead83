"""tests/swin_edges_ref.py against torch and oracle/yolact_ref.py, without a GPU: the references of tests/test_gpu_swin_edges.py are
checked here, and so is the claim of every case in its tables that it reaches the launch edge it is named for.  The float32 CPU
reference's own distance from float64 (the yardstick of the GPU bounds) is printed per case."""
import pytest
import torch
import torch.nn.functional as F

from oracle import yolact_ref as R
from tests import swin_edges_ref as E


def _agree(a, b, tol=1e-12):
    assert E.rel_err(a, b) <= tol, E.rel_err(a, b)


# ---- the references in fp64 against torch ----------------------------------------------------------------------------------------
def test_layernorm_ref_is_torch_layer_norm_in_fp64():
    k = E.ln_case(37, 132)
    x, g, b = (k[n].double().requires_grad_() for n in ('x', 'g', 'b'))
    F.layer_norm(x, (132,), g, b, E.EPS).backward(k['dy'].double())
    got = E.layernorm_ref(k['x'], k['g'], k['b'], E.EPS, torch.float64, k['dy'])
    for a, r in zip(got, (F.layer_norm(x, (132,), g, b, E.EPS), x.grad, g.grad, b.grad)):
        _agree(a, r)
    _agree(E.layernorm_ref(k['x'], k['g'], k['b'], E.EPS, torch.float64), got[0], 0.0)
    assert got[0].dtype == torch.float64 and E.ln_refs(37, 132)[1][0].dtype == torch.float32


def test_patch_merge_ref_is_layer_norm_of_the_gathered_quadrants():
    """Odd H and W: the gather written out with explicit zero padding, then torch's layer_norm and autograd."""
    k = E.merge_case(2, 7, 9, 132)
    x, g, b = (k[n].double().requires_grad_() for n in ('x', 'g', 'b'))
    xp = F.pad(x, (0, 0, 0, 1, 0, 1))
    cat = torch.cat([xp[:, 0::2, 0::2], xp[:, 1::2, 0::2], xp[:, 0::2, 1::2], xp[:, 1::2, 1::2]], -1)
    want = F.layer_norm(cat, (528,), g, b, E.EPS)
    want.backward(k['dy'].double())
    got = E.patch_merge_ln_ref(k['x'], k['g'], k['b'], torch.float64, k['dy'])
    assert got[0].shape == (2, 4, 5, 528)
    for a, r in zip(got, (want, x.grad, g.grad, b.grad)):
        _agree(a, r)


def test_gelu_ref_is_torch_gelu_in_fp64():
    k = E.gelu_grid()
    z = k['z'].double().requires_grad_()
    F.gelu(z).backward(k['dy'].double())
    out, dz = E.gelu_ref(k['z'], torch.float64, k['dy'])
    _agree(out, F.gelu(z), 1e-15)
    _agree(dz, z.grad, 1e-15)


@pytest.mark.parametrize('h,w,heads,shift', [(6, 8, 3, 3), (10, 12, 2, 3), (14, 7, 3, 0)])
def test_attention_ref_is_the_attention_part_of_the_oracle_block(h, w, heads, shift):
    """`R.swin_block` with fc2 = 0 (the MLP adds nothing) and proj = identity is x + attention(norm1(x)); the same from
    `attention_ref` fed the qkv Linear's output: value and the gradients of qkv's input side (through the Linear), the qkv bias
    (Linear share + padded-token share) and the table."""
    b, c = 2, heads * 32
    gen = torch.Generator().manual_seed(h * w + heads)
    sd = {'b.norm1.weight': torch.rand(c, generator=gen) + 0.5, 'b.norm1.bias': torch.randn(c, generator=gen),
          'b.attn.qkv.weight': torch.randn(3 * c, c, generator=gen) * c ** -0.5, 'b.attn.qkv.bias': torch.randn(3 * c, generator=gen),
          'b.attn.proj.weight': torch.eye(c), 'b.attn.proj.bias': torch.zeros(c),
          'b.attn.relative_position_bias_table': torch.randn(169, heads, generator=gen),
          'b.norm2.weight': torch.ones(c), 'b.norm2.bias': torch.zeros(c), 'b.mlp.fc1.weight': torch.randn(8, c, generator=gen),
          'b.mlp.fc1.bias': torch.zeros(8), 'b.mlp.fc2.weight': torch.zeros(c, 8), 'b.mlp.fc2.bias': torch.zeros(c)}
    sd = {n: v.double().requires_grad_() for n, v in sd.items()}
    sd['b.attn.relative_position_index'] = R.swin_rel_index(7)
    x = torch.randn(b, h * w, c, generator=gen).double()
    dout = torch.randn(b, h, w, c, generator=gen).double()
    hp, wp = -(-h // 7) * 7, -(-w // 7) * 7
    want = R.swin_block(x, h, w, sd, 'b', heads, 7, shift, R.swin_shift_mask(hp, wp, 7, 3).double()) - x
    want.backward(dout.reshape(b, h * w, c))
    wq, bq, table = sd['b.attn.qkv.weight'], sd['b.attn.qkv.bias'], sd['b.attn.relative_position_bias_table']
    with torch.no_grad():
        qkv = F.linear(F.layer_norm(x, (c,), sd['b.norm1.weight'], sd['b.norm1.bias'], 1e-5), wq, bq).reshape(b * h * w, 3 * c)
    out, dqkv, dbias_pad, dtable = E.attention_ref(qkv, bq, table, b, h, w, heads, shift, torch.float64, dout)
    _agree(out.reshape(b, h * w, c), want.detach())
    _agree(dtable, table.grad)
    _agree(dqkv.sum(0) + dbias_pad, bq.grad)                  # the Linear's bias gradient is the column sum of dqkv
    xn = F.layer_norm(x, (c,), sd['b.norm1.weight'], sd['b.norm1.bias'], 1e-5).reshape(b * h * w, c)
    _agree(dqkv.t() @ xn.detach(), wq.grad)
    assert (float(dbias_pad.abs().max()) > 0) == (hp * wp > h * w)
    assert qkv.grad is None and out.dtype == torch.float64


# ---- every case reaches its edge -------------------------------------------------------------------------------------------------
def test_layernorm_tables_cover_every_variant_boundary():
    assert set(E.LN_CHANNELS) >= {4, 128, 132, 256, 260, 1532, 1536}       # first / last C of each variant, a ragged last lane group
    assert all(c % 4 == 0 and c <= 1536 for c in E.LN_CHANNELS)
    for m in E.LN_ROWS:
        for c in E.LN_CHANNELS:
            assert E.ln_fwd_launch(m, c)[1] >= m                            # one forward pass
    assert E.ln_bwd_launch(5, 384) == (1, 4) and E.ln_bwd_launch(37, 1536) == (3, 12)     # wide rows: the backward loops already here
    assert [E.ln_fwd_launch(37, c)[0] for c in (128, 256, 260)] == [2, 3, 10]


@pytest.mark.parametrize('m,c', E.LN_FWD_STRIDE)
def test_layernorm_forward_stride_cases_make_a_ragged_second_pass(m, c):
    blocks, per_pass = E.ln_fwd_launch(m, c)
    assert blocks == (4096 if c <= 256 else 8192) and per_pass < m < 2 * per_pass
    # the second pass is shorter than one unrolled row group of a single workgroup: its `m < M` guards are false for most rows
    assert (m - per_pass) < per_pass // 4


@pytest.mark.parametrize('m,c', E.LN_BWD_STRIDE)
def test_layernorm_backward_stride_cases_make_ragged_further_passes(m, c):
    blocks, per_pass = E.ln_bwd_launch(m, c)
    assert blocks == 2048 and per_pass == {96: 32768, 192: 16384, 384: 8192}[c] and m > per_pass and m % per_pass == 37
    trips, read = E.ln_param_grad_trips(blocks)
    assert trips == [(32, 0)] * 16 and read == blocks


def test_param_grad_cases_take_both_sides_of_the_unrolled_condition():
    for m, c in E.LN_PARAM_GRAD:
        blocks, per_pass = E.ln_bwd_launch(m, c)
        trips, read = E.ln_param_grad_trips(blocks)
        assert read == blocks                                                # every partial row exactly once
        if m == 16 * 49 + 3:
            assert blocks == 50 and trips == [(1, 0)] * 2 + [(0, 3)] * 14
        else:
            assert blocks == 114 and trips == [(2, 0)] * 2 + [(1, 3)] * 14
    assert {c for _, c in E.LN_PARAM_GRAD} == {96, 192, 384}


def test_degenerate_rows_are_what_they_claim():
    for c in E.LN_DEGENERATE:
        k = E.ln_case(48, c, True)
        assert bool((k['x'][[1, 7]] == 0.5).all()) and bool((k['x'][[2, 8]] == 0).all())
        assert bool(((k['x'][[3, 9]] - 1000).abs() < 0.1).all()) and float(k['x'][3].std()) > 1e-3
        assert bool((k['g'] == 0).any()) and bool((k['g'] < 0).any())
        out64 = E.ln_refs(48, c, True)[0][0]
        assert float((out64[[1, 2, 7, 8]] - k['b'].double()).abs().max()) == 0.0       # constant rows: beta exactly
        assert bool(torch.isfinite(torch.stack([t.abs().max() for t in E.ln_refs(48, c, True)[0]])).all())


def test_patch_merge_cases():
    for b, h, w, c in E.MERGE_SHAPES:
        m, blocks, per_pass = E.merge_fwd_launch(b, h, w)
        assert m <= per_pass and c % 4 == 0 and 4 * c <= 1536
    assert {(h % 2, w % 2) for _, h, w, _ in E.MERGE_SHAPES} == {(0, 0), (0, 1), (1, 0), (1, 1)}       # each padded quadrant pattern
    b, h, w, c = E.MERGE_STRIDE
    m, blocks, per_pass = E.merge_fwd_launch(b, h, w)
    assert m == 33124 and blocks == 8192 and per_pass == 32768 < m and h % 2 and w % 2
    bb, bper = E.ln_bwd_launch(m, 4 * c, merge=True)
    assert bb == 2048 and bper == 8192 and m % bper


def test_gelu_grid_holds_the_specials_and_the_thresholds():
    z = E.gelu_grid()['z']
    assert z.numel() % 4 == 0 and float(z.min()) == -12 and float(z.max()) == 12
    assert bool(((z == 0) & torch.signbit(z)).any()) and bool(((z == 0) & ~torch.signbit(z)).any())
    tiny = z[(z != 0) & (z.abs() < 2.0 ** -126)]
    assert tiny.numel() >= 4 and float(tiny.abs().min()) == 2.0 ** -149       # denormals survive the table
    lo, zero, _, below, two, _ = E.gelu_thresholds()
    s = torch.tensor(0.70710678118654752440)
    one_plus = lambda v: float(1.0 + torch.erf(torch.tensor(v, dtype=torch.float32) * s))
    assert one_plus(lo) > 0 and one_plus(zero) == 0 and one_plus(below) < 2 and one_plus(two) == 2
    for v in (lo, zero, below, two):
        assert bool((z == v).any())
    out64, dz64 = E.gelu_refs('grid')[0]
    assert float(out64[z == zero][0]) < 0 and float(dz64[z == zero][0]) < 0   # the true values there are tiny, not zero


def test_elementwise_stride_cases():
    blocks, per_pass = E.elementwise_launch(E.GELU_STRIDE_N // 4)
    assert E.GELU_STRIDE_N % 4 == 0 and blocks == 4096 and E.GELU_STRIDE_N // 4 - per_pass == 3
    b, per = E.DROP_PATH
    blocks, per_pass = E.elementwise_launch(b * per // 4)
    edge = (b - 1) * per // 4                                               # float4 index of the last sample boundary
    assert per % 4 == 0 and blocks == 4096 and per_pass < edge < b * per // 4 and edge % 256 != 0 and (per // 4) % 256 != 0
    blocks, per_pass = E.elementwise_launch(E.ADAMW_N)
    assert blocks == 4096 and E.ADAMW_N - per_pass == 3


def test_attention_cases_reach_their_edges():
    units = {s: E.attn_fwd_units(*s[:4]) for s in E.ATTN_CASES}
    assert units[(1, 1, 9, 3, 3)] == 6 and units[(3, 75, 73, 3, 3)] == 1089
    assert sum(u % 4 != 0 for u in units.values()) >= 6                      # partial last forward workgroup
    for slots in (4, 2):
        nwin, per_round = E.attn_bwd_launch(3, 29, 21, 24, slots)
        assert nwin == 45 and per_round == (40 if slots == 4 else 42) and nwin % 4 == 1
        nwin, per_round = E.attn_bwd_launch(3, 75, 73, 3, slots)
        assert nwin == 363 and per_round == 340 and nwin % 4 == 3
    for s in E.ATTN_CASES[:6]:
        nwin, per_round = E.attn_bwd_launch(*s[:4])
        assert nwin <= 2 and per_round == 4                                  # one workgroup per head, idle slots
    assert set(E.ATTN_SATURATED) <= set(E.ATTN_CASES) and set(E.ATTN_SLOTS2) <= set(E.ATTN_CASES)
    # maps smaller than a window, a single window with and without shift, one head, batch 1, exact multiples
    assert {(1, 1, 1, 1, 3), (1, 7, 7, 1, 3), (1, 7, 7, 1, 0), (1, 14, 7, 3, 3)} <= set(E.ATTN_CASES)


@pytest.mark.parametrize('shape', E.ATTN_CASES)
def test_attention_case_references(shape):
    b, h, w, heads, shift = shape
    ref64, ref32 = E.attn_refs(*shape)
    assert all(bool(torch.isfinite(t).all()) for t in ref64)
    padded = (-(-h // 7) * 7) * (-(-w // 7) * 7) > h * w
    assert (float(ref64[2].abs().max()) > 0) == padded                      # the padded tokens' share of the qkv-bias gradient
    print(shape, 'fp32 CPU reference vs fp64:', {n: f'{E.rel_err(a, r):.2e}' for n, a, r in zip(E.ATTN_NAMES, ref32, ref64)})


@pytest.mark.parametrize('shape', E.ATTN_SATURATED)
def test_saturated_attention_cases_saturate(shape):
    case = E.attn_case(*shape, True)
    peak, on_masked, finite = E.saturation_facts(case)
    print(shape, f'q, k scaled by {case["qk_scale"]}: max |logit| {peak:.1f}, {on_masked} real queries with the largest weight on a '
          f'masked key')
    assert peak > 40 and on_masked >= 1 and finite
    ref64, ref32 = E.attn_refs(*shape, True)
    assert all(bool(torch.isfinite(t).all()) for t in ref64)
    # removing the masked keys instead of adding -100 to them is a different function here
    k = case
    logits, mask, real = E.attention_logits(k['qkv'], k['qkv_bias'], k['table'], *shape)
    p_add = F.softmax(logits + mask, -1)
    p_drop = F.softmax(logits.masked_fill(mask.expand_as(logits) < 0, float('-inf')), -1)
    assert float((p_add - p_drop).abs().max()) > 0.5
    print(shape, 'fp32 CPU reference vs fp64:', {n: f'{E.rel_err(a, r):.2e}' for n, a, r in zip(E.ATTN_NAMES, ref32, ref64)})


def test_cpu_fp32_reference_errors_of_the_row_kernels():
    """The yardstick of the GPU bounds, printed: fp32 CPU reference against fp64 per tensor."""
    for m, c in ((37, 96), (37, 1532), (787, 192)):
        ref64, ref32 = E.ln_refs(m, c)
        errs = [E.rel_err(a, r) for a, r in zip(ref32, ref64)]
        print('layernorm', (m, c), [f'{e:.2e}' for e in errs])
        assert max(errs) < 1e-5
    ref64, ref32 = E.ln_refs(48, 96, True)
    print('layernorm degenerate', [f'{E.rel_err(a, r):.2e}' for a, r in zip(ref32, ref64)])
    ref64, ref32 = E.gelu_refs('grid')
    errs = [E.rel_err(a, r) for a, r in zip(ref32, ref64)]
    print('gelu grid', [f'{e:.2e}' for e in errs])
    assert max(errs) < 1e-6
