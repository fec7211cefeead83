"""Pins tests/train_ops_ref.py without a GPU: the float64 reference against torch's fp64 autograd (batch_norm, max_pool2d, interpolate,
optim.SGD), the -inf and NaN routing of the max-pool against ATen's CPU kernels, the geometry mirrors against what the library
answers on the host, and the preconditions every case table of tests/test_gpu_train_ops.py relies on."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import train_ops_ref as R

F64 = torch.float64


def _nchw(x):
    return torch.as_tensor(x).permute(0, 3, 1, 2)


def _nhwc(x):
    return x.permute(0, 2, 3, 1)


# ---- BatchNorm ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('residual,relu', [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize('m,c', [(1, 4), (37, 24), (338, 96), (19, 1536)])
def test_bn_reference_equals_torch_autograd(m, c, residual, relu):
    y, gamma, beta, res, dout, _ = (t.double() for t in R.bn_inputs(m, c, m + c))
    rm0, rv0 = torch.linspace(-1, 1, c, dtype=F64), torch.linspace(0.5, 2, c, dtype=F64)
    eps = float(np.float32(1e-5))
    leaves = [t.clone().requires_grad_(True) for t in (y, gamma, beta, res)]
    rm, rv = rm0.clone(), rv0.clone()
    if m > 1:
        z = F.batch_norm(leaves[0], rm, rv, leaves[1], leaves[2], True, 0.1, eps)
    else:                                   # (torch refuses one value per channel in training mode: the definition, spelled out)
        z = (leaves[0] - leaves[0].mean(0)) / torch.sqrt(leaves[0].var(0, unbiased=False) + eps) * leaves[1] + leaves[2]
    out = z + leaves[3] if residual else z
    out = torch.relu(out) if relu else out
    out.backward(dout)
    ref = R.bn_fwd(y, gamma, beta, 1e-5, 0.1, rm0, rv0, res if residual else None, relu)
    torch.testing.assert_close(ref['out'], out.detach(), rtol=1e-12, atol=1e-12)
    if m > 1:
        torch.testing.assert_close(ref['run_mean'], rm, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(ref['run_var'], rv, rtol=1e-12, atol=1e-12)
    else:
        torch.testing.assert_close(ref['run_var'], 0.9 * rv0, rtol=1e-15, atol=0)                   # M = 1 keeps the biased variance, 0
    mask = (out.detach() > 0) if relu else None
    dy, dres, dgamma, dbeta = R.bn_bwd(dout, y, ref['mean'], ref['invstd'], gamma, mask)
    torch.testing.assert_close(dy, leaves[0].grad, rtol=1e-9, atol=1e-9)
    torch.testing.assert_close(dgamma, leaves[1].grad, rtol=1e-9, atol=1e-9)
    torch.testing.assert_close(dbeta, leaves[2].grad, rtol=1e-9, atol=1e-9)
    if residual:
        torch.testing.assert_close(dres, leaves[3].grad, rtol=0, atol=0)
    # the sums over the kernel's float32 operands are the same sums to float32 rounding of xhat
    s = R.bn_bwd_sum_operands(dout.float(), y.float(), ref['mean'].float(), ref['invstd'].float(), mask)
    d2 = R.bn_bwd(dout.float(), y.float(), ref['mean'].float(), ref['invstd'].float(), gamma, mask)
    torch.testing.assert_close(s[0], d2[3], rtol=1e-12, atol=1e-9)
    torch.testing.assert_close(s[1], d2[2], rtol=1e-5, atol=1e-4)


def test_bn_reference_conditioning_channels():
    y = R.conditioning_input(501, 8, 7)
    ref = R.bn_fwd(y, torch.ones(8), torch.zeros(8), 1e-5)
    assert float(ref['var'][0]) == 0.0 and float(ref['mean'][0]) == 1.5
    assert float(ref['invstd'][0]) == 1.0 / float(np.float32(1e-5)) ** 0.5
    assert float(ref['mean'][1]) == 100.0                                    # exactly, by construction
    two_pass = y[:, 1].double().var(unbiased=False)
    assert abs(float(ref['var'][1]) / float(two_pass) - 1.0) < 1e-9          # E[x^2] - E[x]^2 in fp64 still has ten digits here
    assert abs(float(two_pass) ** 0.5 - 0.1) < 0.01
    assert bool((ref['out'][:, 0] == 0).all())


@pytest.mark.parametrize('act', [R.ACT_NONE, R.ACT_RELU, R.ACT_TANH])
def test_act_bias_reference_equals_torch_autograd(act):
    g = torch.Generator().manual_seed(act)
    pre = torch.randn(77, 352, generator=g, dtype=F64, requires_grad=True)
    bias = torch.randn(352, generator=g, dtype=F64, requires_grad=True)
    dy = torch.randn(77, 352, generator=g, dtype=F64)
    z = pre + bias
    y = z if act == R.ACT_NONE else (torch.relu(z) if act == R.ACT_RELU else torch.tanh(z))
    y.backward(dy)
    dz, dbias = R.act_bias_bwd(dy, y.detach(), act)
    torch.testing.assert_close(dz, pre.grad, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(dbias, bias.grad, rtol=1e-12, atol=1e-12)


# ---- max-pool -------------------------------------------------------------------------------------------------------------------
def _pool_against_aten(x, seed):
    b, h, w, c = x.shape
    dy = R.pool_grad(x, seed)
    xt = _nchw(x.double()).contiguous().requires_grad_(True)
    out_t, idx_t = F.max_pool2d(xt, 3, 2, 1, return_indices=True)
    out_t.backward(_nchw(dy.double()).contiguous())
    out_r, arg_r = R.maxpool_fwd(x)
    assert np.array_equal(out_r, _nhwc(out_t.detach()).numpy(), equal_nan=True)
    assert np.array_equal(R.maxpool_flat_index(arg_r, w), _nhwc(idx_t).numpy())
    dx_r = R.maxpool_bwd(arg_r, dy.numpy(), h, w)
    assert np.array_equal(dx_r, _nhwc(xt.grad).numpy())
    assert np.array_equal(dx_r.astype(np.float32).astype(np.float64), dx_r)              # exact in float32: sums of quarters
    return arg_r, dx_r


@pytest.mark.parametrize('shape', R.POOL_SHAPES, ids=lambda v: 'x'.join(map(str, v)))
def test_maxpool_reference_equals_aten(shape):
    x = R.pool_input(shape, sum(shape))
    assert bool((x >= 0).all())                                              # post-ReLU
    if shape != (1, 1, 1, 4):
        assert R.windows_with_ties(x) > 0
    if shape == (1, 3, 3, 4):
        assert float(x.min()) == float(x.max())
    _pool_against_aten(x, 1)


def test_maxpool_minus_infinity_window_goes_to_its_first_valid_element():
    x = R.pool_inf_input()
    assert bool(torch.isinf(R.window(x, 0, 0)).all()) and R.window(x, 0, 0).shape[1] == 4
    assert bool(torch.isinf(R.window(x, 2, 2)).all()) and R.window(x, 2, 2).shape[1] == 9
    arg, dx = _pool_against_aten(x, 2)
    assert bool((arg[:, 0, 0, :] == 4).all())                                # the border window: position 3*1+1, never the padding at 0
    assert bool((arg[:, 2, 2, :] == 0).all())                                # the interior window: its first element
    dy = R.pool_grad(x, 2).numpy()
    assert dy[0, 0, 0].any() and abs(dx.sum() - dy.sum()) < 1e-9             # no window's gradient is dropped


def test_maxpool_last_nan_of_a_window_wins():
    x = R.pool_nan_input()
    assert [int(torch.isnan(R.window(x, *w)[0, :, 0]).sum()) for w in ((0, 0), (2, 2), (0, 2))] == [1, 2, 3]
    arg, dx = _pool_against_aten(x, 3)
    assert bool((arg[:, 0, 0, :] == 3 * 2 + 1).all())                        # the one NaN at (1, 0)
    assert bool((arg[:, 2, 2, :] == 3 * 2 + 0).all())                        # (5, 3), the later of (3, 4) and (5, 3)
    assert bool((arg[:, 0, 2, :] == 3 * 2 + 2).all())                        # (1, 5), the last of three in a row
    dy = R.pool_grad(x, 3).numpy()
    assert np.isfinite(dx).all() and abs(dx.sum() - dy.sum()) < 1e-9         # every window's gradient lands once, on one element


# ---- bilinear x2 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('align', [False, True])
@pytest.mark.parametrize('shape', R.BILINEAR_SHAPES, ids=lambda v: 'x'.join(map(str, v)))
def test_bilinear_reference_equals_torch_autograd(shape, align):
    b, h, w, c = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=g, dtype=F64)
    dy = torch.randn(b, 2 * h, 2 * w, c, generator=g, dtype=F64)
    xt = _nchw(x).contiguous().requires_grad_(True)
    out = F.interpolate(xt, scale_factor=2, mode='bilinear', align_corners=align)
    out.backward(_nchw(dy).contiguous())
    np.testing.assert_allclose(R.bilinear2x_fwd(x.numpy(), align), _nhwc(out.detach()).numpy(), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(R.bilinear2x_bwd(dy.numpy(), align), _nhwc(xt.grad).numpy(), rtol=1e-12, atol=1e-13)


# ---- SGD, scatter3, head gather, dgrad image ----------------------------------------------------------------------------------
@pytest.mark.parametrize('wd,mom', [(5e-4, 0.9), (0.0, 0.9), (5e-4, 0.0)])
def test_sgd_reference_equals_torch_sgd(wd, mom):
    g = torch.Generator().manual_seed(1)
    lr = 0.01
    q = torch.nn.Parameter(torch.randn(257, generator=g, dtype=F64))
    p, buf = q.detach().clone(), torch.zeros(257, dtype=F64)
    opt = torch.optim.SGD([q], lr=float(np.float32(lr)), momentum=float(np.float32(mom)), weight_decay=float(np.float32(wd)))
    for step in range(4):
        gr = torch.randn(257, generator=g, dtype=F64)
        q.grad = gr.clone()
        opt.step()
        p, buf = R.sgd_step(p, gr, buf, lr, mom, wd, step == 0)
        torch.testing.assert_close(p, q.detach(), rtol=1e-14, atol=1e-15)


def test_scatter3_and_dgrad_image_references():
    src = torch.arange(12.0)
    a, b, c = torch.ones(5), torch.ones(0), torch.ones(7)
    out = R.scatter3(src, [a, b, c], False)
    assert torch.equal(torch.cat(out), src)
    out = R.scatter3(src, [a, b, c], True)
    assert torch.equal(torch.cat(out), src + 1)
    w = np.arange(35 * 5 * 9, dtype=np.float32).reshape(35, 5, 3, 3)
    img = R.dgrad_weight_image(w, 64)
    assert img.shape == (5, 3, 3, 64) and (img[..., 35:] == 0).all()
    assert img[2, 1, 0, 17] == w[17, 2, 1, 0]
    # the transposed filter it stands for: conv_transpose of dy with w == the data gradient
    assert np.array_equal(img[..., :35], np.einsum('oihw->ihwo', w))


def test_head_gather_reference_is_the_backward_of_the_head_layout():
    """Forward of the fused head: per level a [B][hw][pitch] conv output is cut into class / box / tanh(coefficient) blocks and the
    levels are concatenated along the anchors.  The reference must be autograd's gradient of that."""
    na, nc, cd, batch, pix, pitch = 3, 5, 4, 2, [6, 2, 1], 48
    g = torch.Generator().manual_seed(0)
    row, anchor = R.head_levels(batch, pix, na)
    z = torch.randn(row[-1], pitch, generator=g, dtype=F64, requires_grad=True)
    cls, box, coef = [], [], []
    for l, p in enumerate(pix):
        blk = z[row[l]:row[l + 1]].view(batch, p, pitch)
        cls.append(blk[:, :, :na * nc].reshape(batch, p * na, nc))
        box.append(blk[:, :, na * nc:na * (nc + 4)].reshape(batch, p * na, 4))
        coef.append(torch.tanh(blk[:, :, na * (nc + 4):na * (nc + 4 + cd)].reshape(batch, p * na, cd)))
    cls, box, coef = torch.cat(cls, 1), torch.cat(box, 1), torch.cat(coef, 1)
    assert cls.shape[1] == anchor[-1]
    dclass, dbox, dcoef = (torch.randn(t.shape, generator=g, dtype=F64) for t in (cls, box, coef))
    scale = torch.tensor([0.5, 2.0, 3.0], dtype=F64)
    (scale[0] * (cls * dclass).sum() + scale[1] * (box * dbox).sum() + scale[2] * (coef * dcoef).sum()).backward()
    ref = R.head_grad_gather(dclass, dbox, dcoef, coef.detach(), batch, pix, nc, cd, na, pitch, scale)
    torch.testing.assert_close(ref, z.grad, rtol=1e-13, atol=1e-14)
    assert bool((ref[:, na * (nc + 4 + cd):] == 0).all())


# ---- geometry mirrors and case tables -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('m,c', R.ALL_MC, ids=lambda v: str(v))
def test_workspace_mirror_equals_the_library(m, c):
    from yolact_minimal_amd import hip
    lib = hip.lib()
    assert lib.ym_bn_train_fwd_workspace_bytes(m, c) == R.stats_workspace_bytes(m, c)
    assert lib.ym_bn_train_bwd_workspace_bytes(m, c) == R.stats_workspace_bytes(m, c)
    assert R.bias_workspace_bytes(m, c) <= R.stats_workspace_bytes(m, c)     # "ym_bn_train_bwd_workspace_bytes always suffices"


def test_geometry_mirrors_on_known_points():
    assert R.lane_map(24) == dict(C4=6, CQ=6, RL=42, idle=4, passes=1, last_pass_empty=0)
    assert R.lane_map(96)['idle'] == 16 and R.lane_map(352)['idle'] == 80
    assert R.lane_map(1536)['passes'] == 2 and R.lane_map(1536)['last_pass_empty'] == 128
    assert R.stats_grid(338, 64, True) == -(-338 // 256) and R.stats_grid(10 ** 7, 256, True) == 1024
    assert R.stats_grid(8292, 1024, False) == 512 and R.stats_grid(8192, 1024, False) == 512 and R.stats_grid(8191, 1024, False) == 512
    assert R.stats_grid(8176, 1024, False) == 511
    assert R.bias_grid(65539, 1024, False) == 2048 and R.bias_grid(65536, 1024, False) == 2048 and R.bias_grid(32773, 1024, True) == 1024
    assert R.bn_apply_grid(1) == 2 and R.bn_apply_grid(3 * 1024) == 4 and R.bn_apply_grid(10 ** 9) == 8192
    assert [R.fwd_stats_geometry(8, c)['step'] for c in (64, 96, 28, 352, 268)] == [1, 3, 7, 11, None]
    assert R.col_finish_loops(48) == dict(main=0, remainder=3, empty_slice=False)
    assert R.col_finish_loops(49) == dict(main=1, remainder=3, empty_slice=False)      # slice 0: four at once; slice 1: three singly
    assert R.col_finish_loops(15)['empty_slice'] and R.col_finish_loops(1024) == dict(main=16, remainder=0, empty_slice=False)
    assert R.col_loops(17, 1024, 2, 4) == dict(main=2, remainder=1, strides=True, idle_lanes=0)
    assert R.quad_loops(4000, 1024) == {(1, 0), (0, 3)}


def test_case_tables_reach_their_branches():
    # every unrolled loop runs with and without a remainder somewhere in the unroll table, in each mode
    for mode, unroll, rows in ((0, 4, 16), (1, 2, 16), (2, 4, 32)):
        seen = set()
        for m, c in R.UNROLL_SHAPES:
            grid = R.col_grid(m, c, rows, 1024)
            lp = R.col_loops(m, c, grid, unroll)
            assert lp['main'] >= 1
            seen.add(lp['remainder'] > 0)
        assert seen == {False, True}, (mode, seen)
    # the caps
    assert R.stats_grid(8292, 1024, False) == 512 and R.stats_grid(16421, 1024, True) == 1024
    assert R.bias_grid(32773, 1024, True) == 1024 and R.bias_grid(65539, 1024, False) == 2048
    # backward apply: fixed_c true with both loops, false twice, and the large case past the cap
    geo = {mc: R.bwd_apply_geometry(*mc) for mc in R.BWD_APPLY_SHAPES}
    assert geo[(250, 64)]['fixed_c'] and geo[(250, 64)]['loops'] == {(1, 0), (0, 3)}
    assert not geo[(80, 96)]['fixed_c'] and not geo[(61, 24)]['fixed_c']
    m = R.bwd_apply_large_m(256)
    big = R.bwd_apply_geometry(m, 256)
    assert big['capped'] and big['loops'] == {(2, 0), (1, 3)} and m * 256 * 4 < 2 ** 28 and (m, 256) in R.OTHER_MC
    # fwd_stats: every step of the table, the fallback, the raised grid, both loops
    steps = {mc: R.fwd_stats_geometry(*mc) for mc in R.FWD_STATS_SHAPES}
    assert sorted(str(v['step']) for v in steps.values()) == sorted(['1', '3', '7', '11', 'None', '2', '1'])
    assert steps[(1, 2048)]['grid0'] == 1 and steps[(1, 2048)]['grid'] == 2
    assert steps[(250, 64)]['loops'] == {(2, 0), (1, 3)}
    # 256 * step is a multiple of C/4, so a grid rounded to the step always covers C/4 threads
    for c in range(4, 4100, 4):
        geo = R.fwd_stats_geometry(1, c)
        assert not geo['fused'] or geo['grid'] == -(-geo['grid0'] // geo['step']) * geo['step']


def test_relu_masks_take_both_values_in_every_channel():
    for m, c in R.LANE_SHAPES + R.UNROLL_SHAPES:
        out = R.bn_inputs(m, c, 1000 * m + c)[5]
        assert R.mask_takes_both_values(out), (m, c)
        if m > 1:
            assert bool((out > 0).any(0).all()) and bool((out == 0).any(0).all())
    for m, c in R.BWD_APPLY_SHAPES:                                          # there the mask is the forward's own output
        y, gamma, beta, _, _, _ = R.bn_inputs(m, c, 13 * m + c)
        out = R.bn_fwd(y, gamma, beta, 1e-5, relu=True)['out']
        assert R.mask_takes_both_values(out), (m, c)
