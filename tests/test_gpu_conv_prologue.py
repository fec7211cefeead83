"""The conv kernels' argument blocks and prologues at the smallest shapes at which they can go wrong: the wave kernels' own 256-byte
argument block (WaveArgs) with its 1x1 / stride-1 / unpadded fast path, the epilogue operands requested ahead of the K loop, the
tail split, the scalar epilogue's segments (a second kernel argument), and the reordered ConvP of the workgroup kernels (hot block
first, the training groups behind it).  Launches go through tests.test_gpu_ops.run_conv (the same descriptor fields); the reference
is that file's fp64 host convolution at its wave-parity tolerance (rtol 1e-4, atol 1e-5: fp32 accumulation order only).  Every case
runs twice and the two results must be bit-equal."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_ops import _dev, ref_conv, run_conv

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _data(b, cin, h, w, cout, k, stride, pad):
    """Seeded operands of one shape (shared by every epilogue / kernel variant of that shape; never modified)."""
    g = torch.Generator().manual_seed(1000 * cin + 100 * cout + 10 * h + w + b + 7 * k + 3 * stride + pad)
    x = torch.randn(b, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, k, k, generator=g) * (1.0 / (cin * k * k) ** 0.5)
    scale = torch.rand(cout, generator=g) + 0.5
    shift = torch.randn(cout, generator=g) * 0.1
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    res = torch.randn(b, cout, ho, wo, generator=g)
    return x, wt, scale, shift, res


def _check(shape, act=1, use=(True, True, True), **launch):
    """shape = (b, cin, h, w, cout, k, stride, pad); use = (scale, shift, residual) present."""
    k, stride, pad = shape[5:]
    x, wt, scale, shift, res = _data(*shape)
    scale, shift, res = (t if on else None for t, on in zip((scale, shift, res), use))
    got = run_conv(x, wt, scale, shift, res, stride, pad, act, **launch)
    want = ref_conv(x, wt, scale, shift, res, stride, pad, act)
    assert not torch.isnan(got).any()
    torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-5)
    again = run_conv(x, wt, scale, shift, res, stride, pad, act, **launch)
    assert torch.equal(got, again)


# ---- wave-DMA rings: the 1x1 fast path against the borders of M and N -------------------------------------------------------------
# M = 25 (one partial 32-row tile), 36 (32 + 4), 2 x 25 (an image boundary inside a tile); Cout = 40 / 72: rows parked past Cout
@pytest.mark.parametrize('stages', [22, 23])
@pytest.mark.parametrize('cout', [40, 72])
@pytest.mark.parametrize('b,hw', [(1, 5), (1, 6), (2, 5)])
def test_wave_dma_fast_1x1_m_and_n_borders(b, hw, cout, stages):
    _check((b, 64, hw, hw, cout, 1, 1, 0), tile=(32, 32), kwaves=2, stages=stages)


# ---- ... against short K: one K tile (shorter than the ring), three K tiles for four K waves (a wave without a tile) ----------------
@pytest.mark.parametrize('stages', [22, 23])
@pytest.mark.parametrize('cin,kwaves', [(32, 1), (32, 4), (96, 4)])
def test_wave_dma_fast_1x1_short_k(cin, kwaves, stages):
    _check((1, cin, 6, 6, 40, 1, 1, 0), tile=(32, 32), kwaves=kwaves, stages=stages)


# ---- the general path where it is needed: a stride, a border, filter taps ---------------------------------------------------------
@pytest.mark.parametrize('stages', [22, 23])
@pytest.mark.parametrize('hw,k,stride,pad', [(7, 1, 2, 0), (5, 1, 1, 1), (5, 3, 1, 1), (7, 3, 1, 1), (5, 3, 2, 1), (7, 3, 2, 1)])
def test_wave_dma_general_path_still_taken(hw, k, stride, pad, stages):
    _check((1, 64, hw, hw, 40, k, stride, pad), tile=(32, 32), kwaves=2, stages=stages)


# ---- epilogue operands requested ahead of the K loop: null pointers mean "none" ---------------------------------------------------
EPILOGUE_LAUNCHES = [
    dict(tile=(32, 32), kwaves=4, stages=22),
    dict(tile=(32, 32), kwaves=1, stages=22, grid_wgs=1),          # one wave = one tile = one workgroup
    dict(tile=(64, 32), kwaves=2, stages=23),
]


@pytest.mark.parametrize('launch', EPILOGUE_LAUNCHES, ids=['kw4', 'kw1_wpb1', '64x32_kw2'])
@pytest.mark.parametrize('act', [1, 0])
@pytest.mark.parametrize('use_res', [False, True])
@pytest.mark.parametrize('use_shift', [False, True])
@pytest.mark.parametrize('use_scale', [False, True])
def test_wave_dma_epilogue_operand_combinations(use_scale, use_shift, use_res, act, launch):
    _check((1, 64, 6, 6, 40, 1, 1, 0), act, (use_scale, use_shift, use_res), **launch)


# ---- tail split: the last arriver's epilogue, counters handed back at zero -------------------------------------------------------
def test_wave_dma_tail_split_leaves_counters_at_zero():
    from yolact_minimal_amd import hip
    counters = torch.zeros(hip.TILE_COUNTERS, device=_dev(), dtype=torch.int32)
    # M = 96, Cout = 64, Cin = 256: 3 x 2 tiles, the last two as two K slices each; _check runs it twice on the same counters
    _check((1, 256, 8, 12, 64, 1, 1, 0), tile=(32, 32), kwaves=4, stages=22, counters=counters, tail=(2, 2))
    assert int(counters.abs().sum()) == 0
    _check((1, 256, 8, 12, 64, 1, 1, 0), 0, (False, True, False), tile=(32, 32), kwaves=4, stages=22, counters=counters, tail=(2, 2))
    assert int(counters.abs().sum()) == 0


# ---- scalar epilogue (Cout % 4 != 0): the segment table is the kernels' second argument ------------------------------------------
@pytest.mark.parametrize('k,pad,stages,kwaves', [(1, 0, 22, 2), (3, 1, 23, 4), (1, 0, 0, 2)])
def test_wave_non_vector_epilogue(k, pad, stages, kwaves):
    _check((2, 64, 5, 5, 30, k, 1, pad), tile=(32, 32), kwaves=kwaves, stages=stages)


# ---- the register-ring wave kernel shares the argument block (and its 1x1 branch) ---------------------------------------------------
@pytest.mark.parametrize('shape', [(2, 64, 5, 5, 40, 1, 1, 0), (1, 96, 6, 6, 72, 1, 1, 0), (1, 64, 7, 7, 40, 1, 2, 0), (1, 64, 5, 5, 40, 1, 1, 1),
                                   (1, 64, 7, 7, 40, 3, 2, 1)])
@pytest.mark.parametrize('tile,kwaves', [((32, 32), 4), ((64, 64), 1)])
def test_wave_register_ring_kernel(shape, tile, kwaves):
    _check(shape, tile=tile, kwaves=kwaves)


# ---- workgroup kernels (conv_igemm_f32: register double buffer, direct-to-LDS ring, pipelined fragments; the persistent walker):
# the same M, N and K edges at 64x64, once each, on the reordered ConvP -------------------------------------------------------------
WG_SHAPES = [
    (1, 64, 5, 5, 40, 1, 1, 0),       # M = 25, Cout = 40
    (2, 32, 6, 6, 72, 1, 1, 0),       # M = 72 = 64 + 8 (an image boundary inside a tile), Cout = 64 + 8, one K tile
    (1, 96, 6, 6, 40, 1, 1, 0),       # three K tiles
    (1, 64, 7, 7, 40, 1, 2, 0),       # 1x1 stride 2
    (1, 64, 5, 5, 40, 1, 1, 1),       # 1x1 with a border
    (1, 64, 5, 5, 72, 3, 1, 1),
    (1, 64, 7, 7, 40, 3, 2, 1),
]


@pytest.mark.parametrize('stages', [2, 22, 34, 43])
@pytest.mark.parametrize('shape', WG_SHAPES)
def test_workgroup_kernels_edges(shape, stages):
    _check(shape, tile=(64, 64), ksplit=1, stages=stages)


def test_training_launch_still_receives_its_batchnorm_sums():
    """One train-mode conv + BatchNorm through the training binding: the launch carries `bn_sum` / `bn_sumsq` (ConvP's cold block);
    output and running statistics against torch's train-mode batch_norm, at the bounds of tests/test_gpu_train.py."""
    from yolact_minimal_amd.train_engine import ConvBn
    g = torch.Generator().manual_seed(11)
    cin, cout, k, hw = 64, 64, 3, 14
    x = torch.randn(3, cin, hw, hw, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) * (1 / (cin * k * k) ** 0.5)
    gamma, beta = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
    rm, rv = torch.randn(cout, generator=g) * 0.1, torch.rand(cout, generator=g) + 0.5
    rmc, rvc = rm.clone(), rv.clone()
    y = F.relu(F.batch_norm(F.conv2d(x, w, None, 1, 1), rmc, rvc, gamma, beta, True, 0.1, 1e-5))
    dev = _dev()
    rmg, rvg = rm.to(dev), rv.to(dev)
    xg = x.permute(0, 2, 3, 1).contiguous().to(dev)
    with torch.no_grad():
        yg = ConvBn.apply(xg, w.to(dev), gamma.to(dev), beta.to(dev), rmg, rvg, None, 1, 1, True, 0.1, 1e-5)
    torch.testing.assert_close(yg.permute(0, 3, 1, 2).cpu(), y, rtol=1e-4, atol=2e-5)
    torch.testing.assert_close(rmg.cpu(), rmc, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(rvg.cpu(), rvc, rtol=1e-5, atol=1e-6)
