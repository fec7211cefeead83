"""Ordered BatchNorm sums (ym_conv_desc.bn_ordered, ym_bn_partials_finish, train_engine._DETERMINISTIC): the conv epilogues store
per-row partial sums instead of issuing fp64 atomics, one finish launch adds the rows in a documented order, and a training step
in that mode enqueues no launch whose sums depend on the order in which workgroups retire -- so two trainings end bit-identical.

The finish order, restated here in numpy (`finish_np`) exactly as include/yolact_hip.h words it: per term and channel, slice s
(0..15) adds the rows k = s, s + 16, ... in ascending k starting from 0.0, then the 16 slice sums are added in ascending s starting
from 0.0.  IEEE fp64 additions on both sides, so the comparison is bit for bit."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from oracle import yolact_ref as R
from tests.test_gpu_train import _oracle_grads, _rel_err, _grad_sample
from yolact_minimal_amd.config import build_cfg
from yolact_minimal_amd.modules.yolact import Yolact

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 3            # rows behind the partial buffer that a launch must leave alone


@pytest.fixture(autouse=True)
def _restore_switch():
    """The switch is process-wide: whatever a test chose, the tests after it see the default again."""
    from yolact_minimal_amd import train_engine as T
    before = T._DETERMINISTIC
    yield
    T._DETERMINISTIC = before
    T.tuned_table_changed()


def finish_np(part):
    """part [rows][2][C] float64 -> [2][C]: the order of ym_bn_partials_finish."""
    rows = part.shape[0]
    total = np.zeros(part.shape[1:], np.float64)
    for s in range(16):
        acc = np.zeros(part.shape[1:], np.float64)
        for k in range(s, rows, 16):
            acc = acc + part[k]
        total = total + acc
    return total


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _finish(part, rows, c):
    from yolact_minimal_amd import hip
    sums = torch.full((2, c), float('nan'), dtype=torch.float64, device=DEV)
    hip.check(hip.lib().ym_bn_partials_finish(ctypes.c_void_p(part.data_ptr()), rows, c, ctypes.c_void_p(sums.data_ptr()),
                                              hip.stream_ptr()), 'ym_bn_partials_finish')
    torch.cuda.synchronize()
    return sums.cpu().numpy()


def _desc(x, wp, out, kh, stride, pad, k_pad, plan, counters, transposed=False):
    """x [B][H][W][Cin] (dy for a data gradient), out [B][Ho][Wo][Cout]; plan = (tile, ksplit, stages, grid_wgs, tail)."""
    from yolact_minimal_amd import hip
    b, h, w, cin = x.shape
    _, ho, wo, cout = out.shape
    d = hip.ConvDesc()
    d.inp, d.weight = x.data_ptr(), wp.data_ptr()
    d.B, d.H, d.W, d.Cin, d.Cout, d.KH, d.KW = b, h, w, cin, cout, kh, kh
    d.stride, d.pad, d.Ho, d.Wo, d.k_pad, d.nseg = stride, pad, ho, wo, k_pad, 1
    d.seg[0].n_begin, d.seg[0].n_end, d.seg[0].out = 0, cout, out.data_ptr()
    d.seg[0].batch_stride, d.seg[0].pitch, d.seg[0].act = ho * wo * cout, cout, 0
    tile, ksplit, stages, grid_wgs, tail = plan
    d.tile_m, d.tile_n, d.ksplit, d.stages, d.grid_wgs = tile[0], tile[1], ksplit, stages, grid_wgs
    d.tail_tiles, d.tail_ksplit = tail
    d.tile_counters = counters.data_ptr()
    d.transposed = int(transposed)
    return d


def _launch_ordered(d, cout, expect_rows=None):
    """One ordered launch into a NaN-filled partial buffer: (partials [rows][2][cout] as numpy, rows, the device buffer).  Checks that
    every (row < rows, c) was written and that nothing behind those rows was."""
    from yolact_minimal_amd import hip
    L = hip.lib()
    assert L.ym_conv2d_fuses_bn_stats(ctypes.byref(d)) == 1
    d.bn_ordered = 1
    rows = L.ym_conv2d_bn_partial_rows(ctypes.byref(d))
    assert rows > 0
    if expect_rows is not None:
        assert rows == expect_rows, (rows, expect_rows)
    part = torch.full((rows + GUARD, 2, cout), float('nan'), dtype=torch.float64, device=DEV)
    d.bn_sum, d.bn_sumsq = part.data_ptr(), None
    ws = torch.empty(max(hip.conv_workspace_bytes(d), 256), dtype=torch.uint8, device=DEV)
    hip.conv2d_fwd(d, ws)
    torch.cuda.synchronize()
    p = part.cpu().numpy()
    assert np.isfinite(p[:rows]).all(), 'a (row, channel) pair of the partial buffer was not written'
    assert np.isnan(p[rows:]).all(), 'the launch wrote behind ym_conv2d_bn_partial_rows rows'
    return p[:rows], rows, part


def _check_order_and_repeat(d, cout, p, rows, part):
    """finish == numpy restatement of the documented order, bit for bit; a second launch gives the same partials and sums."""
    from yolact_minimal_amd import hip
    sums = _finish(part, rows, cout)
    assert np.array_equal(_bits(sums), _bits(finish_np(p))), 'ym_bn_partials_finish does not add in the documented order'
    part.fill_(float('nan'))
    ws = torch.empty(max(hip.conv_workspace_bytes(d), 256), dtype=torch.uint8, device=DEV)
    hip.conv2d_fwd(d, ws)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(part.cpu().numpy()[:rows]), _bits(p)), 'a second launch wrote other partials'
    assert np.array_equal(_bits(_finish(part, rows, cout)), _bits(sums))
    return sums


def _counters():
    from yolact_minimal_amd import hip
    return torch.zeros(hip.TILE_COUNTERS, device=DEV, dtype=torch.int32)


def _sums_of_output(out, cout):
    y = out.double().reshape(-1, cout)
    return torch.stack([y.sum(0), (y * y).sum(0)]).cpu()


# (name, B, H, W, Cin, Cout, k, plan = (tile, ksplit, stages, grid_wgs, tail), rows the plan writes)
FWD_CASES = [
    ('mfma_1x1', 2, 13, 13, 64, 128, 1, ((64, 64), 1, 22, 0, (0, 0)), 6),            # M = 338: ragged last M tile, two N tiles
    ('mfma_3x3_ksplit2', 1, 10, 10, 64, 64, 3, ((64, 64), 2, 22, 0, (0, 0)), 2),     # arrival counters: the last arriver writes
    ('mfma_1x1_tail', 2, 13, 13, 64, 128, 1, ((64, 64), 1, 22, 0, (2, 2)), 6),       # the last two tiles split into two K slices
    ('ws_64x256', 2, 37, 41, 64, 256, 1, ((64, 256), 1, 53, 0, (0, 0)), None),
    ('ws_128x128_g8', 2, 37, 41, 64, 256, 1, ((128, 128), 1, 52, 8, (0, 0)), 8),     # 2 slices -> 4 walkers x 2 wave rows
    ('ws_256x64', 2, 37, 41, 64, 256, 1, ((256, 64), 1, 54, 0, (0, 0)), None),
]


@pytest.mark.parametrize('case', FWD_CASES, ids=[c[0] for c in FWD_CASES])
def test_forward_partials_cover_their_rows_and_sum_to_the_output(case):
    from yolact_minimal_amd import hip
    name, b, h, w, cin, cout, k, plan, expect_rows = case
    g = torch.Generator().manual_seed(11)
    x = torch.randn(b, h, w, cin, generator=g).to(DEV)
    wt = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    wp = hip.pack_conv_weight(wt.to(DEV), cin, k * k * cin)
    out = torch.full((b, h, w, cout), float('nan'), device=DEV)
    counters = _counters()
    d = _desc(x, wp, out, k, 1, k // 2, k * k * cin, plan, counters)
    p, rows, part = _launch_ordered(d, cout, expect_rows)
    want = torch.nn.functional.conv2d(x.cpu().double().permute(0, 3, 1, 2), wt.double(), None, 1, k // 2).permute(0, 2, 3, 1)
    torch.testing.assert_close(out.cpu().double(), want, rtol=1e-4, atol=1e-4)
    own = _sums_of_output(out, cout)
    torch.testing.assert_close(torch.from_numpy(p.sum(0)), own, rtol=1e-5, atol=1e-3)
    sums = _check_order_and_repeat(d, cout, p, rows, part)
    torch.testing.assert_close(torch.from_numpy(sums), own, rtol=1e-5, atol=1e-3)
    assert int(counters.abs().sum()) == 0
    # the default mode of the same descriptor: atomics into a zeroed [2][Cout], the same sums to fp64 rounding
    acc = torch.zeros(2, cout, dtype=torch.float64, device=DEV)
    d.bn_ordered, d.bn_sum, d.bn_sumsq = 0, acc[0].data_ptr(), acc[1].data_ptr()
    hip.conv2d_fwd(d, torch.empty(max(hip.conv_workspace_bytes(d), 256), dtype=torch.uint8, device=DEV))
    torch.cuda.synchronize()
    torch.testing.assert_close(acc.cpu(), torch.from_numpy(sums), rtol=1e-12, atol=1e-9)


ORDER_CASES = [c for c in FWD_CASES if c[6] == 1]


@pytest.mark.parametrize('case', ORDER_CASES, ids=[c[0] for c in ORDER_CASES])
def test_finish_order_on_cancelling_partials(case):
    """A 1x1 conv whose only non-zero input channel is channel 0, with power-of-two weights: y[r][c] = v_r * w[c][0] exactly.  v_r
    cycles through 2^60, 1, -2^60, 3, 2^-20 in blocks of 7 rows, so every partial row is dominated by +-2^60 terms that cancel across
    rows."""
    from yolact_minimal_amd import hip
    name, b, h, w, cin, cout, k, plan, expect_rows = case
    m = b * h * w
    cyc = torch.tensor([2.0 ** 60, 1.0, -2.0 ** 60, 3.0, 2.0 ** -20])
    v = cyc[(torch.arange(m) // 7) % 5]
    x = torch.zeros(m, cin)
    x[:, 0] = v
    x = x.reshape(b, h, w, cin).to(DEV)
    wt = torch.zeros(cout, cin, 1, 1)
    wt[:, 0, 0, 0] = 2.0 ** -(torch.arange(cout) % 4).float()
    wp = hip.pack_conv_weight(wt.to(DEV), cin, cin)
    out = torch.full((b, h, w, cout), float('nan'), device=DEV)
    counters = _counters()                             # (kept alive: the descriptor holds a raw pointer)
    d = _desc(x, wp, out, 1, 1, 0, cin, plan, counters)
    p, rows, part = _launch_ordered(d, cout, expect_rows)
    assert torch.equal(out.cpu().reshape(m, cout), v[:, None] * wt[:, 0, 0, 0][None, :])          # exact products
    _check_order_and_repeat(d, cout, p, rows, part)
    assert int(counters.abs().sum()) == 0


def test_dgrad_partials_of_the_fused_batchnorm_backward_sums():
    """One transposed launch with bnb_* set (the data gradient of a Bottleneck's 3x3 conv2 at the shape of
    test_bn_backward_sums_ride_on_the_consumers_dgrad: 3 x 19 x 19, 32 planes, carrying bn1's backward sums): partials of sum dz and
    sum dz * xhat against fp64 sums over the launch's own dx."""
    from yolact_minimal_amd import hip
    b, hw, c = 3, 19, 32
    g = torch.Generator().manual_seed(7)
    dz = torch.randn(b, hw, hw, c, generator=g).to(DEV)                     # gradient of conv2's output
    wt = (torch.randn(c, c, 3, 3, generator=g) / (9 * c) ** 0.5).to(DEV)
    wd = torch.empty(c, 3, 3, c, device=DEV)
    hip.check(hip.lib().ym_pack_conv_weight_dgrad(hip.ptr(wt), hip.ptr(wd), c, c, 3, 3, c, hip.stream_ptr()), 'pack')
    y1 = torch.randn(b, hw, hw, c, generator=g).to(DEV)                     # bn1's input (conv1's raw output)
    out1 = torch.relu(torch.randn(b, hw, hw, c, generator=g)).to(DEV)       # bn1's saved output (the ReLU mask)
    mean, invstd = (torch.randn(c, generator=g) * 0.1).to(DEV), (torch.rand(c, generator=g) + 0.5).to(DEV)
    dx = torch.full((b, hw, hw, c), float('nan'), device=DEV)
    counters = _counters()
    d = _desc(dz, wd, dx, 3, 1, 1, 9 * c, ((64, 64), 1, 22, 0, (0, 0)), counters, transposed=True)
    d.bnb_y, d.bnb_out, d.bnb_mean, d.bnb_invstd, d.bnb_relu = y1.data_ptr(), out1.data_ptr(), mean.data_ptr(), invstd.data_ptr(), 1
    p, rows, part = _launch_ordered(d, c, expect_rows=-(-b * hw * hw // 64))
    want = torch.nn.functional.conv_transpose2d(dz.cpu().double().permute(0, 3, 1, 2), wt.cpu().double(), None, 1, 1).permute(0, 2, 3, 1)
    torch.testing.assert_close(dx.cpu().double(), want, rtol=1e-4, atol=1e-4)
    dd = torch.where(out1 > 0, dx, torch.zeros_like(dx)).double().reshape(-1, c)
    xhat = ((y1 - mean) * invstd).double().reshape(-1, c)                   # (fp32 like the kernel, then widened)
    own = torch.stack([dd.sum(0), (dd * xhat).sum(0)]).cpu()
    torch.testing.assert_close(torch.from_numpy(p.sum(0)), own, rtol=1e-5, atol=1e-3)
    sums = _check_order_and_repeat(d, c, p, rows, part)
    torch.testing.assert_close(torch.from_numpy(sums), own, rtol=1e-5, atol=1e-3)


def test_partial_rows_is_zero_where_the_statistics_do_not_fuse():
    from yolact_minimal_amd import hip
    x = torch.zeros(1, 8, 8, 64, device=DEV)
    wp = torch.zeros(64, 64, device=DEV)
    out = torch.zeros(1, 8, 8, 64, device=DEV)
    counters = _counters()
    d = _desc(x, wp, out, 1, 1, 0, 64, ((32, 32), 1, 0, 0, (0, 0)), counters)
    d.kwaves = 4                                                             # the wave-private kernel carries no statistics
    assert hip.lib().ym_conv2d_fuses_bn_stats(ctypes.byref(d)) == 0
    d.bn_ordered = 1
    assert hip.lib().ym_conv2d_bn_partial_rows(ctypes.byref(d)) == 0


@pytest.mark.parametrize('m,c', [(338, 64), (5000, 256)])
def test_bn_train_fwd_with_the_larger_workspace(m, c):
    from yolact_minimal_amd import hip
    L = hip.lib()
    g = torch.Generator().manual_seed(m + c)
    y = (torch.randn(m, c, generator=g) * 2 + 0.5).to(DEV)
    gamma, beta = (torch.rand(c, generator=g) + 0.5).to(DEV), (torch.randn(c, generator=g) * 0.1).to(DEV)
    res = {}
    small, big = 16 * c, L.ym_bn_train_fwd_workspace_bytes(m, c)
    rows = (big - 16 * c) // (16 * c)
    assert rows >= 1 and big == 16 * c + rows * 16 * c
    for name, nbytes in (('small', small), ('big', big)):
        ws = torch.full((nbytes // 8 + GUARD,), float('nan'), dtype=torch.float64, device=DEV)
        out, mean, invstd = torch.empty_like(y), torch.empty(c, device=DEV), torch.empty(c, device=DEV)
        rm, rv = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
        before = L.ym_unordered_sum_launches()
        hip.check(L.ym_bn_train_fwd(hip.ptr(y), m, c, hip.ptr(gamma), hip.ptr(beta), 1e-5, 0.1, hip.ptr(rm), hip.ptr(rv), None, 1,
                                    hip.ptr(out), hip.ptr(mean), hip.ptr(invstd), ctypes.c_void_p(ws.data_ptr()), nbytes,
                                    hip.stream_ptr()), 'ym_bn_train_fwd')
        torch.cuda.synchronize()
        assert L.ym_unordered_sum_launches() - before == (1 if name == 'small' else 0)
        assert bool(torch.isnan(ws[nbytes // 8:]).all())
        res[name] = (ws.cpu().numpy(), out.cpu(), mean.cpu(), invstd.cpu(), rm.cpu(), rv.cpu())
    w = res['big'][0]
    part = w[2 * c:2 * c + rows * 2 * c].reshape(rows, 2, c)
    assert np.isfinite(part).all()
    assert np.array_equal(_bits(w[:2 * c].reshape(2, c)), _bits(finish_np(part)))
    y64 = y.double()
    torch.testing.assert_close(torch.from_numpy(w[:2 * c].reshape(2, c).copy()), torch.stack([y64.sum(0), (y64 * y64).sum(0)]).cpu(),
                               rtol=1e-12, atol=1e-9)
    for i in (2, 3):                                                         # mean, invstd
        torch.testing.assert_close(res['big'][i], res['small'][i], rtol=1e-6, atol=0)
    for i in (1, 4, 5):                                                      # out, running statistics
        torch.testing.assert_close(res['big'][i], res['small'][i], rtol=1e-5, atol=1e-6)


def _step_inputs(batch, size, seed=5):
    img = torch.randn(batch, 3, size, size, generator=torch.Generator().manual_seed(1)).to(DEV)
    boxes, masks = R.synth_targets(batch, size, seed=seed)
    return img, [b.to(DEV) for b in boxes], [m.to(DEV) for m in masks]


@pytest.mark.parametrize('size', [64, 128])
def test_no_unordered_launch_in_an_ordered_step(size):
    from yolact_minimal_amd import hip
    from yolact_minimal_amd import train_engine as T
    from yolact_minimal_amd.trainer import Trainer
    L = hip.lib()
    cfg = build_cfg('res50_coco', 'train', size, train_bs=2, bs_per_gpu=2)
    img, boxes, masks = _step_inputs(2, size)
    moved = {}
    for mode in (False, True):
        torch.manual_seed(3)
        tr = Trainer(Yolact(cfg), cfg, torch.device(DEV), deterministic=mode)
        assert T._DETERMINISTIC is mode
        before = L.ym_unordered_sum_launches()
        losses = tr.step(img, boxes, masks)
        torch.cuda.synchronize()
        moved[mode] = L.ym_unordered_sum_launches() - before
        assert all(np.isfinite(float(l.detach())) for l in losses)
        tr.close()
    assert moved[False] > 0, 'the counter does not see the default mode\'s atomics'
    assert moved[True] == 0, f'{moved[True]} launches of an ordered step end in floating-point atomics'


def test_swin_backward_refuses_the_ordered_mode():
    from yolact_minimal_amd.trainer import Trainer
    cfg = build_cfg('swin_tiny_coco', 'train', 128, train_bs=2, bs_per_gpu=2)
    img, boxes, masks = _step_inputs(2, 128)
    torch.manual_seed(3)
    tr = Trainer(Yolact(cfg), cfg, torch.device(DEV), deterministic=True)
    with pytest.raises(RuntimeError, match='k_window_attention_bwd'):
        tr.step(img, boxes, masks)
    torch.cuda.synchronize()
    tr.close()


def test_ordered_train_step_256_well_conditioned_golden(golden_dir):
    """test_gpu_train.py::test_train_step_256_well_conditioned_golden with the ordered sums on: the same reference fixture
    (tests/golden/train_res50_coco_256_b4.npz), the same assertions and bars."""
    from yolact_minimal_amd import hip
    from yolact_minimal_amd import train_engine as T
    T._DETERMINISTIC = True
    T.tuned_table_changed()
    g = np.load(os.path.join(golden_dir, 'train_res50_coco_256_b4.npz'))
    seed, size, batch = int(g['seed']), 256, 4
    cfg = build_cfg('res50_coco', 'train', size)
    torch.manual_seed(seed)
    net = Yolact(cfg).train()
    sd = net.state_dict()
    R.damp_residual_branches_(sd, seed + 400)
    net.load_state_dict(sd)
    sd0 = {k: v.clone() for k, v in net.state_dict().items()}
    img = torch.randn(batch, 3, size, size, generator=torch.Generator().manual_seed(seed + 300))
    boxes, masks = R.synth_targets(batch, size, seed=seed)
    l32, g32, _ = _oracle_grads(net, sd0, img, boxes, masks, torch.float32)
    l64, g64, _ = _oracle_grads(net, sd0, img, boxes, masks, torch.float64)
    net = net.to(DEV)
    before = hip.lib().ym_unordered_sum_launches()
    losses = net(img.to(DEV), [b.to(DEV) for b in boxes], [m.to(DEV) for m in masks])
    sum(losses).backward()
    torch.cuda.synchronize()
    assert hip.lib().ym_unordered_sum_launches() == before               # (the mode under test did run)
    got = np.array([float(l.detach()) for l in losses])
    np.testing.assert_allclose(got, np.array(l64), rtol=1e-5)
    np.testing.assert_allclose(got, g['losses'], rtol=1e-5)              # the reference's own numbers
    keys = [str(k) for k in g['grad_keys']]
    assert keys == [k for k, _ in net.named_parameters()]
    rows = []
    for i, (k, p) in enumerate(net.named_parameters()):
        gg = p.grad.detach().cpu().double()
        e_gpu, e_cpu = _rel_err(gg, g64[k]), max(_rel_err(g32[k], g64[k]), float(g['grad_err_vs_fp64'][i]))
        n = min(64, _grad_sample(gg).numel())
        d64 = np.abs(_grad_sample(g64[k]).numpy()[:n] - g['grad_sample_fp64'][i][:n]).max() / (float(g['grad_absmax'][i]) + 1e-30)
        assert d64 < 1e-9, (k, d64)
        rows.append((e_gpu / max(3.0 * e_cpu, 1e-4), k, e_gpu, e_cpu))
    e_gpu = np.array([r[2] for r in rows])
    e_ref = np.array([r[3] for r in rows])
    print(f'ordered, 256 px bs=4: gradient error vs fp64 / max|g|: GPU median {np.median(e_gpu):.2e} p90 {np.quantile(e_gpu, 0.9):.2e} max '
          f'{e_gpu.max():.2e}; fp32 CPU reference median {np.median(e_ref):.2e} p90 {np.quantile(e_ref, 0.9):.2e} max {e_ref.max():.2e}')
    assert np.median(e_gpu) <= 1.5 * np.median(e_ref) + 1e-5
    assert np.quantile(e_gpu, 0.9) <= 3.0 * np.quantile(e_ref, 0.9) + 1e-5
    assert e_gpu.max() <= 2.0 * e_ref.max()
    tail = [r for r in rows if not r[1].startswith('backbone.')]
    worst = max(tail)
    assert worst[0] <= 1.0, sorted(tail, reverse=True)[:5]
    np.testing.assert_allclose(net.backbone.bn1.running_mean.cpu().numpy(), g['run_mean_stem'], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(net.backbone.bn1.running_var.cpu().numpy(), g['run_var_stem'], rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize('size,batch', [(128, 8), (256, 4)])
def test_two_ordered_trainings_end_bit_identical(size, batch):
    """Trainer(deterministic=True) twice in one process: res50_custom on the overfit demo's synthetic pictures, 40 steps, fixed seed.
    Every parameter, BatchNorm buffer and momentum buffer must come out with the same bits."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tools'))
    from overfit_demo import make_dataset
    from yolact_minimal_amd.loss import mask_generator
    from yolact_minimal_amd.trainer import Trainer
    dev = torch.device(DEV)
    cfg = build_cfg('res50_custom', 'train', size, train_bs=batch, bs_per_gpu=batch)
    data = make_dataset(16, size, 0)
    imgs = torch.stack([d[0] for d in data]).to(dev)
    gts, mks = [d[1].to(dev) for d in data], [d[2].to(dev) for d in data]

    def train():
        torch.manual_seed(0)
        mask_generator(dev).manual_seed(0x5EED)           # (one generator per process: both runs draw the same sub-samples)
        tr = Trainer(Yolact(cfg), cfg, dev, deterministic=True)
        order = np.random.default_rng(1)
        for _ in range(40):
            pick = order.choice(16, batch, replace=False)
            tr.step(imgs[pick], [gts[i] for i in pick], [mks[i] for i in pick])
        torch.cuda.synchronize()
        state = {k: v.detach().clone() for k, v in tr.net.state_dict().items()}
        state['<momentum>'] = tr.opt.buf.detach().clone()
        tr.close()
        return state

    a, b = train(), train()
    assert a.keys() == b.keys()
    assert all(bool(torch.isfinite(v).all()) for v in a.values() if v.is_floating_point())
    differ = [k for k in a if not torch.equal(a[k], b[k])]
    assert not differ, f'{len(differ)} of {len(a)} tensors differ between two ordered runs, e.g. {differ[:5]}'
