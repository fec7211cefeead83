"""The four training-loss launches at their tile, chunk and saturation edges, each against a plain reference on the CPU
(tests/loss_edges_ref.py, pinned to the oracle by tests/test_loss_edges_cpu.py).

  mask loss    pixel tiles (a wave's second tile, a partial last tile, a full last tile, Hp != Wp), positive tiles (1 .. 128
               positives, the refusal at 129), the sub-sampled path value by value, crop windows at the border, a thin box,
               saturated logits, 17 images (MLB = 16 per launch)
  match        g = 1, g = GMAX = 256, the refusals at 0 and 257, 33 images (MAXB = 32 per launch)
  class + box  smooth-L1 at |d| = 1 and its neighbours, OHEM marks that underflow to -inf, C = 2 and C = 256, the refusal at 257
  semantic     non-square map, 20 classes padded to 32 and contiguous, an image without ground truth, |logit| up to 100, 33 images

Bars: loss rtol 2e-5, gradients rtol 1e-4 with atol 1e-5 * max|reference| (mask), 1e-8 (class / box), 1e-9 (semantic) — the bars
of the tests of the same kernels in tests/test_gpu_train.py; integer outputs exact.  The two float32-against-float32 cases
carry their own measured bars (see SATURATED_BARS / UNDERFLOW_BARS).  Every test prints its figures before it asserts.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import yolact_ref as R
from tests import loss_edges_ref as E
from yolact_minimal_amd.config import build_cfg

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# Float32 device against the float32 oracle on the CPU: expf / logf may differ in the last ulp between the two, so the bars are
# measured, not derived: 4 x the largest figure seen on an MI355X (relative error of the loss, E.rel_err for the gradients), never
# looser than 1e-4 on the loss and 1e-3 on gradients.  The losses come back as float32, so a measured loss error below half an ulp
# of the result (2^-24) counts as 2^-24.  Figures: the two tests' docstrings and docs/experiments.md.
HALF_ULP = 2.0 ** -24
MEASURED_SAT_LOSS, MEASURED_SAT_GRAD = 1.07e-7, 1.45e-6        # saturated mask loss: the larger of the two seeds
MEASURED_UF_LOSS, MEASURED_UF_GRAD = 6.47e-8, 1.54e-7          # underflowing OHEM marks: the larger of the two columns
SATURATED_BARS = dict(loss=min(4 * max(MEASURED_SAT_LOSS, HALF_ULP), 1e-4), grad=min(4 * MEASURED_SAT_GRAD, 1e-3))
UNDERFLOW_BARS = dict(loss=min(4 * max(MEASURED_UF_LOSS, HALF_ULP), 1e-4), grad=min(4 * MEASURED_UF_GRAD, 1e-3))


def _cfg(masks_to_train=None):
    cfg = build_cfg('res50_coco', 'train', 128)
    if masks_to_train is not None:
        cfg.masks_to_train = masks_to_train
    return cfg


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _run_mask(c, cfg):
    from yolact_minimal_amd.loss import lincomb_mask_loss
    pg, cg = c['proto'].to(DEV).requires_grad_(), c['coef'].to(DEV).requires_grad_()
    got = lincomb_mask_loss(cfg, c['pos'].to(DEV), c['anchor_gt'].to(DEV), cg, pg, [m.to(DEV) for m in c['masks']],
                            c['anchor_box'].to(DEV))
    got.backward()
    return got.detach().cpu(), pg.grad.cpu(), cg.grad.cpu()


def _check_mask(got, ref, what, loss_rtol=2e-5, grad_rtol=1e-4):
    """loss and both gradients at the mask-loss bars: rtol on the loss, rtol + 0.1 * rtol * max|reference| on the gradients."""
    loss_err = abs(float(got[0]) / float(ref[0]) - 1)
    print(f'{what}: loss {float(got[0]):.9g} vs {float(ref[0]):.9g} (rel {loss_err:.2e}), dproto rel_err '
          f'{E.rel_err(got[1], ref[1]):.2e}, dcoef rel_err {E.rel_err(got[2], ref[2]):.2e}')
    np.testing.assert_allclose(float(got[0]), float(ref[0]), rtol=loss_rtol)
    for g, r in zip(got[1:], ref[1:]):
        torch.testing.assert_close(g.double(), r.double(), rtol=grad_rtol, atol=0.1 * grad_rtol * float(r.abs().max()))


# ---- 1. mask loss: pixel tiles -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hp,wp', [(96, 96), (97, 97), (64, 128)])
def test_mask_loss_pixel_tiles(hp, wp):
    """256 waves walk the 32-pixel tiles of an image with a grid stride.  96 x 96: 288 tiles, waves 0..31 take a second tile whose
    dcoef contribution is accumulated in registers, the last tile is full; 97 x 97: 295 tiles, the last one holds 1 pixel;
    64 x 128: pixel -> (row, column) with Wp != Hp.  One gt box ends in the bottom right corner, so the second tiles and the very
    last pixel carry loss and gradient (asserted on the reference).  fp64 oracle; rows of non-positives stay exactly zero."""
    gen = torch.Generator().manual_seed(hp)
    corner = torch.tensor([[0.3, 0.55, 1.0, 1.0, 2.0]])                  # reaches the last pixel: the random boxes end at 0.95
    c = E.mask_case([41, 38], hp, wp, 300, seed=hp + wp, boxes=[torch.cat([E.random_boxes(2, gen), corner]) for _ in range(2)])
    ref = E.mask_loss_autograd(c, torch.float64)
    rows = ref[1].reshape(2, hp * wp, 32).abs().sum(-1) > 0
    assert bool(rows[:, -1].all())
    if hp * wp > 256 * 32:                                                # the tiles past the first 256 (64 x 128 has exactly 256)
        assert bool(rows[:, 256 * 32:].any(1).all())
    got = _run_mask(c, _cfg())
    _check_mask(got, ref, f'pixel tiles {hp}x{wp}')
    assert float(got[2][~c['pos']].abs().max()) == 0.0
    assert bool((got[2][c['pos']].abs().sum(-1) > 0).all())


# ---- 2. mask loss: positive tiles --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 31, 32, 33, 64, 65, 96, 97, 128])
def test_mask_loss_positive_tiles(n):
    """The positives of an image are handled in four tiles of 32 (dc[0..3]); every count at which a tile fills, starts or is the
    last (MAXP = 128) against the fp64 oracle, every dcoef row compared.  cfg.masks_to_train = 128: nothing is sub-sampled."""
    c = E.mask_case([n], 34, 34, 300, seed=100 + n)
    ref = E.mask_loss_autograd(c, torch.float64)
    got = _run_mask(c, _cfg(128))
    _check_mask(got, ref, f'{n} positives')
    assert torch.equal(got[2].abs().sum(-1) > 0, c['pos'])


def test_mask_loss_refuses_more_than_128_positives():
    """129 positives do not fit the kernel's four tiles: `ym_mask_loss_fwd_bwd` returns an error before any launch (the outputs
    keep their sentinel), and `lincomb_mask_loss` raises for cfg.masks_to_train = 129."""
    from yolact_minimal_amd import hip
    from yolact_minimal_amd.loss import lincomb_mask_loss
    n, hp = 129, 34
    c = E.mask_case([n], hp, hp, 300, seed=7)
    idx = torch.nonzero(c['pos'][0]).flatten().to(DEV)
    ds = torch.zeros(3, hp, hp, device=DEV)
    dproto, dcoef = torch.full((hp, hp, 32), -7.0, device=DEV), torch.full((300, 32), -7.0, device=DEV)
    acc = torch.full((1,), -7.0, dtype=torch.float64, device=DEV)
    ws = torch.empty(hip.lib().ym_mask_loss_workspace_bytes(), dtype=torch.uint8, device=DEV)
    proto_i, coef_i = c['proto'][0].to(DEV), c['coef'][0].to(DEV)[idx].contiguous()
    box_i, gt_i = c['anchor_box'][0].to(DEV)[idx].contiguous(), c['anchor_gt'][0].to(DEV)[idx].to(torch.int32).contiguous()
    rc = hip.lib().ym_mask_loss_fwd_bwd(
        hip.ptr(proto_i), hip.ptr(coef_i), hip.ptr(box_i), hip.ptr(gt_i, torch.int32), hip.ptr(ds), hip.ptr(idx, torch.int64),
        n, hp, hp, 1.0, 1.0, _vp(acc), hip.ptr(dproto), hip.ptr(dcoef), _vp(ws), ws.numel(), hip.stream_ptr())
    assert rc != 0
    msg = hip.lib().ym_last_error().decode()
    assert 'at most 128 positives' in msg and '129' in msg
    torch.cuda.synchronize()
    assert bool((dproto == -7.0).all()) and bool((dcoef == -7.0).all()) and float(acc) == -7.0
    with pytest.raises(RuntimeError, match='at most 128'):
        lincomb_mask_loss(_cfg(129), c['pos'].to(DEV), c['anchor_gt'].to(DEV), c['coef'].to(DEV), c['proto'].to(DEV),
                          [m.to(DEV) for m in c['masks']], c['anchor_box'].to(DEV))


# ---- 3. mask loss: sub-sampling, exactly -------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', [0, 1])
def test_mask_loss_subsampled_values(seed):
    """340 positives over the cap of 100: the kernel trains min(n_dev, cap) rows and weights them by n_dev / trained (device-side
    counts), and the batch is divided by all 400 positives.  The trained rows are read off the non-zero rows of dcoef; the loss
    and both gradients are then compared with the fp64 restatement of the reference for exactly that subset."""
    from yolact_minimal_amd import loss as L
    c = E.mask_case([340, 60, 0], 34, 34, 900, seed=30 + seed)
    L.mask_generator(DEV).manual_seed(seed)
    got = _run_mask(c, _cfg())
    rows = got[2].abs().sum(-1) > 0
    assert int(rows[0].sum()) == 100 and bool((rows[0] <= c['pos'][0]).all())
    assert torch.equal(rows[1], c['pos'][1]) and not bool(rows[2].any())
    subset = torch.nonzero(rows[0]).flatten()
    ref = E.mask_loss_autograd(c, torch.float64, subsets=[subset, None, None])
    _check_mask(got, ref, f'sub-sampled, seed {seed}')
    assert float(got[1][2].abs().max()) == 0.0


# ---- 4. mask loss: boxes at the edges ----------------------------------------------------------------------------------------
def test_mask_loss_boxes_at_the_map_border():
    """Crop windows clamped at x = 0, x = Wp, y = 0 and y = Hp, one that is the whole map, and a box 1.5 prototype pixels wide whose
    1 / area weight is 75 x the usual; fp64 oracle."""
    bx = E.edge_boxes(34)
    c = E.mask_case([40, 25], 34, 34, 300, seed=9, boxes=[bx, bx.flip(0)])
    for i in range(2):
        assert sorted(set(c['anchor_gt'][i][c['pos'][i]].tolist())) == [0, 1, 2, 3, 4]
    ref = E.mask_loss_autograd(c, torch.float64)
    _check_mask(_run_mask(c, _cfg()), ref, 'border boxes')


# ---- 5. mask loss: saturated logits ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', E.SATURATED_SEEDS)
def test_mask_loss_saturated_logits(seed):
    """|z| up to 58: sigmoid is exactly 1.0f for ~9 % of the pixels inside the windows, where BCE's -100 clamp sets the loss and the
    gradient is exactly 0.  The specification is the oracle in float32 on the CPU (fp64 never saturates).  No pixel lies within
    1e-3 of the z at which float32 saturates (asserted without a GPU), so no element is excluded.
    Measured on an MI355X, seeds 0 / 1: loss 0.0 / 1.07e-7, dproto 1.45e-6 / 1.28e-6, dcoef 7.05e-7 / 7.81e-7 (E.rel_err); the bars are
    4 x the larger: 4.3e-7 on the loss, 5.8e-6 on both gradients."""
    c = E.saturated_case(seed)
    ref = E.mask_loss_autograd(c, torch.float32)
    got = _run_mask(c, _cfg())
    for t in got:
        assert bool(torch.isfinite(t).all())
    bar_l, bar_g = SATURATED_BARS['loss'], SATURATED_BARS['grad']
    _check_mask(got, ref, f'saturated, seed {seed}', loss_rtol=bar_l, grad_rtol=bar_g)


# ---- 6. batch chunks ---------------------------------------------------------------------------------------------------------
CHUNK_COUNTS = {
    '17, image 16 empty': [3, 5, 2, 4, 6, 0, 3, 1, 7, 2, 4, 3, 5, 2, 6, 1, 0],
    '17, image 16 trained': [3, 5, 2, 4, 6, 0, 3, 1, 7, 2, 4, 3, 5, 2, 6, 0, 4],
    '18, image 17 empty': [2, 3, 1, 4, 2, 0, 3, 1, 2, 2, 4, 3, 1, 2, 3, 2, 5, 0],
}


@pytest.mark.parametrize('name', list(CHUNK_COUNTS))
def test_mask_loss_batches_cross_the_launch_chunk(name):
    """MLB = 16 images travel per launch, the host loop hands the next ones to a second launch.  17 images with none of the positives
    in images 5 and 16 (the second launch has nothing to do); 17 with image 16 trained (the second launch writes image 16's
    slices and nobody else's); 18 with image 16 trained and 17 empty.  Every image's dproto / dcoef slice is compared with the
    fp64 oracle by name, images without positives are exactly zero."""
    counts = CHUNK_COUNTS[name]
    c = E.mask_case(counts, 34, 34, 120, seed=len(counts) + counts[16])
    ref = E.mask_loss_autograd(c, torch.float64)
    got = _run_mask(c, _cfg())
    _check_mask(got, ref, name)
    for i, n in enumerate(counts):
        for g, r in ((got[1][i], ref[1][i]), (got[2][i], ref[2][i])):
            if n == 0:
                assert float(g.abs().max()) == 0.0 and float(r.abs().max()) == 0.0, f'image {i}'
            else:
                assert float(r.abs().max()) > 0
                torch.testing.assert_close(g.double(), r, rtol=1e-4, atol=1e-5 * float(r.abs().max()), msg=lambda m: f'image {i}: {m}')


def _match(cfg, boxes, anchors):
    from yolact_minimal_amd import loss as L
    b, n = len(boxes), anchors.shape[0]
    ws = torch.empty(4 * n * b, dtype=torch.uint8, device=DEV)
    off, abox = torch.empty(b, n, 4, device=DEV), torch.empty(b, n, 4, device=DEV)
    conf, agt = torch.empty(b, n, dtype=torch.int64, device=DEV), torch.empty(b, n, dtype=torch.int64, device=DEV)
    boxes_d, anchors_d = [bc.to(DEV) for bc in boxes], anchors.to(DEV)     # named: alive across the launch
    L.match(cfg, boxes_d, anchors_d, off, conf, abox, agt, ws)
    torch.cuda.synchronize()
    return off, conf, abox, agt


def _check_match(out, boxes, anchors):
    """labels, matched gt index and matched box identical to the oracle; encoded offsets to log() rounding, as in
    test_match_anchors_kernel_bit_exact."""
    off, conf, abox, agt = [t.cpu() for t in out]
    for i, bc in enumerate(boxes):
        r_off, r_conf, r_box, r_gt = R.match_anchors(bc[:, :4], anchors, bc[:, 4].long())
        assert torch.equal(conf[i], r_conf), f'image {i}'
        assert torch.equal(agt[i], r_gt), f'image {i}'
        assert torch.equal(abox[i], r_box), f'image {i}'
        torch.testing.assert_close(off[i], r_off, rtol=1e-6, atol=1e-6, msg=lambda m: f'image {i}: {m}')
        assert int((r_conf > 0).sum()) >= 1


def test_match_33_images_cross_the_launch_chunk():
    """MAXB = 32 images per launch: image 32 runs in a second launch whose output pointers are advanced on the host."""
    cfg = build_cfg('res50_coco', 'train', 128)
    anchors = R.anchors_for(128, cfg.scales).float()
    boxes, _ = R.synth_targets(33, 128, n_gt=3, seed=40)
    assert anchors.shape[0] == 1023
    _check_match(_match(cfg, boxes, anchors), boxes, anchors)


def _semantic(seg_dev, masks, boxes):
    from yolact_minimal_amd.loss import semantic_seg_loss
    return semantic_seg_loss(build_cfg('res50_coco', 'train', 128), seg_dev, [m.to(DEV) for m in masks], [b.to(DEV) for b in boxes])


def test_semantic_loss_33_images_cross_the_launch_chunk():
    """MAXB = 32 images per launch at 8 x 8: every image's gradient slice against the fp64 oracle, image 32 by name."""
    g = torch.Generator().manual_seed(6)
    boxes = [E.random_boxes(2, g, num_classes=20) for _ in range(33)]
    masks = [E.rect_targets(bx, 32, 32) for bx in boxes]
    seg = torch.randn(33, 20, 8, 8, generator=g) * 3
    sp = seg.double().requires_grad_()
    ref = E.semantic_loss(sp, [m.double() for m in masks], [bx[:, 4].long() for bx in boxes])
    ref.backward()
    sg = seg.to(DEV).requires_grad_()
    got = _semantic(sg, masks, boxes)
    got.backward()
    print(f'semantic 33 images: {float(got):.9g} vs {float(ref):.9g}')
    np.testing.assert_allclose(float(got.detach()), float(ref.detach()), rtol=2e-5)
    for i in range(33):
        torch.testing.assert_close(sg.grad[i].cpu().double(), sp.grad[i], rtol=1e-4, atol=1e-9, msg=lambda m: f'image {i}: {m}')
    assert float(sg.grad[32].abs().max()) > 0


# ---- 7. match limits ---------------------------------------------------------------------------------------------------------
def test_match_one_ground_truth():
    cfg = build_cfg('res50_coco', 'train', 128)
    anchors = R.anchors_for(128, cfg.scales).float()
    boxes, _ = R.synth_targets(2, 128, n_gt=1, seed=3)
    _check_match(_match(cfg, boxes, anchors), boxes, anchors)


def test_match_256_ground_truths():
    """g = GMAX = 256 fills the kernel's shared gt table: random boxes, every 8th tiny (0.4 % .. 1 % of the image side), rows
    200..209 copies of rows 10..19 with other classes (both claim the same best anchor, the later one wins)."""
    cfg = build_cfg('res50_coco', 'train', 256)
    anchors = R.anchors_for(256, cfg.scales).float()
    g = torch.Generator().manual_seed(12)
    boxes = []
    for _ in range(2):
        xy = torch.rand(256, 2, generator=g) * 0.8 + 0.05
        wh = torch.rand(256, 2, generator=g) * 0.25 + 0.05
        wh[::8] = torch.rand(32, 2, generator=g) * 0.006 + 0.004
        bc = torch.cat([xy, torch.clamp(xy + wh, max=0.99), torch.randint(0, 80, (256, 1), generator=g).float()], 1)
        bc[200:210, :4] = bc[10:20, :4]
        bc[200:210, 4] = (bc[10:20, 4] + 1) % 80
        boxes.append(bc)
    out = _match(cfg, boxes, anchors)
    _check_match(out, boxes, anchors)
    assert int(out[3].max()) == 255


@pytest.mark.parametrize('g', [0, 257])
def test_match_refuses_zero_and_257_ground_truths(g):
    """Outside 1 <= g <= 256 the call is refused with the limit in the message, and nothing is launched: the outputs keep their
    sentinel.  (An image without ground truth has no definition in the reference's match(): max over an empty dimension raises.)"""
    cfg = build_cfg('res50_coco', 'train', 128)
    anchors = R.anchors_for(128, cfg.scales).float()
    gen = torch.Generator().manual_seed(1)
    boxes = [E.random_boxes(3, gen), E.random_boxes(max(g, 1), gen)[:g]]
    from yolact_minimal_amd import loss as L
    b, n = 2, anchors.shape[0]
    ws = torch.empty(4 * n * b, dtype=torch.uint8, device=DEV)
    outs = [torch.full((b, n, 4), -7.0, device=DEV), torch.full((b, n), -7, dtype=torch.int64, device=DEV),
            torch.full((b, n, 4), -7.0, device=DEV), torch.full((b, n), -7, dtype=torch.int64, device=DEV)]
    boxes_d, anchors_d = [bc.to(DEV) for bc in boxes], anchors.to(DEV)
    with pytest.raises(RuntimeError, match='1 <= g <= 256'):
        L.match(cfg, boxes_d, anchors_d, outs[0], outs[1], outs[2], outs[3], ws)
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in outs)


# ---- 8. box loss boundaries --------------------------------------------------------------------------------------------------
def test_box_loss_at_the_smooth_l1_knee():
    """box_p - offsets exactly -1, 1, 0, the float32 neighbours of 1 on both sides, and their negatives (offsets are 0 there, so
    the difference is exact).  Loss and gradient against fp64 autograd; the elements at +-1 and just above take the sign branch,
    whose gradient +-bbox_alpha / num_pos is exact with 32 positives, and must equal the float32 CPU result bit for bit."""
    from yolact_minimal_amd.loss import _ClassBoxLossFn
    g = torch.Generator().manual_seed(8)
    b, n, nc = 1, 300, 5
    class_p = torch.randn(b, n, nc, generator=g)
    box_p = torch.randn(b, n, 4, generator=g) * 1.5
    offsets = torch.randn(b, n, 4, generator=g)
    conf = torch.zeros(b, n, dtype=torch.int64)
    rows = torch.randperm(n, generator=g)[:32]
    conf[0, rows] = torch.randint(1, nc, (32,), generator=g)
    one = torch.tensor(1.0)
    below, above = torch.nextafter(one, torch.tensor(0.0)), torch.nextafter(one, torch.tensor(2.0))
    specials = torch.stack([-one, one, 0 * one, below, above, -above, -below, one])
    assert float(below) < 1.0 < float(above)
    for r in rows[:6].tolist():                                           # 24 elements: every special value three times
        for e in range(4):
            offsets[0, r, e] = 0.0
            box_p[0, r, e] = specials[(rows[:6].tolist().index(r) * 4 + e) % 8]
    d = (box_p - offsets)[0, rows[:6]]
    knee = (d.abs() == 1.0) | (d.abs() == above)
    assert int(knee.sum()) >= 12 and int((d == below).sum()) >= 3
    bp = box_p.double().requires_grad_()
    ref_b = R.box_reg_loss(bp, offsets.double(), conf > 0)
    ref_b.backward()
    ref32 = E.class_box_loss_f32(class_p, box_p, offsets, conf)
    cg, bg = class_p.to(DEV).requires_grad_(), box_p.to(DEV).requires_grad_()
    num_pos = torch.empty(b + 1, dtype=torch.int32, device=DEV)
    got_c, got_b = _ClassBoxLossFn.apply(cg, bg, offsets.to(DEV), conf.to(DEV), num_pos, 1.0, 1.5, 3)
    (got_c + got_b).backward()
    assert num_pos.tolist() == [32, 32]
    np.testing.assert_allclose(float(got_b.detach()), float(ref_b.detach()), rtol=2e-5)
    torch.testing.assert_close(bg.grad.cpu().double(), bp.grad, rtol=1e-4, atol=1e-8)
    got_knee, ref_knee = bg.grad.cpu()[0, rows[:6]][knee], ref32[3][0, rows[:6]][knee]
    assert torch.equal(got_knee, ref_knee)
    assert torch.equal(got_knee.abs(), torch.full_like(got_knee, 1.5 / 32))
    assert float(bg.grad.cpu()[conf <= 0].abs().max()) == 0.0


# ---- 9. OHEM under an underflowing global maximum ----------------------------------------------------------------------------
@pytest.mark.parametrize('col', [0, 7])
def test_ohem_marks_that_underflow_to_minus_infinity(col):
    """The marks subtract the maximum of the whole logit tensor (the reference's quirk): one background row with a logit of +200
    makes exp(x - 200) underflow for every other row, whose mark is then -inf.  The ranking must still put the marks that are 0
    (positives, neutrals) first and take the -inf rows in index order: the selected rows equal the float32 oracle's exactly
    (fp64 would rank by the true marks, which is not what the reference computes).  col = 0: the hot row is a confident
    background, its mark is 0 and its gradient exactly zero; col = 7: its mark is 200 - x0, the largest, and its loss ~200.
    Measured on an MI355X, columns 0 / 7: loss_c 6.47e-8 / 0.0, dclass 1.54e-7 / 1.54e-7 (E.rel_err); the bars are 4 x the larger:
    2.6e-7 on the loss, 6.2e-7 on the gradient."""
    from yolact_minimal_amd.loss import _ClassBoxLossFn
    class_p, box_p, offsets, conf, hot = E.underflow_case(seed=3, col=col)
    ref_c, ref_b, ref_dc, ref_db = E.class_box_loss_f32(class_p, box_p, offsets, conf)
    b = conf.shape[0]
    cg, bg = class_p.to(DEV).requires_grad_(), box_p.to(DEV).requires_grad_()
    num_pos = torch.empty(b + 1, dtype=torch.int32, device=DEV)
    got_c, got_b = _ClassBoxLossFn.apply(cg, bg, offsets.to(DEV), conf.to(DEV), num_pos, 1.0, 1.5, 3)
    (got_c + got_b).backward()
    dclass = cg.grad.cpu()
    loss_err = abs(float(got_c) / float(ref_c) - 1)
    print(f'underflow col {col}: loss_c {float(got_c):.9g} vs {float(ref_c):.9g} (rel {loss_err:.2e}), dclass rel_err '
          f'{E.rel_err(dclass, ref_dc):.2e}')
    assert num_pos.tolist() == (conf > 0).sum(1).tolist() + [int((conf > 0).sum())]
    assert bool(torch.isfinite(dclass).all()) and bool(torch.isfinite(got_c).all())
    assert torch.equal(dclass.abs().sum(-1) > 0, ref_dc.abs().sum(-1) > 0)
    bar_l, bar_g = UNDERFLOW_BARS['loss'], UNDERFLOW_BARS['grad']
    np.testing.assert_allclose(float(got_c.detach()), float(ref_c), rtol=bar_l)
    torch.testing.assert_close(dclass, ref_dc, rtol=bar_g, atol=0.1 * bar_g * float(ref_dc.abs().max()))
    np.testing.assert_allclose(float(got_b.detach()), float(ref_b), rtol=2e-5)


# ---- 10. class count at the limit --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nc', [2, 256])
def test_class_loss_at_the_class_count_limits(nc):
    """C = 256 fills the four registers per lane of the cross-entropy kernel; C = 2 leaves 62 lanes of the wave idle."""
    from yolact_minimal_amd.loss import _ClassBoxLossFn
    g = torch.Generator().manual_seed(nc)
    b, n = 2, 700
    class_p = torch.randn(b, n, nc, generator=g) * 2
    box_p, offsets = torch.randn(b, n, 4, generator=g) * 1.5, torch.randn(b, n, 4, generator=g)
    conf = torch.zeros(b, n, dtype=torch.int64)
    for i in range(b):
        sel = torch.randperm(n, generator=g)
        conf[i, sel[:30]] = torch.randint(1, nc, (30,), generator=g)
        conf[i, sel[30:40]] = -1
    conf[0, torch.nonzero(conf[0] > 0).flatten()[0]] = nc - 1            # the last class is a target
    pos = conf > 0
    cp, bp = class_p.double().requires_grad_(), box_p.double().requires_grad_()
    ref_c, ref_b = R.ohem_class_loss(cp, conf, pos, stable=True), R.box_reg_loss(bp, offsets.double(), pos)
    (ref_c + ref_b).backward()
    cg, bg = class_p.to(DEV).requires_grad_(), box_p.to(DEV).requires_grad_()
    num_pos = torch.empty(b + 1, dtype=torch.int32, device=DEV)
    got_c, got_b = _ClassBoxLossFn.apply(cg, bg, offsets.to(DEV), conf.to(DEV), num_pos, 1.0, 1.5, 3)
    (got_c + got_b).backward()
    print(f'C = {nc}: loss_c {float(got_c):.9g} vs {float(ref_c):.9g}, dclass rel_err {E.rel_err(cg.grad.cpu(), cp.grad):.2e}')
    assert num_pos.tolist() == [30, 30, 60]
    np.testing.assert_allclose(float(got_c.detach()), float(ref_c.detach()), rtol=2e-5)
    np.testing.assert_allclose(float(got_b.detach()), float(ref_b.detach()), rtol=2e-5)
    torch.testing.assert_close(cg.grad.cpu().double(), cp.grad, rtol=1e-4, atol=1e-8)
    torch.testing.assert_close(bg.grad.cpu().double(), bp.grad, rtol=1e-4, atol=1e-8)


def test_class_loss_refuses_257_classes():
    from yolact_minimal_amd.loss import _ClassBoxLossFn
    class_p, box_p, offsets = torch.zeros(1, 64, 257, device=DEV), torch.zeros(1, 64, 4, device=DEV), torch.zeros(1, 64, 4, device=DEV)
    conf = torch.ones(1, 64, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match='class_box_loss: bad shape'):
        _ClassBoxLossFn.apply(class_p, box_p, offsets, conf, torch.empty(2, dtype=torch.int32, device=DEV), 1.0, 1.5, 3)
    torch.cuda.synchronize()


# ---- gt masks at the size of the prediction map ------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w,oh,ow', [(256, 512, 64, 128), (28, 36, 7, 9), (50, 50, 17, 17), (136, 136, 34, 34), (45, 70, 13, 31)])
def test_gt_masks_downsample_has_one_scale_per_axis(h, w, oh, ow):
    """`ym_gt_masks_downsample` = F.interpolate(bilinear, align_corners=False) > 0.5 on non-square maps and at scales that are no
    integer.  (Found by the 64 x 128 case below: the losses used after_nms's resize, which scales both axes by the longer side;
    the mask loss came out 87 x too large.)  Soft random masks, so the threshold is met at arbitrary values: a pixel may differ
    only where the fp64 value is within 1e-6 of 0.5.  On a square map the result equals `ym_mask_resize_binarize` bit for bit,
    which is what the losses called before."""
    from yolact_minimal_amd import hip
    g = torch.Generator().manual_seed(h + ow)
    m = torch.rand(3, h, w, generator=g)
    m[1] = E.rect_targets(E.random_boxes(1, g), h, w)[0]
    want = F.interpolate(m.double()[None], (oh, ow), mode='bilinear', align_corners=False)[0]
    m_d = m.to(DEV)
    out = torch.full((3, oh, ow), -7.0, device=DEV)
    hip.gt_masks_downsample(m_d, oh, ow, out)
    got = out.cpu()
    differs = got != (want > 0.5).float()
    assert bool(((got == 0) | (got == 1)).all())
    assert not bool((differs & ((want - 0.5).abs() > 1e-6)).any())
    assert int(differs.sum()) <= 1
    if h == w and oh == ow:
        old = torch.empty(3, oh, ow, device=DEV)
        hip.mask_resize_binarize(m_d, oh, ow, old)
        assert torch.equal(old, out)


# ---- 11. semantic loss edges -------------------------------------------------------------------------------------------------
def _semantic_edge_inputs():
    """7 x 9 map, 20 classes, three images whose middle one has no ground truth; image 0's first gt (class 4) covers the middle of
    the map, and its channel carries +-60 / +-100 both under the mask and outside it."""
    g = torch.Generator().manual_seed(21)
    boxes = [E.random_boxes(3, g, num_classes=20), torch.zeros(0, 5), E.random_boxes(2, g, num_classes=20)]
    boxes[0][0] = torch.tensor([0.2, 0.2, 0.8, 0.8, 4.0])
    boxes[0][2, 4] = 4.0                                                  # two gts of one class: their masks are OR-ed
    masks = [E.rect_targets(bx, 28, 36) for bx in boxes]
    nhwc = torch.randn(3, 7, 9, 32, generator=g) * 3
    big = torch.tensor([60.0, -60.0, 100.0, -100.0, 17.0, -17.0, 0.0])
    nhwc[0, :, :, 4] = big[torch.arange(63) % 7].reshape(7, 9)
    nhwc[2, :, :, 19] = big[(torch.arange(63) + 3) % 7].reshape(7, 9)
    nhwc[1, 0, :7, 0] = big
    return boxes, masks, nhwc


@pytest.mark.parametrize('padded', [True, False])
def test_semantic_loss_edges(padded):
    """Non-square map, nc = 20 at pitch 32 and contiguous, an image without ground truth between two that have some, logits up to
    +-100 (the stable softplus form: exp(100) overflows float32) against fp64 autograd; padding channels get exactly zero."""
    boxes, masks, nhwc = _semantic_edge_inputs()
    sp = nhwc[..., :20].permute(0, 3, 1, 2).double().contiguous().requires_grad_()
    ref = E.semantic_loss(sp, [m.double() for m in masks], [bx[:, 4].long() for bx in boxes])
    ref.backward()
    tgt0 = F.interpolate(masks[0][None], (7, 9), mode='bilinear', align_corners=False)[0, 0] > 0.5
    for v in (60.0, -60.0, 100.0, -100.0):                                 # the big logits sit on both sides of the mask
        at = nhwc[0, :, :, 4] == v
        assert bool(tgt0[at].any()) and bool((~tgt0)[at].any())
    base = nhwc.to(DEV).requires_grad_()
    sg = base[..., :20].permute(0, 3, 1, 2)
    if not padded:
        sg = sg.contiguous()
    got = _semantic(sg, masks, boxes)
    got.backward()
    gr = base.grad.cpu()
    print(f'semantic edges padded={padded}: {float(got):.9g} vs {float(ref):.9g}, dseg rel_err '
          f'{E.rel_err(gr[..., :20].permute(0, 3, 1, 2), sp.grad):.2e}')
    assert bool(torch.isfinite(gr).all())
    np.testing.assert_allclose(float(got.detach()), float(ref.detach()), rtol=2e-5)
    torch.testing.assert_close(gr[..., :20].permute(0, 3, 1, 2).double(), sp.grad, rtol=1e-4, atol=1e-9)
    assert float(gr[..., 20:].abs().max()) == 0.0
    # the image without ground truth: target all zero, d softplus(v) = sigmoid(v)
    want = torch.sigmoid(nhwc[1, ..., :20].double()) / 7 / 9 / 3
    torch.testing.assert_close(gr[1, ..., :20].double(), want, rtol=1e-4, atol=1e-9)


def test_semantic_loss_of_a_batch_without_any_ground_truth():
    """Every image empty (the kernel receives null gt pointers): the loss is the sum of softplus(v) over the real channels."""
    _, _, nhwc = _semantic_edge_inputs()
    base = nhwc[1:2].contiguous().to(DEV).requires_grad_()
    got = _semantic(base[..., :20].permute(0, 3, 1, 2), [torch.zeros(0, 28, 36)], [torch.zeros(0, 5)])
    got.backward()
    want = F.softplus(nhwc[1, ..., :20].double()).sum() / 7 / 9
    print(f'semantic, no gt: {float(got):.9g} vs {float(want):.9g}')
    np.testing.assert_allclose(float(got.detach()), float(want), rtol=2e-5)
    torch.testing.assert_close(base.grad.cpu()[0, ..., :20].double(), torch.sigmoid(nhwc[1, ..., :20].double()) / 7 / 9, rtol=1e-4, atol=1e-9)
    assert float(base.grad[..., 20:].abs().max()) == 0.0
