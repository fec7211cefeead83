"""tests/loss_edges_ref.py against oracle/yolact_ref.py: the references of tests/test_gpu_loss_edges.py are themselves checked
here, without a GPU, and so are the properties of the committed inputs that the GPU tests lean on."""
import math

import numpy as np
import pytest
import torch

from oracle import yolact_ref as R
from tests import loss_edges_ref as E


def _case():
    return E.mask_case([23, 0, 9], 34, 34, 120, seed=5)


def test_mask_loss_subset_with_every_positive_is_the_oracle():
    """subsets = None, and subsets = the positives spelled out: loss and both gradients equal R.mask_loss to 1e-12."""
    c = _case()
    ref = E.mask_loss_autograd(c, torch.float64)
    spelled = [torch.nonzero(p).flatten() for p in c['pos']]
    for subsets in ([None] * 3, spelled):
        got = E.mask_loss_autograd(c, torch.float64, subsets=subsets)
        for g, r in zip(got, ref):
            assert float((g - r).abs().max()) <= 1e-12 * float(r.abs().max())
    assert float(ref[1][1].abs().max()) == 0.0 and float(ref[0]) > 0


def test_mask_loss_subset_weights_a_strict_subset_like_the_reference():
    """Image 0 trains 7 of its 23 positives: the loss is (23 / 7) * the subset's per-anchor terms plus image 2's terms unweighted,
    divided by all 32 positives — the terms coming from an evaluation that shares nothing with the helper but the inputs."""
    c = _case()
    rows0 = torch.nonzero(c['pos'][0]).flatten()[[0, 3, 4, 9, 15, 21, 22]]
    rows2 = torch.nonzero(c['pos'][2]).flatten()
    got, _, dcoef = E.mask_loss_autograd(c, torch.float64, subsets=[rows0, None, None])
    args = (c['anchor_gt'], c['coef'], c['proto'], c['masks'], c['anchor_box'])
    t0, t2 = E.mask_terms_per_anchor(*args, 0, rows0), E.mask_terms_per_anchor(*args, 2, rows2)
    want = 6.125 * (float(t0.sum()) * 23 / 7 + float(t2.sum())) / 34 / 34 / 32
    np.testing.assert_allclose(float(got), want, rtol=1e-12)
    trained = dcoef.abs().sum(-1) > 0                                    # only the subset has a gradient
    assert torch.equal(torch.nonzero(trained[0]).flatten(), rows0) and torch.equal(trained[2], c['pos'][2])
    # and the terms add up to the oracle when nothing is left out
    full = E.mask_terms_per_anchor(*args, 0, torch.nonzero(c['pos'][0]).flatten())
    np.testing.assert_allclose(float(E.mask_loss_autograd(c, torch.float64)[0]),
                               6.125 * (float(full.sum()) + float(t2.sum())) / 34 / 34 / 32, rtol=1e-12)


def test_rect_targets_downsample_exactly():
    """4x down-sampling of the rectangular masks gives only k / 4: binarisation cannot depend on the precision."""
    m = E.rect_targets(E.random_boxes(3, torch.Generator().manual_seed(1)), 4 * 16, 4 * 32)
    for dt in (torch.float32, torch.float64):
        ds = torch.nn.functional.interpolate(m.to(dt).unsqueeze(0), (16, 32), mode='bilinear', align_corners=False)
        assert bool(((ds * 4).round() == ds * 4).all()) and float(ds.max()) == 1.0


def test_edge_boxes_reach_every_border():
    bx = E.edge_boxes(34)
    x1, x2, y1, y2 = R.crop_window(bx[:, :4].double(), 34, 34)
    assert float(x1[0]) == 0 and float(x2[1]) == 34 and float(y1[2]) == 0 and float(y2[2]) == 34
    assert [float(v[3]) for v in (x1, x2, y1, y2)] == [0, 34, 0, 34]
    np.testing.assert_allclose(float((bx[4, 2] - bx[4, 0]) * 34), 1.5, rtol=1e-6)
    for dt in (torch.float32, torch.float64):                             # both precisions see the same windows
        w = R.crop_window(bx[:, :4].to(dt), 34, 34)
        assert all(torch.equal(torch.ceil(a).long(), torch.ceil(b.to(dt)).long()) for a, b in zip(w, (x1, x2, y1, y2)))


@pytest.mark.parametrize('seed', E.SATURATED_SEEDS)
def test_saturated_case_has_a_finite_float32_reference_and_no_pixel_at_the_flip(seed):
    """max |z| = 58 <= 60; a good share of the pixels is saturated (sigmoid == 1.0f, the -100 clamp applies); the float32 oracle
    gives finite loss and gradients; at most 0.1 % of the pairs (none, for the committed seeds) lie within 1e-3 of the z at which
    float32 sigmoid becomes exactly 1, so the GPU test needs no exclusion mask."""
    c = E.saturated_case(seed)
    near, sat, zmax = E.saturation_flip_share(c)
    assert 20.0 <= zmax <= 60.0
    assert sat > 0.03
    assert near <= 1e-3 and near == 0.0
    loss, dproto, dcoef = E.mask_loss_autograd(c, torch.float32)
    assert math.isfinite(float(loss)) and bool(torch.isfinite(dproto).all()) and bool(torch.isfinite(dcoef).all())
    assert float(dproto.abs().max()) > 0 and float(dcoef.abs().max()) > 0
    # float32 really saturates: the clamp makes the float32 loss differ visibly from fp64, which is why fp64 is not the reference
    loss64 = E.mask_loss_autograd(c, torch.float64)[0]
    assert abs(float(loss) / float(loss64) - 1) > 1e-2
    s = torch.sigmoid(c['proto'][0] @ c['coef'][0][c['pos'][0]].t())
    assert float((s == 1.0).float().mean()) > 0.03


@pytest.mark.parametrize('col', [0, 7])
def test_underflow_case_has_a_finite_float32_reference(col):
    """The +200 logit sends every other background row's mark to -inf in float32 (not in fp64); the float32 oracle stays finite, and
    its negatives are the hot row (when it is not column 0) plus the LOWEST background indices."""
    class_p, box_p, offsets, conf, hot = E.underflow_case(seed=3, col=col)
    flat = class_p.reshape(-1, class_p.shape[-1])
    mark = torch.log(torch.exp(flat - flat.max()).sum(1)) + flat.max() - flat[:, 0]
    bg = (conf == 0).flatten()
    bg[hot] = False
    assert bool(torch.isinf(mark[bg]).all()) and bool((mark[bg] < 0).all())
    m64 = torch.log(torch.exp(flat.double() - flat.double().max()).sum(1))
    assert bool(torch.isfinite(m64).all())
    loss_c, loss_b, dclass, dbox = E.class_box_loss_f32(class_p, box_p, offsets, conf)
    for t in (loss_c, loss_b, dclass, dbox):
        assert bool(torch.isfinite(t).all())
    rows = dclass.abs().sum(-1) > 0
    mark = mark.reshape(conf.shape).clone()
    mark[conf != 0] = 0
    for i in range(conf.shape[0]):                                       # the ranking spelled out: larger mark first, then lower index
        npos = int((conf[i] > 0).sum())
        order = sorted(range(conf.shape[1]), key=lambda a: (-float(mark[i, a]), a))[:3 * npos]
        want = conf[i] > 0
        for a in order:
            if conf[i, a] == 0:
                want[a] = True
        assert int(want.sum()) > npos + 5                                # the ranking reaches into the -inf marks
        if i == 0 and col == 0:
            assert bool(want[hot])                                       # selected, but its gradient is exactly zero: softmax = one-hot
            want[hot] = False
        assert torch.equal(rows[i], want)
        lowest = torch.nonzero((conf[i] == 0) & (torch.arange(conf.shape[1]) != hot)).flatten()
        k = int(want.sum()) - npos - (1 if i == 0 and bool(want[hot]) else 0)
        assert bool(want[lowest[:k]].all())                               # ... and takes the lowest background indices there


def test_class_box_loss_f32_is_the_oracle_in_float32():
    """Away from any underflow the float32 helper agrees with the fp64 oracle to float32 rounding."""
    g = torch.Generator().manual_seed(0)
    class_p, box_p, offsets = torch.randn(2, 400, 9, generator=g), torch.randn(2, 400, 4, generator=g), torch.randn(2, 400, 4, generator=g)
    conf = torch.zeros(2, 400, dtype=torch.int64)
    conf[0, :12], conf[1, 100:130], conf[1, 7] = 3, 5, -1
    cp, bp = class_p.double().requires_grad_(), box_p.double().requires_grad_()
    rc, rb = R.ohem_class_loss(cp, conf, conf > 0, stable=True), R.box_reg_loss(bp, offsets.double(), conf > 0)
    (rc + rb).backward()
    lc, lb, dc, db = E.class_box_loss_f32(class_p, box_p, offsets, conf)
    np.testing.assert_allclose([float(lc), float(lb)], [float(rc.detach()), float(rb.detach())], rtol=1e-5)
    torch.testing.assert_close(dc.double(), cp.grad, rtol=1e-4, atol=1e-8)
    torch.testing.assert_close(db.double(), bp.grad, rtol=1e-4, atol=1e-8)


def test_semantic_loss_helper_is_the_oracle_and_takes_empty_images():
    g = torch.Generator().manual_seed(4)
    boxes = [E.random_boxes(3, g, num_classes=20) for _ in range(3)]
    masks = [E.rect_targets(bx, 28, 36).double() for bx in boxes]
    seg = torch.randn(3, 20, 7, 9, generator=g, dtype=torch.float64)
    cls = [bx[:, 4].long() for bx in boxes]
    np.testing.assert_allclose(float(E.semantic_loss(seg, masks, cls)), float(R.semantic_loss(seg, masks, cls)), rtol=1e-14)
    with_empty = E.semantic_loss(seg, [masks[0], masks[1][:0], masks[2]], [cls[0], cls[1][:0], cls[2]])
    alone = [E.semantic_loss(seg[i:i + 1], [masks[i]], [cls[i]]) for i in (0, 2)]
    softplus = torch.nn.functional.softplus(seg[1]).sum() / 7 / 9
    np.testing.assert_allclose(float(with_empty), float((alone[0] + alone[1] + softplus) / 3), rtol=1e-13)


def test_rel_err_is_the_smallest_passing_rtol():
    ref = torch.tensor([1.0, -2.0, 0.0, 4.0])
    got = ref + torch.tensor([1e-3, 0.0, 1e-4, -2e-3])
    r = E.rel_err(got, ref)
    torch.testing.assert_close(got, ref, rtol=r * 1.0001, atol=0.1 * r * 1.0001 * 4.0)
    with pytest.raises(AssertionError):
        torch.testing.assert_close(got, ref, rtol=r * 0.99, atol=0.1 * r * 0.99 * 4.0)
