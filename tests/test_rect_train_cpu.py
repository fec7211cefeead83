"""Window training, the host half (no GPU): the fp64 restatement of the window losses (tests/rect_train_ref.py) against the unmodified
oracle through a zero-embedding into the square, and `sample_train_aug(window=)`: same draws as the square call, boxes by the
clip / drop / divide rule, samples with nothing inside the window rejected."""
import random

import numpy as np
import pytest
import torch

from oracle import yolact_ref as R
from tests import rect_train_ref as W


@pytest.mark.parametrize('hp,wp', [(24, 32), (32, 24), (20, 28)])
def test_window_mask_loss_restatement_equals_the_oracle_on_the_embedded_square(hp, wp):
    """Boxes that end two prototype rows or more before both cuts: the crop windows (padding 1) never reach the cut, so the oracle's
    `mask_loss` on the prototype map zero-embedded into Pv x Pv with the masks zero-padded to the square is the window loss."""
    pv, b, n_anchor = 32, 3, 120
    g = torch.Generator().manual_seed(5)
    proto = torch.relu(torch.randn(b, hp, wp, 32, generator=g)).double()
    coef = torch.tanh(torch.randn(b, n_anchor, 32, generator=g)).double()
    ey, ex = (hp - 2) / pv, (wp - 2) / pv                                # the largest box end: two rows / columns before the cut
    lo = torch.rand(b, 3, 2, generator=g) * 0.4
    hi = lo + 0.1 + torch.rand(b, 3, 2, generator=g) * 0.5
    gt = torch.cat([lo[..., :1] * ex, lo[..., 1:] * ey, torch.clamp(hi[..., :1], max=1) * ex, torch.clamp(hi[..., 1:], max=1) * ey], -1).double()
    gt[0, 0, 2], gt[0, 0, 3] = ex, ey                                    # one box exactly at that limit
    masks = []
    for i in range(b):
        m = torch.zeros(3, 4 * hp, 4 * wp, dtype=torch.float64)
        for j, (x1, y1, x2, y2) in enumerate((gt[i] * 4 * pv).round().long().tolist()):
            m[j, y1:y2, x1:x2] = 1.0
        masks.append(m)
    pos = torch.zeros(b, n_anchor, dtype=torch.bool)
    anchor_gt = torch.randint(0, 3, (b, n_anchor), generator=g)
    for i, n in enumerate((37, 0, 12)):
        pos[i, torch.randperm(n_anchor, generator=g)[:n]] = True
    anchor_box = torch.stack([gt[i][anchor_gt[i]] for i in range(b)])

    pw_, cw_ = proto.clone().requires_grad_(), coef.clone().requires_grad_()
    got = W.window_mask_loss(pos, anchor_gt, cw_, pw_, masks, anchor_box, pv)
    got.backward()
    emb = W.embed_in_square(proto, pv, (1, 2)).requires_grad_()
    co = coef.clone().requires_grad_()
    ref = R.mask_loss(pos, anchor_gt, co, emb, [W.embed_in_square(m, 4 * pv, (1, 2)) for m in masks], anchor_box)
    ref.backward()
    assert float(ref.detach()) > 0
    np.testing.assert_allclose(float(got.detach()), float(ref.detach()), rtol=1e-13)
    torch.testing.assert_close(pw_.grad, emb.grad[:, :hp, :wp], rtol=1e-12, atol=1e-15)
    torch.testing.assert_close(cw_.grad, co.grad, rtol=1e-12, atol=1e-15)
    outside = emb.grad.clone()
    outside[:, :hp, :wp] = 0
    assert float(outside.abs().max()) == 0.0                             # no gradient appears outside the window
    # the square ground-truth down-sample, cut to [:hp, :wp], is the per-axis down-sample of the cut masks bit for bit
    import torch.nn.functional as F
    for m in masks:
        sq = F.interpolate(W.embed_in_square(m, 4 * pv, (1, 2))[None], (pv, pv), mode='bilinear', align_corners=False)[0]
        cut = F.interpolate(m[None], (hp, wp), mode='bilinear', align_corners=False)[0]
        assert torch.equal(sq[:, :hp, :wp], cut)


def test_window_semantic_loss_restatement_equals_the_oracle_on_the_embedded_square():
    """Logits of -40 in the embedded region: softplus(-40) = 4e-18 per element is below fp64 rounding of the sum, so the oracle's
    semantic loss on the embedded 16 x 16 map equals the window loss on 12 x 16 to rounding (same divisor: sv = 16)."""
    g = torch.Generator().manual_seed(2)
    b, nc, mh, mw, sv = 2, 5, 12, 16, 16
    seg = torch.randn(b, nc, mh, mw, generator=g).double()
    masks = [(torch.rand(3, 8 * mh, 8 * mw, generator=g) > 0.6).double() for _ in range(b)]
    cls = [torch.randint(0, nc, (3,), generator=g) for _ in range(b)]
    got = W.window_semantic_loss(seg, masks, cls, sv)
    emb = torch.full((b, nc, sv, sv), -40.0, dtype=torch.float64)
    emb[:, :, :mh, :mw] = seg
    ref = R.semantic_loss(emb, [W.embed_in_square(m, 8 * sv, (1, 2)) for m in masks], cls)
    np.testing.assert_allclose(float(got), float(ref), rtol=1e-13)


def _sample(seed):
    r = np.random.default_rng(seed)
    h, w = (37, 53) if seed % 2 else (53, 37)
    n = 1 if seed % 3 == 0 else int(r.integers(1, 5))
    x1, y1 = r.uniform(0, w * 0.5, n), r.uniform(0, h * 0.5, n)
    boxes = np.stack([x1, y1, x1 + r.uniform(6, w * 0.5, n), y1 + r.uniform(6, h * 0.5, n)], 1)
    return h, w, boxes, r.integers(0, 80, n)


@pytest.mark.parametrize('window', [(32, 64), (64, 32), (32, 32)])
def test_sample_train_aug_window_draws_like_the_square_and_follows_the_box_rule(window):
    from yolact_minimal_amd.utils.augmentations import sample_train_aug
    size, (hn, wn) = 64, window
    kept = rejected_by_window = 0
    for seed in range(60):
        h, w, boxes, labels = _sample(seed)
        r_sq, r_win = random.Random(seed), random.Random(seed)
        sq = sample_train_aug(h, w, boxes, labels, size, r_sq)
        win = sample_train_aug(h, w, boxes, labels, size, r_win, window=window)
        assert r_sq.getstate() == r_win.getstate()                       # the same draws in the same order
        if sq is None:
            assert win is None                                           # (rejected by a crop: before the window matters)
            continue
        # the geometry the square call decided, carried in plain numpy; first the restatement itself against the square call
        carried, idx = W.carry_boxes(sq, w, boxes)
        want_sq = W.window_box_rule(carried, idx, size, size, size)
        assert want_sq is not None and np.array_equal(want_sq[0], sq.boxes) and np.array_equal(want_sq[1], sq.keep)
        want = W.window_box_rule(carried, idx, size, hn, wn)
        if want is None:
            assert win is None                                           # all boxes outside the window: the sample is rejected
            rejected_by_window += 1
            continue
        for f in ('mirror', 'crop', 'square', 'pad', 'resize', 'final_pad', 'final_crop', 'size', 'brightness', 'contrast', 'saturation', 'hue'):
            assert getattr(win, f) == getattr(sq, f), f
        assert win.window == (hn, wn) and getattr(sq, 'window', None) is None
        assert np.array_equal(win.boxes, want[0]) and np.array_equal(win.keep, want[1])
        assert np.array_equal(win.labels, np.array(labels)[want[1]])
        assert win.boxes[:, [0, 2]].max() <= (wn - 1) / size and win.boxes[:, [1, 3]].max() <= (hn - 1) / size   # in the square's frame
        kept += 1
    assert kept >= 10, (kept, rejected_by_window)            # (a certain rejection by the window: the next test)


def test_sample_outside_the_window_is_rejected_and_bad_windows_raise():
    from yolact_minimal_amd.utils.augmentations import AugPlan, sample_train_aug, sample_train_aug_batch

    class Fixed(random.Random):
        """randint in call order: no brightness, no contrast, no mirror, no random crop, resize to 8 * 32 = 256, final crop at (0, 0)."""

        def __init__(self):
            super().__init__(0)
            self.script = [0, 0, 0, 1, 8, 0, 0]

        def randint(self, a, b):
            v = self.script.pop(0)
            assert a <= v <= b
            return v

        def uniform(self, a, b):
            return a
    # a 64 x 64 picture -> 256 x 256 -> final crop at (0, 0): the box lies in rows 40 .. 60 of the sample, below a 32-row window
    box = np.array([[2.0, 10.0, 12.0, 15.0]])
    assert sample_train_aug(64, 64, box, [3], 64, Fixed()) is not None
    assert sample_train_aug(64, 64, box, [3], 64, Fixed(), window=(32, 64)) is None
    win = sample_train_aug(64, 64, box, [3], 64, Fixed(), window=(64, 32))
    assert isinstance(win, AugPlan) and win.window == (64, 32)
    with pytest.raises(RuntimeError, match='survived'):
        sample_train_aug_batch([(64, 64)], [box], [[3]], 64, Fixed(), window=(32, 64))
    for bad in ((48, 64), (0, 64), (96, 64), (64, 128)):
        with pytest.raises(RuntimeError, match='multiples of 32'):
            sample_train_aug(64, 64, box, [3], 64, Fixed(), window=bad)


def test_window_training_argument_checks_need_no_gpu():
    """The geometry checks of a window forward are host code: anchors of the window, Swin-T and bad shapes raise."""
    from yolact_minimal_amd.config import build_cfg
    from yolact_minimal_amd.modules.yolact import Yolact
    from yolact_minimal_amd.utils.rect import rect_anchor_index
    cfg = build_cfg('res50_coco', 'train', 96)
    net = Yolact(cfg).train()
    net.anchors = torch.tensor(net.anchors).reshape(-1, 4)
    anchors, virtual, levels = net._train_window(torch.zeros(2, 3, 64, 96))
    assert virtual == (24, 12) and levels[0] == (8, 12)
    assert anchors.shape[0] == rect_anchor_index(cfg, 64, 96).numel() == sum(h * w for h, w in levels) * 3
    assert torch.equal(anchors, net.anchors[rect_anchor_index(cfg, 64, 96)])
    for shape in ((2, 3, 64, 128), (2, 3, 128, 64), (2, 3, 48, 96), (2, 3, 64, 80)):
        with pytest.raises(RuntimeError):
            net._train_window(torch.zeros(shape))
    swin = Yolact(build_cfg('swin_tiny_coco', 'train', 96)).train()
    with pytest.raises(RuntimeError, match='Swin'):
        swin._train_window(torch.zeros(2, 3, 64, 96))
