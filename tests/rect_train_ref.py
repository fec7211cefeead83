"""Window training (yolact_minimal_amd/utils/rect.py) restated in plain torch / numpy, for the tests of it.

The network input is the top-left `Hn x Wn` window of the `S x S` sample; everything the network says stays in the square's
frame.  The prototype map is physically `Hp x Wp = Hn/4 x Wn/4` with the virtual extent `Pv = S/4` on both axes, the semantic map
`Hn/8 x Wn/8` with the virtual extent `S/8`:

  * crop window of a positive = box * Pv on both axes, the reference's padding of 1, clamped to Pv and then to the physical map;
  * mask loss * mask_alpha / Pv / Pv, 1 / area from the square-frame box;   semantic loss * semantic_alpha / (S/8) / (S/8) / B.

`window_mask_loss` / `window_semantic_loss` take any float dtype (the tests run them in fp64 under autograd) and are pinned against
the unmodified `oracle.yolact_ref.mask_loss` through `embed_in_square` (tests/test_rect_train_cpu.py).
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import yolact_ref as R


def window_crop_inside(boxes, hp, wp, pv, dtype, padding=1):
    """[hp, wp, n] bool: pixel inside the crop window of box n (0..1 of the square), virtual extent pv, physical map hp x wp."""
    def span(a, b, phys):
        a, b = a * pv, b * pv
        lo, hi = torch.min(a, b), torch.max(a, b)
        lo = torch.clamp(lo - padding, min=0)
        hi = torch.clamp(torch.clamp(hi + padding, max=pv), max=phys)
        return lo, hi
    x1, x2 = span(boxes[:, 0], boxes[:, 2], wp)
    y1, y2 = span(boxes[:, 1], boxes[:, 3], hp)
    xs = torch.arange(wp, dtype=dtype).view(1, -1, 1)
    ys = torch.arange(hp, dtype=dtype).view(-1, 1, 1)
    return (xs >= x1.view(1, 1, -1)) & (xs < x2.view(1, 1, -1)) & (ys >= y1.view(1, 1, -1)) & (ys < y2.view(1, 1, -1))


def window_mask_loss(pos, anchor_gt, coef_p, proto_p, mask_gt, anchor_box, pv, mask_alpha=6.125):
    """proto_p [B, hp, wp, 32], mask_gt[i] [g, 4 hp, 4 wp] (the window of the square's masks), anchor_box [B, N, 4] in 0..1 of the
    square.  No sub-sampling: callers keep the positives within masks_to_train."""
    hp, wp = proto_p.shape[1:3]
    total = 0
    for i in range(coef_p.shape[0]):
        idx = anchor_gt[i][pos[i]]
        if idx.shape[0] == 0:
            continue
        ds = F.interpolate(mask_gt[i].unsqueeze(0), (hp, wp), mode='bilinear', align_corners=False).squeeze(0)
        ds = ds.permute(1, 2, 0).contiguous().gt(0.5).to(proto_p.dtype)
        bx, cf = anchor_box[i][pos[i]], coef_p[i][pos[i]]
        inside = window_crop_inside(bx, hp, wp, pv, proto_p.dtype)
        mp = torch.sigmoid(proto_p[i] @ cf.t()) * inside.to(proto_p.dtype)
        l = F.binary_cross_entropy(torch.clamp(mp, 0, 1), ds[:, :, idx], reduction='none')
        area = (bx[:, 2] - bx[:, 0]) * (bx[:, 3] - bx[:, 1])
        total = total + torch.sum(l.sum(dim=(0, 1)) / area)
    return mask_alpha * total / pv / pv / pos.sum()


def window_semantic_loss(seg_p, mask_gt, class_gt, sv, semantic_alpha=1.0):
    """seg_p [B, C, mh, mw] logits, the top-left window of the sv x sv map."""
    b, nc, mh, mw = seg_p.shape
    total = 0
    for i in range(b):
        ds = F.interpolate(mask_gt[i].unsqueeze(0), (mh, mw), mode='bilinear', align_corners=False).squeeze(0)
        ds = ds.gt(0.5).to(seg_p.dtype)
        tgt = torch.zeros_like(seg_p[i])
        for j in range(ds.shape[0]):
            tgt[class_gt[i][j]] = torch.max(tgt[class_gt[i][j]], ds[j])
        total = total + F.binary_cross_entropy_with_logits(seg_p[i], tgt, reduction='sum')
    return semantic_alpha * total / sv / sv / b


def window_compute_loss(class_p, box_p, coef_p, proto_p, seg_p, box_class, mask_gt, anchors, size):
    """`oracle.yolact_ref.compute_loss` for a window step: the oracle's own match / class / box terms with the window's anchors, the
    restatements above for the mask and semantic terms."""
    b, n = box_p.shape[:2]
    offs = torch.zeros(b, n, 4, dtype=box_p.dtype)
    conf = torch.zeros(b, n, dtype=torch.int64)
    abox = torch.zeros(b, n, 4, dtype=box_p.dtype)
    aidx = torch.zeros(b, n, dtype=torch.int64)
    cls_gt = []
    for i in range(b):
        cls_gt.append(box_class[i][:, -1].long())
        offs[i], conf[i], abox[i], aidx[i] = R.match_anchors(box_class[i][:, :-1], anchors, cls_gt[i])
    pos = conf > 0
    return (R.ohem_class_loss(class_p, conf, pos), R.box_reg_loss(box_p, offs, pos),
            window_mask_loss(pos, aidx, coef_p, proto_p, mask_gt, abox, size // 4),
            window_semantic_loss(seg_p, mask_gt, cls_gt, size // 8))


def embed_in_square(x, side, dims):
    """Zero-embed `x` at the top-left of a tensor whose two dimensions `dims` have extent `side`."""
    shape = list(x.shape)
    for d in dims:
        shape[d] = side
    out = torch.zeros(shape, dtype=x.dtype)
    out[tuple(slice(0, s) for s in x.shape)] = x
    return out


def rect_case(hp, wp, pv, counts, n_anchor=300, seed=0):
    """A mask-loss case on an `hp x wp` map of virtual extent `pv`: per image `counts[i]` positives over 4 ground-truth boxes --
    one inside, one that reaches the cut exactly, one that extends past it (clamped), one small -- with rectangular masks drawn in
    the square's frame and cut to the window.  Returns (proto, coef, pos, anchor_gt, anchor_box, masks)."""
    g = torch.Generator().manual_seed(seed)
    b, size = len(counts), 4 * pv
    proto = torch.relu(torch.randn(b, hp, wp, 32, generator=g))
    coef = torch.tanh(torch.randn(b, n_anchor, 32, generator=g))
    ey, ex = hp / pv, wp / pv                                         # the cut, in 0..1 of the square
    gt = torch.tensor([[0.10 * ex, 0.10 * ey, 0.55 * ex, 0.60 * ey],
                       [0.30 * ex, 0.45 * ey, ex if ex < 1 else 0.8, ey if ey < 1 else 0.8],      # reaches the cut exactly
                       [0.50 * ex, 0.40 * ey, min(1.0, ex + 0.15), min(1.0, ey + 0.15)],          # extends past it
                       [0.05 * ex, 0.70 * ey, 0.25 * ex, 0.90 * ey]])
    full = torch.zeros(4, size, size)
    for j, (x1, y1, x2, y2) in enumerate((gt * size).round().long().tolist()):
        full[j, y1:y2, x1:x2] = 1.0
    masks = [full[:, :4 * hp, :4 * wp].contiguous() for _ in range(b)]
    pos = torch.zeros(b, n_anchor, dtype=torch.bool)
    anchor_gt = torch.randint(0, 4, (b, n_anchor), generator=g)
    for i, n in enumerate(counts):
        pos[i, torch.randperm(n_anchor, generator=g)[:n]] = True
    anchor_box = gt[anchor_gt]
    return proto, coef, pos, anchor_gt, anchor_box, masks


# ---- sample_train_aug(window=): the box bookkeeping in plain numpy -----------------------------------------------------------------
def carry_boxes(plan, img_w, boxes, keep_ratio=0.3):
    """The boxes of a sample through the geometry an AugPlan decided, up to (not including) the final clip: mirror, crop, pad to
    square, resize, pad / crop to the train size.  Returns (boxes [k, 4] in pixels of the S x S sample, indices [k] into the input)."""
    boxes = np.array(boxes, dtype=np.float64).reshape(-1, 4).copy()
    keep = np.arange(boxes.shape[0])
    if plan.mirror:
        boxes[:, 0::2] = img_w - boxes[:, 2::-2]

    def crop(boxes, keep, x1, y1, w, h):
        areas = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
        lo_x, lo_y = np.maximum(float(x1), boxes[:, 0]), np.maximum(float(y1), boxes[:, 1])
        hi_x, hi_y = np.minimum(float(x1 + w), boxes[:, 2]), np.minimum(float(y1 + h), boxes[:, 3])
        inter = np.clip(hi_x - lo_x, 0, 10000) * np.clip(hi_y - lo_y, 0, 10000)
        ok = inter / areas > keep_ratio
        out = np.stack([lo_x - x1, lo_y - y1, hi_x - x1, hi_y - y1], 1)[ok]
        return out, keep[ok]
    boxes, keep = crop(boxes, keep, *plan.crop)          # (no random crop: the whole image, which keeps boxes inside it as they are)
    boxes[:, [0, 2]] += plan.pad[0]
    boxes[:, [1, 3]] += plan.pad[1]
    boxes *= plan.resize / plan.square
    if plan.final_pad is not None:
        boxes[:, [0, 2]] += plan.final_pad[0]
        boxes[:, [1, 3]] += plan.final_pad[1]
    elif plan.final_crop is not None:
        boxes, keep = crop(boxes, keep, plan.final_crop[0], plan.final_crop[1], plan.size, plan.size)
    return boxes, keep


def window_box_rule(boxes, keep, size, hn, wn):
    """Clip x to 0 .. wn - 1 and y to 0 .. hn - 1, drop area <= 20, divide by `size`.  (boxes [k, 4] 0..1, keep [k]) or None."""
    boxes = boxes.copy()
    boxes[:, [0, 2]] = np.clip(boxes[:, [0, 2]], 0, wn - 1)
    boxes[:, [1, 3]] = np.clip(boxes[:, [1, 3]], 0, hn - 1)
    big = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1]) > 20
    if not big.any():
        return None
    return boxes[big] / size, keep[big]
