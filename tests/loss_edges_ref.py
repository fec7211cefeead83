"""Plain references and input builders for tests/test_gpu_loss_edges.py.  Plain torch on the CPU: no GPU is needed, the library is
not called; tests/test_loss_edges_cpu.py pins everything here against oracle/yolact_ref.py.

`mask_loss_subset`   the mask term (reference modules/yolact.py:241-291) INCLUDING the branch the oracle leaves out: an image with
                     more positives than the cap trains a subset.  The subset is an argument (the reference draws it with
                     randperm, the library with its own device generator), everything after the draw is restated: the subset's
                     terms are weighted by positives / len(subset), and the batch is divided by ALL positives, trained or not.
                     The dtype of the operands is the dtype of the arithmetic (float64 for the oracle, float32 where the
                     reference's own rounding is the specification).
`mask_terms_per_anchor`  an independent evaluation, one anchor at a time with a hand-written BCE, of the per-anchor terms
                     sum_pix BCE / area that both functions above add up.
`class_box_loss_f32` the oracle's OHEM class loss (stable ranking) and box loss in float32 with their autograd gradients: the
                     specification where the reference's float32 behaviour is the point (marks that underflow to -inf).
`semantic_loss`      the oracle's semantic loss, extended to images without ground truth (target all zero).

Saturation.  In float32 sigmoid(z) = 1 / (1 + exp(-z)) is exactly 1.0 once exp(-z) <= 2^-24, i.e. z >= SAT_Z = 24 ln 2 = 16.6355:
there log(1 - m) = -inf is clamped to -100 and the gradient is 0, just below it the loss term is 16.6 and the gradient is the
weight.  That jump is in the reference itself, so a pixel whose z lies within FLIP_BAND of SAT_Z may legitimately land on either
side on another device; `saturation_flip_share` counts them (fp64 z, from the inputs alone).
"""
import math

import torch
import torch.nn.functional as F

from oracle import yolact_ref as R

SAT_Z = 24.0 * math.log(2.0)
FLIP_BAND = 1e-3
SATURATED_SEEDS = (0, 1)      # seeds of `saturated_case` with no pair inside the band (tests/test_loss_edges_cpu.py asserts it)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def rect_targets(boxes, h, w):
    """Rectangular {0,1} float masks [g, h, w] of normalised corner boxes [g, >= 4] (like utils/synthetic.synth_targets, but at any
    h x w, so that a 4x down-sampling to a non-square prototype map is exact: every sample is the mean of a 2 x 2 block)."""
    m = torch.zeros(boxes.shape[0], h, w)
    for j, bx in enumerate(boxes[:, :4].tolist()):
        m[j, round(bx[1] * h):round(bx[3] * h), round(bx[0] * w):round(bx[2] * w)] = 1.0
    return m


def random_boxes(g, gen, num_classes=80):
    """[g, 5] boxes (x1, y1, x2, y2, cls) inside [0.05, 0.95] with sides in [0.1, 0.35]."""
    xy = torch.rand(g, 2, generator=gen) * 0.55 + 0.05
    wh = torch.rand(g, 2, generator=gen) * 0.25 + 0.1
    cls = torch.randint(0, num_classes, (g, 1), generator=gen).float()
    return torch.cat([xy, xy + wh, cls], 1)


def mask_case(counts, hp, wp, n_anchor, seed, boxes=None, n_gt=3, coef_scale=1.0):
    """Inputs of the mask term for len(counts) images with counts[i] positives each, drawn from `seed`: prototypes [b, hp, wp, 32],
    coefficients [b, n_anchor, 32], the positives, their gt index and matched box, and the gt masks at 4x the prototype size.
    `boxes`: per-image [g, 5] gt boxes to use instead of random ones."""
    gen = torch.Generator().manual_seed(seed)
    b = len(counts)
    proto = torch.relu(torch.randn(b, hp, wp, 32, generator=gen))
    coef = torch.tanh(torch.randn(b, n_anchor, 32, generator=gen)) * coef_scale
    if boxes is None:
        boxes = [random_boxes(n_gt, gen) for _ in range(b)]
    masks = [rect_targets(bx, 4 * hp, 4 * wp) for bx in boxes]
    pos = torch.zeros(b, n_anchor, dtype=torch.bool)
    anchor_gt = torch.zeros(b, n_anchor, dtype=torch.int64)
    anchor_box = torch.zeros(b, n_anchor, 4)
    for i, c in enumerate(counts):
        pos[i, torch.randperm(n_anchor, generator=gen)[:c]] = True
        anchor_gt[i] = torch.randint(0, boxes[i].shape[0], (n_anchor,), generator=gen)
        anchor_box[i] = boxes[i][anchor_gt[i], :4]
    return dict(proto=proto, coef=coef, pos=pos, anchor_gt=anchor_gt, anchor_box=anchor_box, masks=masks, boxes=boxes)


def edge_boxes(hp):
    """Gt boxes whose crop windows touch every border of an hp x hp map: x1 = 0; x2 = 1; y1 = 0 and y2 = 1; a padded window that is
    the whole map; a box 1.5 prototype pixels wide (weight 1 / area = 75 x that of a typical box).  No coordinate times hp is an
    integer except the exact 0 / hp, so float32 and float64 agree on every window."""
    assert hp == 34
    return torch.tensor([[0.0, 0.2, 0.3, 0.6, 3.0],
                         [0.7, 0.3, 1.0, 0.8, 5.0],
                         [0.4, 0.0, 0.6, 1.0, 7.0],
                         [0.02, 0.02, 0.98, 0.98, 9.0],
                         [0.5, 0.3, 0.5 + 1.5 / hp, 0.6, 11.0]])


def saturated_case(seed, hp=34, n_anchor=200, count=24, zmax=58.0):
    """A one-image mask case whose coefficients are scaled so that max |z| = zmax over the trained anchors (<= 60: exp(60) and
    sigmoid(-60) = 8.8e-27 are normal float32 numbers, nothing enters the denormal band)."""
    c = mask_case([count], hp, hp, n_anchor, seed)
    z = c['proto'][0].double() @ c['coef'][0][c['pos'][0]].double().t()
    c['coef'] = (c['coef'].double() * (zmax / float(z.abs().max()))).float()
    return c


def saturation_flip_share(c):
    """(share of the (pixel, positive) pairs inside their crop window whose fp64 z is within FLIP_BAND of SAT_Z, share of the
    pairs that are saturated, max |z|)."""
    near = sat = total = 0
    zmax = 0.0
    for i in range(c['proto'].shape[0]):
        p = c['pos'][i]
        if not bool(p.any()):
            continue
        z = c['proto'][i].double() @ c['coef'][i][p].double().t()
        inside = R.crop(torch.ones_like(z), c['anchor_box'][i][p].double()) > 0
        near += int(((z - SAT_Z).abs() < FLIP_BAND)[inside].sum())
        sat += int((z >= SAT_Z)[inside].sum())
        total += int(inside.sum())
        zmax = max(zmax, float(z.abs().max()))
    return near / total, sat / total, zmax


# ---- mask term ---------------------------------------------------------------------------------------------------------------
def mask_loss_subset(pos, anchor_gt, coef_p, proto_p, mask_gt, anchor_box, subsets=None, mask_alpha=6.125):
    """The mask term with an explicit trained subset per image.  subsets[i]: int64 anchor indices of image i that are trained (all
    of them positives), or None for "every positive"; `subsets=None` trains every positive of every image."""
    ph, pw = proto_p.shape[1:3]
    total = 0
    for i in range(coef_p.shape[0]):
        ds = F.interpolate(mask_gt[i].unsqueeze(0), (ph, pw), mode='bilinear', align_corners=False).squeeze(0)
        ds = ds.permute(1, 2, 0).contiguous().gt(0.5).to(proto_p.dtype)
        old_num = int(pos[i].sum())
        if old_num == 0:
            continue
        rows = torch.nonzero(pos[i]).flatten() if subsets is None or subsets[i] is None else torch.as_tensor(subsets[i])
        assert bool(pos[i][rows].all()), 'a trained anchor that is not a positive'
        num = rows.numel()
        idx, bx, cf = anchor_gt[i][rows], anchor_box[i][rows], coef_p[i][rows]
        gt = ds[:, :, idx]
        mp = R.crop(torch.sigmoid(proto_p[i] @ cf.t()), bx)
        l = F.binary_cross_entropy(torch.clamp(mp, 0, 1), gt, reduction='none')
        area = (bx[:, 2] - bx[:, 0]) * (bx[:, 3] - bx[:, 1])
        l = l.sum(dim=(0, 1)) / area
        if old_num > num:
            l = l * (old_num / num)
        total = total + torch.sum(l)
    return mask_alpha * total / ph / pw / pos.sum()


def mask_terms_per_anchor(anchor_gt, coef_p, proto_p, mask_gt, anchor_box, image, rows):
    """[len(rows)] float64 terms sum_pix BCE(crop(sigmoid(proto . coef_a)), gt_a) / area_a of image `image`, one anchor and one
    pixel row at a time, with the window and the BCE (log clamped at -100) written out by hand."""
    ph, pw = proto_p.shape[1:3]
    ds = F.interpolate(mask_gt[image].double().unsqueeze(0), (ph, pw), mode='bilinear', align_corners=False).squeeze(0) > 0.5
    out = []
    for a in [int(r) for r in rows]:
        x1, y1, x2, y2 = [float(v) for v in anchor_box[image, a].double()]
        wx1, wx2 = max(min(x1, x2) * pw - 1, 0.0), min(max(x1, x2) * pw + 1, float(pw))
        wy1, wy2 = max(min(y1, y2) * ph - 1, 0.0), min(max(y1, y2) * ph + 1, float(ph))
        cf = coef_p[image, a].double()
        t = ds[int(anchor_gt[image, a])]
        s = 0.0
        for y in range(ph):
            z = proto_p[image, y].double() @ cf                          # [pw]
            for x in range(pw):
                inside = wx1 <= x < wx2 and wy1 <= y < wy2
                m = 1.0 / (1.0 + math.exp(-float(z[x]))) if inside else 0.0
                if bool(t[y, x]):
                    s += 100.0 if m == 0.0 else min(-math.log(m), 100.0)
                else:
                    s += 100.0 if m == 1.0 else min(-math.log1p(-m), 100.0)
        out.append(s / ((x2 - x1) * (y2 - y1)))
    return torch.tensor(out, dtype=torch.float64)


def mask_loss_autograd(c, dtype, subsets=None, masks_to_train=None):
    """(loss, dproto, dcoef) of a `mask_case` in `dtype` on the CPU: `R.mask_loss` (the oracle as it stands), or `mask_loss_subset`
    when `subsets` is given."""
    pr, cf = c['proto'].detach().to(dtype).clone().requires_grad_(), c['coef'].detach().to(dtype).clone().requires_grad_()
    masks, abox = [m.to(dtype) for m in c['masks']], c['anchor_box'].to(dtype)
    if subsets is None:
        loss = R.mask_loss(c['pos'], c['anchor_gt'], cf, pr, masks, abox, masks_to_train=masks_to_train or 10 ** 6)
    else:
        loss = mask_loss_subset(c['pos'], c['anchor_gt'], cf, pr, masks, abox, subsets)
    loss.backward()
    return loss.detach(), pr.grad, cf.grad


# ---- class + box -------------------------------------------------------------------------------------------------------------
def class_box_loss_f32(class_p, box_p, offsets, conf, conf_alpha=1.0, bbox_alpha=1.5, ratio=3):
    """(loss_c, loss_b, dclass, dbox) of the oracle in float32 on the CPU, ranking ties by the lower index."""
    cp, bp = class_p.detach().float().clone().requires_grad_(), box_p.detach().float().clone().requires_grad_()
    pos = conf > 0
    loss_c = R.ohem_class_loss(cp, conf, pos, conf_alpha=conf_alpha, ratio=ratio, stable=True)
    loss_b = R.box_reg_loss(bp, offsets.float(), pos, bbox_alpha=bbox_alpha)
    (loss_c + loss_b).backward()
    return loss_c.detach(), loss_b.detach(), cp.grad, bp.grad


def underflow_case(seed, col, b=2, n=1500, nc=81, npos=10, nneutral=5):
    """Class logits N(0, 2) with one background row of image 0 holding +200 in column `col`: every other row's exp(x - 200)
    underflows in float32, so its mark is log(0) + 200 - x0 = -inf.  With 3 * npos > npos + nneutral + 1 the ranking reaches into
    the -inf marks, which are all equal: the lowest anchor indices are the negatives.  n > 1024: more than one pass of the
    selection kernel's workgroup."""
    gen = torch.Generator().manual_seed(seed)
    class_p = torch.randn(b, n, nc, generator=gen) * 2
    box_p = torch.randn(b, n, 4, generator=gen) * 1.5
    offsets = torch.randn(b, n, 4, generator=gen)
    conf = torch.zeros(b, n, dtype=torch.int64)
    for i in range(b):
        sel = torch.randperm(n, generator=gen)
        conf[i, sel[:npos]] = torch.randint(1, nc, (npos,), generator=gen)
        conf[i, sel[npos:npos + nneutral]] = -1
    hot = int(torch.nonzero(conf[0] == 0).flatten()[n // 2])
    class_p[0, hot, col] = 200.0
    return class_p, box_p, offsets, conf, hot


# ---- semantic ----------------------------------------------------------------------------------------------------------------
def semantic_loss(seg_p, mask_gt, class_gt, semantic_alpha=1.0):
    """`R.semantic_loss` (modules/yolact.py:293-313) that also takes images with no ground truth: their target is all zero, so
    every element contributes softplus(v)."""
    b, nc, mh, mw = seg_p.shape
    total = 0
    for i in range(b):
        tgt = torch.zeros_like(seg_p[i])
        if mask_gt[i].shape[0]:
            ds = F.interpolate(mask_gt[i].unsqueeze(0), (mh, mw), mode='bilinear', align_corners=False).squeeze(0)
            ds = ds.gt(0.5).to(seg_p.dtype)
            for j in range(ds.shape[0]):
                tgt[class_gt[i][j]] = torch.max(tgt[class_gt[i][j]], ds[j])
        total = total + F.binary_cross_entropy_with_logits(seg_p[i], tgt, reduction='sum')
    return semantic_alpha * total / mh / mw / b


# ---- error figures -----------------------------------------------------------------------------------------------------------
def rel_err(got, ref, floor=0.1):
    """The smallest r for which assert_close(got, ref, rtol=r, atol=floor * r * max|ref|) holds: the suite's gradient bars have this
    shape (rtol = 1e-4 with atol = 1e-5 * max|ref|)."""
    got, ref = got.double(), ref.double()
    return float(((got - ref).abs() / (ref.abs() + floor * ref.abs().max())).max())
