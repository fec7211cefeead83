"""`val_aug` on the GPU (SURVEY.md §8f "next" row 1).

Reference: `/root/reference/utils/augmentations.py:219-227` (`pad_to_square :138-165`, `multi_scale_resize :168-189`
= `cv2.resize`, `normalize_and_toRGB :212-216`).  Same call shape — `val_aug(img, val_size)` with an HWC BGR image —
but `img` is a CUDA tensor (uint8 or float32) and the result is a CUDA float32 tensor `[3, S, S]`; one HIP launch, the
padded square is never materialised.  cv2 is not present in the build image, so this row is pinned against a torch
restatement (pad + `F.interpolate(align_corners=False)`, the equivalence the reference itself notes at
`utils/output_utils.py:225`), not against cv2 — "parity unpinned by the reference".
`val_aug_batch(frames, val_size)` is the same for a batch of frames of different sizes (a `FrameBatch`, utils/frames.py) in one launch
of the same kernel: `[B, 3, S, S]`, row b bit for bit `val_aug(frame_b, val_size)`.
"""
import ctypes

import torch

from .. import hip
from ..config import norm_mean, norm_std

_MEAN = (ctypes.c_float * 3)(*[float(v) for v in norm_mean])
_STD = (ctypes.c_float * 3)(*[float(v) for v in norm_std])


def _window(window, val_size, what):
    """`window=None` -> the square; else `(Hn, Wn)` inside it."""
    if window is None:
        return None
    hn, wn = int(window[0]), int(window[1])
    if not (0 < hn <= val_size and 0 < wn <= val_size):
        raise RuntimeError(f'{what}: window {hn} x {wn} is not inside {val_size} x {val_size}')
    return hn, wn


def val_aug(img, val_size, window=None):
    """`window=(Hn, Wn)`: only the top-left `Hn x Wn` of the `[3, S, S]` result, bit for bit (`ym_val_preprocess_window`, the same
    kernel): the input of a rectangular forward (utils/rect.py).  `window=None`: the reference's square."""
    if not (torch.is_tensor(img) and img.is_cuda):
        raise RuntimeError('yolact_minimal_amd.utils.augmentations.val_aug expects a CUDA tensor (HWC, BGR)')
    if img.dtype not in (torch.uint8, torch.float32) or img.dim() != 3 or img.shape[2] != 3:
        raise RuntimeError('val_aug: image must be [H, W, 3] uint8 or float32')
    img = img.contiguous()
    h, w, _ = img.shape
    window = _window(window, int(val_size), 'val_aug')
    if window is not None:
        out = torch.empty(3, *window, dtype=torch.float32, device=img.device)
        with torch.cuda.device(img.device):
            hip.check(hip.lib().ym_val_preprocess_window(ctypes.c_void_p(img.data_ptr()), int(img.dtype == torch.uint8),
                                                         hip.ragged_table([(h, w)], [0]), 1, int(val_size), *window, _MEAN, _STD,
                                                         hip.ptr(out), hip.stream_ptr()), 'ym_val_preprocess_window')
        return out
    out = torch.empty(3, val_size, val_size, dtype=torch.float32, device=img.device)
    with torch.cuda.device(img.device):
        hip.check(hip.lib().ym_val_preprocess(ctypes.c_void_p(img.data_ptr()), int(img.dtype == torch.uint8), h, w, val_size, _MEAN,
                                              _STD, hip.ptr(out), hip.stream_ptr()), 'ym_val_preprocess')
    return out


def val_aug_batch(frames, val_size, out=None, window=None):
    """`val_aug` for B frames of different sizes in ONE launch (`ym_val_preprocess_batch`) -> float32 `[B, 3, S, S]`.
    `frames`: a `FrameBatch` (utils/frames.py), or a list of device HWC BGR tensors (all uint8 or all float32), which is packed
    through `FrameBatch.from_tensors` first.  `out`: a contiguous float32 device tensor whose first B rows `[3, S, S]` are written
    (a pipeline slot's own input buffer); the result is then `out[:B]`.  Row b equals `val_aug(frame_b, val_size)` bit for bit: the
    two entries are one kernel.  No host synchronisation.
    `window=(Hn, Wn)`: rows are `[3, Hn, Wn]`, the top-left window of the square rows bit for bit (`ym_val_preprocess_window`)."""
    from .frames import FrameBatch
    val_size = int(val_size)
    if not isinstance(frames, FrameBatch):
        frames = FrameBatch.from_tensors(frames)
    frames.need_cuda('utils.augmentations.val_aug_batch')
    batch = len(frames)
    if val_size < 1:
        raise RuntimeError(f'val_aug_batch: val_size = {val_size}')
    window = _window(window, val_size, 'val_aug_batch')
    hn, wn = window if window is not None else (val_size, val_size)
    if out is None:
        out = torch.empty(batch, 3, hn, wn, dtype=torch.float32, device=frames.device)
    elif not torch.is_tensor(out) or not out.is_cuda or out.device != frames.device or out.dtype != torch.float32 or out.dim() != 4 or \
            out.shape[0] < batch or tuple(out.shape[1:]) != (3, hn, wn) or not out.is_contiguous():
        raise RuntimeError(f'val_aug_batch: out is a contiguous float32 [>= {batch}, 3, {hn}, {wn}] tensor on the device of the frames')
    if window is not None:
        with torch.cuda.device(frames.device):
            hip.check(hip.lib().ym_val_preprocess_window(ctypes.c_void_p(frames.data.data_ptr()), int(frames.dtype == torch.uint8),
                                                         frames.table(), batch, val_size, hn, wn, _MEAN, _STD, hip.ptr(out),
                                                         hip.stream_ptr()), 'ym_val_preprocess_window')
        return out[:batch]
    with torch.cuda.device(frames.device):
        hip.check(hip.lib().ym_val_preprocess_batch(ctypes.c_void_p(frames.data.data_ptr()), int(frames.dtype == torch.uint8),
                                                    frames.table(), batch, val_size, _MEAN, _STD, hip.ptr(out), hip.stream_ptr()),
                  'ym_val_preprocess_batch')
    return out[:batch]


# ------------------------------------------------------------------------------------------------------------------------
# train_aug.  Reference: utils/augmentations.py:9-252 — photometric_distort :60-77, random_mirror :9-16,
# random_crop / crop :80-136, pad_to_square(during_training) :138-165, multi_scale_resize :168-189, to_train_size :192-209,
# clip_box / remove_small_box / to_01_box :19-36, normalize_and_toRGB :212-216, train_aug :230-252.
#
# The reference runs this chain on the CPU in DataLoader workers: ten numpy / cv2 passes over the image and over every mask.
# Here the RANDOM DECISIONS and the box bookkeeping stay on the host (`sample_train_aug`, a few hundred scalar operations, same
# `random` call order as the reference so that a seeded run makes the same choices), and the pixel work is ONE HIP launch for
# the image and one for the masks: every output pixel walks the chain backwards (train-size pad/crop -> bilinear resize ->
# pad-to-square -> crop -> mirror) to its four source texels, applies the photometric distortion to them, blends, normalises.
# cv2 is absent from the image: resize / HSV follow OpenCV's documented float32 formulas and are pinned against a torch / numpy
# restatement (oracle/augment_ref.py), not against cv2 — "parity unpinned by the reference" for those two steps; the random
# decisions and the geometry are pinned against the reference's own numpy functions (oracle/make_golden_augment.py).
# ------------------------------------------------------------------------------------------------------------------------
import random as _random


class AugPlan:
    """Everything `train_aug` decided for one sample.  Geometry is a chain of integer offsets around ONE bilinear resize:
    original --mirror--> --crop (cx, cy, cw, ch)--> --pad to square q (px, py)--> --resize q -> r--> --final: pad (fx, fy)
    into s or crop (fx, fy) of s--> [s, s]."""
    __slots__ = ('brightness', 'contrast', 'saturation', 'hue', 'mirror', 'crop', 'square', 'pad', 'resize', 'final_pad',
                 'final_crop', 'size', 'boxes', 'labels', 'keep', 'window')


def _train_window(window, train_size, what):
    """`window=None` -> the square sample; else `(Hn, Wn)`: its top-left window, the input of a window training step
    (utils/rect.py) -- both sides positive multiples of 32 and at most `train_size`."""
    if window is None:
        return None
    hn, wn = int(window[0]), int(window[1])
    if hn < 32 or wn < 32 or hn % 32 or wn % 32 or hn > train_size or wn > train_size:
        raise RuntimeError(f'{what}: window {hn} x {wn}: both sides are positive multiples of 32 inside {train_size} x {train_size}')
    return hn, wn


def _crop_boxes(rng, ori_h, crop_h, ori_w, crop_w, boxes, labels, keep_idx, keep_ratio=0.3):
    """The rejection loop of `crop` (:80-125) on boxes only -> (x1, y1, boxes, labels, keep_idx) or None after 1000 tries."""
    import numpy as np
    areas = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    for _ in range(1000):
        x1 = rng.randint(0, ori_w - crop_w)
        y1 = rng.randint(0, ori_h - crop_h)
        mnx = np.maximum(np.float64(x1), boxes[:, 0])
        mny = np.maximum(np.float64(y1), boxes[:, 1])
        mxx = np.minimum(np.float64(x1 + crop_w), boxes[:, 2])
        mxy = np.minimum(np.float64(y1 + crop_h), boxes[:, 3])
        inter = np.clip(mxx - mnx, 0, 10000) * np.clip(mxy - mny, 0, 10000)
        keep = (inter / areas) > keep_ratio
        if keep.any():
            nb = np.stack([mnx, mny, mxx, mxy], 1)[keep]
            nb[:, [0, 2]] -= x1
            nb[:, [1, 3]] -= y1
            return x1, y1, nb, labels[keep], keep_idx[keep]
    return None


def sample_train_aug(img_h, img_w, boxes, labels, train_size, rng=_random, window=None):
    """Draw the random decisions of `train_aug` in the reference's order and carry the boxes through them.
    boxes [n,4] pixels (x1,y1,x2,y2) — float64 like the dataset's `np.array(box_list)` (utils/coco.py:97), labels [n].
    Returns an AugPlan, or None where the reference returns Nones.
    `window=(Hn, Wn)`: the sample is the top-left window of the `train_size` square one.  The draws and their order are those of
    the square call (a seeded run decides the same geometry, `rng` ends in the same state); only the last step differs: boxes are
    clipped to the window (x to 0 .. Wn - 1, y to 0 .. Hn - 1), dropped at area <= 20 and divided by `train_size` -- they stay in
    the square's frame.  None when no box is left in the window."""
    import numpy as np
    window = _train_window(window, int(train_size), 'sample_train_aug')
    p = AugPlan()
    p.window = window
    boxes = np.array(boxes, dtype=np.float64).reshape(-1, 4)
    labels = np.array(labels)
    keep_idx = np.arange(boxes.shape[0])
    # photometric_distort (:60-77)
    p.brightness = rng.uniform(-32, 32) if rng.randint(0, 1) else None
    p.contrast = rng.uniform(0.7, 1.3) if rng.randint(0, 1) else None
    p.saturation = rng.uniform(0.7, 1.3)
    p.hue = rng.uniform(-15., 15.)
    # random_mirror (:9-16)
    p.mirror = bool(rng.randint(0, 1))
    if p.mirror:
        boxes[:, 0::2] = img_w - boxes[:, 2::-2]
    # random_crop (:128-136)
    h, w = img_h, img_w
    p.crop = (0, 0, w, h)
    if not rng.randint(0, 1):
        crop_h = int(rng.uniform(0.6, 1) * h)
        crop_w = int(rng.uniform(0.6, 1) * w)
        r = _crop_boxes(rng, h, crop_h, w, crop_w, boxes, labels, keep_idx)
        if r is None:
            return None
        x1, y1, boxes, labels, keep_idx = r
        p.crop = (x1, y1, crop_w, crop_h)
        h, w = crop_h, crop_w
    # pad_to_square, during_training (:138-163)
    q = max(h, w)
    px = py = 0
    if h < w:
        py = rng.randint(0, w - h)
        boxes[:, [1, 3]] += py
    if h > w:
        px = rng.randint(0, h - w)
        boxes[:, [0, 2]] += px
    p.square, p.pad = q, (px, py)
    # multi_scale_resize (:168-186)
    r_size = rng.randint(8, 24) * 32
    boxes *= r_size / q
    p.resize = r_size
    # to_train_size (:192-209)
    p.final_pad = p.final_crop = None
    if r_size < train_size:
        fy = rng.randint(0, train_size - r_size)
        fx = rng.randint(0, train_size - r_size)
        boxes[:, [1, 3]] += fy
        boxes[:, [0, 2]] += fx
        p.final_pad = (fx, fy)
    elif r_size > train_size:
        r = _crop_boxes(rng, r_size, train_size, r_size, train_size, boxes, labels, keep_idx)
        if r is None:
            return None
        fx, fy, boxes, labels, keep_idx = r
        p.final_crop = (fx, fy)
    p.size = train_size
    # clip_box, remove_small_box, to_01_box (:19-36)
    hn, wn = window if window is not None else (train_size, train_size)
    boxes[:, [0, 2]] = np.clip(boxes[:, [0, 2]], 0, wn - 1)
    boxes[:, [1, 3]] = np.clip(boxes[:, [1, 3]], 0, hn - 1)
    big = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1]) > 20
    boxes, labels, keep_idx = boxes[big], labels[big], keep_idx[big]
    if boxes.shape[0] == 0:
        return None
    boxes[:, [0, 2]] /= train_size
    boxes[:, [1, 3]] /= train_size
    p.boxes, p.labels, p.keep = boxes, labels, keep_idx
    return p


def plan_to_c(plan, img_h, img_w):
    """AugPlan -> the C-ABI `ym_aug_plan`."""
    c = hip.AugPlanC()
    c.H, c.W, c.mirror = img_h, img_w, int(plan.mirror)
    c.cx, c.cy, c.cw, c.ch = plan.crop
    c.q, (c.px, c.py), c.r, c.S = plan.square, plan.pad, plan.resize, plan.size
    c.final_mode, c.fx, c.fy = 0, 0, 0
    if plan.final_pad is not None:
        c.final_mode, (c.fx, c.fy) = 1, plan.final_pad
    elif plan.final_crop is not None:
        c.final_mode, (c.fx, c.fy) = 2, plan.final_crop
    c.has_brightness, c.brightness = int(plan.brightness is not None), float(plan.brightness or 0.0)
    c.has_contrast, c.contrast = int(plan.contrast is not None), float(plan.contrast if plan.contrast is not None else 1.0)
    c.saturation, c.hue = float(plan.saturation), float(plan.hue)
    for i in range(3):
        c.mean[i], c.std[i] = float(norm_mean[i]), float(norm_std[i])
    return c


def _plan_window(plan, window, what):
    """The window a pixel call writes: the explicit `window`, else the one the plan was drawn for, else None (the square)."""
    if window is None:
        return getattr(plan, 'window', None)
    return _train_window(window, int(plan.size), what)


def apply_train_aug(img, masks, plan, window=None):
    """The pixel half of `train_aug` on the device: img [H,W,3] BGR (uint8 / float32) and masks [n,H,W] (uint8 / float32) CUDA
    tensors + an AugPlan -> (image [3,S,S] float32 normalised RGB, masks [k,S,S] float32), two HIP launches.
    `window=(Hn, Wn)` (default: the plan's own): `[3, Hn, Wn]` and `[k, Hn, Wn]`, the square result's `[:Hn, :Wn]` bit for bit."""
    window = _plan_window(plan, window, 'apply_train_aug')
    if window is not None:
        images, views = apply_train_aug_batch([img], [masks], [plan], window=window)
        return images[0], views[0]
    if not (torch.is_tensor(img) and img.is_cuda and masks.is_cuda):
        raise RuntimeError('yolact_minimal_amd.utils.augmentations.train_aug expects CUDA tensors (there is no CPU path)')
    if img.dtype not in (torch.uint8, torch.float32) or masks.dtype not in (torch.uint8, torch.float32):
        raise RuntimeError('train_aug: image / masks must be uint8 or float32')
    img, masks = img.contiguous(), masks.contiguous()
    h, w, _ = img.shape
    c = plan_to_c(plan, h, w)
    s, k = plan.size, len(plan.keep)
    out = torch.empty(3, s, s, dtype=torch.float32, device=img.device)
    mout = torch.empty(k, s, s, dtype=torch.float32, device=img.device)
    keep = torch.as_tensor(plan.keep, dtype=torch.int32).to(img.device)
    with torch.cuda.device(img.device):
        hip.check(hip.lib().ym_train_aug_image(ctypes.c_void_p(img.data_ptr()), int(img.dtype == torch.uint8), ctypes.byref(c),
                                               hip.ptr(out), hip.stream_ptr()), 'ym_train_aug_image')
        hip.check(hip.lib().ym_train_aug_masks(ctypes.c_void_p(masks.data_ptr()), int(masks.dtype == torch.uint8),
                                               hip.ptr(keep, torch.int32), k, ctypes.byref(c), hip.ptr(mout), hip.stream_ptr()),
                  'ym_train_aug_masks')
    return out, mout


def train_aug(img, masks, boxes, labels, train_size, rng=_random, window=None):
    """Reference call shape (`train_aug(img, masks, boxes, labels, train_size)`, utils/augmentations.py:230-252) with CUDA
    tensors for `img` / `masks` and host arrays for `boxes` (pixels) / `labels`: returns (img [3,S,S], masks [k,S,S], boxes [k,4]
    in 0..1, labels [k]) — the arrays as numpy float64 / like the reference — or four Nones when the sample is rejected.
    `window=(Hn, Wn)`: the top-left window of that sample, `[3, Hn, Wn]` / `[k, Hn, Wn]`, boxes in 0..1 of the square."""
    plan = sample_train_aug(img.shape[0], img.shape[1], boxes, labels, train_size, rng, window=window)
    if plan is None:
        return None, None, None, None
    out, mout = apply_train_aug(img, masks, plan)
    return out, mout, plan.boxes, plan.labels


# ------------------------------------------------------------------------------------------------------------------------
# train_aug for a whole training batch: images of different sizes in, ONE [B, 3, S, S] tensor out, one launch pair per batch
# (`ym_train_aug_image_batch` / `ym_train_aug_masks_batch`; B = 17 .. 32 takes two pairs).  The host half draws the B plans on one
# `rng` in sample order, so a seeded run decides exactly what B successive `train_aug` calls decide; the device half writes every
# image straight into its row of the batch tensor (no `torch.stack` copy) and every mask into one [K, S, S] allocation, with ONE
# upload of all the `keep` indices.  The single-sample entries are the one-item instances of the same two kernels: row b of a batch
# equals `train_aug` of sample b bit for bit.
# ------------------------------------------------------------------------------------------------------------------------
def sample_train_aug_batch(sizes, boxes, labels, train_size, rng=_random, window=None):
    """The host half for B samples (no device, no library): `sizes` = [(h, w), ...], `boxes[b]` [n_b, 4] pixels or None (a sample
    without a valid annotation: rejected WITHOUT a draw, as `COCODetection.finish` does), `labels[b]` [n_b].  One `sample_train_aug`
    per sample, in order, on the one `rng`.  Returns `(plans, order)`: `plans[b]` an AugPlan or None (rejected); `order` the
    batch `train_collate` makes of them -- the valid samples in order, then `valid_batch[i]` for each missing slot i (that list
    grows while it is read, so one valid sample can fill several slots).  RuntimeError when no sample survives.
    `window=(Hn, Wn)`: every plan is drawn for that window (`sample_train_aug`)."""
    sizes, boxes, labels = list(sizes), list(boxes), list(labels)
    if not (len(sizes) == len(boxes) == len(labels)):
        raise RuntimeError(f'sample_train_aug_batch: {len(sizes)} sizes, {len(boxes)} box arrays and {len(labels)} label arrays')
    plans = [None if bx is None else sample_train_aug(int(h), int(w), bx, lb, train_size, rng, window=window)
             for (h, w), bx, lb in zip(sizes, boxes, labels)]
    order = [b for b, p in enumerate(plans) if p is not None]
    if not order:
        raise RuntimeError(f'sample_train_aug_batch: none of the {len(plans)} samples of the batch survived the augmentation')
    for i in range(len(plans) - len(order)):
        order.append(order[i])
    return plans, order


def _one_dtype(tensors, what, fn):
    if any(not torch.is_tensor(t) for t in tensors):
        raise RuntimeError(f'{fn}: {what} are device tensors')
    if any(not t.is_cuda or t.device != tensors[0].device for t in tensors):
        raise RuntimeError(f'yolact_minimal_amd.utils.augmentations.{fn} needs CUDA (HIP) tensors on one device; there is no CPU path.')
    if tensors[0].dtype not in (torch.uint8, torch.float32) or any(t.dtype != tensors[0].dtype for t in tensors):
        raise RuntimeError(f'{fn}: the {what} of a batch are all uint8 or all float32')


def apply_train_aug_batch(imgs, masks, plans, out=None, window=None):
    """The pixel half for B samples: `imgs` a `FrameBatch` or a list of device HWC BGR tensors (all uint8 or all float32; they need
    not share an allocation and are not repacked), `masks` a list of device `[n_b, H_b, W_b]` tensors (all uint8 or all float32),
    `plans` B AugPlans (no None: the caller has applied `order`; a repeated sample is the same item twice).  Returns
    `(images [B, 3, S, S] float32, [masks_b [k_b, S, S] float32])`, the masks B views into ONE `[K, S, S]` allocation.  `out`: a
    contiguous float32 device tensor `[>= B, 3, S, S]` whose first B rows are written (the result is then `out[:B]`).  One launch
    per 16 samples for the images, one for the masks; every `keep` index of the batch goes up in one non-blocking copy from pinned
    memory after being checked against n_b on the host.  No host synchronisation.
    `window=(Hn, Wn)` (default: the window the plans were drawn for, which they must share): the results are `[B, 3, Hn, Wn]` and
    `[k_b, Hn, Wn]`, the square results' `[:Hn, :Wn]` bit for bit (`ym_train_aug_*_batch_window`, the same kernels)."""
    from .frames import FrameBatch
    fn = 'apply_train_aug_batch'
    if isinstance(imgs, FrameBatch):
        imgs.need_cuda('utils.augmentations.' + fn)
        imgs = imgs.frames
    elif isinstance(imgs, torch.Tensor) or not hasattr(imgs, '__len__'):
        raise RuntimeError(f'{fn}: a FrameBatch or a list of [H, W, 3] device tensors expected')
    if isinstance(masks, torch.Tensor) or not hasattr(masks, '__len__'):
        raise RuntimeError(f'{fn}: a list of [n, H, W] device tensors expected')
    imgs, masks, plans = list(imgs), list(masks), list(plans)
    batch = len(imgs)
    if not 1 <= batch <= hip.AUG_MAX_SAMPLES:
        raise RuntimeError(f'{fn}: 1 .. {hip.AUG_MAX_SAMPLES} samples per call, got {batch}')
    if len(masks) != batch or len(plans) != batch:
        raise RuntimeError(f'{fn}: {batch} images, {len(masks)} mask tensors and {len(plans)} plans')
    if any(p is None for p in plans):
        raise RuntimeError(f'{fn}: a rejected sample (None) among the plans; apply the order of sample_train_aug_batch first')
    _one_dtype(imgs, 'images', fn)
    _one_dtype(masks, 'masks', fn)
    dev = imgs[0].device
    if masks[0].device != dev:
        raise RuntimeError(f'{fn}: images on {dev}, masks on {masks[0].device}')
    size = int(plans[0].size)
    if window is None and any(getattr(p, 'window', None) != getattr(plans[0], 'window', None) for p in plans):
        raise RuntimeError(f'{fn}: the plans of a batch are drawn for one window')
    window = _plan_window(plans[0], window, fn)
    hn, wn = window if window is not None else (size, size)
    items = (hip.AugItemC * batch)()
    keep_all, alive = [], []
    for b, (img, m, plan) in enumerate(zip(imgs, masks, plans)):
        if img.dim() != 3 or img.shape[2] != 3 or m.dim() != 3 or tuple(m.shape[1:]) != tuple(img.shape[:2]):
            raise RuntimeError(f'{fn}: sample {b}: image {tuple(img.shape)} is [H, W, 3] and masks {tuple(m.shape)} are [n, H, W]')
        if int(plan.size) != size:
            raise RuntimeError(f'{fn}: sample {b}: plan of train size {plan.size} in a batch of {size}')
        keep = [int(v) for v in plan.keep]
        if any(v < 0 or v >= m.shape[0] for v in keep):
            raise RuntimeError(f'{fn}: sample {b}: keep index outside its {m.shape[0]} masks')
        img, m = img.contiguous(), m.contiguous()
        alive += [img, m]
        it = items[b]
        it.plan = plan_to_c(plan, int(img.shape[0]), int(img.shape[1]))
        it.n_masks, it.img, it.masks = int(m.shape[0]), img.data_ptr(), (m.data_ptr() if m.numel() else None)
        it.k, it.row0 = len(keep), len(keep_all)
        keep_all += keep
    total = len(keep_all)
    if out is None:
        out = torch.empty(batch, 3, hn, wn, dtype=torch.float32, device=dev)
    elif not torch.is_tensor(out) or not out.is_cuda or out.device != dev or out.dtype != torch.float32 or out.dim() != 4 or \
            out.shape[0] < batch or tuple(out.shape[1:]) != (3, hn, wn) or not out.is_contiguous():
        raise RuntimeError(f'{fn}: out is a contiguous float32 [>= {batch}, 3, {hn}, {wn}] tensor on the device of the images')
    mout = torch.empty(total, hn, wn, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        keep_dev = None
        if total:
            keep_dev = torch.tensor(keep_all, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
        L = hip.lib()
        if window is not None:
            hip.check(L.ym_train_aug_image_batch_window(items, batch, size, hn, wn, int(imgs[0].dtype == torch.uint8), hip.ptr(out),
                                                        hip.stream_ptr()), 'ym_train_aug_image_batch_window')
            hip.check(L.ym_train_aug_masks_batch_window(items, batch, size, hn, wn, int(masks[0].dtype == torch.uint8),
                                                        hip.ptr(keep_dev, torch.int32), total, hip.ptr(mout), hip.stream_ptr()),
                      'ym_train_aug_masks_batch_window')
            views = [mout[it.row0:it.row0 + it.k] for it in items]
            return out[:batch], views
        hip.check(L.ym_train_aug_image_batch(items, batch, size, int(imgs[0].dtype == torch.uint8), hip.ptr(out), hip.stream_ptr()),
                  'ym_train_aug_image_batch')
        hip.check(L.ym_train_aug_masks_batch(items, batch, size, int(masks[0].dtype == torch.uint8), hip.ptr(keep_dev, torch.int32),
                                             total, hip.ptr(mout), hip.stream_ptr()), 'ym_train_aug_masks_batch')
    views = [mout[it.row0:it.row0 + it.k] for it in items]
    return out[:batch], views


def train_aug_batch(imgs, masks, boxes, labels, train_size, rng=_random, window=None):
    """`train_aug` for a batch: `imgs` / `masks` as for `apply_train_aug_batch`, `boxes[b]` (pixels; None = no valid annotation) and
    `labels[b]` host arrays.  Returns `(images [B, 3, S, S], [masks_b [k_b, S, S]], [boxes_b [k_b, 4] in 0..1], [labels_b [k_b]])`
    in `train_collate`'s batch composition: rejected samples are replaced by repeated valid ones.
    `window=(Hn, Wn)`: the top-left windows of those samples, `[B, 3, Hn, Wn]` / `[k_b, Hn, Wn]`, boxes in 0..1 of the square."""
    from .frames import FrameBatch
    frames = imgs.frames if isinstance(imgs, FrameBatch) else imgs
    if isinstance(frames, torch.Tensor) or not hasattr(frames, '__len__') or isinstance(masks, torch.Tensor) or not hasattr(masks, '__len__'):
        raise RuntimeError('train_aug_batch: a FrameBatch or a list of [H, W, 3] device tensors, and a list of [n, H, W] mask tensors expected')
    frames, masks = list(frames), list(masks)
    if not 1 <= len(frames) <= hip.AUG_MAX_SAMPLES:
        raise RuntimeError(f'train_aug_batch: 1 .. {hip.AUG_MAX_SAMPLES} samples per call, got {len(frames)}')
    if len(masks) != len(frames) or len(boxes) != len(frames) or len(labels) != len(frames):
        raise RuntimeError(f'train_aug_batch: {len(frames)} images, {len(masks)} mask tensors, {len(boxes)} box arrays and '
                           f'{len(labels)} label arrays')
    _one_dtype(frames, 'images', 'train_aug_batch')
    _one_dtype([m for m in masks if m is not None] or frames, 'masks', 'train_aug_batch')
    plans, order = sample_train_aug_batch([(f.shape[0], f.shape[1]) for f in frames], boxes, labels, train_size, rng, window=window)
    images, mviews = apply_train_aug_batch([frames[b] for b in order], [masks[b] for b in order], [plans[b] for b in order])
    return images, mviews, [plans[b].boxes for b in order], [plans[b].labels for b in order]
