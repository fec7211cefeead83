"""numpy restatement of the `draw_img` contract (reference `utils/output_utils.py:327-369`), the oracle of tests/test_gpu_draw.py.

Written from the specification, not from the kernel: boxes, plates and text are PAINTED in the reference's order
`for i in reversed(range(n))` (the kernel instead resolves "the smallest i that touches a pixel"), the class sum is a numpy
reduction, the text is blitted from `font.text_bitmap`.  All integer arithmetic, so comparisons are exact.

  masks   s = (sum_i int(masks[i]) * (ids[i] + 1)) mod (nc - 1); every pixel -> (4 * P[s] + 6 * img + 5) // 10
  boxes   outline (1 px, corners as given, clipped), plate x1..x1+text_w, y1..y1+text_h+5 inclusive, colour P[ids[i] + 1];
          text white, baseline-left (x1, y1 + 15): "{name}: {score:.2f}" or "{name}" (hide_score)
  fps     rows < text_h + 8, columns < text_w + 8 -> 3 * v // 5, then "fps: {fps:.2f}" white, baseline-left (0, text_h + 2)
  cutout  total = img where s != 0 else 255;  obj_i = (img where masks[i] != 0 else 255)[y1:y2, x1:x2]
"""
from types import SimpleNamespace

import numpy as np

from yolact_minimal_amd.config import COLORS, COCO_CLASSES
from yolact_minimal_amd.utils import font

NAME_MAX = 39       # characters of a class name that are drawn (YM_DRAW_NAME_STRIDE - 1)
LABEL_MAX = 44      # characters of a label that are drawn (YM_DRAW_LABEL_MAX)


def make_cfg(**kw):
    cfg = dict(hide_mask=False, hide_bbox=False, hide_score=False, real_time=False, cutout=False, no_crop=False, visual_thre=0.0,
               class_names=COCO_CLASSES, num_classes=len(COCO_CLASSES) + 1)
    cfg.update(kw)
    if 'class_names' in kw and 'num_classes' not in kw:
        cfg['num_classes'] = len(kw['class_names']) + 1
    return SimpleNamespace(**cfg)


def score_text(v):
    """'{v:.2f}' of a float32 the way the device computes it: cents = rint(double(v) * 100), half to even."""
    v = np.float32(v)
    if np.isnan(v):
        return 'nan'
    sign = '-' if np.signbit(v) else ''
    a = abs(np.float64(v))
    if np.isinf(a):
        return sign + 'inf'
    cents = int(np.rint(a * np.float64(100.0)))
    return f'{sign}{cents // 100}.{cents % 100 // 10}{cents % 10}'


def label_text(name, score, hide_score):
    name = font.sanitize(str(name))[:NAME_MAX]
    return (name if hide_score else f'{name}: {score_text(score)}')[:LABEL_MAX]


def _fill(out, xa, xb, ya, yb, colour):
    """inclusive rectangle, clipped to the frame"""
    h, w = out.shape[:2]
    xa, xb, ya, yb = max(xa, 0), min(xb, w - 1), max(ya, 0), min(yb, h - 1)
    if xa <= xb and ya <= yb:
        out[ya:yb + 1, xa:xb + 1] = colour


def _text(out, text, x, baseline):
    bm = font.text_bitmap(text)
    h, w = out.shape[:2]
    top = baseline - (font.HEIGHT - 1)
    ys, xs = np.nonzero(bm)
    ys, xs = ys + top, xs + x
    ok = (ys >= 0) & (ys < h) & (xs >= 0) & (xs < w)
    out[ys[ok], xs[ok]] = 255


def class_sum(ids, masks, nc):
    s = np.zeros(masks.shape[1:], dtype=np.int64)
    for i in range(masks.shape[0]):
        s += masks[i].astype('int') * (int(ids[i]) + 1)
    return s % (nc - 1)


def draw_ref(ids, scores, boxes, masks, img, cfg, fps=None, labels=None):
    """ids int64[n] | None, scores f32[n], boxes int32[n,4], masks f32[n,H,W], img uint8[H,W,3] (all numpy) -> uint8[H,W,3].
    `labels` overrides the label strings (to test the device's score formatting against Python's own)."""
    if ids is None or len(ids) == 0:
        return img
    n = len(ids)
    palette = np.asarray(COLORS).astype(np.int64)
    out = img.copy()
    if not cfg.hide_mask:
        c = palette[class_sum(ids, masks, cfg.num_classes)]
        out = ((4 * c + 6 * img.astype(np.int64) + 5) // 10).astype(np.uint8)
    if not cfg.hide_bbox:
        for i in reversed(range(n)):
            x1, y1, x2, y2 = (int(v) for v in boxes[i])
            colour = palette[int(ids[i]) + 1]
            _fill(out, min(x1, x2), max(x1, x2), y1, y1, colour)
            _fill(out, min(x1, x2), max(x1, x2), y2, y2, colour)
            _fill(out, x1, x1, min(y1, y2), max(y1, y2), colour)
            _fill(out, x2, x2, min(y1, y2), max(y1, y2), colour)
            text = labels[i] if labels is not None else label_text(cfg.class_names[int(ids[i])], scores[i], cfg.hide_score)
            text_w, text_h = font.text_size(text)
            _fill(out, x1, x1 + text_w, y1, y1 + text_h + 5, colour)
            _text(out, text, x1, y1 + 15)
    if cfg.real_time:
        text = f'fps: {fps:.2f}'
        text_w, text_h = font.text_size(text)
        out[0:text_h + 8, 0:text_w + 8] = (3 * out[0:text_h + 8, 0:text_w + 8].astype(np.int64)) // 5
        _text(out, text, 0, text_h + 2)
    return out


def cutout_ref(ids, boxes, masks, img, cfg):
    """-> (total uint8[H,W,3], [obj_i])"""
    s = class_sum(ids, masks, cfg.num_classes)
    total = np.where((s != 0)[:, :, None], img, 255).astype(np.uint8)
    objs = []
    for i in range(len(ids)):
        x1, y1, x2, y2 = (int(v) for v in boxes[i])
        objs.append(np.where((masks[i] != 0)[:, :, None], img, 255).astype(np.uint8)[y1:y2, x1:x2, :])
    return total, objs


def synth(n, h, w, seed, crop=True, wild_boxes=False):
    """Seeded synthetic detections -> (ids, scores, boxes, masks, img) as numpy.  Masks are random blobs inside their boxes
    (`crop`) or anywhere in the frame; `wild_boxes` adds boxes partly / wholly outside the frame, reversed corners and x1 next to
    the right edge."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, 80, n).astype(np.int64)
    scores = np.sort(rng.random(n).astype(np.float32))[::-1].copy()
    boxes = np.zeros((n, 4), dtype=np.int32)
    masks = np.zeros((n, h, w), dtype=np.float32)
    for i in range(n):
        xa, xb = sorted(int(v) for v in rng.integers(0, w, 2))
        ya, yb = sorted(int(v) for v in rng.integers(0, h, 2))
        boxes[i] = (xa, ya, xb, yb)
        blob = (rng.random((h, w)) < 0.6).astype(np.float32)
        if crop:
            win = np.zeros((h, w), dtype=np.float32)
            win[ya:yb + 1, xa:xb + 1] = 1
            blob *= win
        else:
            blob *= (rng.random((h, w)) < 0.3)
        masks[i] = blob
    if wild_boxes and n >= 6:
        boxes[0] = (-w // 3, -h // 4, w // 2, h // 2)            # partly outside, negative corner
        boxes[1] = (w + 5, h + 7, w + 40, h + 30)                # wholly outside
        boxes[2] = (w // 2, h // 2, w // 5, h // 6)              # reversed corners
        boxes[3] = (w - 3, h // 3, w + 20, h - 2)                # x1 next to the right edge: plate clipped
        boxes[4] = (-30, h - 6, w // 4, h + 9)                   # label runs off the bottom and starts left of the frame
        boxes[5] = (w // 4, -9, w // 4, h // 2)                  # zero-width box, plate starts above the frame
    img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    return ids, scores, boxes, masks, img
