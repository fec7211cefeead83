"""`draw_img` with the reference's signature, rendered on the device (csrc/draw.hip).

Reference: `utils/output_utils.py:327-369`.  The reference starts by downloading all `n x img_h x img_w` float32 masks and draws
with cv2 on the host; here the masks, ids, scores and boxes stay where `after_nms` left them and only the finished frame
(`img_h x img_w x 3` bytes) comes back — or nothing at all when the frame is a device tensor.

    draw_img(ids_p, class_p, box_p, mask_p, img_origin, cfg, img_name=None, fps=None) -> frame
        `img_origin`: numpy uint8 [H, W, 3] BGR (one upload, one download, a numpy array comes back, so cv2.imwrite /
        VideoWriter.write work unchanged) or a device uint8 tensor (a device tensor comes back, nothing crosses PCIe).
        `ids_p is None` returns `img_origin` itself, like the reference.
    cutout_mattes(ids_p, box_p, mask_p, img_origin, cfg) -> (total, [obj_0, ...])      what cfg.cutout writes to disk
    draw_batch(dets_padded, imgs, cfg, fps=None) -> uint8 [B, H, W, 3]
        for `after_nms_batch(..., sync=False)`: counts, scores and cfg.visual_thre are consumed on the device, no host read.
        With `imgs` a `FrameBatch` (frames of different sizes) and the per-image mask views of the ragged `after_nms_batch`:
        -> a new `FrameBatch`, still one launch set.

Mask colours, blend, outline / plate geometry, draw order and the score formatting are the reference's, exactly (integer arithmetic
throughout).  The label PIXELS are this package's own fixed-cell bitmap font (`utils/font.py`), not cv2's anti-aliased Hershey Duplex.
The detections must be device tensors; there is no CPU path.  `mask_p` / the masks of `dets_padded` may be a `PackedMasks`
(utils/packed_masks.py) instead of the float32 tensor: same frames, byte for byte, from 1/32 of the mask bytes.
"""
import ctypes

import numpy as np
import torch

from .. import hip
from ..config import COLORS
from . import font as _font
from .packed_masks import PackedMasks

_res_cache = {}


def _flag(cfg, name):
    return bool(getattr(cfg, name, False))


def _resources(device, cfg):
    """Palette, class-name table and font on `device`: uploaded once per (device, class names) and kept."""
    names = tuple(cfg.class_names)
    key = (device.index if device.index is not None else torch.cuda.current_device(), names)
    res = _res_cache.get(key)
    if res is None:
        assert (_font.ADVANCE, _font.HEIGHT) == (hip.DRAW_FONT_ADVANCE, hip.DRAW_FONT_HEIGHT)
        table = np.zeros((max(len(names), 1), hip.DRAW_NAME_STRIDE), dtype=np.uint8)
        for k, name in enumerate(names):
            raw = _font.sanitize(str(name))[:hip.DRAW_NAME_STRIDE - 1].encode('ascii')
            table[k, :len(raw)] = np.frombuffer(raw, dtype=np.uint8)
        palette = np.ascontiguousarray(np.asarray(COLORS), dtype=np.uint8)
        res = _res_cache[key] = dict(
            palette=torch.from_numpy(palette).to(device), palette_n=palette.shape[0],
            names=torch.from_numpy(table).to(device), num_names=len(names),
            font=torch.from_numpy(_font.FONT.astype(np.int16)).to(device))          # bit patterns of the uint16 rows
    return res


def _flags(cfg):
    return ((hip.DRAW_HIDE_MASK if _flag(cfg, 'hide_mask') else 0) | (hip.DRAW_HIDE_BBOX if _flag(cfg, 'hide_bbox') else 0) |
            (hip.DRAW_HIDE_SCORE if _flag(cfg, 'hide_score') else 0) | (hip.DRAW_REAL_TIME if _flag(cfg, 'real_time') else 0))


def _launch(imgs, masks, ids, scores, boxes, counts, cfg, flags, visual_thre, fps, out, cutout_total=None, mask_table=None):
    """The launch set behind `draw_img`, `cutout_mattes` and both arms of `draw_batch`, arguments checked by the caller.  `imgs` /
    `out`: uint8 `[B, H, W, 3]` tensors with `masks` `[B, max_det, H, W]` (or a `PackedMasks`; the uniform entries, which also fill
    `cutout_total`) -- or `FrameBatch`es with `masks` = view 0 of the checked list of per-image views and `mask_table` their table
    (`ym_draw_detections_ragged[_packed]`).  `ids` is `[B, max_det]`, or `[max_det]` for one frame."""
    from .frames import FrameBatch
    from .output_utils import _scratch
    device = imgs.device
    batch, max_det = ids.shape if ids.dim() == 2 else (1, ids.shape[0])
    res = _resources(device, cfg)
    fps_text = None
    if flags & hip.DRAW_REAL_TIME:
        if fps is None:
            raise RuntimeError('draw_img: cfg.real_time needs the fps value')
        fps_text = f'fps: {fps:.2f}'.encode('ascii', 'replace')
    # (PackedMasks: the mask term is read from the bit rows, one word serves 64 pixels of a detection; same output bytes)
    if isinstance(imgs, FrameBatch):
        name, frames, dst, where, cutout = 'ym_draw_detections_ragged', imgs.data, out.data, (imgs.table(), mask_table), ()
    else:
        name, frames, dst, where, cutout = 'ym_draw_detections_batch', imgs, out, imgs.shape[1:3], (hip.ptr(cutout_total, torch.uint8),)
    L = hip.lib()
    with torch.cuda.device(device):
        nbytes = L.ym_draw_workspace_bytes(batch, max_det)
        if nbytes == 0:
            raise RuntimeError('ym_draw_workspace_bytes: ' + L.ym_last_error().decode())
        ws = _scratch(device, nbytes)
        hip.check(getattr(L, name + ('_packed' if isinstance(masks, PackedMasks) else ''))(
            hip.ptr(frames, torch.uint8), _mask_ptr(masks), hip.ptr(ids, torch.int64), hip.ptr(scores), hip.ptr(boxes, torch.int32),
            hip.ptr(counts, torch.int32), batch, max_det, *where, hip.ptr(res['palette'], torch.uint8), res['palette_n'],
            int(cfg.num_classes), hip.ptr(res['names'], torch.uint8), res['num_names'], hip.ptr(res['font'], torch.int16), flags,
            float(visual_thre), fps_text, hip.ptr(dst, torch.uint8), *cutout, ctypes.c_void_p(ws.data_ptr()), ws.numel(),
            hip.stream_ptr()), name)


def _mask_ptr(masks):
    if masks is None:
        return None
    return hip.ptr(masks.bits, torch.int64) if isinstance(masks, PackedMasks) else hip.ptr(masks)


def _device_of(ids_p, what):
    if not torch.is_tensor(ids_p) or not ids_p.is_cuda:
        raise RuntimeError(f'yolact_minimal_amd.utils.draw.{what} needs the detections as CUDA (HIP) tensors, as after_nms returns '
                           f'them; there is no CPU path.')
    return ids_p.device


def _frame_on(img_origin, device):
    """-> (uint8 [1, H, W, 3] on `device`, came_from_numpy)"""
    if isinstance(img_origin, np.ndarray):
        if img_origin.dtype != np.uint8 or img_origin.ndim != 3 or img_origin.shape[2] != 3:
            raise RuntimeError(f'draw_img: expected a uint8 [H, W, 3] frame, got {img_origin.dtype} {img_origin.shape}')
        return torch.from_numpy(np.ascontiguousarray(img_origin)).to(device)[None], True
    if not torch.is_tensor(img_origin) or not img_origin.is_cuda or img_origin.dtype != torch.uint8 or img_origin.dim() != 3 or \
            img_origin.shape[2] != 3:
        raise RuntimeError('draw_img: the frame is a numpy uint8 [H, W, 3] array or a uint8 [H, W, 3] tensor on the device')
    if img_origin.device != device:
        raise RuntimeError(f'draw_img: frame on {img_origin.device}, detections on {device}')
    return img_origin.contiguous()[None], False


def _single_inputs(ids_p, class_p, box_p, mask_p, frame, need_masks, need_scores):
    n = ids_p.shape[0]
    if n > hip.DRAW_MAX_DET:
        raise RuntimeError(f'draw_img: {n} detections, at most {hip.DRAW_MAX_DET} are drawn')
    _, h, w, _ = frame.shape
    masks = None
    if need_masks:
        if mask_p is None or tuple(mask_p.shape) != (n, h, w):
            raise RuntimeError(f'draw_img: masks {None if mask_p is None else tuple(mask_p.shape)} do not fit {n} detections on a '
                               f'{h} x {w} frame')
        masks = mask_p.contiguous()
    if tuple(box_p.shape) != (n, 4):
        raise RuntimeError(f'draw_img: boxes {tuple(box_p.shape)} for {n} detections')
    scores = class_p.contiguous() if need_scores else None
    return n, masks, ids_p.contiguous(), scores, box_p.contiguous()


def draw_img(ids_p, class_p, box_p, mask_p, img_origin, cfg, img_name=None, fps=None):
    if ids_p is None:
        return img_origin
    device = _device_of(ids_p, 'draw_img')
    frame, from_numpy = _frame_on(img_origin, device)
    flags = _flags(cfg)
    n, masks, ids, scores, boxes = _single_inputs(ids_p, class_p, box_p, mask_p, frame, not flags & hip.DRAW_HIDE_MASK,
                                                  not flags & hip.DRAW_HIDE_SCORE)
    out = torch.empty_like(frame)
    _launch(frame, masks, ids, scores, boxes, None, cfg, flags, 0.0, fps, out)
    return out[0].cpu().numpy() if from_numpy else out[0]


def cutout_mattes(ids_p, box_p, mask_p, img_origin, cfg):
    """What the reference's `cfg.cutout` branch writes (`utils/output_utils.py:346-358`), as arrays: `total` = the frame where any
    mask colour is drawn (class sum modulo != 0) and 255 elsewhere; `objs[i]` = (frame where masks[i] != 0 else 255)[y1:y2, x1:x2]
    with Python's slice rules.  numpy frame in -> numpy arrays out, device frame in -> device tensors out.  Reads the boxes on the
    host (the slice bounds).  `(None, [])` without detections."""
    if ids_p is None:
        return None, []
    if _flag(cfg, 'hide_mask'):
        raise RuntimeError('cutout_mattes: cfg.cutout needs the masks (cfg.hide_mask is set)')
    device = _device_of(ids_p, 'cutout_mattes')
    frame, from_numpy = _frame_on(img_origin, device)
    n, masks, ids, _, boxes = _single_inputs(ids_p, None, box_p, mask_p, frame, True, False)
    _, h, w, _ = frame.shape
    total = torch.empty_like(frame)
    _launch(frame, masks, ids, None, boxes, None, cfg, hip.DRAW_HIDE_BBOX | hip.DRAW_HIDE_SCORE, 0.0, None, torch.empty_like(frame), total)
    objs = []
    if n:
        full = torch.empty(n, h, w, 3, dtype=torch.uint8, device=device)
        with torch.cuda.device(device):
            cut = hip.lib().ym_draw_cutout_objects_packed if isinstance(masks, PackedMasks) else hip.lib().ym_draw_cutout_objects
            hip.check(cut(hip.ptr(frame, torch.uint8), _mask_ptr(masks), n, h, w, hip.ptr(full, torch.uint8), hip.stream_ptr()),
                      'ym_draw_cutout_objects')
        for i, (x1, y1, x2, y2) in enumerate(boxes.tolist()):
            objs.append(full[i][y1:y2, x1:x2, :])
    if from_numpy:
        return total[0].cpu().numpy(), [o.cpu().numpy() for o in objs]
    return total[0], objs


def _ragged_mask_table(masks, sizes, max_det, what='draw_batch'):
    """The list of per-image mask views of the ragged `after_nms_batch` -> (view 0, the `ym_after_nms_ragged` table rebuilt from the
    views' data pointers relative to view 0).  Raises unless the views are `[max_det, h_b, w_b]` blocks of ONE allocation in
    `ragged_layout` order."""
    from .output_utils import ragged_layout
    if not isinstance(masks, (list, tuple)) or len(masks) != len(sizes):
        raise RuntimeError(f'{what}: with images of different sizes the masks are the list of {len(sizes)} per-image views that '
                           f'after_nms_batch(dets, hs, ws, ..., sync=False) returns')
    packed = isinstance(masks[0], PackedMasks)
    words = []
    for b, (m, (h, w)) in enumerate(zip(masks, sizes)):
        if isinstance(m, PackedMasks) != packed:
            raise RuntimeError(f'{what}: dense and packed mask views in one batch')
        t = m.bits if packed else m
        if not torch.is_tensor(t) or tuple(m.shape) != (max_det, h, w) or t.dtype != (torch.int64 if packed else torch.float32) or \
                not t.is_contiguous():
            raise RuntimeError(f'{what}: image {b}: masks {tuple(m.shape)} do not fit {max_det} rows on a {h} x {w} frame')
        words.append(t)
    offsets, _ = ragged_layout(sizes, max_det, packed)
    esz = 8 if packed else 4
    base = words[0].data_ptr()
    for b, t in enumerate(words):
        if t.device != words[0].device or t.data_ptr() - base != offsets[b] * esz:
            raise RuntimeError(f'{what}: the mask view of image {b} is not at its place in one ragged_layout allocation')
    return masks[0], hip.ragged_table(sizes, offsets)


def _batch_inputs(dets_padded, frames, frames_device):
    """What both arms of `draw_batch` check of the detections -> (batch, max_det, ids, scores, boxes, counts), contiguous."""
    ids, scores, boxes, _, counts = dets_padded
    for t in (ids, scores, boxes, counts):
        if t is not None and (not torch.is_tensor(t) or not t.is_cuda):
            raise RuntimeError('yolact_minimal_amd.utils.draw.draw_batch needs the detections as CUDA (HIP) tensors, as after_nms_batch '
                               'returns them; there is no CPU path.')
    if ids.dim() != 2 or frames_device != ids.device:
        raise RuntimeError('draw_batch: ids [B, max_det] on the device of the frames expected')
    batch, max_det = ids.shape
    if frames != batch or max_det > hip.DRAW_MAX_DET:
        raise RuntimeError(f'draw_batch: {frames} frames for {batch} detection sets of {max_det} rows (at most {hip.DRAW_MAX_DET})')
    return (batch, max_det) + tuple(t.contiguous() if t is not None else None for t in (ids, scores, boxes, counts))


def draw_batch(dets_padded, imgs, cfg, fps=None, _out=None):
    """Render B frames from `after_nms_batch(dets, img_h, img_w, cfg, sync=False)` = (ids, scores, boxes_px, masks, counts), all
    padded to max_detections rows, in one launch set.  `imgs` is a device uint8 [B, H, W, 3] tensor; so is the result.  Frame b
    equals `draw_img` on `after_nms`'s result for image b: rows past counts[b] and rows under cfg.visual_thre are dropped ON THE
    DEVICE, a frame left without detections comes back unchanged.  No host synchronisation and no device-to-host copy (the palette /
    class-name / font tables are uploaded by the first call for a (device, class names) pair).
    Frames of DIFFERENT sizes: `imgs` is a `FrameBatch` (utils/frames.py) and `masks` the list of per-image views that
    `after_nms_batch(dets, hs, ws, cfg, sync=False)` returns (dense or `PackedMasks`; ignored with `cfg.hide_mask`); the result is a
    new `FrameBatch` of the same sizes (`ym_draw_detections_ragged`: one prep launch and at most two frame launches for the batch).
    (`_out`: the destination `FrameBatch`, for the tests' guard bytes; `_out is imgs` draws in place.)"""
    from .frames import FrameBatch
    flags = _flags(cfg)
    masks, mask_table = (None if flags & hip.DRAW_HIDE_MASK else dets_padded[3]), None
    if isinstance(imgs, FrameBatch):
        imgs.need_cuda('utils.draw.draw_batch')
        if imgs.dtype != torch.uint8:
            raise RuntimeError('draw_batch: the frames are uint8')
        batch, max_det, *dets = _batch_inputs(dets_padded, len(imgs), imgs.device)
        if masks is not None and max_det:
            masks, mask_table = _ragged_mask_table(masks, imgs.sizes, max_det)
            if masks.device != imgs.device:
                raise RuntimeError(f'draw_batch: masks on {masks.device}, detections on {imgs.device}')
        else:
            masks = None
        out = FrameBatch.empty_like(imgs) if _out is None else _out
        if not isinstance(out, FrameBatch) or out.sizes != imgs.sizes or out.dtype != torch.uint8 or out.device != imgs.device:
            raise RuntimeError('draw_batch: the destination is a uint8 FrameBatch of the same sizes on the same device')
    else:
        if _out is not None:
            raise RuntimeError('draw_batch: a destination is taken with a FrameBatch only')
        if not torch.is_tensor(imgs) or not imgs.is_cuda or imgs.dtype != torch.uint8 or imgs.dim() != 4 or imgs.shape[3] != 3:
            raise RuntimeError('draw_batch: imgs is a uint8 [B, H, W, 3] tensor on the device of the detections')
        batch, max_det, *dets = _batch_inputs(dets_padded, imgs.shape[0], imgs.device)
        _, h, w, _ = imgs.shape
        if masks is not None:
            if tuple(masks.shape) != (batch, max_det, h, w):
                raise RuntimeError(f'draw_batch: masks {tuple(masks.shape)} do not fit [{batch}, {max_det}, {h}, {w}]')
            masks = masks.contiguous()
        imgs = imgs.contiguous()
        out = torch.empty_like(imgs)
    _launch(imgs, masks, *dets, cfg, flags, float(getattr(cfg, 'visual_thre', 0) or 0), fps, out, mask_table=mask_table)
    return out
