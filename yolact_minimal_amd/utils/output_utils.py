"""`nms` / `after_nms` with the reference's signatures, executed by HIP kernels.

Reference: `/root/reference/utils/output_utils.py` — nms `:126-163`, fast_nms `:11-43`, traditional_nms
`:84-123` (+ `cython_nms.pyx:24-74`), after_nms `:200-233`; box math in `utils/box_utils.py:8-37,117-168`.

Same call shapes and return conventions:
  nms(class_pred, box_pred, coef_pred, proto_out, anchors, cfg) -> (class_ids int64[n], scores f32[n],
      boxes f32[n,4] in 0..1, coefs f32[n,32], proto[Hp,Wp,32])  or five Nones when nothing passes the
      score threshold;  batch size 1 only, like the reference (`.squeeze()` at :127-130).
  after_nms(ids_p, class_p, box_p, coef_p, proto_p, img_h, img_w, cfg=None, img_name=None) ->
      (ids, scores, boxes int32[n,4] pixels, masks f32[n,img_h,img_w] in {0,1}) or four Nones;
      `box_p` is scaled IN PLACE like the reference (:230).  `packed=True` (or `cfg.packed_masks`): the fourth result is a
      `PackedMasks` (utils/packed_masks.py: 1 bit per pixel, written by the mask kernel itself; the float tensor never exists).
      `window=True` (not in the reference; utils/rect.py): `proto_p` is the top-left `[Hp, Wp]` window of the square prototype map
      of a rectangular forward, its virtual extent is `max(Hp, Wp)` on both axes (`ym_after_nms_window`).
The only host<->device synchronisation is one 4-byte read of the detection count at the end of `nms`
(the reference's boolean-mask gathers synchronise several times per call).

`draw_img` (`:327-369`), `draw_batch` and `cutout_mattes` are the device renderer of `utils/draw.py`, re-exported here.
"""
import contextlib
import ctypes
import os

import torch

from .. import hip
from .packed_masks import PackedMasks, pack_reference, unpack_reference  # noqa: F401  (re-exported)

_anchor_cache = {}
_ws_cache = {}
_plan_cache = {}


def _anchors_on(anchors, device):
    if torch.is_tensor(anchors):
        t = anchors.reshape(-1, 4)
        if t.device != device or t.dtype != torch.float32 or not t.is_contiguous():
            t = t.to(device=device, dtype=torch.float32).contiguous()
        return t
    key = (id(anchors), len(anchors), str(device))
    hit = _anchor_cache.get(key)
    if hit is None or hit[0] is not anchors:
        # the reference rebuilds this tensor from a 74k-float python list on EVERY image (:132-133, ~5 ms)
        t = torch.tensor(anchors, dtype=torch.float32).reshape(-1, 4).to(device)
        _anchor_cache[key] = (anchors, t)
        return t
    return hit[1]


def _nms_buffers(device, ncfg):
    # (scratch is per STREAM: requests in flight on different streams must not share it)
    key = (str(device), torch.cuda.current_stream(device).cuda_stream, ncfg.num_anchors, ncfg.num_classes, ncfg.coef_dim, ncfg.max_det)
    b = _ws_cache.get(key)
    if b is None:
        nbytes = hip.lib().ym_nms_workspace_bytes(ctypes.byref(ncfg))
        if nbytes == 0:
            raise RuntimeError('ym_nms_workspace_bytes: ' + hip.lib().ym_last_error().decode())
        b = dict(ws=torch.empty(nbytes, dtype=torch.uint8, device=device),
                 count=torch.zeros(1, dtype=torch.int32, device=device))
        _ws_cache[key] = b
    return b


def nms(class_pred, box_pred, coef_pred, proto_out, anchors, cfg):
    if not class_pred.is_cuda:
        raise RuntimeError('yolact_minimal_amd.utils.output_utils.nms needs CUDA (HIP) tensors; there is no CPU path.')
    class_p = class_pred.squeeze()
    box_p = box_pred.squeeze()
    coef_p = coef_pred.squeeze()
    proto_p = proto_out.squeeze()
    if class_p.dim() != 2:
        raise RuntimeError('nms() handles one image at a time (batch size 1), like the reference.')
    device = class_p.device
    n_anchors, n_classes = class_p.shape
    anchors_t = _anchors_on(anchors, device)
    if anchors_t.shape[0] != n_anchors:
        raise RuntimeError(f'{anchors_t.shape[0]} anchors for {n_anchors} predictions')

    ncfg = hip.NmsCfg(n_anchors, n_classes, coef_p.shape[1], int(cfg.top_k), int(cfg.max_detections),
                      float(cfg.nms_score_thre), float(cfg.nms_iou_thre), float(getattr(cfg, 'img_size', 544)))
    bufs = _nms_buffers(device, ncfg)
    md = ncfg.max_det
    ids = torch.empty(md, dtype=torch.int64, device=device)
    scores = torch.empty(md, dtype=torch.float32, device=device)
    boxes = torch.empty(md, 4, dtype=torch.float32, device=device)
    coefs = torch.empty(md, ncfg.coef_dim, dtype=torch.float32, device=device)
    fn = hip.lib().ym_detect_greedy_nms if getattr(cfg, 'traditional_nms', False) else hip.lib().ym_detect_fast_nms
    ws = bufs['ws']
    with torch.cuda.device(device):
        rc = fn(hip.ptr(class_p.contiguous()), hip.ptr(box_p.contiguous()), hip.ptr(coef_p.contiguous()),
                hip.ptr(anchors_t), ctypes.byref(ncfg), hip.ptr(bufs['count'], torch.int32),
                hip.ptr(ids, torch.int64), hip.ptr(scores), hip.ptr(boxes), hip.ptr(coefs),
                ctypes.c_void_p(ws.data_ptr()), ws.numel(), hip.stream_ptr())
    hip.check(rc, 'ym_detect_nms')
    n = int(bufs['count'].item())       # the single sync of the post-processing path
    if n == 0:
        return None, None, None, None, None
    return ids[:n], scores[:n], boxes[:n], coefs[:n], proto_p


def _want_packed(cfg, packed):
    return bool(packed) or bool(cfg and getattr(cfg, 'packed_masks', False))


def after_nms(ids_p, class_p, box_p, coef_p, proto_p, img_h, img_w, cfg=None, img_name=None, packed=False, window=False):
    if ids_p is None:
        return None, None, None, None
    packed = _want_packed(cfg, packed)
    if packed and not proto_p.is_cuda:
        raise RuntimeError('yolact_minimal_amd.utils.output_utils.after_nms(packed=True) needs CUDA (HIP) tensors; there is no CPU path.')

    if cfg and getattr(cfg, 'visual_thre', 0) > 0:
        keep = class_p >= cfg.visual_thre
        if not bool(keep.any()):
            return None, None, None, None
        ids_p, class_p, box_p, coef_p = ids_p[keep], class_p[keep], box_p[keep], coef_p[keep]

    if cfg and getattr(cfg, 'save_lincomb', False):
        raise NotImplementedError('draw_lincomb (visualisation, reference output_utils.py:276-324) is out of scope')

    do_crop = not (cfg and getattr(cfg, 'no_crop', False))
    box_c = box_p if box_p.is_contiguous() else box_p.contiguous()
    if window:
        if not proto_p.is_cuda:
            raise RuntimeError('yolact_minimal_amd.utils.output_utils.after_nms(window=True) needs CUDA (HIP) tensors; there is no CPU path.')
        masks, box_px = _after_nms_launch(proto_p.contiguous(), coef_p.contiguous(), box_c, None, [(int(img_h), int(img_w))], do_crop, packed,
                                          window=True)
        masks = masks[0]
    else:
        masks, box_px = _after_nms_launch(proto_p.contiguous(), coef_p.contiguous(), box_c, None, (img_h, img_w), do_crop, packed)
    if box_c is not box_p:
        box_p.copy_(box_c)              # keep the reference's in-place scaling visible to the caller
    return ids_p, class_p, box_px, masks


_ragged_plans = {}
_NO_SWITCH = contextlib.nullcontext()


def _after_nms_launch(proto, coefs, boxes, counts, sizes, do_crop, packed, window=False):
    """The launch set behind `after_nms` and both arms of `after_nms_batch`: allocates and returns `(masks, box_px)` for the
    detections `coefs` [B, max_det, 32] / `boxes` (scaled in place) of `proto` [B, Hp, Wp, 32], or of ONE image without the
    leading B.  `sizes` is one `(h, w)` for every image -- the uniform entries, masks `[B, max_det, h, w]` (packed: the words
    `[B, max_det, h, ceil(w / 64)]`) -- or a LIST of B pairs -- `ym_after_nms_ragged[_packed]`, masks = a list of B views
    `[max_det, h_b, w_b]` of one flat allocation (`ragged_layout`).  Packed masks come wrapped as `PackedMasks`.
    `window`: `proto` is the top-left window of a square map of side `Pv = max(Hp, Wp)` (utils/rect.py); always with a list of sizes
    (`ym_after_nms_window[_packed]`: the ragged entries with the virtual extent, one size being the one-entry table)."""
    L = hip.lib()
    device = proto.device
    *lead, k = coefs.shape
    batch, md = lead if len(lead) == 2 else (1, lead[0])
    *_, hp, wp, _ = proto.shape
    ragged = isinstance(sizes, list)
    pv = max(hp, wp) if window else 0
    if window and not ragged:
        raise RuntimeError('_after_nms_launch: window mode takes a list of sizes')
    if ragged:
        key = (tuple(sizes), md, hp, wp, packed, pv)
        plan = _ragged_plans.get(key)
        if plan is None:
            offsets, total = ragged_layout(sizes, md, packed)
            table = hip.ragged_table(sizes, offsets)
            if len(_ragged_plans) >= 1024:
                _ragged_plans.clear()
            plan = _ragged_plans[key] = (offsets, total, table, L.ym_after_nms_window_workspace_bytes(table, batch, md, hp, wp, pv))
        offsets, total, table, nbytes = plan
        shape, where = (total,), ((table, pv) if window else (table,))
        if window:
            fn, name = (L.ym_after_nms_window_packed if packed else L.ym_after_nms_window), 'ym_after_nms_window'
        else:
            fn, name = (L.ym_after_nms_ragged_packed if packed else L.ym_after_nms_ragged), 'ym_after_nms_ragged'
    else:
        img_h, img_w = sizes
        nbytes = L.ym_after_nms_batch_workspace_bytes(md, hp, wp, img_h, img_w)
        shape, where = (*lead, img_h, (img_w + 63) // 64 if packed else img_w), (img_h, img_w)     # (int64 words of PackedMasks)
        fn, name = (L.ym_after_nms_batch_packed if packed else L.ym_after_nms_batch), 'ym_after_nms_batch'
    # (tensors on the current device: no device switch around the launch, as in nms_batch)
    with _NO_SWITCH if device.index == torch.cuda.current_device() else torch.cuda.device(device):
        masks = torch.empty(*shape, dtype=torch.int64 if packed else torch.float32, device=device)
        box_px = torch.empty(*lead, 4, dtype=torch.int32, device=device)
        ws = _scratch(device, nbytes) if nbytes else None
        hip.check(fn(hip.ptr(proto), hip.ptr(coefs), hip.ptr(boxes), hip.ptr(counts, torch.int32), batch, md, hp, wp, k, *where,
                     int(do_crop), hip.ptr(masks, masks.dtype), hip.ptr(box_px, torch.int32),
                     ctypes.c_void_p(ws.data_ptr()) if ws is not None else None, nbytes, hip.stream_ptr()), name)
    if not ragged:
        return (PackedMasks._wrap(masks, img_h, img_w) if packed else masks), box_px
    if packed:
        return [PackedMasks._wrap(masks[o:o + md * h * ((w + 63) // 64)].view(md, h, -1), h, w) for (h, w), o in zip(sizes, offsets)], box_px
    return [masks[o:o + md * h * w].view(md, h, w) for (h, w), o in zip(sizes, offsets)], box_px


_scratch_bufs = {}


def _scratch(device, nbytes):
    key = (str(device), torch.cuda.current_stream(device).cuda_stream)
    b = _scratch_bufs.get(key)
    if b is None or b.numel() < nbytes:
        b = _scratch_bufs[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return b


# ---- batched post-processing (the reference's nms / after_nms are batch-1 only; eval.py loops) ---------------
class BatchDetections:
    """Device-resident result of `nms_batch` for B images, padded to max_detections rows per image.  `counts` stays on the device;
    `after_nms_batch` consumes it there, and the ONE host read of the batch happens in `after_nms_batch` (or `.split()`)."""

    def __init__(self, counts, ids, scores, boxes, coefs, proto):
        self.counts, self.ids, self.scores, self.boxes, self.coefs, self.proto = counts, ids, scores, boxes, coefs, proto

    def split(self):
        """Per-image 5-tuples exactly as `nms` returns them (five Nones for an image without detections)."""
        out = []
        for b, n in enumerate(self.counts.tolist()):             # the one host read
            out.append((None,) * 5 if n == 0 else
                       (self.ids[b, :n], self.scores[b, :n], self.boxes[b, :n], self.coefs[b, :n], self.proto[b]))
        return out


def nms_batch(class_pred, box_pred, coef_pred, proto_out, anchors, cfg):
    """`nms` for a whole batch [B, N, *] in one launch set, no host synchronisation: fast_nms, or with `cfg.traditional_nms` the
    greedy per-class path (`ym_detect_greedy_nms_batch`; `nms()` runs it as a batch of one).  Per image the result equals `nms(class_pred[b:b+1], ...)`
    (tests/test_gpu_postproc.py::test_batched_postprocessing_equals_per_image, tests/test_gpu_greedy_batch.py)."""
    if not class_pred.is_cuda:
        raise RuntimeError('yolact_minimal_amd.utils.output_utils.nms_batch needs CUDA (HIP) tensors; there is no CPU path.')
    if class_pred.dim() != 3:
        raise RuntimeError('nms_batch expects [B, N, C] predictions')
    device = class_pred.device
    batch, n_anchors, n_classes = class_pred.shape
    anchors_t = _anchors_on(anchors, device)
    if anchors_t.shape[0] != n_anchors:
        raise RuntimeError(f'{anchors_t.shape[0]} anchors for {n_anchors} predictions')
    # everything that depends only on the shapes and the thresholds is built once: an eager call spends its time between the
    # caller's line and the first launch HERE (~20 us of Python against ~68 us of device time: bench.post_bench's two columns)
    greedy = bool(getattr(cfg, 'traditional_nms', False))
    pkey = (device.index, batch, n_anchors, n_classes, coef_pred.shape[2], cfg.top_k, cfg.max_detections, cfg.nms_score_thre,
            cfg.nms_iou_thre, getattr(cfg, 'img_size', 544), greedy)
    plan = _plan_cache.get(pkey)
    L = hip.lib()
    if plan is None:
        ncfg = hip.NmsCfg(n_anchors, n_classes, coef_pred.shape[2], int(cfg.top_k), int(cfg.max_detections),
                          float(cfg.nms_score_thre), float(cfg.nms_iou_thre), float(getattr(cfg, 'img_size', 544)))
        # (the two paths carve different workspaces: the entry, its name and its size travel together)
        name = 'ym_detect_greedy_nms_batch' if greedy else 'ym_detect_fast_nms_batch'
        ws_bytes = L.ym_greedy_nms_batch_workspace_bytes if greedy else L.ym_nms_batch_workspace_bytes
        nbytes = ws_bytes(ctypes.byref(ncfg), batch)
        if nbytes == 0:
            raise RuntimeError(('ym_greedy_nms_batch_workspace_bytes: ' if greedy else 'ym_nms_batch_workspace_bytes: ') + L.ym_last_error().decode())
        plan = _plan_cache[pkey] = (ncfg, ctypes.byref(ncfg), nbytes, getattr(L, name), name)
    ncfg, ncfg_ref, nbytes, entry, entry_name = plan
    md = ncfg.max_det
    other_device = torch.cuda.current_device() != device.index
    if other_device:
        prev = torch.cuda.current_device()
        torch.cuda.set_device(device)
    try:
        stream = torch.cuda.current_stream().cuda_stream
        key = ('batch', device.index, stream, batch, n_anchors, n_classes, greedy)      # (scratch is per STREAM, like _nms_buffers)
        ws = _ws_cache.get(key)
        if ws is None or ws.numel() < nbytes:
            ws = _ws_cache[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
        counts = torch.empty(batch, dtype=torch.int32, device=device)
        ids = torch.empty(batch, md, dtype=torch.int64, device=device)
        scores = torch.empty(batch, md, dtype=torch.float32, device=device)
        boxes = torch.empty(batch, md, 4, dtype=torch.float32, device=device)
        coefs = torch.empty(batch, md, ncfg.coef_dim, dtype=torch.float32, device=device)
        hip.check(entry(hip.ptr(class_pred.contiguous()), hip.ptr(box_pred.contiguous()), hip.ptr(coef_pred.contiguous()),
                        hip.ptr(anchors_t), ncfg_ref, batch, hip.ptr(counts, torch.int32),
                        hip.ptr(ids, torch.int64), hip.ptr(scores), hip.ptr(boxes), hip.ptr(coefs),
                        ctypes.c_void_p(ws.data_ptr()), ws.numel(), ctypes.c_void_p(stream)), entry_name)
    finally:
        if other_device:
            torch.cuda.set_device(prev)
    return BatchDetections(counts, ids, scores, boxes, coefs, proto_out)


def ragged_layout(sizes, max_det, packed=False):
    """Where `ym_after_nms_ragged[_packed]` puts the masks of a batch whose images differ in size: `(offsets, total)` in elements
    (floats, or 64-bit words when `packed`) of ONE flat buffer.  Image b's block is `[max_det, h_b, w_b]` floats (packed:
    `[max_det, h_b, ceil(w_b / 64)]` words) at `offsets[b]`; every block starts at a multiple of 256 bytes (the dense kernel stores 16
    bytes at a time, and an odd `max_det` x odd height x odd width would leave the next block misaligned); `total` ends the last
    block.  Pure Python: no GPU, no library."""
    max_det = int(max_det)
    if max_det < 1:
        raise RuntimeError(f'ragged_layout: max_det = {max_det}')
    return hip.aligned_layout('ragged_layout', sizes, 8 if packed else 4, lambda h, w: max_det * h * ((w + 63) // 64 if packed else w))


def after_nms_batch(dets, img_h, img_w, cfg=None, sync=True, packed=False, window=False):
    """`after_nms` for every image of a `BatchDetections` in one launch set.  Returns a list of per-image 4-tuples like `after_nms`
    -- or, with `sync=False`, the padded device tensors (ids, scores, boxes_px, masks, counts) without any host read.
    `packed=True` (or `cfg.packed_masks`): the masks are `PackedMasks`.
    Ints `img_h`, `img_w`: all images are resized to that one size (a bench / fixed-size serving batch); the padded masks are
    `[B, max_det, img_h, img_w]` (packed: `[B, max_det, img_h, ceil(img_w / 64)]` words).
    Sequences of B heights and B widths: every image at its OWN size (`ym_after_nms_ragged`, also when the sizes are all equal);
    the padded `masks` is then a list of B per-image views `[max_det, h_b, w_b]` of one flat allocation (`ragged_layout`), each
    what the consumers of one image's padded rows take (`DeviceAPData.add`, `rle_encode`, `draw_img`).
    `window=True`: `dets.proto` is the `[B, Hp, Wp, 32]` window of a rectangular forward (utils/rect.py; `ym_after_nms_window`).  The
    window entries take the size table, so ints `img_h`, `img_w` mean B entries of that size and `masks` is the list of views."""
    packed = _want_packed(cfg, packed)
    batch, md = dets.ids.shape
    if window and not hasattr(img_h, '__len__') and not hasattr(img_w, '__len__'):
        img_h, img_w = [int(img_h)] * batch, [int(img_w)] * batch
    do_crop = not (cfg and getattr(cfg, 'no_crop', False))
    if cfg and getattr(cfg, 'save_lincomb', False):
        raise NotImplementedError('draw_lincomb (visualisation, reference output_utils.py:276-324) is out of scope')
    if hasattr(img_h, '__len__') or hasattr(img_w, '__len__'):
        if not (hasattr(img_h, '__len__') and hasattr(img_w, '__len__')) or len(img_h) != batch or len(img_w) != batch:
            raise RuntimeError(f'after_nms_batch: {batch} heights and {batch} widths expected for a batch of {batch} images')
        sizes = [(int(h), int(w)) for h, w in zip(img_h, img_w)]
        ragged_layout(sizes, md, packed)                          # (size and batch-bound errors, before any launch)
        if not dets.proto.is_cuda:
            raise RuntimeError('yolact_minimal_amd.utils.output_utils.after_nms_batch needs CUDA (HIP) tensors; there is no CPU path.')
    else:
        sizes = (img_h, img_w)
    masks, box_px = _after_nms_launch(dets.proto.contiguous(), dets.coefs, dets.boxes, dets.counts, sizes, do_crop, packed, window=bool(window))
    if not sync:
        return dets.ids, dets.scores, box_px, masks, dets.counts
    vt = float(getattr(cfg, 'visual_thre', 0) or 0) if cfg else 0.0
    return unpad_detections(dets.ids, dets.scores, box_px, masks, dets.counts.tolist(), vt)     # the ONE host read of the whole batch


def unpad_detections(ids, scores, box_px, masks, counts_list, visual_thre=0.0):
    """The padded rows of `after_nms_batch(sync=False)` and the counts as a HOST list -> per-image 4-tuples like `after_nms`:
    `(None,) * 4` for an image without detections, also when `visual_thre` (detect.py's score filter: per detection, so it
    commutes with the post-processing) removes all of them.  `masks`: the padded tensor, a `PackedMasks`, or the list of per-image
    views.  Plain indexing, so it runs on CPU tensors too."""
    out = []
    for b, n in enumerate(counts_list):
        if n == 0:
            out.append((None,) * 4)
            continue
        r = (ids[b, :n], scores[b, :n], box_px[b, :n], masks[b][:n])
        if visual_thre > 0:
            keep = r[1] >= visual_thre
            r = tuple(t[keep] for t in r) if bool(keep.any()) else (None,) * 4
        out.append(r)
    return out


from .draw import draw_img, draw_batch, cutout_mattes  # noqa: E402,F401  (the device renderer; it imports _scratch from here lazily)
