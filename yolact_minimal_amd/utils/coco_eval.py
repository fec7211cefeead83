"""COCO-protocol evaluation on the device: what `eval.py --coco_api` gets from `pycocotools.cocoeval.COCOeval` (`eval.py:90-104`).

`pycocotools` does not exist on this stack, so the protocol is restated from the published cocoapi algorithm: `cocoeval.py`
`evaluate` / `computeIoU` / `evaluateImg` / `accumulate` / `summarize` and `common/maskApi.c` `bbIou` / `rleIou`, with cocoapi's
default parameters (`CocoParams` = `Params.setDetParams`, `useCats = 1`).  It is a different protocol from the reference's own
`prep_metrics` / `calc_map` (`utils/device_metrics.py`): crowd regions, area ranges, `maxDets`, average recall, `iou >= t` matching
where the LAST gt wins among equal IoUs.  Parity with the real cocoapi is unpinned (the yardstick is `tests/coco_eval_ref.py`).

`DeviceCOCOeval` keeps its state in a device log (`include/yolact_hip.h`, "device-resident COCO evaluator"): `add` is
`ym_coco_iou_box` + `ym_coco_iou_mask_packed` + `ym_coco_match_log` on the caller's stream and reads nothing on the host;
`accumulate` is one stable device sort, `ym_coco_accumulate` and ONE download of the `precision` / `recall` grids in cocoapi's shapes;
`summarize` is host numpy on those grids (`summarize_grids`, exactly cocoapi's `_summarize`).  Every image handed to `add` counts,
also one without detections (its gts lower recall); `score_results` hands it every image of the annotation file, as `COCOeval` does.

`add_batch` is the metric stage of a whole request of B <= 32 images of different sizes in ONE call
(`ym_eval_coco_add_ragged_packed`: at most three launches, packed masks only) against a `COCOGtBatch`; the log is the one B `add`
calls leave.  `evaluate.evaluate_coco_pipelined` drives either with several requests in flight.

Ground truth comes from the annotation file (`coco_gt`, `coco_gt_batch`), not from the val loader, which drops crowds and normalises
boxes.

Not covered: `keypoints`, `useCats = 0`, merging evaluators across ranks, NaN scores, more than 512 gts per image.
"""
import ctypes
import json

import numpy as np
import torch

from .. import hip
from .packed_masks import PackedMasks, as_packed

KINDS = ('bbox', 'segm')


class CocoParams:
    """cocoeval.py `Params.setDetParams`: the defaults, as the arrays the kernels are handed (nothing is recomputed on the device)."""

    def __init__(self):
        self.iouThrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
        self.recThrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
        self.maxDets = [1, 10, 100]
        self.areaRng = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
        self.areaRngLbl = ['all', 'small', 'medium', 'large']
        self.useCats = 1
        self.eps = float(np.spacing(1))


def summarize_grids(precision, recall, params=None):
    """cocoeval.py `summarize` / `_summarizeDets` on `precision` [T, R, K, A, M] and `recall` [T, K, A, M] (host numpy only):
    (stats float64 [12], the twelve lines cocoapi prints, joined by newlines)."""
    p = CocoParams() if params is None else params
    lines = []

    def _summarize(ap=1, iouThr=None, areaRng='all', maxDets=100):
        iStr = ' {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'
        titleStr = 'Average Precision' if ap == 1 else 'Average Recall'
        typeStr = '(AP)' if ap == 1 else '(AR)'
        iouStr = '{:0.2f}:{:0.2f}'.format(p.iouThrs[0], p.iouThrs[-1]) if iouThr is None else '{:0.2f}'.format(iouThr)
        aind = [i for i, aRng in enumerate(p.areaRngLbl) if aRng == areaRng]
        mind = [i for i, mDet in enumerate(p.maxDets) if mDet == maxDets]
        s = precision if ap == 1 else recall
        if iouThr is not None:
            s = s[np.where(iouThr == p.iouThrs)[0]]
        s = s[:, :, :, aind, mind] if ap == 1 else s[:, :, aind, mind]
        mean_s = -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
        lines.append(iStr.format(titleStr, typeStr, iouStr, areaRng, maxDets, mean_s))
        return mean_s

    last = p.maxDets[2]
    stats = np.zeros((12,))
    stats[0] = _summarize(1)
    stats[1] = _summarize(1, iouThr=.5, maxDets=last)
    stats[2] = _summarize(1, iouThr=.75, maxDets=last)
    stats[3] = _summarize(1, areaRng='small', maxDets=last)
    stats[4] = _summarize(1, areaRng='medium', maxDets=last)
    stats[5] = _summarize(1, areaRng='large', maxDets=last)
    stats[6] = _summarize(0, maxDets=p.maxDets[0])
    stats[7] = _summarize(0, maxDets=p.maxDets[1])
    stats[8] = _summarize(0, maxDets=last)
    stats[9] = _summarize(0, areaRng='small', maxDets=last)
    stats[10] = _summarize(0, areaRng='medium', maxDets=last)
    stats[11] = _summarize(0, areaRng='large', maxDets=last)
    return stats, '\n'.join(lines)


# ---- ground truth from the annotation file ------------------------------------------------------------------------------------
def coco_gt_records(coco, image_id, label_map):
    """Host half of `coco_gt`: the image's annotations in file order as plain records `{'cls', 'iscrowd', 'area', 'bbox',
    'segmentation'}` (`cls` = `label_map[category_id] - 1`, the class index of the network's heads; crowds are KEPT).  An
    annotation whose category the label map does not know is no ground truth of any evaluated category and is left out."""
    out = []
    for a in coco.imgToAnns.get(image_id, []):
        if a['category_id'] not in label_map:
            continue
        out.append({'cls': int(label_map[a['category_id']]) - 1, 'iscrowd': int(a.get('iscrowd', 0)), 'area': float(a['area']),
                    'bbox': [float(v) for v in a['bbox']], 'segmentation': a.get('segmentation')})
    return out


class COCOGt:
    """The ground truth of one image on the device: `cls` int32 [g], `crowd` uint8 [g], `area` float64 [g], `bbox` float64 [g, 4]
    ([x, y, w, h]) and `masks`, a `PackedMasks` [g, height, width] (None when only `bbox` is evaluated)."""

    __slots__ = ('g', 'cls', 'crowd', 'area', 'bbox', 'masks', 'height', 'width')

    @classmethod
    def from_arrays(cls_, cls, crowd, area, bbox, masks, height, width, device):
        """Host arrays (one upload each) and `masks`: None, a `PackedMasks`, or a dense [g, height, width] tensor (packed here)."""
        self = object.__new__(cls_)
        dev = torch.device(device)
        self.g, self.height, self.width = int(len(cls)), int(height), int(width)
        up = lambda a, dt, shape: torch.from_numpy(np.ascontiguousarray(a, dtype=dt).reshape(shape)).to(dev)   # noqa: E731
        self.cls, self.crowd = up(cls, np.int32, (self.g,)), up(crowd, np.uint8, (self.g,))
        self.area, self.bbox = up(area, np.float64, (self.g,)), up(bbox, np.float64, (self.g, 4))
        if masks is not None and not isinstance(masks, PackedMasks):
            masks = masks.to(dev)
            masks = as_packed(masks, self.height, self.width) if self.g else None
        if masks is not None and len(masks) != self.g:
            raise RuntimeError(f'COCOGt: {self.g} annotations but {len(masks)} masks')
        self.masks = masks
        return self


def coco_gt(coco, image_id, label_map, device='cuda', masks=True):
    """The gt bundle of image `image_id` of the `COCO` index: `coco_gt_records`, the masks rasterised on the device
    (`anns_to_masks` at the image record's height and width) and bit-packed."""
    from .coco import anns_to_masks
    rec = coco_gt_records(coco, image_id, label_map)
    info = coco.imgs[image_id]
    h, w = int(info['height']), int(info['width'])
    m = None
    if masks and rec:
        m = PackedMasks.pack(anns_to_masks([r['segmentation'] for r in rec], h, w, device))
    return COCOGt.from_arrays([r['cls'] for r in rec], [r['iscrowd'] for r in rec], [r['area'] for r in rec],
                              [r['bbox'] for r in rec], m, h, w, device)


def _resolved(device):
    """`device` with its index filled in: 'cuda' names the current device, so it equals 'cuda:N' for that N."""
    d = torch.device(device)
    return torch.device('cuda', torch.cuda.current_device()) if d.type == 'cuda' and d.index is None else d


class COCOGtBatch:
    """The ground truth of the B <= 32 images of one request on the device, as `ym_eval_coco_add_ragged_packed` takes it:
    `sizes` [(height, width)] and `first` [B + 1] on the host (image b owns the annotations `first[b] .. first[b + 1]`); `cls` int32
    [G], `crowd` uint8 [G], `area` float64 [G], `bbox` float64 [G, 4] (None when G = 0); with masks, `bits` = ONE flat int64 tensor of
    packed blocks `[g_b, h_b, ceil(w_b / 64)]` at `offsets[b]` (every block at a multiple of 256 bytes; None when G = 0) and `table`,
    their `hip.ragged_table`.  `table is None`: the bundle has no masks ('bbox' only)."""

    __slots__ = ('sizes', 'first', 'cls', 'crowd', 'area', 'bbox', 'bits', 'offsets', 'table', 'device')

    def __len__(self):
        return len(self.sizes)

    def masks(self, b):
        """Image b's gt masks: a `PackedMasks` view `[g_b, h_b, w_b]` of `bits` (None without masks or without annotations)."""
        g, (h, w) = self.first[b + 1] - self.first[b], self.sizes[b]
        if self.table is None or not g:
            return None
        wq = (w + 63) // 64
        return PackedMasks(self.bits[self.offsets[b]:self.offsets[b] + g * h * wq].view(g, h, wq), h, w)

    @classmethod
    def _empty(cls_, sizes, g, device, masks, what):
        self = object.__new__(cls_)
        self.sizes, self.device = [(int(h), int(w)) for h, w in sizes], torch.device(device)
        self.first = [0]
        for v in g:
            self.first.append(self.first[-1] + int(v))
        self.cls = self.crowd = self.area = self.bbox = self.bits = self.offsets = self.table = None
        if masks:
            rows = iter(g)                                      # (aligned_layout asks for the extents in image order)
            self.offsets, total = hip.aligned_layout(what, self.sizes, 8, lambda h, w: next(rows) * h * ((w + 63) // 64))
            self.table = hip.ragged_table(self.sizes, self.offsets)
            if self.first[-1]:
                self.bits = torch.empty(max(total, 1), dtype=torch.int64, device=self.device)
        elif not 1 <= len(self.sizes) <= hip.RAGGED_MAX_IMAGES:
            raise RuntimeError(f'{what}: 1 .. {hip.RAGGED_MAX_IMAGES} images per call, got {len(self.sizes)}')
        return self

    @classmethod
    def from_gts(cls_, gts):
        """The per-image bundles `[COCOGt, ...]` of a request as one: device-side concatenation of the scalar fields and one copy
        of every image's packed masks into its block.  The bundle has masks when every image that has annotations brought them."""
        what = 'COCOGtBatch.from_gts'
        gts = list(gts)
        if not gts or any(not isinstance(gt, COCOGt) for gt in gts):
            raise RuntimeError(f'{what}: a non-empty list of COCOGt expected')
        live = [gt for gt in gts if gt.g]
        masks = all(gt.masks is not None for gt in live)
        self = cls_._empty([(gt.height, gt.width) for gt in gts], [gt.g for gt in gts], gts[0].cls.device, masks, what)
        if live:
            join = lambda ts: ts[0].contiguous() if len(ts) == 1 else torch.cat(ts, 0)   # noqa: E731
            self.cls, self.crowd = join([gt.cls for gt in live]), join([gt.crowd for gt in live])
            self.area, self.bbox = join([gt.area for gt in live]), join([gt.bbox for gt in live])
        if masks:
            for b, gt in enumerate(gts):
                if gt.g:
                    if (gt.masks.height, gt.masks.width) != (gt.height, gt.width):
                        raise RuntimeError(f'{what}: image {b}: masks of {gt.masks.height} x {gt.masks.width} in a {gt.height} x {gt.width} image')
                    self.masks(b).bits.copy_(gt.masks.bits)
        return self


def coco_gt_batch(coco, image_ids, label_map, device='cuda', masks=True, live=None):
    """The gt bundle of the images `image_ids` (at most 32) of the `COCO` index, built from the annotation file: `coco_gt_records`
    per image, ONE upload of the scalar fields, and with `masks` one `anns_to_masks_batch` (the ragged rasteriser) plus ONE
    `ym_pack_masks_ragged` launch.  Equal to `COCOGtBatch.from_gts([coco_gt(coco, i, ...) for i in image_ids])`.  `live`: one flag
    per image; an entry whose flag is false is a request's padding and brings its size only (no annotation of it is decoded,
    uploaded or rasterised)."""
    from .coco import anns_to_masks_batch
    what = 'coco_gt_batch'
    dev = torch.device(device)
    image_ids = list(image_ids)
    live = [True] * len(image_ids) if live is None else list(live)
    if len(live) != len(image_ids):
        raise RuntimeError(f'{what}: {len(image_ids)} image ids but {len(live)} live flags')
    recs = [coco_gt_records(coco, i, label_map) if keep else [] for i, keep in zip(image_ids, live)]
    sizes = [(int(coco.imgs[i]['height']), int(coco.imgs[i]['width'])) for i in image_ids]
    g = [len(r) for r in recs]
    self = COCOGtBatch._empty(sizes, g, dev, masks, what)
    flat = [r for rec in recs for r in rec]
    total = len(flat)
    if not total:
        return self
    with torch.cuda.device(dev):
        # bbox fp64 [G][4] | area fp64 [G] | cls int32 [G] | crowd uint8 [G] in one host buffer: every array starts at a multiple of its
        # element size
        host = np.empty(45 * total, np.uint8)
        host[:32 * total].view(np.float64)[:] = np.asarray([r['bbox'] for r in flat], np.float64).reshape(-1)
        host[32 * total:40 * total].view(np.float64)[:] = [r['area'] for r in flat]
        host[40 * total:44 * total].view(np.int32)[:] = [r['cls'] for r in flat]
        host[44 * total:] = [r['iscrowd'] for r in flat]
        up = torch.from_numpy(host).to(dev)
        self.bbox, self.area = up[:32 * total].view(torch.float64).view(total, 4), up[32 * total:40 * total].view(torch.float64)
        self.cls, self.crowd = up[40 * total:44 * total].view(torch.int32), up[44 * total:]
        if masks:
            dense = anns_to_masks_batch([[r['segmentation'] for r in rec] for rec in recs], sizes, dev)
            own = [b for b in range(len(sizes)) if g[b]]
            hip.check(hip.lib().ym_pack_masks_ragged(
                (ctypes.c_void_p * len(own))(*[dense[b].data_ptr() for b in own]), 1, (ctypes.c_int32 * len(own))(*[g[b] for b in own]),
                hip.ragged_table([sizes[b] for b in own], [self.offsets[b] for b in own]), len(own), hip.ptr(self.bits, torch.int64),
                hip.stream_ptr()), 'ym_pack_masks_ragged')
    return self


class DeviceCOCOeval:
    """`DeviceCOCOeval(num_classes, device, max_det=100, kinds=('bbox', 'segm'), capacity_images=256)`: see the module text.
    `max_det` is the number of detection rows an image may bring (the log's row stride); cocoapi's `maxDets` stay [1, 10, 100].  The
    log grows by doubling; image slots may be filled in any order and from several streams; cocoapi walks images in ascending
    image id, so the image index is that order."""

    def __init__(self, num_classes, device, max_det=100, kinds=KINDS, capacity_images=256, params=None):
        self.num_classes, self.device, self.max_det = int(num_classes), torch.device(device), int(max_det)
        self.kinds = tuple(kinds)
        self.params = p = CocoParams() if params is None else params
        if not self.kinds or any(k not in KINDS for k in self.kinds):
            raise RuntimeError(f"DeviceCOCOeval: kinds are 'bbox' and / or 'segm', got {kinds}")
        if not 0 < len(p.iouThrs) <= hip.EVAL_MAX_THRESHOLDS or len(p.areaRng) != hip.COCO_AREAS:
            raise RuntimeError(f'DeviceCOCOeval: 1 .. {hip.EVAL_MAX_THRESHOLDS} IoU thresholds and {hip.COCO_AREAS} area ranges')
        if not 0 < self.max_det <= hip.EVAL_MAX_DET or self.num_classes <= 0:
            raise RuntimeError(f'DeviceCOCOeval: need 0 < max_det <= {hip.EVAL_MAX_DET} and num_classes > 0')
        if self.device.type != 'cuda':
            raise RuntimeError('yolact_minimal_amd has no CPU path: DeviceCOCOeval needs a CUDA/HIP device')
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(self.device)     # noqa: E731
        # (the only uploads of the evaluator's life: `add` never copies from the host)
        self.thr, self.rec_thr = up(p.iouThrs, np.float64), up(p.recThrs, np.float64)
        self.area_rng, self.max_dets = up(np.asarray(p.areaRng, np.float64).reshape(-1), np.float64), up(sorted(p.maxDets), np.int32)
        self.npig = torch.zeros(hip.COCO_AREAS, self.num_classes, dtype=torch.int64, device=self.device)
        self.class_rows = torch.zeros(self.num_classes, dtype=torch.int32, device=self.device)
        self.capacity = 0
        self.score = self.cls = self.rank = self.flags = None
        self._seen = set()
        self._writers = {}
        self._grown = None
        self._synced = set()
        with torch.cuda.device(self.device):
            self._grow(max(1, int(capacity_images)))

    # ---- log storage (as DeviceAPData) ------------------------------------------------------------------------------------
    def _grow(self, capacity):
        cur = torch.cuda.current_stream(self.device)
        rows = capacity * self.max_det
        score = torch.zeros(rows, dtype=torch.float32, device=self.device)
        cls = torch.full((rows,), -1, dtype=torch.int32, device=self.device)
        rank = torch.zeros(rows, dtype=torch.int32, device=self.device)
        flags = torch.zeros(rows, hip.COCO_WORDS_PER_ROW, dtype=torch.int32, device=self.device)
        if self.capacity:
            old = self.capacity * self.max_det
            for st in self._writers.values():                   # every row written so far is copied: the copy runs behind the writers
                if st != cur:
                    cur.wait_stream(st)
            for new, prev in ((score, self.score), (cls, self.cls), (rank, self.rank), (flags, self.flags)):
                new[:old].copy_(prev)
                prev.record_stream(cur)
        self._grown = torch.cuda.Event()
        self._grown.record(cur)
        self._writers = {}
        self._synced = {cur.cuda_stream}
        self.score, self.cls, self.rank, self.flags, self.capacity = score, cls, rank, flags, capacity

    def _join_writers(self):
        cur = torch.cuda.current_stream(self.device)
        for st in self._writers.values():
            if st != cur:
                cur.wait_stream(st)
        if self._grown is not None and cur.cuda_stream not in self._synced:
            cur.wait_event(self._grown)
            self._synced.add(cur.cuda_stream)
        return cur

    @property
    def images(self):
        """Image slots consumed so far."""
        return len(self._seen)

    # ---- evaluateImg --------------------------------------------------------------------------------------------------------
    def add(self, ids, scores, boxes_px, masks, counts, gt, image_index=None):
        """One image: padded device detections (`after_nms`' tensors; `counts` = a device int32 or None for "all rows") against
        its `COCOGt`.  Rows whose pixel box is empty are no detections (`eval.py:65`).  `ids=None` (or no rows): the image only
        counts its gts.  Runs on the current stream; no host read."""
        if ids is None or int(ids.shape[-1]) == 0:
            return self._add(None, None, None, None, None, None, gt, image_index)
        if ids.dim() == 2 and ids.shape[0] == 1:                # a leading batch dimension of 1
            ids, scores, boxes_px, masks = ids[0], scores[0], boxes_px[0], masks[0]
        if boxes_px is None or boxes_px.dim() != 2 or boxes_px.shape[0] != ids.shape[0] or boxes_px.shape[1] != 4:
            raise RuntimeError(f'DeviceCOCOeval.add: pixel boxes [{ids.shape[0]}, 4] expected')
        xywh = None
        if 'bbox' in self.kinds:
            b = boxes_px.to(torch.float64)
            xywh = torch.cat([b[:, :2], b[:, 2:] - b[:, :2]], dim=1)
        return self._add(ids, scores, counts, boxes_px.to(torch.int32).contiguous(), xywh, masks, gt, image_index)

    def _add(self, ids, scores, counts, boxes_px, xywh, masks, gt, image_index):
        """`add` behind its argument forms: `boxes_px` (validity, may be None = every row below the count) and the bbox as fp64
        `xywh` are separate, so `score_results` can hand in the JSON's boxes as they are."""
        index = len(self._seen) if image_index is None else int(image_index)
        if index < 0 or index in self._seen:
            raise RuntimeError(f'DeviceCOCOeval.add: image index {index} was added before' if index >= 0 else
                               f'DeviceCOCOeval.add: image index {index} < 0')
        if not isinstance(gt, COCOGt):
            raise RuntimeError('DeviceCOCOeval.add: gt is a COCOGt (coco_gt / COCOGt.from_arrays)')
        n = 0 if ids is None else int(ids.shape[0])
        g = gt.g
        if n > self.max_det:
            raise RuntimeError(f'DeviceCOCOeval.add: at most max_det = {self.max_det} detection rows, got {n}')
        if g > hip.COCO_MAX_GT:
            raise RuntimeError(f'DeviceCOCOeval.add: at most {hip.COCO_MAX_GT} ground-truth annotations per image, got {g}')
        if n and (scores.numel() != n or (counts is not None and counts.numel() < 1)):
            raise RuntimeError(f'DeviceCOCOeval.add: {n} ids but {scores.numel()} scores (or an empty count tensor)')
        segm, bbox = 'segm' in self.kinds, 'bbox' in self.kinds
        if n and segm:
            if masks is None or len(masks) != n or (g and gt.masks is None):
                raise RuntimeError(f"DeviceCOCOeval.add: 'segm' needs {n} detection masks and the gt masks")
            if isinstance(masks, PackedMasks) and (masks.height, masks.width) != (gt.height, gt.width):
                raise RuntimeError(f'DeviceCOCOeval.add: masks of {masks.height} x {masks.width} in a {gt.height} x {gt.width} image')
        if n and bbox and (xywh is None or tuple(xywh.shape) != (n, 4)):
            raise RuntimeError(f"DeviceCOCOeval.add: 'bbox' needs [{n}, 4] boxes")
        # (the argument checks are above this line and the index is consumed only behind the launch that writes its rows: a call
        # that raises leaves the evaluator as it was)
        L = hip.lib()
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            if index >= self.capacity:
                cap = self.capacity
                while cap <= index:
                    cap *= 2
                self._grow(cap)
            elif self._grown is not None and cur.cuda_stream not in self._synced:
                cur.wait_event(self._grown)
                self._synced.add(cur.cuda_stream)
            iou_box = iou_mask = area_box = area_mask = None
            if n and bbox:
                xywh = xywh.contiguous()
                area_box = xywh[:, 2] * xywh[:, 3]
                if g:
                    iou_box = torch.empty(n, g, dtype=torch.float64, device=self.device)
                    hip.check(L.ym_coco_iou_box(hip.ptr(xywh, torch.float64), n, hip.ptr(gt.bbox, torch.float64), g,
                                                hip.ptr(gt.crowd, torch.uint8), hip.ptr(iou_box, torch.float64), hip.stream_ptr()),
                              'ym_coco_iou_box')
            if n and segm:
                pm = as_packed(masks, gt.height, gt.width).contiguous()
                words = gt.height * pm.bits.shape[-1]
                area_mask = torch.empty(n, dtype=torch.int32, device=self.device)
                if g:
                    gbits, gcrowd, gg = gt.masks.bits.contiguous(), gt.crowd, g
                else:                                           # the detections' areas are still needed: one empty stand-in gt row
                    gbits = torch.zeros(1, gt.height, pm.bits.shape[-1], dtype=torch.int64, device=self.device)
                    gcrowd, gg = torch.zeros(1, dtype=torch.uint8, device=self.device), 1
                iou_mask = torch.empty(n, gg, dtype=torch.float64, device=self.device)
                hip.check(L.ym_coco_iou_mask_packed(hip.ptr(pm.bits, torch.int64), n, hip.ptr(gbits, torch.int64), gg, words,
                                                    hip.ptr(gcrowd, torch.uint8), hip.ptr(iou_mask, torch.float64),
                                                    hip.ptr(area_mask, torch.int32), hip.stream_ptr()), 'ym_coco_iou_mask_packed')
            hip.check(L.ym_coco_match_log(
                hip.ptr(ids.contiguous(), torch.int64) if n else None, hip.ptr(scores.contiguous()) if n else None,
                hip.ptr(counts, torch.int32) if (n and counts is not None) else None, n,
                hip.ptr(boxes_px, torch.int32) if (n and boxes_px is not None) else None,
                hip.ptr(iou_box, torch.float64), hip.ptr(iou_mask, torch.float64), hip.ptr(area_box, torch.float64),
                hip.ptr(area_mask, torch.int32), hip.ptr(gt.cls, torch.int32) if g else None,
                hip.ptr(gt.crowd, torch.uint8) if g else None, hip.ptr(gt.area, torch.float64) if g else None, g,
                hip.ptr(self.thr, torch.float64), len(self.params.iouThrs), hip.ptr(self.area_rng, torch.float64), self.num_classes,
                int(max(self.params.maxDets)), hip.ptr(self.score), hip.ptr(self.cls, torch.int32), hip.ptr(self.rank, torch.int32),
                hip.ptr(self.flags, torch.int32), index * self.max_det, hip.ptr(self.npig, torch.int64),
                hip.ptr(self.class_rows, torch.int32), hip.stream_ptr()), 'ym_coco_match_log')
            self._seen.add(index)
            self._writers[cur.cuda_stream] = cur
        return index

    def add_batch(self, ids, scores, boxes_px, masks, counts, gt_batch, image_indices, mask_table=None):
        """One request of B <= 32 images of different sizes in ONE call (`ym_eval_coco_add_ragged_packed`: at most three launches
        and nothing else on the device); the log and the counters end up exactly as after `add` on each image.  Runs on the
        current stream; no host read.
          ids / scores `[B, max_det]`, boxes_px int32 `[B, max_det, 4]`, counts int32 `[B]`: `after_nms_batch(..., sync=False)` rows,
          with `max_det` the evaluator's.  Without 'bbox', `boxes_px` may be None: every row below its count is then a detection
          (with the boxes, a row whose pixel box is empty is none, `eval.py:65`);
          masks ('segm' only, else ignored): the list of B `PackedMasks` views that `after_nms_batch(dets, hs, ws, ..., packed=True)`
          returns -- or, with `mask_table` (their `hip.ragged_table`), view 0 alone.  Dense masks raise;
          gt_batch: the `COCOGtBatch` of the B images (`coco_gt_batch` / `COCOGtBatch.from_gts`);
          image_indices: B image slots, `None` = the entry is padding (nothing of it is read, written or counted).
        Returns the slots added.  A refused call (bad arguments, more than 512 annotations in an image) consumes no image index and
        writes no log row; like `add`, it may already have grown the log for its largest index (capacity and buffers change, contents
        do not) when the refusal comes from the C entry."""
        from .draw import _ragged_mask_table
        from .output_utils import _scratch
        what = 'DeviceCOCOeval.add_batch'
        if not isinstance(gt_batch, COCOGtBatch):
            raise RuntimeError(f'{what}: gt_batch is a COCOGtBatch (coco_gt_batch / COCOGtBatch.from_gts)')
        sizes, gt_first = gt_batch.sizes, gt_batch.first
        batch, md = len(sizes), self.max_det
        segm, bbox = 'segm' in self.kinds, 'bbox' in self.kinds
        if tuple(ids.shape) != (batch, md) or tuple(scores.shape) != (batch, md) or (boxes_px is None and bbox) or \
                (boxes_px is not None and tuple(boxes_px.shape) != (batch, md, 4)) or counts is None or counts.numel() != batch or \
                len(image_indices) != batch:
            raise RuntimeError(f'{what}: ids / scores [{batch}, {md}], boxes_px [{batch}, {md}, 4], {batch} counts and {batch} image indices '
                               f"expected (max_det is the evaluator's; the gt bundle holds {batch} images), got {tuple(ids.shape)} / "
                               f'{tuple(scores.shape)} / {None if boxes_px is None else tuple(boxes_px.shape)}')
        if _resolved(gt_batch.device) != _resolved(self.device):
            raise RuntimeError(f'{what}: the gt bundle is on {gt_batch.device}, the evaluator on {self.device}')
        if segm:
            if gt_batch.table is None:
                raise RuntimeError(f"{what}: 'segm' needs a gt bundle with masks")
            if mask_table is None:
                first = masks[0] if isinstance(masks, (list, tuple)) and len(masks) else masks
                if not isinstance(first, PackedMasks):
                    raise RuntimeError(f'{what}: the batched metric stage takes packed masks only (after_nms_batch(..., packed=True))')
                masks, mask_table = _ragged_mask_table(masks, sizes, md, what)
            elif not isinstance(masks, PackedMasks):
                raise RuntimeError(f'{what}: the batched metric stage takes packed masks only (after_nms_batch(..., packed=True))')
        index = [-1 if i is None else int(i) for i in image_indices]
        live = [i for i in index if i >= 0]
        if any(i < 0 for i, given in zip(index, image_indices) if given is not None) or len(set(live)) != len(live) or \
                any(i in self._seen for i in live):
            raise RuntimeError(f'{what}: image indices {live} are negative, repeated or were added before')
        most = max(gt_first[b + 1] - gt_first[b] for b in range(batch))
        if most > hip.COCO_MAX_GT:
            raise RuntimeError(f'{what}: at most {hip.COCO_MAX_GT} ground-truth annotations per image, got {most}')
        if not live:
            return []
        kinds = sum(1 << KINDS.index(kd) for kd in self.kinds)
        L = hip.lib()
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            first_c = (ctypes.c_int32 * (batch + 1))(*gt_first)
            index_c = (ctypes.c_int64 * batch)(*index)
            nbytes = L.ym_eval_coco_add_ragged_workspace_bytes(mask_table if segm else None, first_c, batch, md, kinds)
            if nbytes == 0:
                raise RuntimeError(f'{what}: ym_eval_coco_add_ragged_workspace_bytes refuses these sizes (h * ceil(w / 64) < 2^24 words per '
                                   f'mask): {sizes}, gt rows {gt_first}')
            ws = _scratch(self.device, nbytes)
            # (the log grows for the largest index first; like `add`, the indices are consumed only behind the launch that writes them)
            if max(live) >= self.capacity:
                cap = self.capacity
                while cap <= max(live):
                    cap *= 2
                self._grow(cap)
            elif self._grown is not None and cur.cuda_stream not in self._synced:
                cur.wait_event(self._grown)
                self._synced.add(cur.cuda_stream)
            have = gt_first[-1] > 0
            hip.check(L.ym_eval_coco_add_ragged_packed(
                hip.ptr(ids, torch.int64), hip.ptr(scores), hip.ptr(boxes_px, torch.int32), hip.ptr(counts, torch.int32), batch, md,
                hip.ptr(masks.bits, torch.int64) if segm else None, mask_table if segm else None,
                hip.ptr(gt_batch.cls, torch.int32) if have else None, hip.ptr(gt_batch.crowd, torch.uint8) if have else None,
                hip.ptr(gt_batch.area, torch.float64) if have else None, hip.ptr(gt_batch.bbox, torch.float64) if have and bbox else None,
                first_c, hip.ptr(gt_batch.bits, torch.int64) if have and segm else None, gt_batch.table if segm else None, index_c,
                hip.ptr(self.thr, torch.float64), len(self.params.iouThrs), hip.ptr(self.area_rng, torch.float64), self.num_classes,
                int(max(self.params.maxDets)), kinds, hip.ptr(self.score), hip.ptr(self.cls, torch.int32),
                hip.ptr(self.rank, torch.int32), hip.ptr(self.flags, torch.int32), self.capacity * md, hip.ptr(self.npig, torch.int64),
                hip.ptr(self.class_rows, torch.int32), ctypes.c_void_p(ws.data_ptr()), ws.numel(), hip.stream_ptr()),
                'ym_eval_coco_add_ragged_packed')
            self._seen.update(live)
            self._writers[cur.cuda_stream] = cur
        return live

    # ---- accumulate / summarize ---------------------------------------------------------------------------------------------
    def _sorted_order(self):
        """(rows, order int64 [rows], seg int64 [classes + 1]): the log positions in (class ascending, score descending, log position
        ascending) order -- cocoapi's mergesort of -score over the per-image concatenation, images in index order and an image's
        rows in rank order (equal scores keep row order inside an image) -- built like `DeviceAPData._sorted_order`."""
        nc = self.num_classes
        rows = self.capacity * self.max_det
        bits = (self.score + 0.0).view(torch.int32).to(torch.int64)
        mono = torch.where(bits < 0, ~bits, bits | 0x80000000) & 0xffffffff
        key = ((self.cls.to(torch.int64) + 1) << 32) | (0xffffffff - mono)
        order = torch.sort(key, stable=True).indices
        seg = torch.zeros(nc + 1, dtype=torch.int64, device=self.device)
        seg[1:] = torch.cumsum(self.class_rows, 0, dtype=torch.int64)
        seg += rows - seg[nc:]
        return rows, order, seg

    def accumulate(self):
        """{'bbox': (precision [T, R, K, A, M], recall [T, K, A, M]), 'segm': ...} as float64 numpy, -1 where cocoapi leaves -1."""
        p = self.params
        t, r, k, a, m = len(p.iouThrs), len(p.recThrs), self.num_classes, hip.COCO_AREAS, len(p.maxDets)
        with torch.cuda.device(self.device):
            self._join_writers()
            rows, order, seg = self._sorted_order()
            np_, nr = 2 * t * r * k * a * m, 2 * t * k * a * m
            out = torch.full((np_ + nr,), -1.0, dtype=torch.float64, device=self.device)
            nb = hip.lib().ym_coco_accumulate_workspace_bytes(rows)
            ws = torch.empty(nb, dtype=torch.uint8, device=self.device)
            kinds = sum(1 << KINDS.index(kd) for kd in self.kinds)
            hip.check(hip.lib().ym_coco_accumulate(
                hip.ptr(self.flags, torch.int32), hip.ptr(self.rank, torch.int32), hip.ptr(order, torch.int64), rows,
                hip.ptr(seg, torch.int64), hip.ptr(self.npig, torch.int64), hip.ptr(self.rec_thr, torch.float64), r,
                hip.ptr(self.max_dets, torch.int32), m, t, k, p.eps, kinds, ctypes.c_void_p(out.data_ptr()),
                ctypes.c_void_p(out.data_ptr() + np_ * 8), ctypes.c_void_p(ws.data_ptr()), nb, hip.stream_ptr()), 'ym_coco_accumulate')
            host = out.cpu().numpy()
        precision, recall = host[:np_].reshape(2, t, r, k, a, m), host[np_:].reshape(2, t, k, a, m)
        return {kd: (precision[KINDS.index(kd)], recall[KINDS.index(kd)]) for kd in self.kinds}

    def summarize(self, grids=None):
        """{'bbox': (stats [12], text), 'segm': ...} (`summarize_grids` on `accumulate()`'s grids)."""
        grids = self.accumulate() if grids is None else grids
        return {kd: summarize_grids(grids[kd][0], grids[kd][1], self.params) for kd in self.kinds}

    def log(self):
        """The log on the host (tests, debugging): (cls int32 [rows], rank int32 [rows], flags uint32 [rows, 8], npig int64 [4, K])."""
        with torch.cuda.device(self.device):
            self._join_writers()
            cls, rank, flags, npig = (x.cpu().numpy() for x in (self.cls, self.rank, self.flags, self.npig))
        return cls, rank, flags.view(np.uint32), npig


# ---- eval.py:90-104 from the dumped files --------------------------------------------------------------------------------------
def score_results(ann_file, bbox_json=None, mask_json=None, device='cuda', label_map=None):
    """`COCOeval(COCO(ann_file), gt.loadRes(file), kind)` + evaluate / accumulate / summarize for the given detection dumps
    (`MakeJson.dump`'s files; each can be scored alone): {'bbox' / 'segm': {'stats', 'text', 'precision', 'recall'}}.  Every image
    of the annotation file is evaluated, in ascending image id.  `label_map`: category id -> 1-based class (default: the
    annotation file's categories in ascending id, cocoapi's `catIds`).  A detection whose `image_id` is not in the annotation
    file is an error, like `loadRes`; scores are taken as float32 (what `MakeJson` wrote)."""
    from .coco import COCO, anns_to_masks
    coco = COCO(ann_file, device=device)
    if label_map is None:
        label_map = {cid: k + 1 for k, cid in enumerate(sorted(coco.cats))}
    num_classes = max(label_map.values())
    img_ids = sorted(coco.imgs)
    out = {}
    for kind, path in (('bbox', bbox_json), ('segm', mask_json)):
        if path is None:
            continue
        with open(path) as f:
            dets = json.load(f)
        per_img = {}
        for d in dets:
            if d['image_id'] not in coco.imgs:
                raise AssertionError('Results do not correspond to current coco set')
            if d['category_id'] not in label_map:
                raise RuntimeError(f"score_results: category {d['category_id']} of {path} is not in the label map")
            per_img.setdefault(d['image_id'], []).append(d)
        most = max([len(v) for v in per_img.values()] + [1])
        if most > hip.EVAL_MAX_DET:
            raise RuntimeError(f'score_results: {most} detections in one image, at most {hip.EVAL_MAX_DET}')
        ev = DeviceCOCOeval(num_classes, device, max_det=most, kinds=(kind,), capacity_images=max(1, len(img_ids)))
        dev = ev.device
        for index, img_id in enumerate(img_ids):
            gt = coco_gt(coco, img_id, label_map, dev, masks=kind == 'segm')
            mine = per_img.get(img_id, [])
            if not mine:
                ev._add(None, None, None, None, None, None, gt, index)
                continue
            ids = torch.tensor([label_map[d['category_id']] - 1 for d in mine], dtype=torch.int64).to(dev)
            scores = torch.tensor([d['score'] for d in mine], dtype=torch.float64).to(torch.float32).to(dev)
            xywh = masks = None
            if kind == 'bbox':
                xywh = torch.tensor([d['bbox'] for d in mine], dtype=torch.float64).reshape(-1, 4).to(dev)
            else:
                masks = PackedMasks.pack(anns_to_masks([d['segmentation'] for d in mine], gt.height, gt.width, dev))
            ev._add(ids, scores, None, None, xywh, masks, gt, index)
        grids = ev.accumulate()
        stats, text = ev.summarize(grids)[kind]
        out[kind] = {'stats': stats, 'text': text, 'precision': grids[kind][0], 'recall': grids[kind][1]}
    return out
