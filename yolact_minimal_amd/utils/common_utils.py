"""Evaluation step right after `after_nms`: `prep_metrics` with its IoU caches and greedy matching on
the device.  Reference: `/root/reference/utils/common_utils.py:107-262` (`APDataObject`, `prep_metrics`, `calc_map`), called
from `eval.py:69,106`.

The reference computes `mask_iou` / `box_iou` on the device, copies both [n, g] matrices to the host and walks a triple python
loop (class x threshold x iou type) with a `.item()` per candidate pair.  Here: `ym_mask_iou` (bit-row popcounts, each mask read
once), `ym_box_iou`, then `ym_match_detections` resolves all 2 x T matchings in one launch; the host reads back ONE uint8
tensor [2, T, n] and only does the AP bookkeeping (lists of (score, is_true)), which stays Python like the reference.
"""
import ctypes

import numpy as np
import torch

from .. import hip
from .box_utils import box_iou, mask_iou
from .packed_masks import PackedMasks


class APDataObject:
    """Accumulator of one (IoU type, IoU threshold, class) cell of the mAP table: the (score, hit?) pairs of every prediction and
    the number of ground-truth instances.  Same public surface as the reference's bookkeeping class (`utils/common_utils.py:107-171`:
    `push`, `add_gt_positives`, `is_empty`, `get_ap`, `data_points`, `num_gt_positives`); `get_ap` is evaluated on arrays and returns
    the reference's value bit for bit (pinned by tests/golden/metrics.npz: the divisions are the same IEEE operations and the
    101 samples are added in the same order)."""
    RECALL_GRID = np.arange(101) / 100                      # COCO's 101 recall thresholds 0.00 ... 1.00

    def __init__(self):
        self.data_points = []                               # [(score, is_true_positive)]
        self.num_gt_positives = 0

    def push(self, score, is_true):
        self.data_points.append((score, is_true))

    def add_gt_positives(self, num_positives):
        self.num_gt_positives += num_positives

    def is_empty(self):
        return not self.data_points and self.num_gt_positives == 0

    def get_ap(self):
        """Area under the monotone precision envelope sampled at the 101 recall thresholds (a threshold beyond the reached recall
        contributes 0)."""
        if self.num_gt_positives == 0:
            return 0
        self.data_points.sort(key=lambda p: -p[0])          # (kept in place and stable, like the reference: callers look at it)
        n = len(self.data_points)
        if n == 0:
            return 0.0
        hits = np.fromiter((bool(p[1]) for p in self.data_points), dtype=np.int64, count=n)
        tp = np.cumsum(hits)
        precision = tp / np.arange(1, n + 1)                # tp / (tp + fp) after each prediction
        recall = tp / self.num_gt_positives
        envelope = np.maximum.accumulate(precision[::-1])[::-1]
        first = np.searchsorted(recall, self.RECALL_GRID, side='left')      # first prediction that reaches each threshold
        samples = np.where(first < n, envelope[np.minimum(first, n - 1)], 0.0)
        return sum(samples.tolist()) / 101                  # left-to-right sum of python floats: the reference's rounding


_thr_cache = {}


def match_detections(iou_box, iou_mask, ids_p, gt_classes, iou_thres, num_classes):
    """[2, T, n] uint8 on the host: does prediction i find an unused same-class gt above threshold t (box / mask IoU)?"""
    dev = iou_box.device
    n, g, t = iou_box.shape[0], iou_box.shape[1], len(iou_thres)
    both = torch.tensor(list(ids_p) + list(gt_classes), dtype=torch.int32).to(dev)        # one H2D copy for the two class lists
    pred, gtc = both[:n], both[n:]
    key = (dev, tuple(iou_thres))
    thr = _thr_cache.get(key)
    if thr is None:
        if len(_thr_cache) > 16:
            _thr_cache.clear()
        thr = _thr_cache[key] = torch.tensor(iou_thres, dtype=torch.float64).to(dev)
    matched = torch.empty(2, t, n, dtype=torch.uint8, device=dev)       # (every prediction belongs to one class < num_classes: all written)
    hip.check(hip.lib().ym_match_detections(hip.ptr(iou_box), hip.ptr(iou_mask), hip.ptr(pred, torch.int32),
                                            hip.ptr(gtc, torch.int32), n, g, hip.ptr(thr, torch.float64), t, num_classes,
                                            ctypes.c_void_p(matched.data_ptr()), hip.stream_ptr()), 'ym_match_detections')
    return matched.cpu().numpy()


def prep_metrics(ap_data, ids_p, classes_p, boxes_p, masks_p, gt, gt_masks, height, width, iou_thres):
    """Same arguments, mutations and `ap_data` updates as the reference (common_utils.py:174-216): `gt` boxes are scaled to
    pixels IN PLACE; classes are visited as `set(ids_p + gt_classes)`; per class / threshold / iou type the gt positives are
    added and one (score, is_true) is pushed per prediction of that class, in prediction order."""
    gt_boxes = gt[:, :4]
    gt_boxes[:, 0::2] *= width                 # (columns 0, 2 / 1, 3 as strided views: no index tensors, one launch each)
    gt_boxes[:, 1::2] *= height
    gt_classes = gt[:, 4].int().tolist()
    if not isinstance(gt_masks, PackedMasks):               # (a PackedMasks on either side: mask_iou packs the other one)
        gt_masks = gt_masks.reshape(-1, height * width)
    if not isinstance(masks_p, PackedMasks):
        masks_p = masks_p.reshape(-1, height * width)
    ids_p = [int(i) for i in ids_p]

    iou_mask = mask_iou(masks_p, gt_masks, to_cpu=False)
    iou_box = box_iou(boxes_p.float(), gt_boxes.float())
    num_classes = max(ids_p + gt_classes) + 1
    matched = match_detections(iou_box, iou_mask, ids_p, gt_classes, iou_thres, num_classes)

    # host bookkeeping (a third of the loop's metric stage at 100 detections: 2 x 10 x classes cells per image): the flags become
    # nested python lists ONCE, predictions are grouped by class once; per cell only the reference's two updates remain
    flags = matched.astype(bool).tolist()                    # [iou type][threshold][prediction]
    by_class = {}
    for i, pred_class in enumerate(ids_p):
        by_class.setdefault(pred_class, []).append(i)        # prediction order is kept
    for _class in set(ids_p + gt_classes):
        num_gt_per_class = gt_classes.count(_class)
        mine = by_class.get(_class, ())
        scores = [classes_p[i] for i in mine]
        for iou_idx in range(len(iou_thres)):
            for type_idx, iou_type in enumerate(('box', 'mask')):
                ap_obj = ap_data[iou_type][iou_idx][_class]
                ap_obj.add_gt_positives(num_gt_per_class)
                if mine:
                    row = flags[type_idx][iou_idx]
                    ap_obj.data_points.extend(zip(scores, [row[i] for i in mine]))


def map_table(cell_ap, iou_thres, num_classes, step):
    """The arithmetic and the text of `calc_map` over `cell_ap(kind, t, c)` -> the AP of that cell, or None when the cell is empty:
    shared by the host accumulator below and `device_metrics.DeviceAPData.calc_map` (whose APs come from `ym_eval_ap`)."""
    def mean_ap(kind, t):
        vals = [v for v in (cell_ap(kind, t, c) for c in range(num_classes)) if v is not None]
        return sum(vals) / len(vals) * 100 if vals else 0

    rows = [[f'{step // 1000}k' if step else '', 'all'] + [int(t * 100) for t in iou_thres]]
    for kind in ('box', 'mask'):
        per_thr = [mean_ap(kind, t) for t in range(len(iou_thres))]
        rows.append([kind] + [round(v, 2) for v in [sum(per_thr) / len(per_thr)] + per_thr])
    return '\n'.join(' | '.join(str(c) for c in row) for row in rows), rows[1], rows[2]


def calc_map(ap_data, iou_thres, num_classes, step):
    """mAP table of the reference's `calc_map` (common_utils.py:219-255) from the AP grid [iou type][threshold][class]: per
    (type, threshold) the mean AP (x 100) over the classes that hold data, then the mean over the thresholds as 'all'.  Python float
    sums in class / threshold order, so the rounded rows equal the reference's (tests/golden/metrics_*.npz).  Returns
    (table text, box row, mask row); the table is plain ' | '-joined rows (terminaltables is a formatting dependency)."""
    def cell_ap(kind, t, c):
        cell = ap_data[kind][t][c]
        return None if cell.is_empty() else cell.get_ap()

    return map_table(cell_ap, iou_thres, num_classes, step)


def rle_encode(masks, cap_runs=4096):
    """COCO RLE of binary masks [n, h, w] on the device (`ym_rle_encode`) -> list of {'size': [h, w], 'counts': str}, i.e.
    `pycocotools.mask.encode(np.asfortranarray(m.astype(np.uint8)))` with `counts` decoded to ascii (common_utils.py:90-91).
    Only the compressed strings (a few hundred bytes per mask) cross PCIe."""
    if not masks.is_cuda:
        raise RuntimeError('yolact_minimal_amd has no CPU path: rle_encode needs CUDA/HIP tensors')
    if isinstance(masks, PackedMasks):                      # the same strings from 1/32 of the bytes (`ym_rle_encode_packed`)
        n, h, w = masks.shape
        m = masks.bits.contiguous()
        encode, src = hip.lib().ym_rle_encode_packed, hip.ptr(m, torch.int64)
    else:
        m = masks.to(torch.float32).contiguous()
        n, h, w = m.shape
        encode, src = hip.lib().ym_rle_encode, hip.ptr(m)
    dev = m.device
    while True:
        cap_str = cap_runs * 4
        counts = torch.empty(n, cap_runs, dtype=torch.int32, device=dev)
        ws = torch.empty(n, cap_runs, dtype=torch.int32, device=dev)
        meta = torch.empty(2, n, dtype=torch.int32, device=dev)
        out = torch.empty(n, cap_str, dtype=torch.uint8, device=dev)
        hip.check(encode(src, n, h, w, ctypes.c_void_p(counts.data_ptr()), cap_runs,
                         ctypes.c_void_p(meta[0].data_ptr()), ctypes.c_void_p(out.data_ptr()), cap_str,
                         ctypes.c_void_p(meta[1].data_ptr()), ctypes.c_void_p(ws.data_ptr()), ws.numel() * 4,
                         hip.stream_ptr()), 'ym_rle_encode')
        nruns, slen = meta.cpu().tolist()
        if min(slen) >= 0:
            break
        cap_runs = max(cap_runs * 2, max(nruns) + 1)            # a mask was busier than the buffers: grow and redo
    longest = max(slen)
    host = out[:, :max(longest, 1)].cpu().numpy()
    return [{'size': [h, w], 'counts': host[i, :slen[i]].tobytes().decode('ascii')} for i in range(n)]


class MakeJson:
    """Detection dumps for the COCO API (reference common_utils.py:66-104, eval.py:59-67).  `add_mask` accepts the dense
    [h, w] mask like the reference (host or device), one mask of a `PackedMasks`, or an RLE dict from `rle_encode` (batch the
    image's masks there)."""

    def __init__(self, coco_label_map=None):
        from ..config import COCO_LABEL_MAP
        self.bbox_data, self.mask_data = [], []
        self.coco_cats = {}
        for coco_id, real_id in (COCO_LABEL_MAP if coco_label_map is None else coco_label_map).items():
            self.coco_cats[real_id - 1] = coco_id

    def _cat(self, category_id):
        return self.coco_cats[int(category_id)]

    def add_bbox(self, image_id, category_id, bbox, score):
        bbox = [bbox[0], bbox[1], bbox[2] - bbox[0], bbox[3] - bbox[1]]
        bbox = [round(float(x) * 10) / 10 for x in bbox]        # nearest 10th, as COCO suggests
        self.bbox_data.append({'image_id': int(image_id), 'category_id': self._cat(category_id), 'bbox': bbox,
                               'score': float(score)})

    def add_mask(self, image_id, category_id, segmentation, score):
        if isinstance(segmentation, PackedMasks):            # one packed [h, w] mask (or [1, h, w])
            pm = segmentation if segmentation.dim() == 3 else PackedMasks(segmentation.bits[None], segmentation.height, segmentation.width)
            segmentation = rle_encode(pm)[0]
        elif not isinstance(segmentation, dict):
            seg = torch.as_tensor(segmentation)
            if not seg.is_cuda:
                seg = seg.cuda()
            segmentation = rle_encode(seg[None])[0]
        self.mask_data.append({'image_id': int(image_id), 'category_id': self._cat(category_id),
                               'segmentation': segmentation, 'score': float(score)})

    def dump(self, bbox_path='results/bbox_detections.json', mask_path='results/mask_detections.json'):
        import json
        for data, path in ((self.bbox_data, bbox_path), (self.mask_data, mask_path)):
            with open(path, 'w') as f:
                json.dump(data, f)


class _JsonRequest:
    """One request of `BatchMakeJson`: where it stands among the records added one by one, and its numpy blocks once collected.
    While its launches may still run it is also the token that keeps the mask allocation and its transfer block alive."""
    __slots__ = ('bbox_at', 'mask_at', 'image_ids', 'sizes', 'records', 'blob', 'redone', 'event', 'block', 'masks', 'offsets',
                 'cap_runs', 'device')


class _JsonBlock:
    """The buffers of one request in flight: header + records on the device and their pinned host copy (one fixed-size D2H), the
    compact string buffer, the event behind the copy.  Taken from and given back to `BatchMakeJson`'s free list."""
    __slots__ = ('key', 'out', 'host', 'strings', 'event')


class BatchMakeJson(MakeJson):
    """`MakeJson` as a pipeline consumer: `add_batch` takes the `after_nms_batch(..., sync=False, packed=True)` rows of a request of
    B <= 32 images of different sizes (`ym_rle_encode_ragged_packed`: at most three launches) and reads nothing on the host; the
    records of a request are fetched once its event has completed (by a later `add_batch`, or by `dump`), and the per-detection
    dicts are built by `dump` alone: in request order, inside a request in (image, row) order, under eval.py:65's filter -- the files
    are byte for byte those of `rle_encode` -> `add_bbox` / `add_mask` image by image.  Records added through `add_bbox` /
    `add_mask` keep their position between the requests."""

    def __init__(self, coco_label_map=None):
        super().__init__(coco_label_map)
        self._requests = []                                 # in add order, until `finish` folds them into bbox_data / mask_data
        self._tokens = []                                   # the requests whose launches may still run
        self._free = {}                                     # (device, B, max_det, cap_runs) -> [_JsonBlock]
        self._side = {}                                     # device -> the stream the collected strings are copied on

    # ---- the request --------------------------------------------------------------------------------------------------------
    def add_batch(self, ids, scores, boxes_px, masks, counts, image_ids, mask_table=None, cap_runs=4096):
        """ids / scores `[B, max_det]`, boxes_px int32 `[B, max_det, 4]`, counts int32 `[B]`; `masks`: the list of B `PackedMasks`
        views of the ragged `after_nms_batch`, view 0 with `mask_table` (their `hip.ragged_table`), or the uniform padded
        `PackedMasks [B, max_det, H, Wq]`; dense masks raise.  `image_ids`: one per image, `None` = the entry is padding.  Runs on
        the current stream, no host read: the launches, one asynchronous D2H of header + records into a pinned block of the free
        list, an event.  A mask of more than `cap_runs` runs is encoded again by `rle_encode` when the request is collected."""
        from .draw import _ragged_mask_table
        from .output_utils import _scratch
        what = 'BatchMakeJson.add_batch'
        if not torch.is_tensor(ids) or not ids.is_cuda or ids.dim() != 2:
            raise RuntimeError(f'{what}: ids [B, max_det] as a CUDA (HIP) tensor expected; there is no CPU path')
        batch, md = ids.shape
        if tuple(scores.shape) != (batch, md) or boxes_px is None or tuple(boxes_px.shape) != (batch, md, 4) or counts is None or \
                counts.numel() != batch or len(image_ids) != batch:
            raise RuntimeError(f'{what}: ids / scores [{batch}, {md}], boxes_px [{batch}, {md}, 4], {batch} counts and {batch} image ids '
                               f'expected, got {tuple(scores.shape)} / {None if boxes_px is None else tuple(boxes_px.shape)} / '
                               f'{None if counts is None else counts.numel()} / {len(image_ids)}')
        packed_only = f'{what}: the batched stages take packed masks only (after_nms_batch(..., packed=True))'
        if mask_table is not None:
            if not isinstance(masks, PackedMasks) or len(mask_table) != batch:
                raise RuntimeError(packed_only + f'; with mask_table: view 0 and {batch} table entries')
            sizes = [(e.img_h, e.img_w) for e in mask_table]
            offsets = [e.offset for e in mask_table]
        elif isinstance(masks, (list, tuple)):
            if not len(masks) or not isinstance(masks[0], PackedMasks):
                raise RuntimeError(packed_only)
            sizes = [(m.height, m.width) for m in masks]
            masks, mask_table = _ragged_mask_table(masks, sizes, md, what)
            offsets = [e.offset for e in mask_table]
        elif isinstance(masks, PackedMasks):                    # the uniform padded form: B blocks of one size back to back
            h, w = masks.height, masks.width
            if masks.dim() != 4 or masks.shape != (batch, md, h, w) or not masks.bits.is_contiguous():
                raise RuntimeError(f'{what}: uniform masks are a contiguous PackedMasks [{batch}, {md}, H, Wq], got {masks.shape}')
            sizes = [(h, w)] * batch
            offsets = [b * md * h * masks.bits.shape[3] for b in range(batch)]
            mask_table = hip.ragged_table(sizes, offsets)
        else:
            raise RuntimeError(packed_only)
        dev = ids.device
        if masks.bits.device != dev:
            raise RuntimeError(f'{what}: masks on {masks.bits.device}, detections on {dev}')
        self._collect_done()
        L = hip.lib()
        with torch.cuda.device(dev):
            nbytes = L.ym_rle_encode_ragged_workspace_bytes(mask_table, batch, md, int(cap_runs))
            if nbytes == 0:
                raise RuntimeError(f'{what}: ym_rle_encode_ragged_workspace_bytes refuses {batch} images of {sizes} with max_det {md} and '
                                   f'cap_runs {cap_runs} (width <= 4096, h * w < 2^31, B * max_det * 4 * cap_runs < 2^31)')
            blk = self._take_block(dev, batch, md, int(cap_runs))
            ws = _scratch(dev, nbytes)
            live = (ctypes.c_uint8 * batch)(*[i is not None for i in image_ids])
            hip.check(L.ym_rle_encode_ragged_packed(
                hip.ptr(ids.contiguous(), torch.int64), hip.ptr(scores.contiguous()), hip.ptr(boxes_px.contiguous(), torch.int32),
                hip.ptr(counts.contiguous(), torch.int32), batch, md, hip.ptr(masks.bits, torch.int64), mask_table, live, int(cap_runs),
                ctypes.c_void_p(blk.out.data_ptr() + 16), ctypes.c_void_p(blk.strings.data_ptr()), blk.strings.numel(),
                ctypes.c_void_p(blk.out.data_ptr()), ctypes.c_void_p(ws.data_ptr()), ws.numel(), hip.stream_ptr()),
                'ym_rle_encode_ragged_packed')
            blk.host.copy_(blk.out, non_blocking=True)
            blk.event.record()
        req = self._new_request(image_ids, sizes)
        req.event, req.block, req.masks, req.offsets, req.cap_runs, req.device = blk.event, blk, masks, offsets, int(cap_runs), dev
        self._tokens.append(req)

    def add_records(self, records, strings, image_ids, sizes):
        """A request that is already on the host: `records` `[B, max_det]` of `hip.RLE_RECORD_DTYPE` (state 0 or 1), `strings` the
        bytes their str_off / str_len index, one image id (`None` = padding) and one (h, w) per image."""
        records = np.asarray(records, dtype=np.dtype(hip.RLE_RECORD_DTYPE))
        if records.ndim != 2 or records.shape[0] != len(image_ids) or len(sizes) != len(image_ids) or (records['state'] == 2).any():
            raise RuntimeError(f'BatchMakeJson.add_records: records [B, max_det] of state 0 / 1 with B image ids and B sizes expected, got '
                               f'{records.shape} for {len(image_ids)} ids and {len(sizes)} sizes')
        req = self._new_request(image_ids, sizes)
        req.records, req.blob = records.copy(), np.frombuffer(bytes(strings), dtype=np.uint8)

    def _new_request(self, image_ids, sizes):
        req = _JsonRequest()
        req.bbox_at, req.mask_at = len(self.bbox_data), len(self.mask_data)
        req.image_ids, req.sizes = list(image_ids), [(int(h), int(w)) for h, w in sizes]
        req.records = req.blob = req.event = req.block = req.masks = req.offsets = None
        req.redone = {}
        self._requests.append(req)
        return req

    def _take_block(self, dev, batch, md, cap_runs):
        key = (str(dev), batch, md, cap_runs)
        free = self._free.setdefault(key, [])
        if free:
            return free.pop()
        blk = _JsonBlock()
        rows = batch * md
        nbytes = 16 + rows * ctypes.sizeof(hip.RleRecord)
        blk.key = key
        blk.out = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        blk.host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        blk.strings = torch.empty(rows * cap_runs * hip.RLE_SLAB_PER_RUN, dtype=torch.uint8, device=dev)
        blk.event = torch.cuda.Event()
        return blk

    # ---- collecting ---------------------------------------------------------------------------------------------------------
    def _collect_done(self):
        """Every queued request whose event has completed; never waits for one that has not."""
        waiting = []
        for req in self._tokens:
            if req.event.query():
                self._collect(req)
            else:
                waiting.append(req)
        self._tokens = waiting

    def _collect(self, req):
        """The finished request as numpy blocks: the record array, exactly header[0] string bytes, and the strings of the rows that
        did not fit (`rle_encode` on the held mask view).  The copies run on a stream of their own: the caller's current stream
        may hold a forward pass that has only just been queued."""
        blk, dev = req.block, req.device
        host = blk.host.numpy()
        total = int(host[:16].view('<i4')[0])
        batch = len(req.image_ids)
        req.records = host[16:].view(np.dtype(hip.RLE_RECORD_DTYPE)).reshape(batch, -1).copy()
        side = self._side.get(str(dev))
        if side is None:
            side = self._side[str(dev)] = torch.cuda.Stream(dev)
        with torch.cuda.device(dev), torch.cuda.stream(side):
            req.blob = blk.strings[:total].cpu().numpy() if total else np.zeros(0, dtype=np.uint8)
            over = np.argwhere(req.records['state'] == 2)
            if len(over):
                req.masks.record_stream(side)                   # (allocated on the request's stream, read here)
                base = req.masks.bits
                for b, r in over.tolist():
                    h, w = req.sizes[b]
                    wq = (w + 63) // 64
                    row = base.as_strided((1, h, wq), (h * wq, wq, 1), base.storage_offset() + req.offsets[b] + r * h * wq)
                    need = int(req.records['nruns'][b, r])
                    req.redone[(b, r)] = rle_encode(PackedMasks(row, h, w), cap_runs=max(2 * req.cap_runs, need + 1))[0]['counts']
        self._free[blk.key].append(blk)
        req.event = req.block = req.masks = None

    def wait(self):
        """Wait for the requests in flight and collect them.  Returns the requests not yet folded into the lists, in order, as
        `(records [B, max_det], string bytes, image ids)` numpy blocks."""
        for req in self._tokens:
            req.event.synchronize()
            self._collect(req)
        self._tokens = []
        return [(req.records, req.blob, req.image_ids) for req in self._requests]

    def finish(self):
        """Wait for the requests in flight, collect them, and fold every request into `bbox_data` / `mask_data` at its place."""
        self.wait()
        if not self._requests:
            return
        singles = (self.bbox_data, self.mask_data)
        self.bbox_data, self.mask_data = [], []
        at = [0, 0]
        for req in self._requests:
            self.bbox_data += singles[0][at[0]:req.bbox_at]
            self.mask_data += singles[1][at[1]:req.mask_at]
            at = [req.bbox_at, req.mask_at]
            rec, blob = req.records, req.blob
            for b, r in np.argwhere(rec['state'] != 0).tolist():
                one = rec[b, r]
                if req.image_ids[b] is None:                    # (padding: the device marks none of its rows)
                    continue
                if one['state'] == 1:
                    counts = blob[one['str_off']:one['str_off'] + one['str_len']].tobytes().decode('ascii')
                else:
                    counts = req.redone[(b, r)]
                h, w = req.sizes[b]
                MakeJson.add_bbox(self, req.image_ids[b], one['class_id'], one['box'], one['score'])
                MakeJson.add_mask(self, req.image_ids[b], one['class_id'], {'size': [h, w], 'counts': counts}, one['score'])
        self.bbox_data += singles[0][at[0]:]
        self.mask_data += singles[1][at[1]:]
        self._requests = []

    def dump(self, bbox_path='results/bbox_detections.json', mask_path='results/mask_detections.json'):
        self.finish()
        super().dump(bbox_path, mask_path)


# ---- harness helpers the reference scripts import from this module (host only) -----------------------------------------
class ProgressBar:
    """`ProgressBar(length, max_val).get_bar(i)` -> a `length`-character bar (reference common_utils.py:15-38; eval.py:32,81)."""

    def __init__(self, length, max_val):
        self.length, self.max_val = int(length), max_val
        self.string = self.get_bar(0)

    def get_bar(self, new_val):
        filled = int(self.length * (min(new_val, self.max_val) / self.max_val)) if self.max_val else self.length
        self.string = '█' * filled + '░' * (self.length - filled)
        return self.string


def _replace_checkpoint(prefix, cfg_name, new_name, net):
    import glob
    import os
    old = [p for p in glob.glob(f'weights/{prefix}*') if cfg_name in p]
    assert len(old) <= 1, f'Error, multiple {prefix} weight found.'
    for p in old:
        os.remove(p)
    print(f"\nSaving the {prefix} model as '{new_name}'.\n")
    # (clones: under a Trainer / the module's own training state parameters and BatchNorm buffers are views of flat buffers, and
    #  torch.save would write each flat storage whole and share it between the entries; the reference's files hold one storage per key)
    torch.save({k: v.detach().clone() for k, v in net.state_dict().items()}, f'weights/{new_name}')


def save_best(net, mask_map, cfg_name, step):
    """Keep `weights/best_<mask mAP>_<cfg>_<step>.pth` if `mask_map` is at least the stored best (reference common_utils.py:41-53,
    train.py:174; the file-name convention is what eval.py / train.py --resume parse)."""
    import glob
    old = [p for p in glob.glob('weights/best*') if cfg_name in p]
    assert len(old) <= 1, 'Error, multiple best weight found.'
    best = float(old[0].split('/')[-1].split('_')[1]) if old else 0.
    if mask_map >= best:
        _replace_checkpoint('best', cfg_name, f'best_{mask_map}_{cfg_name}_{step}.pth', net)


def save_latest(net, cfg_name, step):
    """`weights/latest_<cfg>_<step>.pth`, replacing the previous one (reference common_utils.py:56-63, train.py:184,196)."""
    _replace_checkpoint('latest', cfg_name, f'latest_{cfg_name}_{step}.pth', net)


from .device_metrics import DeviceAPData  # noqa: E402,F401  (the device-resident accumulator; it imports map_table from here lazily)
from .coco_eval import COCOGtBatch, DeviceCOCOeval, coco_gt, coco_gt_batch, score_results  # noqa: E402,F401  (the COCO-protocol evaluator: eval.py --coco_api's second half)
