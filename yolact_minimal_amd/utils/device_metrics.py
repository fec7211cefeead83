"""Device-resident mAP accumulator: `prep_metrics` without a host read and `calc_map` from one AP kernel.

Reference: `utils/common_utils.py:107-262` (`APDataObject`, `prep_metrics`, `calc_map`) as `eval.py:35-69,106` drives them.  The host
path (`common_utils.prep_metrics`) downloads the class ids and scores of every image, uploads the class lists, reads the match
flags back and extends 2 x T x classes python lists, so every image is a synchronisation point and evaluation cannot run with
several requests in flight.  `DeviceAPData` keeps what those lists hold in a device LOG instead (`include/yolact_hip.h`,
"device-resident mAP accumulator"): one row per (image slot, detection row) with the score, the class (-1 = no data point) and the
2T match flags, plus the ground-truth instances per class.  `add` is `ym_mask_iou(_packed)` + `ym_box_iou` + `ym_eval_match_log`
on the caller's stream; `calc_map` is one stable device sort, `ym_eval_ap` and ONE download of the AP grid.  `to_ap_data()` rebuilds
the host accumulator from the log (the bridge to everything that takes `ap_data`).

Not covered: merging accumulators across ranks, more than 512 gt instances per image, NaN scores as data points (a NaN below the
count would be ordered by its bit pattern, not like python's sort).  The `--coco_api` branch's scores (the COCO protocol: crowds, area
ranges, maxDets, average recall) are `utils/coco_eval.py`'s `DeviceCOCOeval`.
"""
import ctypes

import numpy as np
import torch

from .. import hip
from .box_utils import box_iou, mask_iou
from .packed_masks import PackedMasks


class DeviceAPData:
    """`DeviceAPData(num_classes, iou_thres, device, max_det=100, capacity_images=256)`: see the module text.  The log grows by
    doubling (whole image slots, one device copy); image slots may be filled in any order and from several streams."""

    def __init__(self, num_classes, iou_thres, device, max_det=100, capacity_images=256):
        self.num_classes, self.iou_thres, self.device = int(num_classes), [float(t) for t in iou_thres], torch.device(device)
        self.max_det = int(max_det)
        if not 0 < len(self.iou_thres) <= hip.EVAL_MAX_THRESHOLDS:
            raise RuntimeError(f'DeviceAPData: 1 .. {hip.EVAL_MAX_THRESHOLDS} IoU thresholds (2T flag bits per log row), got {len(self.iou_thres)}')
        if not 0 < self.max_det <= hip.EVAL_MAX_DET or self.num_classes <= 0:
            raise RuntimeError(f'DeviceAPData: need 0 < max_det <= {hip.EVAL_MAX_DET} and num_classes > 0')
        if self.device.type != 'cuda':
            raise RuntimeError('yolact_minimal_amd has no CPU path: DeviceAPData needs a CUDA/HIP device')
        # (the one pageable upload of the accumulator's life: `add` never copies from the host)
        self.thr = torch.tensor(self.iou_thres, dtype=torch.float64).to(self.device)
        self.gt_count = torch.zeros(self.num_classes, dtype=torch.int64, device=self.device)
        self.class_rows = torch.zeros(self.num_classes, dtype=torch.int32, device=self.device)
        self.capacity = 0
        self.score = self.cls = self.flags = None
        self._seen = set()
        self._writers = {}                      # stream id -> torch stream that has written to the current log
        self._grown = None                      # event behind the last growth copy; streams wait for it once (`_synced`)
        self._synced = set()
        with torch.cuda.device(self.device):
            self._grow(max(1, int(capacity_images)))

    # ---- log storage ------------------------------------------------------------------------------------------------------
    def _grow(self, capacity):
        cur = torch.cuda.current_stream(self.device)
        rows = capacity * self.max_det
        score = torch.zeros(rows, dtype=torch.float32, device=self.device)
        cls = torch.full((rows,), -1, dtype=torch.int32, device=self.device)
        flags = torch.zeros(rows, dtype=torch.int32, device=self.device)
        if self.capacity:
            old = self.capacity * self.max_det
            for st in self._writers.values():                   # every row written so far is copied: the copy runs behind the writers
                if st != cur:
                    cur.wait_stream(st)
            for new, prev in ((score, self.score), (cls, self.cls), (flags, self.flags)):
                new[:old].copy_(prev)
                prev.record_stream(cur)                         # (freed below; allocated on another stream, read by this copy)
        # streams other than this one write to the new log behind its fill / copy: they wait for this event once
        self._grown = torch.cuda.Event()
        self._grown.record(cur)
        self._writers = {}
        self._synced = {cur.cuda_stream}
        self.score, self.cls, self.flags, self.capacity = score, cls, flags, capacity

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

    # ---- prep_metrics ------------------------------------------------------------------------------------------------------
    def add(self, ids, scores, boxes_px, masks, counts, gt, gt_masks, height, width, image_index=None):
        """One image: padded device detections (`after_nms_batch(sync=False)` rows, or `after_nms`' with `counts=None`) against its
        ground truth, as `prep_metrics` takes it (`gt` boxes are scaled to pixels IN PLACE).  Runs on the current stream; no host read."""
        index = len(self._seen) if image_index is None else int(image_index)
        if index < 0 or index in self._seen:
            raise RuntimeError(f'DeviceAPData.add: image index {index} was added before' if index >= 0 else
                               f'DeviceAPData.add: image index {index} < 0')
        if ids.dim() == 2 and ids.shape[0] == 1:                # a leading batch dimension of 1
            ids, scores, boxes_px, masks = ids[0], scores[0], boxes_px[0], masks[0]
        n = int(ids.shape[0])
        if not 0 < n <= self.max_det:
            raise RuntimeError(f'DeviceAPData.add: 1 .. max_det = {self.max_det} detection rows expected, got {n}')
        if scores.numel() != n or boxes_px.shape[0] != n or (counts is not None and counts.numel() < 1):
            raise RuntimeError(f'DeviceAPData.add: {n} ids but {scores.numel()} scores / {boxes_px.shape[0]} boxes (or an empty count tensor)')
        if gt.dim() != 2 or (gt.shape[0] and gt.shape[1] != 5):
            raise RuntimeError(f'DeviceAPData.add: gt [g, 5] expected, got {tuple(gt.shape)}')
        g = int(gt.shape[0])
        if g and (len(masks) != n or len(gt_masks) != g):
            raise RuntimeError(f'DeviceAPData.add: {n} detection rows and {g} gt instances but {len(masks)} / {len(gt_masks)} masks')
        # (the argument checks are above this line, and the index is consumed only behind the launch that writes its rows: a call
        # that raises -- here, or in `ym_eval_match_log` for more gt instances than it takes -- leaves the accumulator as it was)
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            if index >= self.capacity:
                cap = self.capacity
                while cap <= index:
                    cap *= 2
                self._grow(cap)
            elif self._grown is not None and cur.cuda_stream not in self._synced:
                cur.wait_event(self._grown)                     # this stream writes to the new log: behind the copy that filled it
                self._synced.add(cur.cuda_stream)
            gt_boxes = gt[:, :4]
            gt_boxes[:, 0::2] *= width
            gt_boxes[:, 1::2] *= height
            iou_box = iou_mask = None
            if g:
                if not isinstance(gt_masks, PackedMasks):
                    gt_masks = gt_masks.reshape(-1, height * width)
                if not isinstance(masks, PackedMasks):
                    masks = masks.reshape(-1, height * width)
                iou_mask = mask_iou(masks, gt_masks, to_cpu=False)
                iou_box = box_iou(boxes_px.float(), gt_boxes.float())
            gt_c = gt if gt.dtype == torch.float32 and gt.is_contiguous() else gt.float().contiguous()
            hip.check(hip.lib().ym_eval_match_log(
                hip.ptr(ids.contiguous(), torch.int64), hip.ptr(scores.contiguous()),
                hip.ptr(counts, torch.int32) if counts is not None else None, n, hip.ptr(iou_box), hip.ptr(iou_mask),
                hip.ptr(gt_c) if g else None, g, hip.ptr(self.thr, torch.float64), len(self.iou_thres), self.num_classes,
                hip.ptr(self.score), hip.ptr(self.cls, torch.int32), hip.ptr(self.flags, torch.int32), index * self.max_det,
                hip.ptr(self.gt_count, torch.int64), hip.ptr(self.class_rows, torch.int32), hip.stream_ptr()), 'ym_eval_match_log')
            self._seen.add(index)
            self._writers[cur.cuda_stream] = cur
        return index

    # ---- calc_map ----------------------------------------------------------------------------------------------------------
    def _sorted_order(self):
        """(rows, order int64 [rows], seg int64 [classes + 1]) on the device: what `ym_eval_ap` takes.  The log positions in (class
        ascending, score descending, log position ascending) order and the classes' segment offsets into it."""
        nc = self.num_classes
        rows = self.capacity * self.max_det
        # ONE stable sort of a 64-bit key: class + 1 in the high word (-1 = no data point sorts first), the score's
        # descending order in the low word (fp32 bits made monotone and inverted; -0.0 is folded into 0.0 first, python's
        # key -score ties them), equal keys stay in log position = push order
        bits = (self.score + 0.0).view(torch.int32).to(torch.int64)
        mono = torch.where(bits < 0, ~bits, bits | 0x80000000) & 0xffffffff
        key = ((self.cls.to(torch.int64) + 1) << 32) | (0xffffffff - mono)
        order = torch.sort(key, stable=True).indices
        seg = torch.zeros(nc + 1, dtype=torch.int64, device=self.device)
        seg[1:] = torch.cumsum(self.class_rows, 0, dtype=torch.int64)
        seg += rows - seg[nc:]                                  # the rows of class -1 come first
        return rows, order, seg

    def _launch_ap(self, rows, order, seg, out, ws):
        """`ym_eval_ap` on the current stream: AP grid and empty flags into `out` (2 T classes fp64, then classes uint8)."""
        t, nc = len(self.iou_thres), self.num_classes
        hip.check(hip.lib().ym_eval_ap(hip.ptr(self.flags, torch.int32), hip.ptr(order, torch.int64), rows, hip.ptr(seg, torch.int64),
                                       hip.ptr(self.gt_count, torch.int64), t, nc, ctypes.c_void_p(out.data_ptr()),
                                       ctypes.c_void_p(out.data_ptr() + 2 * t * nc * 8), ctypes.c_void_p(ws.data_ptr()), ws.numel(),
                                       hip.stream_ptr()), 'ym_eval_ap')

    def ap_grid(self):
        """(ap float64 [2, T, classes], empty bool [classes]) on the host: one stable sort, `ym_eval_ap`, one download."""
        t, nc = len(self.iou_thres), self.num_classes
        with torch.cuda.device(self.device):
            self._join_writers()
            rows, order, seg = self._sorted_order()
            out = torch.empty(2 * t * nc * 8 + nc, dtype=torch.uint8, device=self.device)
            nb = hip.lib().ym_eval_ap_workspace_bytes(rows)
            ws = torch.empty(nb, dtype=torch.uint8, device=self.device)
            self._launch_ap(rows, order, seg, out, ws)
            host = out.cpu().numpy()
        return host[:2 * t * nc * 8].view(np.float64).reshape(2, t, nc), host[2 * t * nc * 8:].astype(bool)

    def calc_map(self, step=None):
        """`common_utils.calc_map`'s (table text, box row, mask row) from the device APs (same python float means: `map_table`)."""
        from .common_utils import map_table
        ap, empty = self.ap_grid()
        ap, empty = ap.tolist(), empty.tolist()
        return map_table(lambda kind, k, c: None if empty[c] else ap[kind == 'mask'][k][c], self.iou_thres, self.num_classes, step)

    # ---- the host accumulator the log stands for ---------------------------------------------------------------------------
    def to_ap_data(self):
        """{'box': [[APDataObject ...]], 'mask': ...} as the host `prep_metrics` would have built it: the (float(score), bool) points
        in push order (image index, then detection row) and the same `num_gt_positives`."""
        from .common_utils import APDataObject
        t, nc = len(self.iou_thres), self.num_classes
        with torch.cuda.device(self.device):
            self._join_writers()
            score, cls, flags, gt_count = (x.cpu().numpy() for x in (self.score, self.cls, self.flags, self.gt_count))
        ap_data = {kind: [[APDataObject() for _ in range(nc)] for _ in range(t)] for kind in ('box', 'mask')}
        rows = np.nonzero(cls >= 0)[0]
        for c in range(nc):
            mine = rows[cls[rows] == c]
            sc = [float(s) for s in score[mine]]
            fl = flags[mine].view(np.uint32)
            for type_idx, kind in enumerate(('box', 'mask')):
                for k in range(t):
                    cell = ap_data[kind][k][c]
                    cell.num_gt_positives = int(gt_count[c])
                    cell.data_points = list(zip(sc, (((fl >> (type_idx * t + k)) & 1) != 0).tolist()))
        return ap_data
