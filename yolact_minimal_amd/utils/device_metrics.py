"""Device-resident mAP accumulator: `prep_metrics` without a host read and `calc_map` from one AP kernel.

Reference: `utils/common_utils.py:107-262` (`APDataObject`, `prep_metrics`, `calc_map`) as `eval.py:35-69,106` drives them.  The host
path (`common_utils.prep_metrics`) downloads the class ids and scores of every image, uploads the class lists, reads the match
flags back and extends 2 x T x classes python lists, so every image is a synchronisation point and evaluation cannot run with
several requests in flight.  `DeviceAPData` keeps what those lists hold in a device LOG instead (`include/yolact_hip.h`,
"device-resident mAP accumulator"): one row per (image slot, detection row) with the score, the class (-1 = no data point) and the
2T match flags, plus the ground-truth instances per class.  `add` is `ym_mask_iou(_packed)` + `ym_box_iou` + `ym_eval_match_log`
on the caller's stream (`add_batch`: the images of one mixed-size request in one `ym_eval_add_ragged_packed` call, packed masks
only, same log); `calc_map` is one stable device sort, `ym_eval_ap` and ONE download of the AP grid.  `to_ap_data()` rebuilds
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

    def add_batch(self, ids, scores, boxes_px, masks, counts, gts, gt_masks, sizes, image_indices, mask_table=None):
        """One request of B <= 32 images of different sizes in ONE call (`ym_eval_add_ragged_packed`: at most three launches, plus one
        `torch.cat` of the gt rows and one `ym_pack_masks_ragged` launch when gt masks arrive dense); the log and the counters end
        up exactly as after `add` on each image.  Runs on the current stream; no host read.
          ids / scores `[B, max_det]`, boxes_px `[B, max_det, 4]`, counts int32 `[B]`: `after_nms_batch(..., sync=False)` rows, with
          `max_det` the accumulator's;
          masks: the list of B `PackedMasks` views that `after_nms_batch(dets, hs, ws, ..., packed=True)` returns -- or, with
          `mask_table` (their `hip.ragged_table`), view 0 alone: the two forms `draw_batch` and its launch take.  Dense masks raise;
          gts: B tensors `[g_b, 5]` (normalised boxes, class).  Unlike `add`, this call does NOT scale them in place: the kernel
          scales the boxes as it reads them, to the same fp32 values;
          gt_masks: B dense `[g_b, h_b, w_b]` tensors (float32 / uint8 / bool) or `PackedMasks`;
          sizes: B `(h_b, w_b)`; image_indices: B image slots, `None` = the entry is padding (its gts and gt_masks are not looked at).
        A refused call (bad arguments, more than 512 gt instances in an image) leaves the accumulator as it was."""
        from .draw import _ragged_mask_table
        what = 'DeviceAPData.add_batch'
        sizes = [(int(h), int(w)) for h, w in sizes]
        batch, md = len(sizes), self.max_det
        if not 1 <= batch <= hip.RAGGED_MAX_IMAGES:
            raise RuntimeError(f'{what}: 1 .. {hip.RAGGED_MAX_IMAGES} images per call, got {batch}')
        if tuple(ids.shape) != (batch, md) or tuple(scores.shape) != (batch, md) or tuple(boxes_px.shape) != (batch, md, 4) or \
                counts is None or counts.numel() != batch:
            raise RuntimeError(f'{what}: ids / scores [{batch}, {md}], boxes_px [{batch}, {md}, 4] and {batch} counts expected (max_det is the '
                               f"accumulator's), got {tuple(ids.shape)} / {tuple(scores.shape)} / {tuple(boxes_px.shape)}")
        if len(gts) != batch or len(gt_masks) != batch or len(image_indices) != batch:
            raise RuntimeError(f'{what}: {batch} sizes but {len(gts)} gts / {len(gt_masks)} gt_masks / {len(image_indices)} image indices')
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
        if not live:
            return []
        gt_rows, gt_first = [], [0]
        for b in range(batch):
            g = 0
            if index[b] >= 0:
                gt = gts[b]
                if gt.dim() != 2 or (gt.shape[0] and gt.shape[1] != 5):
                    raise RuntimeError(f'{what}: image {b}: gt [g, 5] expected, got {tuple(gt.shape)}')
                g = int(gt.shape[0])
                if len(gt_masks[b]) != g:
                    raise RuntimeError(f'{what}: image {b}: {g} gt instances but {len(gt_masks[b])} gt masks')
                if g:
                    gt_rows.append(gt if gt.dtype == torch.float32 else gt.float())
            gt_first.append(gt_first[-1] + g)
        L = hip.lib()
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            first_c = (ctypes.c_int32 * (batch + 1))(*gt_first)
            index_c = (ctypes.c_int64 * batch)(*index)
            nbytes = L.ym_eval_add_ragged_workspace_bytes(mask_table, first_c, batch, md)
            if nbytes == 0:
                raise RuntimeError(f'{what}: ym_eval_add_ragged_workspace_bytes refuses these sizes (at most 512 gt instances per image and '
                                   f'h * ceil(w / 64) < 2^18 words per mask): {sizes}, gt rows {gt_first}')
            gt_all = (gt_rows[0].contiguous() if len(gt_rows) == 1 else torch.cat(gt_rows, 0)) if gt_rows else None
            gt_bits, gt_table, held = self._gt_blocks(gt_masks, sizes, gt_first, what)   # (`held`: alive until the launch is enqueued)
            from .output_utils import _scratch
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
            hip.check(L.ym_eval_add_ragged_packed(
                hip.ptr(ids, torch.int64), hip.ptr(scores), hip.ptr(boxes_px, torch.int32), hip.ptr(counts, torch.int32), batch, md,
                hip.ptr(masks.bits, torch.int64), mask_table, hip.ptr(gt_all), first_c,
                ctypes.c_void_p(gt_bits) if gt_bits else None, gt_table, index_c, hip.ptr(self.thr, torch.float64), len(self.iou_thres),
                self.num_classes, hip.ptr(self.score), hip.ptr(self.cls, torch.int32), hip.ptr(self.flags, torch.int32),
                self.capacity * md, hip.ptr(self.gt_count, torch.int64), hip.ptr(self.class_rows, torch.int32),
                ctypes.c_void_p(ws.data_ptr()), ws.numel(), hip.stream_ptr()), 'ym_eval_add_ragged_packed')
            del held
            self._seen.update(live)
            self._writers[cur.cuda_stream] = cur
        return live

    def _gt_blocks(self, gt_masks, sizes, gt_first, what):
        """The gt masks of a request as `ym_eval_add_ragged_packed` takes them -> (address of `gt_bits`, the `gt_blocks` table, the
        tensors behind the two).  A
        `PackedMasks` stays where it is (copied only if it starts at no multiple of 256 bytes); the dense tensors are packed into one
        new allocation by ONE `ym_pack_masks_ragged` launch.  The table's offsets count from the lowest block."""
        batch = len(sizes)
        g = [gt_first[b + 1] - gt_first[b] for b in range(batch)]
        keep = []
        at = [0] * batch
        dense = [b for b in range(batch) if g[b] and not isinstance(gt_masks[b], PackedMasks)]
        for b in range(batch):
            if not g[b] or b in dense:
                continue
            pm, (h, w) = gt_masks[b], sizes[b]
            if (pm.height, pm.width) != (h, w) or pm.bits.dim() != 3 or pm.bits.device != self.device:
                raise RuntimeError(f'{what}: image {b}: packed gt masks {pm.shape} on {pm.device} for a {h} x {w} image on {self.device}')
            bits = pm.bits.contiguous()
            if bits.data_ptr() % hip.RAGGED_ALIGN_BYTES:
                bits = bits.clone()
            keep.append(bits)
            at[b] = bits.data_ptr()
        if dense:
            src = []
            for b in dense:
                m, (h, w) = gt_masks[b], sizes[b]
                if not torch.is_tensor(m) or not m.is_cuda or m.device != self.device or tuple(m.shape) != (g[b], h, w):
                    raise RuntimeError(f'{what}: image {b}: gt masks [{g[b]}, {h}, {w}] on {self.device} expected, got '
                                       f'{tuple(m.shape) if torch.is_tensor(m) else type(m).__name__}')
                if m.dtype == torch.bool:
                    m = m.contiguous().view(torch.uint8)
                src.append(m)
            u8 = all(m.dtype == torch.uint8 for m in src)
            src = [m.contiguous() if m.dtype == (torch.uint8 if u8 else torch.float32) else m.float().contiguous() for m in src]
            rows = iter([g[b] for b in dense])                 # (aligned_layout asks for the extents in image order)
            offsets, total = hip.aligned_layout(what, [sizes[b] for b in dense], 8, lambda h, w: next(rows) * h * ((w + 63) // 64))
            packed = torch.empty(max(total, 1), dtype=torch.int64, device=self.device)
            hip.check(hip.lib().ym_pack_masks_ragged(
                (ctypes.c_void_p * len(dense))(*[m.data_ptr() for m in src]), int(u8), (ctypes.c_int32 * len(dense))(*[g[b] for b in dense]),
                hip.ragged_table([sizes[b] for b in dense], offsets), len(dense), hip.ptr(packed, torch.int64), hip.stream_ptr()),
                'ym_pack_masks_ragged')
            keep.append(packed)
            for b, o in zip(dense, offsets):
                at[b] = packed.data_ptr() + 8 * o
        used = [a for a in at if a]
        base = min(used) if used else 0
        # (an image without ground truth owns an empty block: it may lie anywhere, so it lies at the base)
        return base, hip.ragged_table(sizes, [(a - base) // 8 if a else 0 for a in at]), keep

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
