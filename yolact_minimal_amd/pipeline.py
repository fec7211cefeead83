"""Serving with several independent requests in flight on one MI355X (batch 1: 400 -> 600-617 img/s; batch 8: 700 -> 760 forward-only).

The reference evaluates one image at a time (`eval.py:36-69`: forward -> nms -> after_nms, a device synchronisation around each).
On this part a bs=1 forward is a chain of ~190 dependent launches of 0.6-1.4 GFLOP each: every launch pays a kernel boundary, an
address set-up + cold-L2 round trip and an epilogue (~9 us in round 3, ~6 us since round 4) around ~7 us of MFMA work, so ONE chain keeps the matrix pipe ~35-43 %
busy whatever the kernels do.  Requests are independent, so the way to fill the chip at batch size 1 is to have several of them in
flight: `RequestPipeline` owns `depth` complete engines (activations, split-K scratch, arrival counters, hipGraph: nothing shared
but the read-only weights) and `depth` HIP streams, and runs request i on slot i % depth.  Each request is still ONE image through
`Yolact.forward` -> `nms` -> `after_nms` with ONE host read (its detection count, which `after_nms` needs to size what it returns);
the count is copied to pinned host memory behind the request and read when the slot comes up again, so the host never waits on
the request it has just enqueued.  `cfg.traditional_nms` is served the same way (`nms_batch` picks the batched greedy entry).
With batch > 1 a request may give every image its own output size (`submit(out_hw=[(h, w), ...])`: `after_nms_batch` with per-image
sizes, one launch set, the size table in the kernel arguments, so nothing is copied or synchronised per request).
`submit_frames(FrameBatch)` is the whole request for frames of different sizes: uint8 frames in (`val_aug_batch` on the slot's
stream), and with `draw=True` drawn uint8 frames of those sizes out (the ragged `draw_batch`), no host read in between.
`RequestPipeline(net, cfg, height, width, ...)` with `height != width` serves in WINDOW mode (utils/rect.py): the network runs on the
top-left `height x width` of its square input only -- the anchors are `net.anchors_for(height, width)`, `after_nms_batch` gets
`window=True`, `submit_frames` pre-processes into the window and refuses frames whose picture does not fit it;
`RequestPipeline.for_frames` picks the window from the frame sizes.  Opt-in, not a parity path; `height == width` is untouched.

Measured mid-round 3 (res101_coco 544 px, MI355X, forward + nms + after_nms(480x640)): depth 1: 325 img/s, 2: 468, 3: 545, 4: 594, 5: 495,
8: 479; with round 4's kernels 3: 580, 4: 603-617, 5: 499, 6: 527 -- the part schedules four compute pipes; GPU_MAX_HW_QUEUES must be >= depth + 1 (ROCm multiplexes HIP streams onto 4
hardware queues by default and two streams that share a queue do not overlap): set it to 8 before the first HIP call
(`RequestPipeline` warns when the variable is missing or too small: it cannot be changed once the runtime is up).
"""
import os
import warnings

import torch

from .engine import InferEngine
from .utils.augmentations import val_aug_batch
from .utils.draw import draw_batch
from .utils.frames import FrameBatch
from .utils.output_utils import nms_batch, after_nms_batch, unpad_detections
from .utils.rect import rect_window

_streams = {}


class _Consumed:
    """What `submit(consumer=...)` leaves in a slot: the consumer's return value and the request's event."""
    __slots__ = ('value', 'event')

    def __init__(self, value, event):
        self.value, self.event = value, event


def _stream_set(device, n):
    """One process-wide set of streams per device: every pipeline overlaps on the SAME streams (= the same hardware queues)."""
    key = torch.device(device)
    lst = _streams.setdefault(key, [])
    while len(lst) < n:
        lst.append(torch.cuda.Stream(device=device))
    return lst[:n]


def hw_queues_ok(depth):
    """Does the HIP runtime have a hardware queue for each of `depth` slot streams plus the caller's stream?  (ROCm reads
    GPU_MAX_HW_QUEUES when it creates its first stream; the default is 4.)"""
    try:
        q = int(os.environ.get('GPU_MAX_HW_QUEUES', '4'))
    except ValueError:
        q = 4
    return q >= depth + 1


class RequestPipeline:
    """`depth` requests in flight.  `submit()` returns the FINISHED result of the request that used the slot before; results are
    fresh tensors the caller owns (network outputs are copied off the slot's buffers before the slot runs again).
    `return_outputs=False` (throughput measurements of the forward alone): `submit()` / `drain()` hand back nothing for
    `with_post=False` and the copy is skipped.  `timed=True`: every request is bracketed by HIP events on its slot's stream and
    `latencies_ms` collects the per-request device latency (bench.py: p50 / p99 and the Little's-law check).
    `packed_masks=True`: the fourth result is a `PackedMasks` (1 bit per pixel: 3.84 MB instead of 123 MB per request at 480x640,
    for the `depth` results in flight and for whatever the caller still owns)."""

    def __init__(self, net, cfg, height, width, device, depth=4, out_hw=(480, 640), with_post=True, batch=1, return_outputs=True,
                 timed=False, packed_masks=False):
        self.packed_masks = bool(packed_masks)          # results carry PackedMasks (utils/packed_masks.py) instead of float32 masks
        self.net, self.cfg, self.device, self.depth, self.batch = net, cfg, torch.device(device), depth, batch
        self.out_hw, self.with_post, self.return_outputs, self.timed = out_hw, with_post, return_outputs, timed
        if depth > 1 and not hw_queues_ok(depth):
            warnings.warn(f'RequestPipeline(depth={depth}): GPU_MAX_HW_QUEUES={os.environ.get("GPU_MAX_HW_QUEUES", "unset (4)")} < '
                          f'{depth + 1}; HIP streams that share a hardware queue do not overlap -- export GPU_MAX_HW_QUEUES=8 before the '
                          f'first HIP call', RuntimeWarning, stacklevel=2)
        # slots of a pipeline with requests in flight read the throughput-tuned entries of the table (engine._entry)
        self.engines = [InferEngine(net, batch, height, width, device, mode='throughput' if depth > 1 else 'latency') for _ in range(depth)]
        self.streams = _stream_set(device, depth)
        self.counts_host = [torch.zeros(batch, dtype=torch.int32).pin_memory() for _ in range(depth)]
        self.events = [torch.cuda.Event() for _ in range(depth)]
        self.t0 = [torch.cuda.Event(enable_timing=True) for _ in range(depth)] if timed else None
        self.t1 = [torch.cuda.Event(enable_timing=True) for _ in range(depth)] if timed else None
        self.latencies_ms = []
        self.pending = [None] * depth
        self.frame_inputs = [None] * depth              # submit_frames: a slot's input before its engine's graph exists
        self.window = (int(height), int(width)) if int(height) != int(width) else None
        if self.window is not None:
            self.anchors = net.anchors_for(height, width, device)
        else:
            self.anchors = torch.tensor(net.anchors, dtype=torch.float32).reshape(-1, 4).to(device) \
                if not torch.is_tensor(net.anchors) else net.anchors.to(device)
        self.vt = float(getattr(cfg, 'visual_thre', 0) or 0)
        self.submitted = 0
        self.detections = 0

    @classmethod
    def for_frames(cls, net, cfg, frame_hw, device, **kwargs):
        """A pipeline whose network input is the window of the frame sizes `frame_hw` = [(h, w), ...] (or one pair):
        `rect_window(frame_hw, cfg.img_size)`.  Square frames, or landscape and portrait together, give the square pipeline."""
        height, width = rect_window(frame_hw, cfg.img_size)
        return cls(net, cfg, height, width, device, **kwargs)

    def warm_up(self, img, head_outputs=None, rounds=4):
        """Capture every slot's hipGraph (first run of an engine) and push `rounds` requests through every slot, outside any timed
        region: the first requests of a pipeline allocate their result tensors (123 MB of masks per request at 480x640) with
        hipMalloc until the caching allocator holds enough blocks for `depth` requests in flight plus the results the caller
        still owns, and the part ramps its clocks; a server is warm, so the pipeline warms itself.

        Side effects the caller should know: `submitted`, `detections` and `latencies_ms` are RESET to zero / empty afterwards
        (statistics collected before the call are discarded), and with the default `head_outputs=None` the warm-up requests
        post-process the network's own outputs (a random-init net: degenerate detection counts, full-size mask tensors all the
        same).  `rounds=0` captures the graphs only (the cost of the pipeline before round 5)."""
        torch.cuda.synchronize(self.device)
        for e, st in zip(self.engines, self.streams):
            with torch.cuda.stream(st):
                e.run(img)
        torch.cuda.synchronize(self.device)
        if rounds <= 0:
            return
        timed, self.timed = self.timed, False
        for _ in range(rounds * self.depth):
            self.submit(img, head_outputs)
        self.drain()
        torch.cuda.synchronize(self.device)
        self.timed = timed
        self.submitted = self.detections = 0
        self.latencies_ms = []

    def finish(self, slot):
        """Result of the request that last used `slot`: (ids, scores, boxes_px, masks) like `after_nms` (None x 4 without
        detections -- also when `cfg.visual_thre` removes all of them, `utils/output_utils.py:204-212` of the reference; a list of
        such tuples, one per image, when batch > 1), or None if the slot is idle.  Without post-processing: copies of the slot's
        four network outputs (None with `return_outputs=False`)."""
        pend = self.pending[slot]
        if pend is None:
            return None
        self.pending[slot] = None
        if not self.with_post:
            pend.synchronize()
            if self.timed:
                self.latencies_ms.append(self.t0[slot].elapsed_time(self.t1[slot]))
            if not self.return_outputs:
                return None
            # the slot's own buffers are overwritten by its next request: hand out copies, made on the caller's stream (the slot's
            # next run is ordered behind that stream by `submit`)
            return tuple(t.clone() for t in self.engines[slot].outputs())
        if isinstance(pend, _Consumed):                   # the detections were consumed on the slot's stream: nothing is read back
            pend.event.synchronize()
            if self.timed:
                self.latencies_ms.append(self.t0[slot].elapsed_time(self.t1[slot]))
            if isinstance(pend.value, FrameBatch):        # (drawn on the slot's stream, read on the caller's: as for the detections below)
                pend.value.record_stream(torch.cuda.current_stream(self.device))
            return pend.value
        ids, scores, box_px, masks, counts, ev = pend
        ev.synchronize()                                  # THIS request only
        if self.timed:
            self.latencies_ms.append(self.t0[slot].elapsed_time(self.t1[slot]))
        # the results were allocated on the slot's stream and are consumed on the caller's: tell the allocator, or the slot's next
        # request could be handed the block while a kernel of the caller still reads it
        cur = torch.cuda.current_stream(self.device)
        for t in (ids, scores, box_px, masks[0] if isinstance(masks, list) else masks):   # (per-image views share one allocation)
            t.record_stream(cur)
        out = unpad_detections(ids, scores, box_px, masks, self.counts_host[slot].tolist(), self.vt)
        self.detections += sum(int(r[0].shape[0]) for r in out if r[0] is not None)
        return out[0] if self.batch == 1 else out

    def submit(self, img, head_outputs=None, out_hw=None, consumer=None):
        """Enqueue one request ([batch,3,H,W] images, device resident) on the next slot and return the finished result of the request
        that used this slot before (None the first `depth` times).  `head_outputs`: post-process these (class, box, coef, proto)
        tensors instead of the forward's own outputs (bench.py: a random-init network yields degenerate detections).
        `out_hw`: this request's output size (default: the pipeline's); with batch > 1 also a list of `batch` (h, w) pairs, one per
        image: the results then come at those sizes (`after_nms_batch` with per-image sizes; a consumer's `masks` is its list of
        per-image views), while a single pair keeps meaning "all images" through the uniform entry.
        `consumer`: a callable run ON THE SLOT'S STREAM, right behind the post-processing, with the padded device tensors `(ids, scores, boxes_px, masks, counts)` of
        `after_nms_batch(sync=False)`; `finish` / `drain` then hand back ITS return value for the request instead of the detections,
        and no detection count is read on the host (`utils/device_metrics.DeviceAPData.add` is such a consumer).  What `finish` does
        with that count is therefore not done for such a request: `detections` is not advanced, and the `cfg.visual_thre` filter is
        not applied -- the consumer would see unfiltered rows, so a consumer with `cfg.visual_thre` > 0 raises.
        The request is ordered behind everything the caller's current stream has queued; the caller must not overwrite `img` before
        the request has finished (use one input buffer per slot when images arrive by H2D copy)."""
        if consumer is not None and not self.with_post:
            raise RuntimeError('RequestPipeline.submit: a consumer takes the post-processed detections (with_post=True)')
        if consumer is not None and self.vt > 0:
            raise RuntimeError(f'RequestPipeline.submit: cfg.visual_thre = {self.vt} is applied where the count is read on the host; '
                               'a consumer would be handed the unfiltered rows')
        hw = self.out_hw if out_hw is None else out_hw
        if len(hw) and hasattr(hw[0], '__len__'):         # one (h, w) pair per image
            if self.batch == 1 or len(hw) != self.batch or any(len(p) != 2 for p in hw):
                raise RuntimeError(f'RequestPipeline.submit: out_hw is one (h, w) pair, or with batch > 1 a list of {self.batch} pairs')
            out_h, out_w = [int(p[0]) for p in hw], [int(p[1]) for p in hw]
        else:
            out_h, out_w = hw
        return self._enqueue(img, head_outputs, out_h, out_w, consumer)

    def _enqueue(self, img, head_outputs, out_h, out_w, consumer, frames=None):
        """The request itself, behind `submit` and `submit_frames` (arguments checked there).  `frames`: the slot's input is
        `val_aug_batch(frames)`, made on the slot's stream."""
        slot = self.submitted % self.depth
        self.submitted += 1
        done = self.finish(slot)
        ev = self.events[slot]
        # `img` / `head_outputs` were produced on the caller's stream (an H2D copy, `val_aug`), and `finish` may have queued copies
        # of the slot's previous outputs there: the slot's stream starts behind that
        self.streams[slot].wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(self.streams[slot]):
            eng = self.engines[slot]
            if self.timed:
                self.t0[slot].record()
            if frames is not None:
                # straight into the buffer the engine's graph reads (its `copy_` of a tensor onto itself is then a no-op); before
                # the graph exists, into a buffer of the slot's own
                buf = eng.static_img if getattr(eng, 'graph', None) is not None else self._frame_input(slot)
                img = val_aug_batch(frames, self.cfg.img_size if self.window else eng.H, out=buf, window=self.window)
                frames.record_stream(self.streams[slot])       # the caller may drop `frames` while the slot still reads them
            eng.run(img)
            if self.with_post:
                cls, box, coef, proto = head_outputs if head_outputs is not None else eng.outputs()
                r = after_nms_batch(nms_batch(cls, box, coef, proto, self.anchors, self.cfg), out_h, out_w, self.cfg,
                                    sync=False, packed=self.packed_masks, window=self.window is not None)
                if consumer is None:
                    self.counts_host[slot].copy_(r[4], non_blocking=True)
                else:
                    value = consumer(*r)
                if self.timed:
                    self.t1[slot].record()
                ev.record()
                self.pending[slot] = r + (ev,) if consumer is None else _Consumed(value, ev)
            else:
                if self.timed:
                    self.t1[slot].record()
                ev.record()
                self.pending[slot] = ev
        return done

    def _frame_input(self, slot):
        if self.frame_inputs[slot] is None:
            eng = self.engines[slot]
            self.frame_inputs[slot] = torch.empty(self.batch, 3, eng.H, eng.W, dtype=torch.float32, device=self.device)
        return self.frame_inputs[slot]

    def submit_frames(self, frames, head_outputs=None, draw=False, consumer=None):
        """The whole request for `batch` frames of their own sizes, from the uint8 frames on: `frames` is a `FrameBatch`
        (utils/frames.py; `len(frames) == batch`, also for batch 1).  On the slot's stream: `val_aug_batch` into the slot's input
        buffer -> forward -> `nms_batch` -> `after_nms_batch` at the frames' own sizes (the ragged entries).  The result, handed
        back like `submit`'s when the slot comes up again:
          `draw=True`: the drawn frames, a new `FrameBatch` (the ragged `draw_batch`).  No count is read on the host, and because
              `draw_batch` applies `cfg.visual_thre` on the device this is allowed with `visual_thre > 0`;
          `consumer`: its return value, exactly as for `submit` (per-image mask views; refused with `visual_thre > 0`);
          neither: what `submit(val_aug_batch(frames), out_hw=frames.sizes)` returns.
        Without post-processing (`with_post=False`) only the input path differs from `submit`.  `head_outputs` as for `submit`.
        The caller may drop `frames` right away (the allocator is told that the slot's stream reads them) but must not overwrite
        them before the request has finished."""
        if not isinstance(frames, FrameBatch):
            raise RuntimeError('RequestPipeline.submit_frames: frames is a FrameBatch (yolact_minimal_amd.utils.frames)')
        if len(frames) != self.batch:
            raise RuntimeError(f'RequestPipeline.submit_frames: {len(frames)} frames for a pipeline of batch {self.batch}')
        frames.need_cuda('pipeline.RequestPipeline.submit_frames')
        if (draw or consumer is not None) and not self.with_post:
            raise RuntimeError('RequestPipeline.submit_frames: drawing / a consumer takes the post-processed detections (with_post=True)')
        if draw and consumer is not None:
            raise RuntimeError('RequestPipeline.submit_frames: draw=True or a consumer, not both')
        if draw and frames.dtype != torch.uint8:
            raise RuntimeError('RequestPipeline.submit_frames: draw=True needs uint8 frames')
        if consumer is not None and self.vt > 0:
            raise RuntimeError(f'RequestPipeline.submit_frames: cfg.visual_thre = {self.vt} is applied where the count is read on the '
                               'host; a consumer would be handed the unfiltered rows')
        if self.device.index is not None and frames.device != self.device:
            raise RuntimeError(f'RequestPipeline.submit_frames: frames on {frames.device}, pipeline on {self.device}')
        if self.window is not None:
            need = rect_window(frames.sizes, self.cfg.img_size)
            if need[0] > self.window[0] or need[1] > self.window[1]:
                raise RuntimeError(f'RequestPipeline.submit_frames: frames {frames.sizes} need a {need[0]} x {need[1]} window at '
                                   f'{self.cfg.img_size} px, the pipeline was built for {self.window[0]} x {self.window[1]}')
        if draw:
            cfg = self.cfg

            def consumer(*r):
                return draw_batch(r, frames, cfg)
        return self._enqueue(None, head_outputs, [h for h, _ in frames.sizes], [w for _, w in frames.sizes], consumer, frames=frames)

    def drain(self):
        """Finish everything in flight, oldest first."""
        out = []
        for k in range(self.depth):
            slot = (self.submitted + k) % self.depth
            busy = self.pending[slot] is not None
            r = self.finish(slot)
            if busy and (r is not None or self.with_post):
                out.append(r)
        return out
