"""Evaluation with several requests in flight: eval.py's loop (`eval.py:35-69,106`) through `RequestPipeline` and the
device-resident accumulator (`utils/device_metrics.DeviceAPData`).

The reference evaluates one image at a time and its `prep_metrics` reads the detections on the host, so every image is a
synchronisation point.  Here every image is one pipeline request (forward -> nms -> after_nms on the slot's stream) whose consumer
is `DeviceAPData.add(..., image_index=i)` on that same stream: nothing of an image is read on the host, and the log keeps the
sample order whatever order the slots finish in.  The one download is `calc_map`'s AP grid at the end.  Requests of several images
(`batch` > 1) add image by image by default, or with `batched_metrics=True` through one `DeviceAPData.add_batch` per request.
`evaluate_coco_pipelined` runs the same requests into `utils/coco_eval.DeviceCOCOeval` (the COCO protocol's twelve numbers), image by
image or through one `DeviceCOCOeval.add_batch` per request, and `evaluate_json_pipelined` into the detection dumps
(`utils/common_utils.BatchMakeJson`, one `add_batch` per request).
"""
import torch

from .pipeline import RequestPipeline
from .utils.coco_eval import KINDS, DeviceCOCOeval, coco_gt, coco_gt_batch
from .utils.device_metrics import DeviceAPData

IOU_THRES = [x / 100 for x in range(50, 100, 5)]                              # eval.py:24


def eval_pipeline(net, cfg, img, img_h, img_w, depth=4, packed_masks=True, batch=1):
    """The `RequestPipeline` `evaluate_pipelined` runs on, with its hipGraphs captured on `img`: build it once and hand it to several
    calls (`pipe=`) where the same network evaluates more than one sample set -- four engines and their capture are no part of a set.
    `batch` > 1: requests of `batch` images (`img` is one image, or already a batch of that many)."""
    device = next(net.parameters()).device
    pipe = RequestPipeline(net, cfg, img.shape[2], img.shape[3], device, depth=depth, out_hw=(img_h, img_w), packed_masks=packed_masks,
                           batch=batch)
    img = img.to(device)
    if batch > 1 and img.shape[0] != batch:
        img = img[:1].expand(batch, -1, -1, -1).contiguous()
    pipe.warm_up(img, rounds=0)
    return pipe


def _submit_groups(net, cfg, items, device, batch, depth, packed_masks, pipe, metric_stage):
    """The grouping and padding loop of every batched evaluation: `items` yields `(img on the device, tensors to keep alive until the
    slot has read them, payload, img_h, img_w)`; `batch` consecutive items form one request, every image at its own output size; a
    short last group is padded by repeating its last item.  On the slot's stream the request's consumer calls
    `metric_stage(first, real, payloads, sizes, ids, scores, boxes_px, masks, counts)`: `first` = the position of the group's first
    item, `real` = the items that are no padding, `payloads` / `sizes` = all `batch` entries.  Returns the pipeline."""
    group = []

    def flush(pipe):
        first = group[0][0]
        real = len(group)
        entries = group + [group[-1]] * (batch - real)
        imgs = torch.cat([e[1] for e in entries], 0)
        sizes = [(e[4], e[5]) for e in entries]
        if pipe is None:
            pipe = eval_pipeline(net, cfg, imgs, sizes[0][0], sizes[0][1], depth, packed_masks, batch)
        held = [t for e in group for t in (e[1],) + tuple(e[2])] + [imgs]
        payloads = [e[3] for e in entries]

        def consume(ids, scores, boxes_px, masks, counts):
            slot_stream = torch.cuda.current_stream(device)
            for t in held:                                      # made on the caller's stream, read on the slot's
                t.record_stream(slot_stream)
            metric_stage(first, real, payloads, sizes, ids, scores, boxes_px, masks, counts)

        pipe.submit(imgs, out_hw=sizes, consumer=consume)
        del group[:]
        return pipe

    for i, (img, held, payload, img_h, img_w) in enumerate(items):
        group.append((i, img, held, payload, int(img_h), int(img_w)))
        if len(group) == batch:
            pipe = flush(pipe)
    if group:
        pipe = flush(pipe)
    return pipe


def _evaluate_batched(net, cfg, samples, acc, batch, depth, packed_masks, pipe, batched_metrics=False):
    """`batch` consecutive samples per request (`_submit_groups`); a padded entry is never added.  `batched_metrics`: one
    `DeviceAPData.add_batch` per request instead of one `add` per image (packed masks only)."""
    device = acc.device

    def items():
        for img, gt, gt_masks, img_h, img_w in samples:
            gt, gt_masks = gt.to(device), gt_masks.to(device)
            yield img.to(device), (gt, gt_masks), (gt, gt_masks), img_h, img_w

    def metric_stage(first, real, payloads, sizes, ids, scores, boxes_px, masks, counts):
        if batched_metrics:                                     # (the whole request, padding marked by an index of None)
            acc.add_batch(ids, scores, boxes_px, masks, counts, [p[0] for p in payloads], [p[1] for p in payloads], sizes,
                          [first + b if b < real else None for b in range(batch)])
            return
        for b in range(real):                                   # (one image's padded rows and its count: what `add` takes)
            acc.add(ids[b], scores[b], boxes_px[b], masks[b], counts[b:b + 1], payloads[b][0], payloads[b][1], sizes[b][0], sizes[b][1],
                    image_index=first + b)

    return _submit_groups(net, cfg, items(), device, batch, depth, packed_masks, pipe, metric_stage)


def evaluate_pipelined(net, cfg, samples, depth=4, packed_masks=True, step=None, pipe=None, batch=1, batched_metrics=False):
    """`samples` yields eval.py's `(img [1,3,H,W], gt [g,5], gt_masks [g,h,w], img_h, img_w)`; all images share one input size.
    `pipe`: an idle pipeline of `eval_pipeline` to run on (`depth`, `packed_masks` and `batch` are then the pipeline's); by default
    one is built on the first sample.  `batch` > 1: `batch` consecutive samples form one request, each image post-processed at its own
    `(img_h, img_w)` (`after_nms_batch` with per-image sizes) and added on the slot's stream image by image; a short last request is
    padded with copies of its last image, which are not added.  `batched_metrics=True` (with `batch` > 1 and packed masks; dense
    masks raise before anything runs): the metric stage of a request is ONE `DeviceAPData.add_batch` on the slot's stream instead
    of one `add` per image; the log is the same.  Returns ((table text, box row, mask row), the DeviceAPData)."""
    device = next(net.parameters()).device
    if pipe is not None:
        batch, packed_masks = pipe.batch, pipe.packed_masks
    if batched_metrics and batch > 1 and not packed_masks:
        raise RuntimeError('evaluate_pipelined: batched_metrics=True needs packed masks (the batched metric stage is packed-only)')
    acc = DeviceAPData(len(cfg.class_names), IOU_THRES, device, max_det=cfg.max_detections)
    if batch > 1:
        pipe = _evaluate_batched(net, cfg, samples, acc, batch, depth, packed_masks, pipe, batched_metrics)
        if pipe is not None:
            pipe.drain()
        return acc.calc_map(step), acc
    for i, (img, gt, gt_masks, img_h, img_w) in enumerate(samples):
        img, gt, gt_masks = img.to(device), gt.to(device), gt_masks.to(device)
        if pipe is None:
            pipe = eval_pipeline(net, cfg, img, img_h, img_w, depth, packed_masks)

        def consume(ids, scores, boxes_px, masks, counts, i=i, img=img, gt=gt, gt_masks=gt_masks, img_h=img_h, img_w=img_w):
            slot_stream = torch.cuda.current_stream(device)
            for t in (img, gt, gt_masks):                       # made on the caller's stream, read on the slot's
                t.record_stream(slot_stream)
            return acc.add(ids, scores, boxes_px, masks, counts, gt, gt_masks, img_h, img_w, image_index=i)

        pipe.submit(img, out_hw=(img_h, img_w), consumer=consume)
    if pipe is not None:
        pipe.drain()
    return acc.calc_map(step), acc


def evaluate_coco_pipelined(net, cfg, samples, coco, image_ids, depth=4, packed_masks=True, pipe=None, batch=1, batched_metrics=False,
                            kinds=KINDS):
    """`evaluate_pipelined`'s requests scored by the COCO protocol (`utils/coco_eval.DeviceCOCOeval`, the twelve numbers of
    `eval.py --coco_api`): sample i is image `image_ids[i]` of the `COCO` index `coco`, whose annotations are the ground truth (the
    sample's own `gt` / `gt_masks` are not looked at: the val loader drops crowds).  The evaluator's image index is the rank of the
    image id in `sorted(coco.imgs)`, as `eval_loop(coco_api='score')` assigns it; every sample counts, also one without detections.
    The metric stage runs on the slot's stream: one `DeviceCOCOeval.add` per image against `coco_gt`, or with `batched_metrics=True`
    (`batch` > 1, packed masks only; dense masks raise before anything runs) ONE `add_batch` per request against `coco_gt_batch`; the log is the
    same.  A short last request is padded with copies of its last image, which are not added.  With `batch` = 1 a request is one image
    and `batched_metrics=True` runs the per-image `add` all the same; unlike `evaluate_pipelined`, which ignores the flag at batch 1,
    this call refuses `batched_metrics=True` with dense masks at every batch size.  `pipe`, `depth`, `packed_masks`,
    `batch`: as for `evaluate_pipelined`.  Returns (`ev.summarize()`, the DeviceCOCOeval)."""
    device = next(net.parameters()).device
    if pipe is not None:
        batch, packed_masks = pipe.batch, pipe.packed_masks
    if batched_metrics and not packed_masks:
        raise RuntimeError('evaluate_coco_pipelined: batched_metrics=True needs packed masks (the batched metric stage is packed-only)')
    image_ids = list(image_ids)
    slot = {img_id: k for k, img_id in enumerate(sorted(coco.imgs))}
    ev = DeviceCOCOeval(len(cfg.class_names), device, max_det=cfg.max_detections, kinds=kinds, capacity_images=max(1, len(slot)))
    want_masks = 'segm' in ev.kinds

    def items():
        for i, (img, _, _, img_h, img_w) in enumerate(samples):
            yield img.to(device), (), image_ids[i], img_h, img_w

    def metric_stage(first, real, payloads, sizes, ids, scores, boxes_px, masks, counts):
        if batched_metrics:                                     # (the whole request, padding marked by an index of None)
            live = [b < real for b in range(len(payloads))]     # (a padding entry brings its size, not its annotations)
            ev.add_batch(ids, scores, boxes_px, masks, counts, coco_gt_batch(coco, payloads, cfg.continuous_id, device, want_masks, live),
                         [slot[p] if keep else None for p, keep in zip(payloads, live)])
            return
        for b in range(real):
            ev.add(ids[b], scores[b], boxes_px[b], masks[b], counts[b:b + 1], coco_gt(coco, payloads[b], cfg.continuous_id, device, want_masks),
                   image_index=slot[payloads[b]])

    if batch > 1:
        pipe = _submit_groups(net, cfg, items(), device, batch, depth, packed_masks, pipe, metric_stage)
    else:                                                       # (requests of one image: the uniform entry, one `add` each)
        for img, _, img_id, img_h, img_w in items():
            if pipe is None:
                pipe = eval_pipeline(net, cfg, img, img_h, img_w, depth, packed_masks)

            def consume(ids, scores, boxes_px, masks, counts, img=img, img_id=img_id):
                img.record_stream(torch.cuda.current_stream(device))
                return ev.add(ids, scores, boxes_px, masks, counts, coco_gt(coco, img_id, cfg.continuous_id, device, want_masks),
                              image_index=slot[img_id])

            pipe.submit(img, out_hw=(img_h, img_w), consumer=consume)
    if pipe is not None:
        pipe.drain()
    return ev.summarize(), ev


def evaluate_json_pipelined(net, cfg, samples, image_ids, depth=4, pipe=None, batch=1, make_json=None):
    """`evaluate_pipelined`'s requests dumped for the COCO API (`eval.py --coco_api`'s `bbox_detections.json` /
    `mask_detections.json`): sample i is image `image_ids[i]`, and the metric stage of a request is ONE
    `utils/common_utils.BatchMakeJson.add_batch` on the slot's stream -- no host read; the records of a request are fetched when a
    later request finds its event completed, the rest by `dump`.  Packed masks only (a `pipe` with dense masks raises before anything
    runs).  A short last request is padded with copies of its last image, which yield no record.  With `batch` = 1 a request is the
    uniform entry's batch of one.  `pipe`, `depth`, `batch`: as for `evaluate_pipelined`; `make_json`: a `BatchMakeJson` to add to.
    Returns the `BatchMakeJson` (`dump(bbox_path, mask_path)` writes the files; `dropin/reference_loops.coco_summary` scores it)."""
    from .utils.common_utils import BatchMakeJson
    device = next(net.parameters()).device
    if pipe is not None:
        batch = pipe.batch
        if not pipe.packed_masks:
            raise RuntimeError('evaluate_json_pipelined: the pipeline must produce packed masks (BatchMakeJson.add_batch is packed-only)')
    dumps = BatchMakeJson() if make_json is None else make_json
    if not isinstance(dumps, BatchMakeJson):
        raise RuntimeError('evaluate_json_pipelined: make_json is a BatchMakeJson')
    image_ids = list(image_ids)

    def items():
        for i, (img, _, _, img_h, img_w) in enumerate(samples):
            yield img.to(device), (), image_ids[i], img_h, img_w

    def metric_stage(first, real, payloads, sizes, ids, scores, boxes_px, masks, counts):
        dumps.add_batch(ids, scores, boxes_px, masks, counts, [p if b < real else None for b, p in enumerate(payloads)])

    if batch > 1:
        pipe = _submit_groups(net, cfg, items(), device, batch, depth, True, pipe, metric_stage)
    else:                                                       # (requests of one image: the uniform entry's batch of one)
        for img, _, img_id, img_h, img_w in items():
            if pipe is None:
                pipe = eval_pipeline(net, cfg, img, img_h, img_w, depth, True)

            def consume(ids, scores, boxes_px, masks, counts, img=img, img_id=img_id):
                img.record_stream(torch.cuda.current_stream(device))
                dumps.add_batch(ids, scores, boxes_px, masks, counts, [img_id])

            pipe.submit(img, out_hw=(img_h, img_w), consumer=consume)
    if pipe is not None:
        pipe.drain()
    return dumps
