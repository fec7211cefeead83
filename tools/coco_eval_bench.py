#!/usr/bin/env python3
"""Device time of the COCO-protocol evaluator (utils/coco_eval.py) on the README's eval-loop workload: res101_coco at 544 px
(`bench.detecting_net`), 480 x 640 outputs with bit-packed masks, ~100 detections and 15 ground-truth annotations per image.  The
ground truth is cut from the network's own detections (boxes, masks and classes of 15 of them, two of them marked crowd), so the
matching finds true positives and the categories with many rows have ground truth.

Two legs, alternated `--rounds` times in ONE process, each timed with device events over a window of at least `--window-ms` of
back-to-back calls:
  coco_add   `DeviceCOCOeval.add` (ym_coco_iou_box + ym_coco_iou_mask_packed + ym_coco_match_log)
  ap_add     `DeviceAPData.add` on the same detections and the same gt masks (the reference's own protocol, for scale)
and `DeviceCOCOeval.accumulate()` (sort + ym_coco_accumulate + download) on a log of `--log-images` images x 80 classes filled by
`add`.

The batched metric stage (`--sections batch`): 8 images cycling through the six output sizes of profiles/eval_add_ragged.md, ~100
detections x 15 gt (two crowds) each, packed masks.  Eight `DeviceCOCOeval.add` against ONE `add_batch`
(ym_eval_coco_add_ragged_packed) on the same rows and ground truth, alternated `--rounds` times, device and wall milliseconds per 8
images; and `evaluate_coco_pipelined` at batch 8 / depth 2 over `--images` images of an in-memory annotation index, with one `add` per
image and with one `add_batch` per request, alternated the same way (images per second; here the ground truth is built from the
annotations inside the stage, by `coco_gt` or `coco_gt_batch`).

`--sections` picks among add, accumulate and batch (default: add,accumulate).  Prints one JSON line: every round, medians and ranges."""
import argparse
import gc
import json
import math
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, 'dropin'), REPO]

H, W, G = 480, 640, 15
SIZES = [(480, 640), (640, 480), (427, 640), (375, 500), (500, 333), (640, 640)]


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    gc.collect()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters, (time.perf_counter() - t0) * 1e3 / iters


def calls_for(fn, window_ms):
    fn()
    _, wall = timed(fn, 3)
    return max(10, int(math.ceil(window_ms / max(wall, 1e-3))))


def summary(rows):
    return {k: {'median': float(np.median(v)), 'range': [min(v), max(v)]} for k, v in rows.items()}


def own_gt(ids, boxes, masks, nc):
    """Ground truth cut from an image's own detections: G of them (half of the busiest class), two marked crowd ->
    (classes, crowd flags, areas, [x, y, w, h] boxes, their packed masks)."""
    big = int(torch.bincount(ids, minlength=nc).argmax())
    of_big, others = torch.nonzero(ids == big)[:, 0][:G // 2], torch.nonzero(ids != big)[:, 0]
    sel = torch.cat([of_big, others[:G - of_big.numel()]])
    g = int(sel.numel())
    gt_masks = masks[sel]
    b = boxes[sel].cpu().numpy().astype(np.float64)
    crowd = np.zeros(g, np.uint8)
    crowd[[1, g - 1]] = 1
    area = gt_masks.dense().sum((1, 2)).cpu().numpy().astype(np.float64)
    return (sel, ids[sel].cpu().numpy().astype(np.int32), crowd, area, np.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1),
            gt_masks)


LOG = ('score', 'cls', 'rank', 'flags', 'npig', 'class_rows')


def batch_section(net, cfg, img, o, args):
    """`--sections batch`: see the module text."""
    from yolact_minimal_amd.evaluate import eval_pipeline, evaluate_coco_pipelined
    from yolact_minimal_amd.utils.coco import COCO
    from yolact_minimal_amd.utils.coco_eval import COCOGt, COCOGtBatch, DeviceCOCOeval
    from yolact_minimal_amd.utils.common_utils import rle_encode
    from yolact_minimal_amd.utils.output_utils import after_nms, after_nms_batch, nms, nms_batch
    dev = img.device
    nc = len(cfg.class_names)
    cats = {v - 1: k for k, v in cfg.continuous_id.items()}        # class index -> COCO category id
    r = nms(*o, net.anchors, cfg)
    gts, anns_of = {}, {}
    for h, w in SIZES:
        ids, scores, boxes, masks = after_nms(r[0], r[1], r[2].clone(), r[3], r[4], h, w, packed=True)
        _, cls, crowd, area, xywh, gt_masks = own_gt(ids, boxes, masks, nc)
        gts[(h, w)] = COCOGt.from_arrays(cls, crowd, area, xywh, gt_masks, h, w, dev)
        rles = rle_encode(gt_masks)
        anns_of[(h, w)] = [{'category_id': cats[int(c)], 'iscrowd': int(k), 'area': float(a), 'bbox': [float(v) for v in bx],
                            'segmentation': rle} for c, k, a, bx, rle in zip(cls, crowd, area, xywh, rles)]
    sizes8 = [SIZES[i % len(SIZES)] for i in range(8)]
    o8 = [t.expand(8, *t.shape[1:]).contiguous() for t in o]
    anchors = torch.tensor(net.anchors, dtype=torch.float32).reshape(-1, 4).to(dev)
    dets = nms_batch(*o8, anchors, cfg)
    ids, scores, boxes_px, masks, counts = after_nms_batch(dets, [s[0] for s in sizes8], [s[1] for s in sizes8], cfg, sync=False, packed=True)
    gt8 = [gts[s] for s in sizes8]
    bundle = COCOGtBatch.from_gts(gt8)

    def window(batched, iters):
        ev = DeviceCOCOeval(nc, dev, max_det=cfg.max_detections, capacity_images=8 * iters)     # (no log growth inside the window)
        step = iter(range(iters))

        def once():
            i = next(step)
            if batched:
                ev.add_batch(ids, scores, boxes_px, masks, counts, bundle, list(range(8 * i, 8 * i + 8)))
            else:
                for b in range(8):
                    ev.add(ids[b], scores[b], boxes_px[b], masks[b], counts[b:b + 1], gt8[b], image_index=8 * i + b)
        return timed(once, iters), ev
    _, a = window(False, 4)
    _, b = window(True, 4)
    assert all(torch.equal(getattr(a, n), getattr(b, n)) for n in LOG), 'add_batch and add disagree on the same rows'
    # (each leg's window is sized from its OWN warmed wall time per call, so that both last at least --window-ms)
    iters = {batched: max(10, int(math.ceil(1.1 * args.window_ms / max(window(batched, 50)[0][1], 1e-3)))) for batched in (False, True)}
    rows = {f'{k}_{unit}_ms': [] for k in ('eight_add', 'add_batch') for unit in ('device', 'wall')}
    spans = {'eight_add': [], 'add_batch': []}
    for _ in range(args.rounds):
        for batched, k in ((False, 'eight_add'), (True, 'add_batch')):
            (d, w_), _ = window(batched, iters[batched])
            rows[f'{k}_device_ms'].append(round(d, 4))
            rows[f'{k}_wall_ms'].append(round(w_, 4))
            spans[k].append(round(w_ * iters[batched], 1))
    out = {'sizes': sizes8, 'counts': counts.tolist(), 'gt': [g.g for g in gt8], 'crowds': 2,
           'calls_per_window': {'eight_add': iters[False], 'add_batch': iters[True]}, 'window_wall_ms_rounds': spans,
           'window_ms': args.window_ms, 'rounds': args.rounds, 'stage_8_images_ms_rounds': rows, 'stage_8_images_ms': summary(rows),
           'logs_equal': True}

    # the stage inside the whole loop: one pipeline, the same images, an in-memory annotation index
    coco = COCO(device=dev)
    image_ids = list(range(1, args.images + 1))
    coco.dataset = {'images': [{'id': i, 'height': SIZES[(i - 1) % len(SIZES)][0], 'width': SIZES[(i - 1) % len(SIZES)][1]} for i in image_ids],
                    'categories': [{'id': k, 'name': str(k)} for k in sorted(cfg.continuous_id)], 'annotations': []}
    for i in image_ids:
        for ann in anns_of[SIZES[(i - 1) % len(SIZES)]]:
            coco.dataset['annotations'].append({**ann, 'id': len(coco.dataset['annotations']) + 1, 'image_id': i})
    coco.createIndex()
    pipe = eval_pipeline(net, cfg, img, 480, 640, depth=2, batch=8)

    def loader(n):
        return [(img, None, None, s[0], s[1]) for s in (SIZES[i % len(SIZES)] for i in range(n))]

    def leg(n, batched, keep=None):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, ev = evaluate_coco_pipelined(net, cfg, loader(n), coco, image_ids[:n], pipe=pipe, batched_metrics=batched)
        torch.cuda.synchronize()
        rate = n / (time.perf_counter() - t0)
        if keep is not None:
            keep.append(ev)
        return rate
    evs = []
    for flag in (False, True):                                    # warm-up: allocator, clocks; and the two logs
        leg(32, flag)
        leg(24, flag, keep=evs)
    assert all(torch.equal(getattr(evs[0], n), getattr(evs[1], n)) for n in LOG), 'add_batch and add disagree on the same requests'
    loop = {'b8_d2_add': [], 'b8_d2_add_batch': []}
    for _ in range(args.rounds):
        loop['b8_d2_add'].append(round(leg(args.images, False), 2))
        loop['b8_d2_add_batch'].append(round(leg(args.images, True), 2))
    pipe.drain()
    out.update(loop_images=args.images, loop_img_per_s_rounds=loop, loop_img_per_s=summary(loop), loop_logs_equal=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--log-images', type=int, default=5000, help='log size of the accumulate timing')
    ap.add_argument('--images', type=int, default=192, help='images per pass of a pipeline leg (--sections batch)')
    ap.add_argument('--window-ms', type=float, default=300.0, help='least wall time of a timed window of calls')
    ap.add_argument('--sections', default='add,accumulate', help='comma-separated: add, accumulate, batch')
    args = ap.parse_args()
    sections = set(args.sections.split(','))
    assert torch.cuda.is_available(), 'coco_eval_bench measures on the GPU; there is nothing to measure without one'
    import bench
    import reference_loops as L
    from yolact_minimal_amd.utils.coco_eval import COCOGt
    from yolact_minimal_amd.utils.common_utils import DeviceAPData, DeviceCOCOeval
    from yolact_minimal_amd.utils.output_utils import after_nms, nms
    dev = torch.device('cuda:0')
    net, cfg, img = bench.detecting_net('res101_coco', 544, dev)
    nc = len(cfg.class_names)
    with torch.no_grad():
        o = [t.clone() for t in net(img)]
    result = {'workload': 'res101_coco 544 px, 480x640 packed masks', 'rounds': args.rounds, 'window_ms': args.window_ms}
    if 'batch' in sections:
        result['batch'] = batch_section(net, cfg, img, o, args)
        net._engines.clear()
    if not sections & {'add', 'accumulate'}:
        print(json.dumps(result))
        return
    ids, scores, boxes, masks = after_nms(*nms(*o, net.anchors, cfg), H, W, packed=True)
    sel, cls, crowd, area, xywh, gt_masks = own_gt(ids, boxes, masks, nc)
    g = int(sel.numel())
    coco_gt = COCOGt.from_arrays(cls, crowd, area, xywh, gt_masks, H, W, dev)
    gt = torch.cat([boxes[sel].float() / torch.tensor([W, H, W, H], dtype=torch.float32).to(dev), ids[sel].float()[:, None]], 1)

    def new_coco(capacity):
        return DeviceCOCOeval(nc, dev, max_det=cfg.max_detections, capacity_images=capacity)

    def new_ap(capacity):
        return DeviceAPData(nc, L.IOU_THRES, dev, max_det=cfg.max_detections, capacity_images=capacity)

    result.update(detections=int(ids.shape[0]), gt=g, crowds=2)
    if 'add' in sections:
        ev, acc = new_coco(256), new_ap(256)
        n_coco = calls_for(lambda: ev.add(ids, scores, boxes, masks, None, coco_gt), args.window_ms)
        n_ap = calls_for(lambda: acc.add(ids, scores, boxes, masks, None, gt.clone(), gt_masks, H, W), args.window_ms)
        rows = {'coco_add_device_ms': [], 'coco_add_wall_ms': [], 'ap_add_device_ms': [], 'ap_add_wall_ms': []}
        for _ in range(args.rounds):
            ev, acc = new_coco(n_coco), new_ap(n_ap)                 # (no log growth inside the window)
            d, w_ = timed(lambda: ev.add(ids, scores, boxes, masks, None, coco_gt), n_coco)
            rows['coco_add_device_ms'].append(round(d, 4))
            rows['coco_add_wall_ms'].append(round(w_, 4))
            d, w_ = timed(lambda: acc.add(ids, scores, boxes, masks, None, gt.clone(), gt_masks, H, W), n_ap)
            rows['ap_add_device_ms'].append(round(d, 4))
            rows['ap_add_wall_ms'].append(round(w_, 4))
        result.update(calls_per_window={'coco_add': n_coco, 'ap_add': n_ap}, add_ms_rounds=rows, add_ms=summary(rows))
    if 'accumulate' not in sections:
        print(json.dumps(result))
        return

    ev = new_coco(args.log_images)
    for _ in range(args.log_images):
        ev.add(ids, scores, boxes, masks, None, coco_gt)
    grids = ev.accumulate()
    stats = {k: ev.summarize(grids)[k][0].round(4).tolist() for k in grids}
    n_acc = calls_for(ev.accumulate, args.window_ms)
    acc_rows = {'accumulate_device_ms': [], 'accumulate_wall_ms': []}
    for _ in range(args.rounds):
        d, w_ = timed(ev.accumulate, n_acc)
        acc_rows['accumulate_device_ms'].append(round(d, 4))
        acc_rows['accumulate_wall_ms'].append(round(w_, 4))
    result['accumulate'] = dict(images=args.log_images, classes=nc, rows=ev.capacity * ev.max_det,
                                data_points=int(ev.class_rows.sum()), calls_per_window=n_acc, stats=stats, rounds=acc_rows,
                                **summary(acc_rows))
    print(json.dumps(result))


if __name__ == '__main__':
    main()
