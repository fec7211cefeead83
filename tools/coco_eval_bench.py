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
`add`.  Prints one JSON line: every round, medians and ranges."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--log-images', type=int, default=5000, help='log size of the accumulate timing')
    ap.add_argument('--window-ms', type=float, default=300.0, help='least wall time of a timed window of calls')
    args = ap.parse_args()
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
        o = net(img)
    ids, scores, boxes, masks = after_nms(*nms(*o, net.anchors, cfg), H, W, packed=True)
    big = int(torch.bincount(ids, minlength=nc).argmax())
    of_big, others = torch.nonzero(ids == big)[:, 0][:G // 2], torch.nonzero(ids != big)[:, 0]
    sel = torch.cat([of_big, others[:G - of_big.numel()]])
    g = int(sel.numel())
    gt_masks = masks[sel]
    b = boxes[sel].cpu().numpy().astype(np.float64)
    crowd = np.zeros(g, np.uint8)
    crowd[[1, g - 1]] = 1
    area = gt_masks.dense().sum((1, 2)).cpu().numpy().astype(np.float64)
    coco_gt = COCOGt.from_arrays(ids[sel].cpu().numpy().astype(np.int32), crowd, area,
                                 np.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1), gt_masks, H, W, dev)
    gt = torch.cat([boxes[sel].float() / torch.tensor([W, H, W, H], dtype=torch.float32).to(dev), ids[sel].float()[:, None]], 1)

    def new_coco(capacity):
        return DeviceCOCOeval(nc, dev, max_det=cfg.max_detections, capacity_images=capacity)

    def new_ap(capacity):
        return DeviceAPData(nc, L.IOU_THRES, dev, max_det=cfg.max_detections, capacity_images=capacity)

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
    result = {'workload': 'res101_coco 544 px, 480x640 packed masks', 'detections': int(ids.shape[0]), 'gt': g, 'crowds': 2,
              'rounds': args.rounds, 'window_ms': args.window_ms, 'calls_per_window': {'coco_add': n_coco, 'ap_add': n_ap},
              'add_ms_rounds': rows, 'add_ms': summary(rows)}

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
