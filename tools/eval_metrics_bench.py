#!/usr/bin/env python3
"""What the device-resident mAP accumulator (utils/device_metrics.py) buys on the README's eval-loop workload: res101_coco at
544 px (`bench.detecting_net`), 480 x 640 outputs, ~100 detections and 15 ground-truth instances per image.  The ground truth is
cut from the network's own detections (boxes, masks and classes of 15 of them, the most frequent class among them), so that the
matching finds true positives and the classes with many rows have ground truth: their AP cells are walked, not skipped.

Three legs, alternated `--rounds` times in ONE process (the baseline is the same build in the same process, minutes apart at most):
  host       `dropin/reference_loops.eval_loop` as it is: `prep_metrics` with its host lists (the yardstick)
  device     `eval_loop(device_metrics=True)`: same loop, the metric stage is `DeviceAPData.add`
  pipelined  `evaluate.evaluate_pipelined(pipe=...)`: the loop as requests of ONE depth-4 pipeline built and captured before the
             timing (`evaluate.eval_pipeline`), whose consumer is `add`
GPU_MAX_HW_QUEUES is raised to 8 before the first HIP call, as tests/conftest.py does (an exported smaller value is overridden: the
pipelined leg needs a hardware queue per slot).  Every leg evaluates the same `--images` samples and ends synchronised (`eval_loop`
synchronises before it stops its clock; the pipelined leg's clock includes `drain()` and `calc_map`).  Also: device and wall time of
one `add`, of `calc_map`, and of `ym_eval_ap` alone on a log of `--log-images` images filled by `add`; each of these is timed over
a window of at least `--window-ms` of back-to-back calls.  Prints one JSON line: every round, medians and ranges."""
import argparse
import gc
import json
import math
import os
import sys
import time

try:
    _queues = int(os.environ.get('GPU_MAX_HW_QUEUES', '0'))
except ValueError:
    _queues = 0
if _queues < 8:
    os.environ['GPU_MAX_HW_QUEUES'] = '8'

import numpy as np  # noqa: E402
import torch  # noqa: E402

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
    """How many back-to-back calls of `fn` fill `window_ms` of wall time (from a short calibration run, which also warms it up)."""
    fn()
    _, wall = timed(fn, 3)
    return max(10, int(math.ceil(window_ms / max(wall, 1e-3))))


def summary(rows):
    return {k: {'median': float(np.median(v)), 'range': [min(v), max(v)]} for k, v in rows.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--images', type=int, default=192, help='images per pass of a leg')
    ap.add_argument('--log-images', type=int, default=5000, help='log size of the AP-kernel timing')
    ap.add_argument('--depth', type=int, default=4)
    ap.add_argument('--window-ms', type=float, default=500.0, help='least wall time of a timed window of calls')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'eval_metrics_bench measures on the GPU; there is nothing to measure without one'
    import bench
    import reference_loops as L
    from yolact_minimal_amd import hip
    from yolact_minimal_amd.evaluate import eval_pipeline, evaluate_pipelined
    from yolact_minimal_amd.utils.common_utils import APDataObject, DeviceAPData, prep_metrics
    from yolact_minimal_amd.utils.output_utils import after_nms, nms
    dev = torch.device('cuda:0')
    net, cfg, img = bench.detecting_net('res101_coco', 544, dev)
    nc = len(cfg.class_names)
    with torch.no_grad():
        o = net(img)
    ids, scores, boxes, masks = after_nms(*nms(*o, net.anchors, cfg), H, W)
    # ground truth = G of the image's own detections: up to G // 2 of the most frequent class, then the best-scoring others
    big = int(torch.bincount(ids, minlength=nc).argmax())
    of_big, others = torch.nonzero(ids == big)[:, 0][:G // 2], torch.nonzero(ids != big)[:, 0]
    sel = torch.cat([of_big, others[:G - of_big.numel()]])
    gt = torch.cat([boxes[sel].float() / torch.tensor([W, H, W, H], dtype=torch.float32).to(dev), ids[sel].float()[:, None]], 1)
    gt_masks = (masks[sel] > 0.5).float()

    def loader(n=args.images):
        return [(img, gt.clone(), gt_masks, H, W) for _ in range(n)]

    pipe = eval_pipeline(net, cfg, img, H, W, depth=args.depth)

    def pipelined(s):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        evaluate_pipelined(net, cfg, s, pipe=pipe)
        torch.cuda.synchronize()
        return len(s), time.perf_counter() - t0
    legs = {
        'host': lambda s: L.eval_loop(net, cfg, s)[2:],
        'device': lambda s: L.eval_loop(net, cfg, s, device_metrics=True)[2:],
        'pipelined': pipelined,
    }
    tables = {}
    for name, leg in legs.items():                               # warm-up: engines, allocator; and the legs must agree
        leg(loader(16))
    tables['host'] = L.table(L.eval_loop(net, cfg, loader(8))[0], cfg, step=0)[0]
    tables['device'] = L.table(L.eval_loop(net, cfg, loader(8), device_metrics=True)[0], cfg, step=0)[0]
    tables['pipelined'] = evaluate_pipelined(net, cfg, loader(8), step=0, pipe=pipe)[0][0]
    assert tables['host'] == tables['device'] == tables['pipelined'], tables
    rows = {k: [] for k in legs}
    for _ in range(args.rounds):
        for name, leg in legs.items():
            seen, sec = leg(loader())
            rows[name].append(round(seen / sec, 2))
    result = {'workload': 'res101_coco 544 px, 480x640 outputs', 'images_per_pass': args.images, 'rounds': args.rounds,
              'depth': args.depth, 'GPU_MAX_HW_QUEUES': os.environ.get('GPU_MAX_HW_QUEUES'), 'img_per_s_rounds': rows,
              'img_per_s': summary(rows), 'detections': int(ids.shape[0]), 'gt': int(gt.shape[0]), 'window_ms': args.window_ms}

    # one add / one calc_map / one host prep_metrics on the loop's own detections
    stage = {'add_device_ms': [], 'add_wall_ms': [], 'calc_map_device_ms': [], 'calc_map_wall_ms': [], 'host_prep_metrics_wall_ms': []}

    def new_acc(capacity):
        return DeviceAPData(nc, L.IOU_THRES, dev, max_det=cfg.max_detections, capacity_images=capacity)

    def host_prep(ap_host):
        prep_metrics(ap_host, list(ids.cpu().numpy().astype(int)), list(scores.cpu().numpy().astype(float)), boxes, masks, gt.clone(),
                     gt_masks, H, W, L.IOU_THRES)
    acc = new_acc(256)
    n_add = calls_for(lambda: acc.add(ids, scores, boxes, masks, None, gt.clone(), gt_masks, H, W), args.window_ms)
    acc_map = new_acc(256)                                       # calc_map on a full log of 256 images
    for _ in range(256):
        acc_map.add(ids, scores, boxes, masks, None, gt.clone(), gt_masks, H, W)
    n_map = calls_for(lambda: acc_map.calc_map(0), args.window_ms)
    ap_host = {k: [[APDataObject() for _ in range(nc)] for _ in L.IOU_THRES] for k in ('box', 'mask')}
    n_host = calls_for(lambda: host_prep(ap_host), args.window_ms)
    for _ in range(args.rounds):
        acc = new_acc(n_add)                                     # (no log growth inside the window)
        d, w_ = timed(lambda: acc.add(ids, scores, boxes, masks, None, gt.clone(), gt_masks, H, W), n_add)
        stage['add_device_ms'].append(round(d, 4))
        stage['add_wall_ms'].append(round(w_, 4))
        d, w_ = timed(lambda: acc_map.calc_map(0), n_map)
        stage['calc_map_device_ms'].append(round(d, 4))
        stage['calc_map_wall_ms'].append(round(w_, 4))
        ap_host = {k: [[APDataObject() for _ in range(nc)] for _ in L.IOU_THRES] for k in ('box', 'mask')}
        _, w_ = timed(lambda: host_prep(ap_host), n_host)
        stage['host_prep_metrics_wall_ms'].append(round(w_, 4))
    result['stage_ms'] = summary(stage)
    result['stage_calls_per_window'] = {'add': n_add, 'calc_map': n_map, 'host_prep_metrics': n_host, 'calc_map_log_images': 256}

    # ym_eval_ap on a log of --log-images images, every one of them added like the loop adds it
    acc = new_acc(args.log_images)
    for _ in range(args.log_images):
        acc.add(ids, scores, boxes, masks, None, gt.clone(), gt_masks, H, W)
    class_rows, gt_count = acc.class_rows.tolist(), acc.gt_count.tolist()
    largest = int(np.argmax(class_rows))
    passes = class_rows[largest] / hip.EVAL_AP_ROWS_PER_PASS
    assert gt_count[largest] > 0 and passes > 8, \
        f'the largest class ({largest}: {class_rows[largest]} rows, {gt_count[largest]} gt) must have ground truth and many passes of rows'
    grid, _ = acc.ap_grid()
    ap_ms = {'ap_grid_device_ms': [], 'ap_grid_wall_ms': [], 'ym_eval_ap_device_ms': []}
    n_grid = calls_for(acc.ap_grid, args.window_ms)
    # the kernels alone (sort and download excluded): the accumulator's own launch with its order precomputed
    rows_n, order, seg = acc._sorted_order()
    out = torch.empty(grid.size * 8 + nc, dtype=torch.uint8, device=dev)
    ws = torch.empty(hip.lib().ym_eval_ap_workspace_bytes(rows_n), dtype=torch.uint8, device=dev)

    def kernel():
        acc._launch_ap(rows_n, order, seg, out, ws)
    n_kernel = calls_for(kernel, args.window_ms)
    assert np.array_equal(out.cpu().numpy()[:grid.size * 8].view(np.float64).reshape(grid.shape), grid)
    for _ in range(args.rounds):
        d, w_ = timed(acc.ap_grid, n_grid)
        ap_ms['ap_grid_device_ms'].append(round(d, 4))
        ap_ms['ap_grid_wall_ms'].append(round(w_, 4))
        ap_ms['ym_eval_ap_device_ms'].append(round(timed(kernel, n_kernel)[0], 4))
    result['ap_on_log'] = dict(images=args.log_images, rows=rows_n, data_points=int(sum(class_rows)), largest_class=largest,
                               largest_class_rows=class_rows[largest], largest_class_gt=gt_count[largest],
                               largest_class_passes=round(passes, 1), largest_class_ap_box50=float(grid[0, 0, largest]),
                               classes_with_rows_and_gt=int(sum(1 for r, g_ in zip(class_rows, gt_count) if r and g_)),
                               calls_per_window={'ap_grid': n_grid, 'ym_eval_ap': n_kernel}, **summary(ap_ms))
    print(json.dumps(result))


if __name__ == '__main__':
    main()
