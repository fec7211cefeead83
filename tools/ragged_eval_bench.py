#!/usr/bin/env python3
"""What mixed-size batches buy on an evaluation whose images differ in size: res101_coco at 544 px (`bench.detecting_net`), 192
samples whose output sizes cycle through a COCO-like list (480x640, 640x480, 427x640, 375x500, 500x333, 640x640), ~100 detections
and 15 ground-truth instances per image.  The ground truth of a size is cut from the network's own detections at that size (boxes,
masks and classes of 15 of them), as tools/eval_metrics_bench.py does.

Three legs, alternated `--rounds` times in ONE process, each on a pipeline built and captured before the timing:
  b1_d4   `evaluate_pipelined` with batch-1 requests, four in flight: the path before mixed-size batches (the yardstick)
  b8_d2   requests of 8 images, each post-processed at its own size (`ym_after_nms_ragged_packed`), two in flight
  b4_d2   requests of 4 images, two in flight
GPU_MAX_HW_QUEUES is raised to 8 before the first HIP call, as tests/conftest.py does.  Every leg evaluates the same samples and
ends synchronised; its clock includes `drain()` and `calc_map`.
Also: device and wall time of ONE `after_nms_batch` over 8 of those sizes (packed and dense) against the same eight images through
eight `after_nms` calls, each over windows of at least `--window-ms` of back-to-back calls.  Prints one JSON line."""
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

SIZES = [(480, 640), (640, 480), (427, 640), (375, 500), (500, 333), (640, 640)]
G = 15


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
    ap.add_argument('--images', type=int, default=192, help='images per pass of a leg')
    ap.add_argument('--window-ms', type=float, default=300.0, help='least wall time of a timed window of calls')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'ragged_eval_bench measures on the GPU; there is nothing to measure without one'
    import bench
    from yolact_minimal_amd.evaluate import eval_pipeline, evaluate_pipelined
    from yolact_minimal_amd.utils.output_utils import BatchDetections, after_nms, after_nms_batch, nms, nms_batch
    dev = torch.device('cuda:0')
    net, cfg, img = bench.detecting_net('res101_coco', 544, dev)
    nc = len(cfg.class_names)
    with torch.no_grad():
        o = [t.clone() for t in net(img)]
    r = nms(*o, net.anchors, cfg)
    gts = {}
    for h, w in SIZES:                                            # ground truth = G of the image's own detections at this size
        ids, scores, boxes, masks = after_nms(r[0], r[1], r[2].clone(), r[3], r[4], h, w)
        big = int(torch.bincount(ids, minlength=nc).argmax())
        of_big, others = torch.nonzero(ids == big)[:, 0][:G // 2], torch.nonzero(ids != big)[:, 0]
        sel = torch.cat([of_big, others[:G - of_big.numel()]])
        gt = torch.cat([boxes[sel].float() / torch.tensor([w, h, w, h], dtype=torch.float32).to(dev), ids[sel].float()[:, None]], 1)
        gts[(h, w)] = (gt, (masks[sel] > 0.5).float())
    detections = int(r[0].shape[0])

    def loader(n=args.images):
        return [(img, gts[s][0].clone(), gts[s][1], s[0], s[1]) for s in (SIZES[i % len(SIZES)] for i in range(n))]

    legs = {'b1_d4': (1, 4), 'b8_d2': (8, 2), 'b4_d2': (4, 2)}
    pipes = {k: eval_pipeline(net, cfg, img, 480, 640, depth=d, batch=b) for k, (b, d) in legs.items()}

    def leg(name, samples, step=None):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        table, _ = evaluate_pipelined(net, cfg, samples, pipe=pipes[name], step=step)
        torch.cuda.synchronize()
        return len(samples) / (time.perf_counter() - t0), table
    tables = {}
    for name in legs:                                             # warm-up: allocator, clocks; and what the legs report
        leg(name, loader(32))
        tables[name] = leg(name, loader(24), step=0)[1][0]
    rows = {k: [] for k in legs}
    for _ in range(args.rounds):
        for name in legs:
            rows[name].append(round(leg(name, loader())[0], 2))
    result = {'workload': 'res101_coco 544 px, output sizes cycling through ' + ', '.join(f'{h}x{w}' for h, w in SIZES),
              'images_per_pass': args.images, 'rounds': args.rounds, 'legs': {k: {'batch': b, 'depth': d} for k, (b, d) in legs.items()},
              'GPU_MAX_HW_QUEUES': os.environ.get('GPU_MAX_HW_QUEUES'), 'img_per_s_rounds': rows, 'img_per_s': summary(rows),
              'detections': detections, 'gt': G, 'window_ms': args.window_ms,
              # (a batch-8 forward reads other plan rows than a batch-1 forward: another rounding, so equality is reported, not required)
              'tables_equal_b1_d4': {k: tables[k] == tables['b1_d4'] for k in legs}}
    for p in pipes.values():
        p.drain()
    del pipes
    net._engines.clear()

    # one after_nms_batch over 8 sizes against eight after_nms calls, on the same eight images
    sizes8 = [SIZES[i % len(SIZES)] for i in range(8)]
    hs, ws = [s[0] for s in sizes8], [s[1] for s in sizes8]
    o8 = [t.expand(8, *t.shape[1:]).contiguous() for t in o]
    anchors = torch.tensor(net.anchors, dtype=torch.float32).reshape(-1, 4).to(dev)
    dets = nms_batch(*o8, anchors, cfg)
    split = dets.split()
    box_b, box_1 = dets.boxes.clone(), [s[2].clone() for s in split]
    work = BatchDetections(dets.counts, dets.ids, dets.scores, box_b, dets.coefs, dets.proto)

    def ragged(packed):
        box_b.copy_(dets.boxes)                                   # (after_nms scales its boxes in place)
        return after_nms_batch(work, hs, ws, cfg, sync=False, packed=packed)

    def per_image(packed):
        out = []
        for s, bx, (h, w) in zip(split, box_1, sizes8):
            bx.copy_(s[2])
            out.append(after_nms(s[0], s[1], bx, s[3], s[4], h, w, cfg, packed=packed))
        return out
    for packed in (False, True):                                  # the two must agree before either is timed
        got, want = ragged(packed), per_image(packed)
        for b, w_ in enumerate(want):
            n = w_[0].shape[0]
            a, c = got[3][b][:n], w_[3]
            assert torch.equal(a.bits if packed else a, c.bits if packed else c) and torch.equal(got[2][b, :n], w_[2])
    fns = {'ragged_packed': lambda: ragged(True), 'eight_after_nms_packed': lambda: per_image(True),
           'ragged_dense': lambda: ragged(False), 'eight_after_nms_dense': lambda: per_image(False)}
    calls = {k: calls_for(f, args.window_ms) for k, f in fns.items()}
    stage = {f'{k}_{unit}_ms': [] for k in fns for unit in ('device', 'wall')}
    for _ in range(args.rounds):
        for k, f in fns.items():
            d, w_ = timed(f, calls[k])
            stage[k + '_device_ms'].append(round(d, 4))
            stage[k + '_wall_ms'].append(round(w_, 4))
    result['after_nms_8_images_ms'] = summary(stage)
    result['after_nms_8_images_sizes'] = sizes8
    result['after_nms_calls_per_window'] = calls
    print(json.dumps(result))


if __name__ == '__main__':
    main()
