#!/usr/bin/env python3
"""What rectangular inference ("window mode", yolact_minimal_amd/utils/rect.py) is worth in serving: res101_coco at 544 px
(`bench.build_net`), uint8 frames of 480x640 (window 416x544) and of 1080x1920 (window 320x544), 100 detections per frame from the
dense synthetic head outputs (`utils.synthetic.synth_head_outputs`, seed 1, as bench.py) with every anchor outside the window set to
background, so that the square and the window pipeline post-process the SAME detections.

ONE process.  Per frame size a square pipeline (`RequestPipeline(net, cfg, 544, 544)`, the yardstick) and a window pipeline
(`RequestPipeline.for_frames`) on the same net, both depth 4, batch 1, packed masks; a leg is `--frames` requests of
`submit_frames(FrameBatch of one frame, head_outputs)` -- val_aug, forward, nms, after_nms at the frame's size, one pinned count
read per request -- timed as frames per second of wall time with a device synchronise at the end.  The legs are alternated
`--rounds` times.  Before anything is timed the two pipelines' results are compared (ids, scores, pixel boxes, mask bits).

Also reported: where the conv launches of each engine got their plan ('table' row of tuned_gfx950.json, 'nearest' row re-derived
by plan_transfer.py, the planner's 'heuristic'): the window shapes have no rows of their own unless `YM_AUTOTUNE=1` made them.

`--accuracy`: one accuracy reading, no bar.  Trains the tools/overfit_demo.py res50 128 px recipe once, cuts its 16 pictures and their
ground truth to the top 96 rows, and scores them through the square path (96 picture rows + 32 rows of padding = 0.0) and through the
window path (96 x 128) with the device mAP (`utils.device_metrics.DeviceAPData`).

GPU_MAX_HW_QUEUES is raised to 8 before the first HIP call, as tests/conftest.py does.  Prints one JSON line; `--md PATH` also writes
the tables of profiles/rect_serving.md."""
import argparse
import collections
import gc
import json
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
sys.path[:0] = [os.path.join(REPO, 'dropin'), REPO, os.path.join(REPO, 'tools')]

FRAMES = [(480, 640), (1080, 1920)]


def summary(v):
    return {'median': float(np.median(v)), 'range': [min(v), max(v)]}


def plan_sources(engine):
    """{'table': n, 'nearest': n, 'heuristic': n, ...} over the conv launches of one engine."""
    return dict(collections.Counter(str(c.plan_source).split(':')[0] for c in engine.convs))


def same_results(a, b):
    if a[0] is None or b[0] is None:
        return a[0] is None and b[0] is None
    return all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and torch.equal(a[3].bits, b[3].bits)


def serving(args, dev):
    import bench
    from yolact_minimal_amd import rect_anchor_index, rect_window
    from yolact_minimal_amd.pipeline import RequestPipeline
    from yolact_minimal_amd.utils.frames import FrameBatch
    from yolact_minimal_amd.utils.synthetic import synth_head_outputs
    size = 544
    net, cfg = bench.build_net('res101_coco', size, dev)
    cfg.visual_thre = 0
    n_sq = len(net.anchors) // 4
    base = synth_head_outputs(n_sq, num_classes=cfg.num_classes, proto_hw=size // 4, seed=1)
    rng = np.random.default_rng(0)
    square = RequestPipeline(net, cfg, size, size, dev, depth=4, batch=1, packed_masks=True)
    out = {'square_plan_sources': plan_sources(square.engines[0]), 'frames': {}}
    warmed = False
    for h, w in FRAMES:
        hn, wn = rect_window([(h, w)], size)
        idx = rect_anchor_index(cfg, hn, wn)
        outside = torch.ones(n_sq, dtype=torch.bool)
        outside[idx] = False
        cls = base[0].clone()
        cls[0, outside] = 0
        cls[0, outside, 0] = 1
        head_sq = [t.to(dev) for t in (cls, base[1], base[2], base[3])]
        head_win = [cls[:, idx].contiguous().to(dev), base[1][:, idx].contiguous().to(dev), base[2][:, idx].contiguous().to(dev),
                    base[3][:, :hn // 4, :wn // 4].contiguous().to(dev)]
        fb = FrameBatch.from_numpy([rng.integers(0, 256, (h, w, 3)).astype(np.uint8)], dev)
        window = RequestPipeline.for_frames(net, cfg, [(h, w)], dev, depth=4, batch=1, packed_masks=True)
        assert window.window == (hn, wn)
        if not warmed:
            square.warm_up(torch.zeros(1, 3, size, size, device=dev), head_sq)
            warmed = True
        window.warm_up(torch.zeros(1, 3, hn, wn, device=dev), head_win)
        legs = {'square': (square, head_sq), 'window': (window, head_win)}

        def leg(name, n, keep=False):
            pipe, head = legs[name]
            res = []
            for _ in range(n):
                r = pipe.submit_frames(fb, head)
                if keep and r is not None:
                    res.append(r)
            tail = pipe.drain()
            return res + tail if keep else n
        first = {k: leg(k, 8, keep=True) for k in legs}
        torch.cuda.synchronize()
        equal = len(first['square']) == len(first['window']) == 8 and all(same_results(a, b) for a, b in zip(first['square'], first['window']))
        detections = int(first['window'][0][0].shape[0]) if first['window'][0][0] is not None else 0
        del first
        for k in legs:
            leg(k, args.frames)
        rows = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k in legs:
                gc.collect()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                n = leg(k, args.frames)
                torch.cuda.synchronize()
                rows[k].append(round(n / (time.perf_counter() - t0), 2))
        # the forward alone, one request at a time on the caller's stream (device time from HIP events)
        fwd = {}
        for k, (pipe, _) in legs.items():
            eng = pipe.engines[0]
            x = torch.zeros(1, 3, eng.H, eng.W, device=dev)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(10):
                eng.run(x)
            torch.cuda.synchronize()
            a.record()
            for _ in range(100):
                eng.run(x)
            b.record()
            torch.cuda.synchronize()
            fwd[k] = round(a.elapsed_time(b) / 100, 4)
        out['frames'][f'{h}x{w}'] = {'window': [hn, wn], 'detections': detections, 'results_equal': bool(equal), 'frames_per_s_rounds': rows,
                                     'frames_per_s': {k: summary(v) for k, v in rows.items()}, 'forward_alone_ms': fwd,
                                     'window_plan_sources': plan_sources(window.engines[0]),
                                     'input_rows_fraction': round(hn * wn / (size * size), 4)}
        del window, legs
        gc.collect()
    net._engines.clear()
    return out


def accuracy(dev, steps):
    """box / mask mAP of the overfit recipe's pictures cut to their top 96 rows, square path and window path."""
    import overfit_demo as od
    from yolact_minimal_amd.config import build_cfg
    from yolact_minimal_amd.modules.yolact import Yolact
    from yolact_minimal_amd.trainer import Trainer
    from yolact_minimal_amd.utils.device_metrics import DeviceAPData
    from yolact_minimal_amd.utils.output_utils import after_nms, nms
    size, cut, batch, n_images, seed = 128, 96, 8, 16, 0
    cfg = build_cfg('res50_custom', 'train', size, train_bs=batch, bs_per_gpu=batch)
    torch.manual_seed(seed)
    net = Yolact(cfg)
    tr = Trainer(net, cfg, dev, 1, dev.index or 0)
    data = od.make_dataset(n_images, size, seed)
    imgs = torch.stack([d[0] for d in data]).to(dev)
    gts, mks = [d[1].to(dev) for d in data], [d[2].to(dev) for d in data]
    order = np.random.default_rng(seed + 1)
    for _ in range(steps):
        pick = order.choice(n_images, batch, replace=False)
        tr.step(imgs[pick], [gts[i] for i in pick], [mks[i] for i in pick])
    torch.cuda.synchronize()
    net.eval()
    thres = [x / 100 for x in range(50, 100, 5)]
    nc = len(cfg.class_names)
    acc = {k: DeviceAPData(nc, thres, dev) for k in ('square', 'window')}
    kept = 0
    with torch.no_grad():
        for img, gt, masks in data:
            m = masks[:, :cut]                                   # ground truth cut like the picture; instances cut away are dropped
            keep = m.flatten(1).sum(1) > 0
            m, cls = m[keep], gt[keep, 4]
            boxes = []
            for one in m:
                ys, xs = torch.nonzero(one, as_tuple=True)
                boxes.append([xs.min().item() / size, ys.min().item() / cut, (xs.max().item() + 1) / size, (ys.max().item() + 1) / cut])
            gt_cut = torch.cat([torch.tensor(boxes, dtype=torch.float32).reshape(-1, 4), cls.reshape(-1, 1)], 1)
            kept += int(keep.sum())
            top = img[:, :cut].to(dev)
            padded = torch.zeros(1, 3, size, size, device=dev)
            padded[0, :, :cut] = top                             # the square input: picture at the top, padding = exactly 0.0 below
            for name, x, anchors, window in (('square', padded, net.anchors, False),
                                             ('window', top[None].contiguous(), net.anchors_for(cut, size, dev), True)):
                o = net(x)
                r = after_nms(*nms(o[0], o[1], o[2], o[3], anchors, cfg), cut, size, cfg, window=window)
                if r[0] is None:
                    continue
                acc[name].add(r[0], r[1], r[2], r[3], None, gt_cut.clone().to(dev), m.contiguous().to(dev), cut, size)
    res = {'recipe': f'tools/overfit_demo.py res50_custom {size} px, {n_images} pictures, batch {batch}, {steps} steps, seed {seed}',
           'cut': [cut, size], 'gt_instances_kept': kept}
    for name in acc:
        _, row_box, row_mask = acc[name].calc_map()
        res[name] = {'box_map': row_box[1], 'mask_map': row_mask[1], 'images_with_detections': acc[name].images}
    net._engines.clear()
    return res


def markdown(res):
    lines = []
    if 'serving' in res:
        s = res['serving']
        lines += ['| frame | window | input pixels | square frames/s (range) | window frames/s (range) | ratio | forward alone, square / window ms | results equal |',
                  '|---|---|---|---|---|---|---|---|']
        for key, f in s['frames'].items():
            sq, wi = f['frames_per_s']['square'], f['frames_per_s']['window']
            lines.append(f"| {key} | {f['window'][0]}x{f['window'][1]} | {f['input_rows_fraction']:.3f} | {sq['median']:.1f} ({sq['range'][0]:.1f} – {sq['range'][1]:.1f}) | "
                         f"{wi['median']:.1f} ({wi['range'][0]:.1f} – {wi['range'][1]:.1f}) | {wi['median'] / sq['median']:.3f} | "
                         f"{f['forward_alone_ms']['square']:.3f} / {f['forward_alone_ms']['window']:.3f} | {f['results_equal']} |")
        lines += ['', '| engine | conv launches by plan source |', '|---|---|', f"| square 544x544 | {s['square_plan_sources']} |"]
        for key, f in s['frames'].items():
            lines.append(f"| window {f['window'][0]}x{f['window'][1]} | {f['window_plan_sources']} |")
        lines.append('')
    if 'accuracy' in res:
        a = res['accuracy']
        lines += [f"Accuracy reading, no bar ({a['recipe']}; pictures and ground truth cut to {a['cut'][0]}x{a['cut'][1]}, "
                  f"{a['gt_instances_kept']} gt instances):", '', '| path | box mAP | mask mAP |', '|---|---|---|',
                  f"| square (128x128 input, 32 rows of padding) | {a['square']['box_map']} | {a['square']['mask_map']} |",
                  f"| window (96x128 input) | {a['window']['box_map']} | {a['window']['mask_map']} |", '']
    return '\n'.join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--frames', type=int, default=192, help='requests per pass of a leg')
    ap.add_argument('--accuracy', action='store_true', help='also train the overfit recipe and score the cut pictures on both paths')
    ap.add_argument('--accuracy-only', action='store_true')
    ap.add_argument('--steps', type=int, default=600, help='training steps of the accuracy reading')
    ap.add_argument('--md', default=None, help='also write the result tables as markdown to this path')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'rect_serving_bench measures on the GPU; there is nothing to measure without one'
    dev = torch.device('cuda:0')
    result = {'rounds': args.rounds, 'frames_per_pass': args.frames, 'GPU_MAX_HW_QUEUES': os.environ.get('GPU_MAX_HW_QUEUES'),
              'YM_AUTOTUNE': os.environ.get('YM_AUTOTUNE')}
    if not args.accuracy_only:
        result['serving'] = serving(args, dev)
        print(json.dumps({'serving': result['serving']}), file=sys.stderr, flush=True)      # (kept should a later stage fail)
    if args.accuracy or args.accuracy_only:
        result['accuracy'] = accuracy(dev, args.steps)
    if args.md:
        with open(args.md, 'w') as fh:
            fh.write(markdown(result))
    print(json.dumps(result))


if __name__ == '__main__':
    main()
