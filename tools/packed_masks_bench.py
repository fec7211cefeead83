#!/usr/bin/env python3
"""What bit-packed masks (`after_nms(..., packed=True)`, utils/packed_masks.py) cost and save per stage, against the dense float32
path on the same detections: the `dense544` head outputs post-processed to 480 x 640, 100 and 10 detections.

Stages: after_nms, mask_iou (15 ground-truth masks), prep_metrics, rle_encode, draw_img (device frame), the host download of the
masks (`.cpu().numpy()` against `PackedMasks.numpy()`), and `dropin/reference_loops.eval_loop` in its three branches (img/s).
The baseline is the dense path of the same build, measured in the same process: dense and packed are alternated `--rounds` times;
per stage a window holds as many calls as fill `--window-ms` (at least `--iters`), timed with HIP events (device ms per call) and
with the host clock around the synchronised window (wall ms per call).  Prints one JSON line with every round, the medians, the
spread (min / max) and the mask bytes each stage moves.  `--profile` runs a fixed number of calls of every stage, dense then
packed, for `rocprofv3 --kernel-trace --stats -- python tools/packed_masks_bench.py --profile` + `tools/prof_summary.py`."""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, 'dropin'), REPO]
from oracle import yolact_ref as R  # noqa: E402
from yolact_minimal_amd.config import build_cfg  # noqa: E402
from yolact_minimal_amd.utils.box_utils import mask_iou  # noqa: E402
from yolact_minimal_amd.utils.common_utils import APDataObject, prep_metrics, rle_encode  # noqa: E402
from yolact_minimal_amd.utils.output_utils import PackedMasks, nms, after_nms, draw_img  # noqa: E402

H, W = 480, 640
G = 15                            # ground-truth masks per image
WQ = (W + 63) // 64
HBM_PEAK_MEASURED = 6.29e12      # bytes/s, float4 copy on the MI355X (8.0e12 is the data-sheet figure)
THRES = [x / 100 for x in range(50, 100, 5)]


def timed(fn, iters):
    """(device ms, wall ms) per call of a synchronised window of `iters` calls.  The cyclic garbage collector runs between the
    windows, not inside them: prep_metrics builds 1600 AP cells per call, and a full collection (tens of ms with torch loaded)
    that happens to fall into a 150 ms window is a property of the window, not of the stage."""
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


def ground_truth(dev):
    rng = np.random.default_rng(5)
    gt = np.zeros((G, 5), dtype=np.float32)
    masks = np.zeros((G, H, W), dtype=np.uint8)
    for j in range(G):
        x1, y1 = rng.integers(0, W - 40), rng.integers(0, H - 40)
        x2, y2 = rng.integers(x1 + 20, W), rng.integers(y1 + 20, H)
        gt[j] = (x1 / W, y1 / H, x2 / W, y2 / H, rng.integers(0, 80))
        masks[j, y1:y2, x1:x2] = 1
    return torch.from_numpy(gt).to(dev), torch.from_numpy(masks).to(dev)


def stages(n, dev):
    """{stage: (dense fn, packed fn)}, {stage: (dense mask bytes, packed mask bytes)} on n detections"""
    cfg = build_cfg('res101_coco', 'val', 544)
    cfg.max_detections = n
    for name in ('hide_mask', 'hide_bbox', 'hide_score', 'real_time', 'cutout'):
        setattr(cfg, name, False)
    cls, box, coef, proto = (t.to(dev) for t in R.synth_head_outputs(18525, seed=1))
    anchors = R.anchors_for(544, [24, 48, 96, 192, 384]).to(dev)
    r = nms(cls, box, coef, proto, anchors, cfg)
    assert r[0] is not None and r[0].numel() == n, f'wanted {n} detections'
    ids, scores, boxes, masks = after_nms(r[0], r[1], r[2].clone(), r[3], r[4], H, W, cfg)
    _, _, pboxes, pm = after_nms(r[0], r[1], r[2].clone(), r[3], r[4], H, W, cfg, packed=True)
    assert torch.equal(pboxes, boxes) and torch.equal(pm.dense(), masks), 'the packed path must compute what the dense path computes'
    gt, gt_masks = ground_truth(dev)
    gt_f32, gt_pm = gt_masks.float(), PackedMasks.pack(gt_masks)
    frame = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (H, W, 3)).astype(np.uint8)).to(dev)
    ids_l, scores_l = [int(i) for i in ids.cpu()], [float(s) for s in scores.cpu()]
    box_in = r[2].clone()

    def new_ap():
        return {k: [[APDataObject() for _ in range(80)] for _ in THRES] for k in ('box', 'mask')}

    def post(packed):
        box_in.copy_(r[2])                                              # (after_nms scales its boxes in place)
        return after_nms(r[0], r[1], box_in, r[3], r[4], H, W, cfg, packed=packed)

    fns = {
        'after_nms': (lambda: post(False), lambda: post(True)),
        'mask_iou': (lambda: mask_iou(masks.reshape(n, -1), gt_f32.reshape(G, -1), to_cpu=False), lambda: mask_iou(pm, gt_pm, to_cpu=False)),
        'prep_metrics': (lambda: prep_metrics(new_ap(), ids_l, scores_l, boxes, masks, gt.clone(), gt_f32, H, W, THRES),
                         lambda: prep_metrics(new_ap(), ids_l, scores_l, boxes, pm, gt.clone(), gt_pm, H, W, THRES)),
        'rle_encode': (lambda: rle_encode(masks), lambda: rle_encode(pm)),
        'draw_img': (lambda: draw_img(ids, scores, boxes, masks, frame, cfg), lambda: draw_img(ids, scores, boxes, pm, frame, cfg)),
        'download': (lambda: masks.cpu().numpy(), lambda: pm.numpy()),
    }
    d, p, f = n * H * W * 4, n * H * WQ * 8, H * W * 3
    gd, gp = G * H * W * 4, G * H * WQ * 8
    mask_bytes = {'after_nms': (d, p), 'mask_iou': (d + gd, p + gp), 'prep_metrics': (d + gd, p + gp), 'rle_encode': (2 * d, 2 * p),
                  'draw_img': (d + 2 * f, p + 2 * f), 'download': (d, p)}
    return fns, mask_bytes


def eval_loops(args, dev):
    """img/s of the reference's eval loop (dropin/reference_loops.py) with dense and packed masks, per branch"""
    import bench
    import reference_loops as L
    from yolact_minimal_amd.utils.synthetic import synth_eval_case
    net, cfg, img = bench.detecting_net('res101_coco', 544, dev)
    _, _, _, _, gt, gt_masks, _, _ = synth_eval_case(1, 40, G, H, W, 10)
    images = args.eval_images

    def loader():
        return [(img, gt.clone(), gt_masks, H, W) for _ in range(images)]

    out = {}
    for name, api in (('prep_metrics', False), ('coco_api', True), ('coco_api_device_rle', 'device')):
        rows = {'dense': [], 'packed': []}
        for packed in (False, True):
            L.eval_loop(net, cfg, loader()[:2], coco_api=api, packed_masks=packed)                  # warm-up
        for _ in range(args.rounds):
            for key, packed in (('dense', False), ('packed', True)):
                _, _, seen, sec = L.eval_loop(net, cfg, loader(), coco_api=api, packed_masks=packed)
                rows[key].append(round(seen / sec, 2))
        out[name] = dict(rows, median={k: float(np.median(v)) for k, v in rows.items()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--window-ms', type=float, default=150.0)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--profile', action='store_true')
    ap.add_argument('--dets', default='100,10', help='detection counts, comma separated')
    ap.add_argument('--eval-images', type=int, default=24, help='images per eval_loop pass (0: skip the loops)')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'packed_masks_bench measures on the GPU; there is nothing to measure without one'
    gc.disable()
    dev = torch.device('cuda:0')
    result = {'frame': [H, W], 'gt_masks': G, 'window_ms': args.window_ms, 'rounds': args.rounds, 'unit': 'ms per call',
              'hbm_peak_measured_bytes_per_s': HBM_PEAK_MEASURED, 'cases': {}}
    for n in (int(v) for v in args.dets.split(',')):
        fns, mask_bytes = stages(n, dev)
        case = result['cases'][str(n)] = {}
        for stage, pair in fns.items():
            if args.profile:
                for fn in pair:
                    for _ in range(args.warmup + args.iters):
                        fn()
                torch.cuda.synchronize()
                case[stage] = {'mask_bytes': dict(zip(('dense', 'packed'), mask_bytes[stage])), 'calls_each': args.warmup + args.iters}
                continue
            iters = []
            for fn in pair:
                for _ in range(args.warmup):
                    fn()
                iters.append(max(args.iters, int(args.window_ms / max(timed(fn, args.iters)[1], 1e-3)) + 1))
            rows = {'dense_device': [], 'dense_wall': [], 'packed_device': [], 'packed_wall': []}
            for _ in range(args.rounds):
                for key, fn, it in (('dense', pair[0], iters[0]), ('packed', pair[1], iters[1])):
                    dev_ms, wall_ms = timed(fn, it)
                    rows[key + '_device'].append(round(dev_ms, 4))
                    rows[key + '_wall'].append(round(wall_ms, 4))
            case[stage] = dict(rows, calls_per_window=iters, mask_bytes=dict(zip(('dense', 'packed'), mask_bytes[stage])),
                               median={k: float(np.median(v)) for k, v in rows.items()},
                               spread={k: [min(v), max(v)] for k, v in rows.items()})
    if args.eval_images > 0 and not args.profile:
        gc.enable()                                  # (the loops run as a user runs them)
        result['eval_loop_img_per_s'] = eval_loops(args, dev)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
