#!/usr/bin/env python3
"""What drawing the detections costs in the detect loop, old route against new, on the same `after_nms` tensors at 480 x 640.

  baseline  the first statement of the reference's draw_img alone (`utils/output_utils.py:331-335`): the four `.cpu().numpy()`
            downloads of ids, scores, boxes and the n x H x W float32 masks.  A LOWER bound of the host route, which then still
            blends and draws with cv2.
  new       `draw_img` with a numpy frame in and a numpy frame out: one upload, the kernels of csrc/draw.hip, one download.
  device    `draw_img` with a device frame in and out (the kernels and their launch path only), for information.

Device events around a synchronised window, after a warm-up; the versions are alternated `--rounds` times in one process.  A
window holds as many calls as fill `--window-ms` (at least `--iters`): a window of a few milliseconds measures the host's scheduler
as much as the work.  Prints one JSON line.  `--profile` runs only the device-frame path (for `rocprofv3 --kernel-trace --stats -- python
tools/draw_bench.py --profile --dets 100`, then `tools/prof_summary.py` on the result) and prints the mask bytes a call reads, to turn the kernel time into achieved bandwidth."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import yolact_ref as R  # noqa: E402
from yolact_minimal_amd.config import build_cfg  # noqa: E402
from yolact_minimal_amd.utils.output_utils import nms, after_nms, draw_img  # noqa: E402

H, W = 480, 640
HBM_PEAK_MEASURED = 6.29e12      # bytes/s, float4 copy on the MI355X (8.0e12 is the data-sheet figure)


def detections(n, dev):
    cfg = build_cfg('res101_coco', 'val', 544)
    cfg.max_detections = n
    for name in ('hide_mask', 'hide_bbox', 'hide_score', 'real_time', 'cutout'):
        setattr(cfg, name, False)
    cls, box, coef, proto = (t.to(dev) for t in R.synth_head_outputs(18525, seed=1))
    anchors = R.anchors_for(544, [24, 48, 96, 192, 384]).to(dev)
    r = nms(cls, box, coef, proto, anchors, cfg)
    out = after_nms(r[0], r[1], r[2], r[3], r[4], H, W, cfg)
    assert out[0] is not None and out[0].numel() == n, f'wanted {n} detections'
    return cfg, out


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters           # ms per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--window-ms', type=float, default=250.0)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--profile', action='store_true')
    ap.add_argument('--dets', default='100,10', help='detection counts, comma separated')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'draw_bench measures on the GPU; there is nothing to measure without one'
    dev = torch.device('cuda:0')
    frame = np.random.default_rng(0).integers(0, 256, (H, W, 3)).astype(np.uint8)
    frame_dev = torch.from_numpy(frame).to(dev)
    result = {'frame': [H, W], 'window_ms': args.window_ms, 'rounds': args.rounds, 'unit': 'ms per call', 'cases': {}}
    for n in (int(v) for v in args.dets.split(',')):
        cfg, (ids, scores, boxes, masks) = detections(n, dev)
        mask_bytes = n * H * W * 4

        def baseline():
            return ids.cpu().numpy(), scores.cpu().numpy(), boxes.cpu().numpy(), masks.cpu().numpy()

        def new():
            return draw_img(ids, scores, boxes, masks, frame, cfg)

        def device():
            return draw_img(ids, scores, boxes, masks, frame_dev, cfg)

        if args.profile:
            for _ in range(args.warmup + args.iters):
                device()
            torch.cuda.synchronize()
            result['cases'][str(n)] = {'mask_bytes_read_per_call': mask_bytes, 'calls': args.warmup + args.iters,
                                       'hbm_peak_measured_bytes_per_s': HBM_PEAK_MEASURED}
            continue
        iters = {}
        for fn in (baseline, new, device):
            for _ in range(args.warmup):
                fn()
            iters[fn.__name__] = max(args.iters, int(args.window_ms / timed(fn, args.iters)) + 1)
        rows = {'baseline': [], 'new': [], 'device': []}
        for _ in range(args.rounds):
            for name, fn in (('baseline', baseline), ('new', new), ('device', device)):
                rows[name].append(round(timed(fn, iters[name]), 4))
        result['cases'][str(n)] = dict(
            rows, calls_per_window=iters, new_below_baseline_in_every_round=all(a < b for a, b in zip(rows['new'], rows['baseline'])),
            pcie_bytes_per_frame={'baseline': mask_bytes + n * (8 + 4 + 16), 'new': 2 * H * W * 3},
            median={k: float(np.median(v)) for k, v in rows.items()})
    print(json.dumps(result))


if __name__ == '__main__':
    main()
