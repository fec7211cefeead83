#!/usr/bin/env python3
"""Training step time (Trainer.step: forward + loss + backward + SGD, one GPU) at another `--img_size` / batch, under whatever plan
source the environment selects (`YM_TUNED_NEAREST=0`: shapes without a row run on the planner heuristic; default: on the row
of the nearest tuned shape, plan_transfer.py; `YM_TUNED_PATH`: a candidate table).  One JSON line.
  python tools/train_size_bench.py --cfg res101_coco --size 416 --batch 8
`--window HN WN`: window training (utils/rect.py) against the square step, ONE process, ONE trainer (the image shape is the switch):
the same batch as `[B, 3, S, S]` and cut to `[B, 3, HN, WN]`, the two legs alternated `--rounds` times after a warm-up of both, each
round `--steps` steps between two device synchronisations.  Reports per leg the median and the range of the rounds and the ratio
of the medians.  The window shapes have no rows in the tuned table: they run on plans transferred from the nearest tuned shapes.
  python tools/train_size_bench.py --cfg res101_coco --size 544 --batch 8 --window 416 544"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def window_bench(cfg_name, size, batch, window, steps, rounds, dev):
    from yolact_minimal_amd.config import build_cfg
    from yolact_minimal_amd.modules.yolact import Yolact
    from yolact_minimal_amd.trainer import Trainer
    from yolact_minimal_amd.utils.synthetic import synth_targets
    hn, wn = window
    cfg = build_cfg(cfg_name, 'train', size, train_bs=batch, bs_per_gpu=batch)
    torch.manual_seed(0)
    net = Yolact(cfg)
    tr = Trainer(net, cfg, dev, 1, dev.index or 0)
    img = torch.randn(batch, 3, size, size, generator=torch.Generator().manual_seed(100)).to(dev)
    boxes, masks = synth_targets(batch, size, seed=0)
    boxes = [b.to(dev) for b in boxes]
    legs = {'square': (img, [m.to(dev) for m in masks]),
            'window': (img[:, :, :hn, :wn].contiguous(), [m[:, :hn, :wn].contiguous().to(dev) for m in masks])}
    losses = {}
    for name, (x, m) in legs.items():                       # warm-up: plans, workspaces, allocator
        for _ in range(3):
            losses[name] = tr.step(x, boxes, m)
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    for _ in range(rounds):
        for name, (x, m) in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                losses[name] = tr.step(x, boxes, m)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / steps * 1e3)
    out = {}
    for name, v in ms.items():
        s = sorted(v)
        out[name] = dict(ms_per_step_median=round(s[len(s) // 2], 2), ms_per_step_range=[round(s[0], 2), round(s[-1], 2)],
                         rounds=[round(t, 2) for t in v], last_losses=[round(float(l.detach()), 4) for l in losses[name]],
                         finite=all(bool(torch.isfinite(l)) for l in losses[name]))
    ratios = sorted(w / s for w, s in zip(ms['window'], ms['square']))
    out['ratio_window_to_square'] = dict(of_medians=round(out['window']['ms_per_step_median'] / out['square']['ms_per_step_median'], 4),
                                         per_round_range=[round(ratios[0], 4), round(ratios[-1], 4)])
    out['input_pixel_ratio'] = round(hn * wn / (size * size), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cfg', default='res101_coco')
    ap.add_argument('--size', type=int, default=416)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--tag', default='')
    ap.add_argument('--window', type=int, nargs=2, metavar=('HN', 'WN'), default=None,
                    help='time the window step [B, 3, HN, WN] against the square step at --size, alternated in this process')
    ap.add_argument('--rounds', type=int, default=5, help='with --window: alternations of the two legs')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    if args.window is not None:
        r = window_bench(args.cfg, args.size, args.batch, tuple(args.window), args.steps, args.rounds, dev)
        print(json.dumps(dict(tag=args.tag, cfg=args.cfg, size=args.size, batch=args.batch, window_shape=list(args.window), steps=args.steps, **r)),
              flush=True)
        return
    r = bench.train_bench(args.cfg, args.size, args.batch, args.steps, 3, 1, 0, dev, lambda: None)
    print(json.dumps(dict(tag=args.tag, cfg=args.cfg, size=args.size, batch=args.batch, ms_per_step=r['ms_per_step'], img_s=r['img_s'],
                          losses=r.get('last_losses'), finite=r.get('finite'))), flush=True)


if __name__ == '__main__':
    main()
