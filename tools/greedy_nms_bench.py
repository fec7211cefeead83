#!/usr/bin/env python3
"""What `--traditional_nms` costs through `nms()` (`ym_detect_greedy_nms`, the batch of one plus the host read of the count) and through
`nms_batch` with `cfg.traditional_nms` (`ym_detect_greedy_nms_batch`: suppression in chunks of 64 sorted candidates), on the 544 px
geometry: `synth_head_outputs(18525, seed=1, bg_bias=4.0)` (dense, up to 879 candidates per class) and `seed=2, bg_bias=9.0`
(sparse, up to 279).

One process.  Per input the variants are alternated `--rounds` times after `--warmup` calls each; a window holds as many calls as
fill `--window-ms` (at least `--iters`); the figure is HIP-event time per call around the window.  Variants:
  nms_greedy        `nms()` with the flag: the single-image entry plus its one host read of the count, as a caller gets it
  batch_greedy_b1 / _b8   `nms_batch` with the flag, 1 and 8 images (8 copies of the input)
  batch_fast_b1 / _b8     `nms_batch` without it (fast_nms), for scale
Before anything is timed the batched results are compared with `nms()`'s, bit for bit.  Prints one JSON line (every round, medians,
min / max, workspace bytes per image) and writes the table to `--out`.  `profiles/greedy_nms_batch_544.md` is the record of the
retired one-barrier-per-candidate kernels, `profiles/greedy_nms_one_path_544.md` of their removal."""
import argparse
import ctypes
import gc
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO]
from oracle import yolact_ref as R  # noqa: E402
from yolact_minimal_amd import hip  # noqa: E402
from yolact_minimal_amd.config import build_cfg  # noqa: E402
from yolact_minimal_amd.utils.output_utils import nms, nms_batch  # noqa: E402

INPUTS = (('dense544', dict(seed=1, bg_bias=4.0)), ('sparse544', dict(seed=2, bg_bias=9.0)))
ORDER = ('nms_greedy', 'batch_greedy_b1', 'batch_greedy_b8', 'batch_fast_b1', 'batch_fast_b8')


def timed(fn, iters):
    """(device ms, wall ms) per call of a synchronised window of `iters` calls"""
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


def nms_cfg(cfg, n_anchors, n_classes):
    return hip.NmsCfg(n_anchors, n_classes, 32, int(cfg.top_k), int(cfg.max_detections), float(cfg.nms_score_thre),
                      float(cfg.nms_iou_thre), float(cfg.img_size))


def variants(head, anchors, dev):
    greedy, fast = build_cfg('res101_coco', 'val', 544), build_cfg('res101_coco', 'val', 544)
    greedy.traditional_nms, fast.traditional_nms = True, False
    one = [t.to(dev) for t in head]
    eight = [t.expand(8, *t.shape[1:]).contiguous() for t in one]
    a = anchors.to(dev)
    # the batched path computes what nms() computes
    want = nms(*one, a, greedy)
    for batch in (one, eight):
        for got in nms_batch(*batch, a, greedy).split():
            assert all(torch.equal(x, y) for x, y in zip(got[:4], want[:4])), 'nms_batch(traditional_nms) differs from nms()'
    ncfg = nms_cfg(greedy, one[0].shape[1], one[0].shape[2])
    fns = {'nms_greedy': lambda: nms(*one, a, greedy),
           'batch_greedy_b1': lambda: nms_batch(*one, a, greedy), 'batch_greedy_b8': lambda: nms_batch(*eight, a, greedy),
           'batch_fast_b1': lambda: nms_batch(*one, a, fast), 'batch_fast_b8': lambda: nms_batch(*eight, a, fast)}
    ws_bytes = int(hip.lib().ym_nms_workspace_bytes(ctypes.byref(ncfg)))
    assert ws_bytes == int(hip.lib().ym_greedy_nms_batch_workspace_bytes(ctypes.byref(ncfg), 1))
    return fns, ws_bytes, int(want[0].numel())


def write_table(path, result, argv):
    lines = ['# Greedy NMS (`--traditional_nms`) through `nms()` and `nms_batch`, 544 px', '',
             f'`{argv}` on one MI355X.  One process; per input the variants are alternated {result["rounds"]} times after '
             f'{result["warmup"]} warm-up calls each; a window holds as many calls as fill {result["window_ms"]:g} ms (at least '
             f'{result["iters"]}); HIP-event time per call around the window, median with (min–max) of the windows.  `nms_greedy` is '
             '`nms()` with `cfg.traditional_nms` (the single-image entry `ym_detect_greedy_nms`, a batch of one, plus its host read of '
             'the count), `batch_greedy_b*` `nms_batch` with the flag (`ym_detect_greedy_nms_batch`) on 1 and 8 images, `batch_fast_b*` '
             '`nms_batch` without it.  '
             'The batched results were compared with `nms()`\'s bit for bit before timing.', '']
    lines += [f'Workspace per image (N = 18525, C = 81), either greedy entry: {result["workspace_bytes_per_image"]} bytes.', '']
    for name, case in result['cases'].items():
        lines += [f'### {name} ({case["detections"]} detections)', '', '| variant | ms per call (min–max) | ms per image | calls per window |',
                  '|---|---|---|---|']
        for v in ORDER:
            imgs = 8 if v.endswith('_b8') else 1
            lo, hi = case['spread'][v]
            lines.append(f'| {v} | {case["median"][v]:.4f} ({lo:.4f}–{hi:.4f}) | {case["median"][v] / imgs:.4f} | {case["calls_per_window"][v]} |')
        r = case['ratios']
        lines += ['', f'nms_greedy / batch_greedy_b1 = {r["nms_greedy_over_batch_b1"]:.2f}, batch_greedy_b8 per image = '
                      f'{r["batch_b8_ms_per_image"]:.4f} ms.', '']
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        f.write('\n'.join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--window-ms', type=float, default=150.0)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'greedy_nms_544.md'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'greedy_nms_bench measures on the GPU; there is nothing to measure without one'
    gc.disable()
    dev = torch.device('cuda:0')
    anchors = R.anchors_for(544, [24, 48, 96, 192, 384])
    result = {'unit': 'ms per call (HIP events)', 'rounds': args.rounds, 'warmup': args.warmup, 'window_ms': args.window_ms,
              'iters': args.iters, 'cases': {}}
    for name, kw in INPUTS:
        fns, ws_bytes, n_det = variants(R.synth_head_outputs(18525, **kw), anchors, dev)
        result['workspace_bytes_per_image'] = ws_bytes
        iters = {}
        for v in ORDER:
            for _ in range(args.warmup):
                fns[v]()
            iters[v] = max(args.iters, int(args.window_ms / max(timed(fns[v], args.iters)[1], 1e-3)) + 1)
        rows = {v: [] for v in ORDER}
        for _ in range(args.rounds):
            for v in ORDER:
                rows[v].append(round(timed(fns[v], iters[v])[0], 5))
        med = {v: float(np.median(r)) for v, r in rows.items()}
        result['cases'][name] = dict(detections=n_det, rows=rows, calls_per_window=iters, median=med,
                                     spread={v: [min(r), max(r)] for v, r in rows.items()},
                                     ratios={'nms_greedy_over_batch_b1': med['nms_greedy'] / med['batch_greedy_b1'],
                                             'batch_b8_ms_per_image': med['batch_greedy_b8'] / 8})
    argv = 'python tools/greedy_nms_bench.py' + ''.join(f' --{k.replace("_", "-")} {getattr(args, k):g}' for k in ('iters', 'rounds', 'window_ms', 'warmup'))
    write_table(args.out, result, argv)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
