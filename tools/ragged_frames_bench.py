#!/usr/bin/env python3
"""What the two ends of a mixed-size request cost per image and in one batched call: res101_coco at 544 px (`bench.build_net`), 8 uint8
frames whose sizes cycle through the six of tools/ragged_eval_bench.py (480x640, 640x480, 427x640, 375x500, 500x333, 640x640), 100
detections per frame from the dense synthetic head outputs (`utils.synthetic.synth_head_outputs`, seed 1, as bench.py).

Every pair is alternated `--rounds` times in ONE process; the yardstick of each is the per-image path as it was before the batched
stages existed, in the same process.  Results of the two sides are compared exactly before anything is timed.
  (a) eight `val_aug` calls + `torch.cat`            against  one `val_aug_batch` over a `FrameBatch`
  (b) eight `draw_img` calls (dense and packed masks) against  one ragged `draw_batch`
      device time from HIP events and wall time, each over windows of at least `--window-ms` of back-to-back calls
  (c) the whole chain, uint8 frames in -> drawn uint8 frames out, packed masks, `--frames` frames per pass, frames per second of wall
      time with a device synchronise at the end:
        b1_d4  batch-1 requests, four in flight: `val_aug` per frame on the caller's stream, `submit(out_hw=(h, w), consumer=...)`
               whose consumer is the per-image draw stage (`draw_batch` on the one frame as a [1, H, W, 3] tensor: it takes the count
               and `cfg.visual_thre` on the device, so nothing is read on the host)
        b8_d2  `submit_frames(FrameBatch, draw=True)`, requests of 8 frames, two in flight
GPU_MAX_HW_QUEUES is raised to 8 before the first HIP call, as tests/conftest.py does.  Prints one JSON line; `--md PATH` also writes
the tables of profiles/ragged_frames.md."""
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
BATCH = 8


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


def markdown(res):
    def cell(s, scale=1.0, digits=1):
        return f"{s['median'] * scale:.{digits}f} ({s['range'][0] * scale:.{digits}f} – {s['range'][1] * scale:.{digits}f})"
    st, ch = res['stages_ms'], res['chain_frames_per_s']
    lines = ['| 8 frames, 100 detections each | calls per window | device µs per call (range) | wall µs per call (range) |', '|---|---|---|---|']
    for key, label in (('eight_val_aug_cat', 'eight `val_aug` + `torch.cat` (yardstick)'), ('val_aug_batch', 'one `val_aug_batch`'),
                       ('eight_draw_img_dense', 'eight `draw_img`, dense masks (yardstick)'), ('draw_batch_dense', 'one ragged `draw_batch`, dense'),
                       ('eight_draw_img_packed', 'eight `draw_img`, packed masks (yardstick)'), ('draw_batch_packed', 'one ragged `draw_batch`, packed')):
        lines.append(f"| {label} | {res['calls_per_window'][key]} | {cell(st[key + '_device_ms'], 1e3)} | {cell(st[key + '_wall_ms'], 1e3)} |")
    lines += ['', '| whole chain, packed masks | frames/s median | range |', '|---|---|---|',
              f"| batch-1 requests, 4 in flight, per-image `val_aug` and draw stage (yardstick) | {ch['b1_d4']['median']:.1f} | "
              f"{ch['b1_d4']['range'][0]:.1f} – {ch['b1_d4']['range'][1]:.1f} |",
              f"| `submit_frames(draw=True)`, requests of 8 frames, 2 in flight | {ch['b8_d2']['median']:.1f} | "
              f"{ch['b8_d2']['range'][0]:.1f} – {ch['b8_d2']['range'][1]:.1f} |", '']
    return '\n'.join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--frames', type=int, default=192, help='frames per pass of a chain leg')
    ap.add_argument('--window-ms', type=float, default=300.0, help='least wall time of a timed window of calls')
    ap.add_argument('--md', default=None, help='also write the result tables as markdown to this path')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'ragged_frames_bench measures on the GPU; there is nothing to measure without one'
    assert args.frames % BATCH == 0
    import bench
    from yolact_minimal_amd.pipeline import RequestPipeline
    from yolact_minimal_amd.utils.augmentations import val_aug, val_aug_batch
    from yolact_minimal_amd.utils.draw import draw_batch, draw_img
    from yolact_minimal_amd.utils.frames import FrameBatch
    from yolact_minimal_amd.utils.output_utils import BatchDetections, after_nms_batch, nms_batch
    from yolact_minimal_amd.utils.synthetic import synth_head_outputs
    dev = torch.device('cuda:0')
    size = 544
    net, cfg = bench.build_net('res101_coco', size, dev)
    for name in ('hide_mask', 'hide_bbox', 'hide_score', 'real_time', 'cutout'):
        setattr(cfg, name, False)
    cfg.visual_thre = 0
    sizes = [SIZES[i % len(SIZES)] for i in range(BATCH)]
    hs, ws = [s[0] for s in sizes], [s[1] for s in sizes]
    rng = np.random.default_rng(0)
    fb = FrameBatch.from_numpy([rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes], dev)
    singles = [f.clone() for f in fb.frames]                       # the per-image path's frames: separate tensors, as a reader makes them
    head1 = [t.to(dev) for t in synth_head_outputs(len(net.anchors) // 4, num_classes=cfg.num_classes, proto_hw=size // 4, seed=1)]
    head8 = [t.expand(BATCH, *t.shape[1:]).contiguous() for t in head1]
    anchors = torch.tensor(net.anchors, dtype=torch.float32).reshape(-1, 4).to(dev)

    # ---- (a) ----
    def eight_val_aug():
        return torch.cat([val_aug(f, size)[None] for f in singles])

    def one_val_aug_batch():
        return val_aug_batch(fb, size)
    assert torch.equal(eight_val_aug().view(torch.int32), one_val_aug_batch().view(torch.int32))

    # ---- (b) ----
    dets = nms_batch(*head8, anchors, cfg)
    counts = dets.counts.tolist()
    fns = {'eight_val_aug_cat': eight_val_aug, 'val_aug_batch': one_val_aug_batch}
    keep = []
    for packed in (False, True):
        work = BatchDetections(dets.counts, dets.ids, dets.scores, dets.boxes.clone(), dets.coefs, dets.proto)
        padded = after_nms_batch(work, hs, ws, cfg, sync=False, packed=packed)
        ids, scores, boxes, masks, _ = padded
        rows = [(ids[b, :n], scores[b, :n], boxes[b, :n], masks[b][:n]) for b, n in enumerate(counts)]
        keep.append((padded, rows))

        def eight_draw_img(rows=rows):
            return [draw_img(*r, f, cfg) for r, f in zip(rows, singles)]

        def one_draw_batch(padded=padded):
            return draw_batch(padded, fb, cfg)
        for a, b in zip(eight_draw_img(), one_draw_batch().frames):
            assert torch.equal(a, b)
        tag = 'packed' if packed else 'dense'
        fns['eight_draw_img_' + tag], fns['draw_batch_' + tag] = eight_draw_img, one_draw_batch
    calls = {k: calls_for(f, args.window_ms) for k, f in fns.items()}
    stage = {f'{k}_{unit}_ms': [] for k in fns for unit in ('device', 'wall')}
    for _ in range(args.rounds):
        for k, f in fns.items():
            d, w_ = timed(f, calls[k])
            stage[k + '_device_ms'].append(round(d, 5))
            stage[k + '_wall_ms'].append(round(w_, 5))
    del keep, fns

    # ---- (c) ----
    img1, img8 = torch.zeros(1, 3, size, size, device=dev), torch.zeros(BATCH, 3, size, size, device=dev)
    pipe1 = RequestPipeline(net, cfg, size, size, dev, depth=4, batch=1, packed_masks=True)
    pipe1.warm_up(img1, head1)
    pipe8 = RequestPipeline(net, cfg, size, size, dev, depth=2, batch=BATCH, packed_masks=True)
    pipe8.warm_up(img8, head8)

    def leg_b1_d4(n):
        out = []
        for i in range(n):
            f = singles[i % BATCH]
            x = val_aug(f, size)[None]
            x.record_stream(pipe1.streams[pipe1.submitted % pipe1.depth])       # (made here, read by the slot's stream)
            r = pipe1.submit(x, head1, out_hw=sizes[i % BATCH], consumer=lambda *r, f=f: draw_batch(r, f[None], cfg))
            if r is not None:
                out.append(r[0])
        return out + [r[0] for r in pipe1.drain()]

    def leg_b8_d2(n):
        out = []
        for _ in range(n // BATCH):
            r = pipe8.submit_frames(fb, head8, draw=True)
            if r is not None:
                out += r.frames
        for r in pipe8.drain():
            out += r.frames
        return out
    legs = {'b1_d4': leg_b1_d4, 'b8_d2': leg_b8_d2}
    first = {k: f(2 * BATCH) for k, f in legs.items()}             # warm-up, and: do the two chains draw the same frames?
    torch.cuda.synchronize()
    # (a batch-8 forward reads other plan rows than a batch-1 forward, but the detections here come from the same synthetic head
    # outputs, so the drawn frames must agree exactly)
    assert len(first['b1_d4']) == len(first['b8_d2']) == 2 * BATCH
    chains_equal = all(torch.equal(a, b) for a, b in zip(first['b1_d4'], first['b8_d2']))
    del first
    rows = {k: [] for k in legs}
    for k, f in legs.items():
        f(args.frames)
    for _ in range(args.rounds):
        for k, f in legs.items():
            gc.collect()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = len(f(args.frames))
            torch.cuda.synchronize()
            rows[k].append(round(n / (time.perf_counter() - t0), 2))
    result = {'workload': f'res101_coco {size} px, {BATCH} frames cycling through ' + ', '.join(f'{h}x{w}' for h, w in SIZES) +
                          ', 100 detections each (dense synthetic head outputs)', 'detections': counts, 'rounds': args.rounds,
              'window_ms': args.window_ms, 'GPU_MAX_HW_QUEUES': os.environ.get('GPU_MAX_HW_QUEUES'), 'calls_per_window': calls,
              'stages_ms': summary(stage), 'frames_per_pass': args.frames, 'chain_frames_per_s_rounds': rows,
              'chain_frames_per_s': summary(rows), 'chains_draw_equal_frames': chains_equal}
    if args.md:
        with open(args.md, 'w') as fh:
            fh.write(markdown(result))
    net._engines.clear()
    print(json.dumps(result))


if __name__ == '__main__':
    main()
