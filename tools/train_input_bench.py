#!/usr/bin/env python3
"""What a training batch's augmentation costs per sample and in one batched call: 8 synthetic uint8 samples whose sizes cycle through
480x640, 640x480, 427x640, 375x500, 500x333 and 640x640, 6 instance masks each (`utils.synthetic.synth_sample`), augmented to 544 px.
The plans are drawn once from a fixed seed and reused by both paths; the yardstick of each pair is the per-sample path in the same
process, and the two sides are compared exactly before anything is timed.  Every pair is alternated `--rounds` times in ONE process.
  (a) pixel half, images uploaded from host memory, masks already on the device (where the rasteriser leaves them):
        eight uploads + eight `apply_train_aug` + the `torch.stack` of `train_collate`
        against one `FrameBatch.from_numpy` + one `apply_train_aug_batch`
  (b) the loader's consumer half on a dataset written by `oracle.coco_ref.write_synth_dataset` (8 JPEG images of the same six sizes,
      polygon annotations), records read once outside the timed region:
        eight `COCODetection.finish` + `train_collate`   against   one `COCODetection.finish_batch`
  (c) the rasteriser alone on the same records (polygon annotations, masks born on the device):
        eight `COCO.annsToMasks`   against   one `COCO.annsToMasksBatch` (one packed upload, one `ym_ann_to_mask_ragged` launch)
  (d) with `--against OTHER.so` (another build of the library, e.g. the parent commit's): `ym_poly_to_mask` on one 480x640 image with 7
      polygon annotations through both libraries in this one process, outputs compared first, `--against-calls` calls per window.
Device time from HIP events and host wall time (uploads included, a device synchronise at the end), each over windows of at least
`--window-ms` of back-to-back calls.  Prints one JSON line; `--md PATH` also writes the table of profiles/train_aug_batch.md."""
import argparse
import gc
import json
import math
import os
import random
import sys
import tempfile
import time
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO]

SIZES = [(480, 640), (640, 480), (427, 640), (375, 500), (500, 333), (640, 640)]
BATCH, MASKS, TRAIN_SIZE, PLAN_SEED = 8, 6, 544, 2


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


LABELS = (('eight_apply_stack', 'eight uploads + eight `apply_train_aug` + `torch.stack` (yardstick)'),
          ('apply_batch', 'one `FrameBatch.from_numpy` + one `apply_train_aug_batch`'),
          ('eight_finish_collate', 'eight `finish` + `train_collate` (yardstick)'),
          ('finish_batch', 'one `finish_batch`'),
          ('eight_anns_to_masks', 'eight `annsToMasks` (yardstick)'),
          ('anns_to_masks_batch', 'one `annsToMasksBatch`'))


def markdown(res):
    def cell(s):
        return f"{s['median'] * 1e3:.1f} ({s['range'][0] * 1e3:.1f} – {s['range'][1] * 1e3:.1f})"
    st = res['stages_ms']
    lines = [f"| 8 samples -> [8, 3, {TRAIN_SIZE}, {TRAIN_SIZE}] | calls per window | device µs per batch (range) | wall µs per batch (range) |",
             '|---|---|---|---|']
    for key, label in LABELS:
        lines.append(f"| {label} | {res['calls_per_window'][key]} | {cell(st[key + '_device_ms'])} | {cell(st[key + '_wall_ms'])} |")
    if 'poly_to_mask_us' in res:
        pm = res['poly_to_mask_us']
        lines += ['', '| `ym_poly_to_mask`, 480x640, 7 annotations | other library | this library |', '|---|---|---|',
                  '| device µs per call (range) | ' + ' | '.join(f"{pm[k]['median']:.2f} ({pm[k]['range'][0]:.2f} – {pm[k]['range'][1]:.2f})"
                                                                 for k in ('other', 'this')) + ' |']
    return '\n'.join(lines + [''])


def poly_to_mask_pair(other_path, rounds, calls, dev):
    """(d): `ym_poly_to_mask` of the library at `other_path` against this tree's, alternated in one process; device µs per call."""
    import ctypes
    from yolact_minimal_amd import hip
    from yolact_minimal_amd.utils.synthetic import synth_polygons
    h, w, n = 480, 640, 7
    xy, poly_off, ann_off = [], [0], [0]
    for seg in synth_polygons(5, h, w, n=n):
        for poly in seg:
            xy.extend(poly[:2 * (len(poly) // 2)])
            poly_off.append(poly_off[-1] + len(poly) // 2)
        ann_off.append(len(poly_off) - 1)
    d_xy = torch.tensor(xy, dtype=torch.float64, device=dev)
    d_po, d_ao = torch.tensor(poly_off, dtype=torch.int32, device=dev), torch.tensor(ann_off, dtype=torch.int32, device=dev)
    this, other = hip.lib(), ctypes.CDLL(other_path)
    other.ym_poly_to_mask.argtypes, other.ym_poly_to_mask.restype = this.ym_poly_to_mask.argtypes, ctypes.c_int
    assert this.ym_ann_to_mask_workspace_bytes(n, h, w) == 0
    outs = {k: torch.full((n, h, w), 7, dtype=torch.uint8, device=dev) for k in ('other', 'this')}

    def call(key):
        lib = this if key == 'this' else other
        rc = lib.ym_poly_to_mask(d_xy.data_ptr(), d_po.data_ptr(), d_ao.data_ptr(), n, h, w, outs[key].data_ptr(), None, 0,
                                 hip.stream_ptr())
        assert rc == 0, (key, rc)
    call('other')
    call('this')
    assert torch.equal(outs['other'], outs['this']) and int(outs['this'].max()) == 1, 'the two libraries rasterise differently'
    rows = {'other': [], 'this': []}
    for _ in range(rounds):
        for key in rows:
            rows[key].append(round(timed(lambda: call(key), calls)[0] * 1e3, 4))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--window-ms', type=float, default=300.0, help='least wall time of a timed window of calls')
    ap.add_argument('--against', default=None, help='another build of libyolact_hip.so: measure ym_poly_to_mask against it (d)')
    ap.add_argument('--against-calls', type=int, default=2000, help='ym_poly_to_mask calls per window of (d)')
    ap.add_argument('--md', default=None, help='also write the result table as markdown to this path')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'train_input_bench measures on the GPU; there is nothing to measure without one'
    from oracle.coco_ref import write_synth_dataset
    from yolact_minimal_amd.config import COCO_LABEL_MAP
    from yolact_minimal_amd.utils import coco as K
    from yolact_minimal_amd.utils.augmentations import apply_train_aug, apply_train_aug_batch, sample_train_aug
    from yolact_minimal_amd.utils.frames import FrameBatch
    from yolact_minimal_amd.utils.synthetic import synth_sample
    dev = torch.device('cuda:0')

    # ---- (a) ----
    samples = [synth_sample(i, *SIZES[i % len(SIZES)], MASKS) for i in range(BATCH)]
    rng, plans = random.Random(PLAN_SEED), []
    for img, _, boxes, labels in samples:
        plan = None
        while plan is None:                                          # (a rejected draw is drawn again: both paths need B plans)
            plan = sample_train_aug(img.shape[0], img.shape[1], boxes, labels, TRAIN_SIZE, rng)
        plans.append(plan)
    host_imgs = [s[0] for s in samples]
    masks = [torch.from_numpy(s[1]).to(dev) for s in samples]

    def eight_apply_stack():
        got = [apply_train_aug(torch.from_numpy(img).to(dev), m, p) for img, m, p in zip(host_imgs, masks, plans)]
        return torch.stack([g[0] for g in got], 0), [g[1] for g in got]

    def apply_batch():
        return apply_train_aug_batch(FrameBatch.from_numpy(host_imgs, dev), masks, plans)
    a, b = eight_apply_stack(), apply_batch()
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1])), 'the two pixel paths differ'
    del a, b

    # ---- (b) ----
    with tempfile.TemporaryDirectory() as root:
        ann = write_synth_dataset(root, n_images=BATCH, seed=4, sizes=SIZES)
        cfg = types.SimpleNamespace(train_imgs=root + '/imgs', val_imgs=root + '/imgs', train_ann=ann, val_ann=ann, img_size=TRAIN_SIZE,
                                    continuous_id=COCO_LABEL_MAP, val_num=-1, image=root + '/imgs')
        ds = K.COCODetection(cfg, 'train', device=dev)
        recs = [ds.read(i) for i in range(BATCH)]

    def eight_finish_collate():
        ds.rng = random.Random(11)
        return K.train_collate([ds.finish(r) for r in recs])

    def finish_batch():
        ds.rng = random.Random(11)
        return ds.finish_batch(recs)
    a, b = eight_finish_collate(), finish_batch()
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1] + a[2], b[1] + b[2])), 'the two loader paths differ'
    del a, b

    # ---- (c) ----
    ann_lists = [r['anns'] for r in recs]
    assert all(ann_lists), 'every record of the bench dataset keeps at least one annotation'

    def eight_anns_to_masks():
        return [ds.coco.annsToMasks(anns) for anns in ann_lists]

    def anns_to_masks_batch():
        return ds.coco.annsToMasksBatch(ann_lists)
    a, b = eight_anns_to_masks(), anns_to_masks_batch()
    assert len(a) == len(b) == BATCH and all(torch.equal(x, y) for x, y in zip(a, b)), 'the two rasteriser paths differ'
    del a, b

    fns = {'eight_apply_stack': eight_apply_stack, 'apply_batch': apply_batch, 'eight_finish_collate': eight_finish_collate,
           'finish_batch': finish_batch, 'eight_anns_to_masks': eight_anns_to_masks, 'anns_to_masks_batch': anns_to_masks_batch}
    calls = {k: calls_for(f, args.window_ms) for k, f in fns.items()}
    stage = {f'{k}_{unit}_ms': [] for k in fns for unit in ('device', 'wall')}
    for _ in range(args.rounds):
        for k, f in fns.items():
            d, w = timed(f, calls[k])
            stage[k + '_device_ms'].append(round(d, 5))
            stage[k + '_wall_ms'].append(round(w, 5))
    result = {'workload': f'{BATCH} uint8 samples cycling through ' + ', '.join(f'{h}x{w}' for h, w in SIZES) +
                          f', {MASKS} masks each (pixel half) / write_synth_dataset seed 4 (loader half), train size {TRAIN_SIZE}',
              'mask_rows': sum(len(p.keep) for p in plans), 'annotations': sum(len(a) for a in ann_lists), 'rounds': args.rounds,
              'window_ms': args.window_ms, 'calls_per_window': calls, 'stages_ms_rounds': stage, 'stages_ms': summary(stage)}
    if args.against:
        rows = poly_to_mask_pair(args.against, args.rounds, args.against_calls, dev)
        result['poly_to_mask_us_rounds'], result['poly_to_mask_us'] = rows, summary(rows)
    if args.md:
        with open(args.md, 'w') as fh:
            fh.write(markdown(result))
    print(json.dumps(result))


if __name__ == '__main__':
    main()
