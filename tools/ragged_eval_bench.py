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
eight `after_nms` calls, each over windows of at least `--window-ms` of back-to-back calls.
The metric stage (`--sections metrics`): the b8_d2 pipeline with `batched_metrics=False` (one `DeviceAPData.add` per image: the
yardstick) and `True` (one `add_batch` per request), alternated `--rounds` times in the same process; and device and wall time of ONE
`add_batch` over 8 of those sizes against eight `add` calls on the same rows, at ~100 and at 10 detections per image x 15 gt.
The detection dumps (`--sections json`, not in the default set): (a) eight per-image `rle_encode` calls plus the three `.cpu()` reads
of an image's ids, scores and boxes against ONE `BatchMakeJson.add_batch` plus its collection, on the same eight images; (b) the b8_d2
pipeline whose results are read back per request and fed to a `MakeJson` image by image (the yardstick) against
`evaluate_json_pipelined` on the same pipeline, alternated `--rounds` times, each clocked until its records are on the host and until
its two files are written.  The two dumps must be byte-identical before either is timed.
`--sections` picks among legs, after_nms, metrics and json (default: the first three).  Prints one JSON line."""
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


def metric_stage(padded, sizes8, gts, cfg, nc, dev, args):
    """ONE `add_batch` over the eight images of `padded` (the ragged packed `after_nms_batch` result) against eight `add` calls on the
    same rows, with the counts as they are and clamped to 10: device (HIP events) and wall milliseconds per 8 images.  Every call
    writes fresh image slots of an accumulator that was sized before the window; the gts `add` scales in place are cloned before it."""
    from yolact_minimal_amd.evaluate import IOU_THRES
    from yolact_minimal_amd.utils.device_metrics import DeviceAPData
    ids, scores, boxes_px, masks, counts = padded
    gt8, gm8 = [gts[s][0] for s in sizes8], [gts[s][1] for s in sizes8]
    out = {}
    for label, cnt in (('n100', counts), ('n10', torch.clamp(counts, max=10))):
        out[label + '_counts'] = cnt.tolist()

        def window(batched, iters, cnt=cnt):
            acc = DeviceAPData(nc, IOU_THRES, dev, max_det=cfg.max_detections, capacity_images=8 * iters)
            pool = [[g.clone() for g in gt8] for _ in range(iters)]
            step = iter(range(iters))

            def once():
                i = next(step)
                if batched:
                    acc.add_batch(ids, scores, boxes_px, masks, cnt, pool[i], gm8, sizes8, list(range(8 * i, 8 * i + 8)))
                else:
                    for b in range(8):
                        acc.add(ids[b], scores[b], boxes_px[b], masks[b], cnt[b:b + 1], pool[i][b], gm8[b], sizes8[b][0], sizes8[b][1],
                                image_index=8 * i + b)
            return timed(once, iters), acc
        (_, wall), a = window(False, 4)
        _, b = window(True, 4)
        assert all(torch.equal(getattr(a, n), getattr(b, n)) for n in ('score', 'cls', 'flags', 'gt_count', 'class_rows'))
        iters = {False: max(10, int(math.ceil(args.window_ms / max(wall, 1e-3)))), True: 0}
        iters[True] = iters[False]
        rows = {f'{label}_{k}_{unit}_ms': [] for k in ('eight_add', 'add_batch') for unit in ('device', 'wall')}
        for _ in range(args.rounds):
            for batched, k in ((False, 'eight_add'), (True, 'add_batch')):
                (d, w_), _ = window(batched, iters[batched])
                rows[f'{label}_{k}_device_ms'].append(round(d, 4))
                rows[f'{label}_{k}_wall_ms'].append(round(w_, 4))
        out.update(summary(rows))
        out[label + '_calls_per_window'] = iters[False]
    return out


def per_image_json(make_json, image_id, ids_p, class_p, boxes_p, masks_p):
    """One image into a `MakeJson` the way dropin/reference_loops.py's `coco_api='device'` branch does it: three `.cpu()` reads, one
    `rle_encode`, eval.py:65's filter."""
    from yolact_minimal_amd.utils.common_utils import rle_encode
    ids_p = list(ids_p.cpu().numpy().astype(int))
    class_p = list(class_p.cpu().numpy().astype(float))
    boxes_p = boxes_p.cpu().numpy()
    rles = rle_encode(masks_p)
    for j in range(len(rles)):
        if (boxes_p[j, 3] - boxes_p[j, 1]) * (boxes_p[j, 2] - boxes_p[j, 0]) > 0:
            make_json.add_bbox(image_id, ids_p[j], boxes_p[j, :], class_p[j])
            make_json.add_mask(image_id, ids_p[j], rles[j], class_p[j])


def json_stage(padded, args):
    """(a) the stage alone on the eight images of `padded`: device (HIP events) and wall milliseconds per 8 images."""
    from yolact_minimal_amd.utils.common_utils import BatchMakeJson, MakeJson
    ids, scores, boxes_px, masks, counts = padded
    n = counts.tolist()
    image_ids = list(range(8))

    def eight(make_json=None):
        for b in range(8):
            if make_json is not None:
                per_image_json(make_json, b, ids[b, :n[b]], scores[b, :n[b]], boxes_px[b, :n[b]], masks[b][:n[b]])
            else:                                                 # (the stage without the dicts: what add_batch + collect replaces)
                from yolact_minimal_amd.utils.common_utils import rle_encode
                ids[b, :n[b]].cpu(), scores[b, :n[b]].cpu(), boxes_px[b, :n[b]].cpu(), rle_encode(masks[b][:n[b]])
    holder = [BatchMakeJson()]

    def batched():
        holder[0].add_batch(ids, scores, boxes_px, masks, counts, image_ids)
        holder[0].wait()
    one, many = MakeJson(), BatchMakeJson()
    eight(one)
    many.add_batch(ids, scores, boxes_px, masks, counts, image_ids)
    many.finish()
    assert json.dumps(one.bbox_data) == json.dumps(many.bbox_data) and json.dumps(one.mask_data) == json.dumps(many.mask_data)
    fns = {'eight_rle_encode': eight, 'add_batch_collect': batched}
    calls = {k: calls_for(f, args.window_ms) for k, f in fns.items()}
    rows = {f'{k}_{unit}_ms': [] for k in fns for unit in ('device', 'wall')}
    for _ in range(args.rounds):
        for k, f in fns.items():
            holder[0] = BatchMakeJson()                           # (a window's requests are dropped with it)
            d, w_ = timed(f, calls[k])
            rows[k + '_device_ms'].append(round(d, 4))
            rows[k + '_wall_ms'].append(round(w_, 4))
    out = summary(rows)
    out['counts'] = n
    out['records'] = len(one.mask_data)
    out['calls_per_window'] = calls
    return out


def json_loop(net, cfg, pipe, loader, args):
    """(b) the loop at the pipeline's batch and depth: read every request back and feed a `MakeJson` image by image (the yardstick)
    against `evaluate_json_pipelined`; images per second until the records are on the host, and until the two files are written."""
    import tempfile
    from yolact_minimal_amd.evaluate import evaluate_json_pipelined
    from yolact_minimal_amd.utils.common_utils import MakeJson
    batch = pipe.batch

    def yardstick(samples):
        make_json, queued = MakeJson(), []

        def feed(done):
            first, real = queued.pop(0)
            for b in range(real):
                if done[b][0] is not None:
                    per_image_json(make_json, first + b, *done[b])
        for first in range(0, len(samples), batch):
            entries = samples[first:first + batch]
            real = len(entries)
            entries = entries + [entries[-1]] * (batch - real)
            imgs = torch.cat([e[0] for e in entries], 0)
            queued.append((first, real))
            done = pipe.submit(imgs, out_hw=[(e[3], e[4]) for e in entries])
            if done is not None:
                feed(done)
        for done in pipe.drain():
            feed(done)
        return make_json

    def pipelined(samples):
        make_json = evaluate_json_pipelined(net, cfg, samples, list(range(len(samples))), pipe=pipe)
        make_json.wait()
        return make_json

    def leg(fn, samples, tmp):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        make_json = fn(samples)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        paths = (os.path.join(tmp, 'bbox_detections.json'), os.path.join(tmp, 'mask_detections.json'))
        make_json.dump(*paths)
        t2 = time.perf_counter()
        return len(samples) / (t1 - t0), len(samples) / (t2 - t0), paths
    fns = {'per_image': yardstick, 'add_batch': pipelined}
    rows = {f'{k}_{what}': [] for k in fns for what in ('on_host', 'files_written')}
    with tempfile.TemporaryDirectory() as tmp:
        files = {}
        for k, fn in fns.items():                                 # warm-up, then the files at the timed sizes (short last group included)
            leg(fn, loader(32), tmp)
            files[k] = [open(p, 'rb').read() for p in leg(fn, loader(args.images - 3), tmp)[2]]
        assert files['per_image'] == files['add_batch'], 'the per-image dumps and the add_batch dumps differ'
        for _ in range(args.rounds):
            for k, fn in fns.items():
                on_host, written, _ = leg(fn, loader(), tmp)
                rows[k + '_on_host'].append(round(on_host, 2))
                rows[k + '_files_written'].append(round(written, 2))
    return {'img_per_s_rounds': rows, 'img_per_s': summary(rows), 'dumps_identical': True,
            'dump_bytes': [len(b) for b in files['add_batch']], 'batch': batch, 'depth': pipe.depth}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--images', type=int, default=192, help='images per pass of a leg')
    ap.add_argument('--window-ms', type=float, default=300.0, help='least wall time of a timed window of calls')
    ap.add_argument('--sections', default='legs,after_nms,metrics', help='comma-separated: legs, after_nms, metrics, json')
    args = ap.parse_args()
    sections = set(args.sections.split(','))
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
    if 'legs' not in sections:
        legs = {'b8_d2': (8, 2)} if sections & {'metrics', 'json'} else {}
    pipes = {k: eval_pipeline(net, cfg, img, 480, 640, depth=d, batch=b) for k, (b, d) in legs.items()}

    def leg(name, samples, step=None, batched_metrics=False, keep=None):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        table, acc = evaluate_pipelined(net, cfg, samples, pipe=pipes[name], step=step, batched_metrics=batched_metrics)
        torch.cuda.synchronize()
        rate = len(samples) / (time.perf_counter() - t0)
        if keep is not None:
            keep.append(acc)
        return rate, table
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
              'tables_equal_b1_d4': {k: tables[k] == tables['b1_d4'] for k in legs if 'b1_d4' in legs}}
    if 'metrics' in sections:
        # the metric stage inside the whole loop: same pipeline, same samples, per-image `add` against one `add_batch` per request
        accs = []
        for flag in (False, True):
            leg('b8_d2', loader(32), batched_metrics=flag)
            leg('b8_d2', loader(24), step=0, batched_metrics=flag, keep=accs)
        same = all(torch.equal(getattr(accs[0], n), getattr(accs[1], n)) for n in ('score', 'cls', 'flags', 'gt_count', 'class_rows'))
        assert same, 'add_batch and add disagree on the same requests'
        loop = {'b8_d2_add': [], 'b8_d2_add_batch': []}
        for _ in range(args.rounds):
            loop['b8_d2_add'].append(round(leg('b8_d2', loader())[0], 2))
            loop['b8_d2_add_batch'].append(round(leg('b8_d2', loader(), batched_metrics=True)[0], 2))
        result['metric_stage_loop_img_per_s_rounds'] = loop
        result['metric_stage_loop_img_per_s'] = summary(loop)
        result['metric_stage_logs_equal'] = same
    if 'json' in sections:
        result['json_loop'] = json_loop(net, cfg, pipes['b8_d2'], loader, args)
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
    if 'metrics' in sections:
        result['metric_stage_8_images_ms'] = metric_stage(ragged(True), sizes8, gts, cfg, nc, dev, args)
    if 'json' in sections:
        result['json_stage_8_images_ms'] = json_stage(ragged(True), args)
    if 'after_nms' not in sections:
        print(json.dumps(result))
        return
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
