#!/usr/bin/env python3
"""Coordinate descent on the forward time of ONE request (hipGraph replay of the whole plan), shape by shape, over the wave-private
DMA-ring kernel's configurations.  The per-launch tuner (tools/tune_wave.py, a launch repeated back to back) undervalues kernels
without a cross-workgroup K-slice exchange: in the dependent chain of a real forward the exchange's last arriver delays the NEXT
launch (tools/chain_trace_rt.py: a layer3 block 20.7 -> 17.6 us per launch with the wave kernels, where back-to-back timing of the
3x3 shows a tie).  So: candidates are pre-filtered by their own launch time (within --slack of the best) and then judged by the
plan's forward time; a change is kept if it wins twice.

    python tools/tune_forward.py [--batch 1] [--cfg res101_coco] [--write] [--out file.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import bench  # noqa: E402
from yolact_minimal_amd import conv_tuning, engine as E, plan_transfer  # noqa: E402
from yolact_minimal_amd.conv_plan import ConvPlan, from_entry  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=1)
ap.add_argument('--cfg', default='res101_coco')
ap.add_argument('--write', action='store_true')
ap.add_argument('--out', default='')
ap.add_argument('--max-m', type=int, default=20000)
ap.add_argument('--slack', type=float, default=1.2)
ap.add_argument('--replays', type=int, default=40)
ap.add_argument('--size', type=int, default=544, help='--img_size of the plan that is tuned')
ap.add_argument('--alt', default='', help='comma-separated table files: their row for a shape (exact, or transferred from the nearest tuned '
                'shape: plan_transfer.py) is a candidate too, whatever its own launch time')
ap.add_argument('--inflight', type=int, default=1, help='> 1: optimise the img/s of a RequestPipeline with that many requests in flight; winners are written as <sig>_tp')
args = ap.parse_args()
dev = torch.device('cuda:0')
net, cfg = bench.build_net(args.cfg, args.size, dev)
img = torch.randn(args.batch, 3, args.size, args.size, device=dev)
alts = [json.load(open(f)) for f in args.alt.split(',') if f]
pipe = None
if args.inflight > 1:
    os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')
    from yolact_minimal_amd.pipeline import RequestPipeline
    pipe = RequestPipeline(net, cfg, args.size, args.size, dev, depth=args.inflight, with_post=False, batch=args.batch, return_outputs=False)
    pipe.warm_up(img)
    eng = pipe.engines[0]
else:
    eng = net._engine(img)
    eng.run(img)
torch.cuda.synchronize()
big = torch.empty(1 << 28, device=dev, dtype=torch.uint8)


def launch_time(d, iters=20):
    return conv_tuning.time_conv(d, big, iters=iters, reps=3, warmup=2, sync_each_rep=True)


def forward_ms():
    if pipe is not None:              # ms per request with `inflight` requests overlapped
        import time
        pipe.warm_up(img)
        best = 1e30
        n = args.replays * args.inflight
        for _ in range(2):
            for _ in range(2 * args.inflight):
                pipe.submit(img)
            pipe.drain()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                pipe.submit(img)
            pipe.drain()
            torch.cuda.synchronize()
            best = min(best, (time.perf_counter() - t0) / n * 1e3)
        return best
    eng.run(img)                      # (re)captures the graph after a retune
    torch.cuda.synchronize()
    return conv_tuning.time_launch(lambda: eng.run(img), iters=args.replays, reps=2, warmup=0) / 1e3


def put(sig, v):
    for e in (pipe.engines if pipe is not None else [eng]):
        for c in e.convs:
            if c.sig == sig:
                c.plan = v
        e.retune()


groups = {}
for c in eng.convs:
    d = c.desc
    if c.stem or d.nlevels or d.Cin % 32 or d.B * d.Ho * d.Wo > args.max_m:
        continue
    groups.setdefault(c.sig, []).append(c)
base_ms = forward_ms()
print(f'start: forward {base_ms:.4f} ms ({args.cfg}, batch {args.batch}); {len(groups)} shapes', flush=True)
cur_ms, kept = base_ms, {}
# shapes by their share of the launches' time (count x launch time)
order = []
for sig, cs in groups.items():
    t = launch_time(cs[0].desc)
    order.append((-(t or 0) * len(cs), sig, t))
for _, sig, t0 in sorted(order):
    cs = groups[sig]
    c, d = cs[0], cs[0].desc
    cur = c.plan
    M = d.B * d.Ho * d.Wo
    cands = []
    # (fewer waves per workgroup: single tiles are balanced over the CUs; tail split: the tiles past the last full round of 256 CUs
    #  are computed as K slices in the CUs' second slots)
    for v in conv_tuning.wave_dma_candidates(M, d.Cout, d.k_pad // 32, tail=d.nseg == 1 and bool(d.tile_counters)):
        keep = ConvPlan.of(d)
        v.apply(d)
        t = launch_time(d)
        keep.apply(d)
        if t is not None:
            cands.append((t, v))
    if pipe is not None:              # the latency entry is a candidate too (the slot may currently run a `_tp` row)
        alt = from_entry(E.tuned_table().get(sig))
        if alt is not None:
            cands.append((0.0, alt))
    for tab in alts:                  # another table's choice for this shape (its own row, or the nearest tuned shape's, re-derived)
        alt = from_entry(plan_transfer.lookup(tab, sig, M, d.Cout, d.k_pad // 32, d.nseg)[0])
        if alt is not None and alt != cur and all(alt != v for _, v in cands):
            cands.append((0.0, alt))
    cands.sort()
    tried = 0
    t_ref = min([t0] + [t for t, _ in cands if t > 0])
    for t, v in cands:
        if v == cur or t > args.slack * t_ref or tried >= (7 if pipe is not None else 5 + len(alts)):
            continue
        tried += 1
        put(sig, v)
        ms = forward_ms()
        tag = ''
        if ms < cur_ms * 0.998:
            ms2 = forward_ms()
            if max(ms, ms2) < cur_ms * 0.998:
                cur_ms, cur, kept[sig], tag = max(ms, ms2), v, v.to_row(), '  <-- kept'
        print(f'{sig:42s} x{len(cs):2d} launch {t0:6.2f} -> {t:6.2f} us {list(v)} forward {ms:.4f} ms{tag}', flush=True)
        put(sig, cur)
final = forward_ms()
print(f'final: forward {base_ms:.4f} -> {final:.4f} ms; {len(kept)} entries change', flush=True)
if pipe is not None:
    kept = {k + '_tp': v for k, v in kept.items()}
if args.out:
    json.dump(kept, open(args.out, 'w'), indent=0, sort_keys=True)
if args.write and kept:
    # rows change the summation order of their layers: they reach the committed table only through the reference-digest gate
    from tools.table_gate import merge_rows, GateRefused
    torch.cuda.synchronize()
    try:
        merge_rows(kept, E.TUNED_PATH)
        print(f'wrote {len(kept)} rows to {E.TUNED_PATH} (544 px reference digests green under the candidate table)')
    except GateRefused as exc:
        print(f'REFUSED: {exc}')
        sys.exit(3)
