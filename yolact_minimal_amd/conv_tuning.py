"""The sweeps that produce rows of the tuned table: which plans are tried for a shape, and how a candidate is timed.  engine.py
(InferEngine.autotune), train_engine.py (the inline training sweep) and the tuners under tools/ all come here.

Two layers.  The candidate lists are pure functions of integers and flags that return ConvPlan / WgradPlan lists in the order in
which they are timed: no tensor, no library call, no environment read, so the CPU suite pins them (tests/test_conv_tuning_cpu.py).
Below them: the one launch timer, the keep-the-first-clear-winner loop, and the inline training sweep with its state."""
import os

from .conv_plan import ConvPlan, WgradPlan
from .hip import ACT_NONE, ACT_RELU, TILE_COUNTERS

# ---- candidate lists ------------------------------------------------------------------------------------------------------------


def _tiles(M, N, tm, tn):
    return -(-M // tm) * -(-N // tn)


def ksplit_ok(ks, wgs, nkt):
    """A K split over `ks` workgroups per tile: none where the tiles fill the chip anyway, two K tiles per slice at least, and a
    bounded grid."""
    return ks == 1 or not (wgs >= 1024 or ks * 2 > nkt or wgs * ks > 8192)


def tail_rounds(wgs, cus):
    """Tiles in the last partial round over `cus` CUs x 1 or 2 workgroups: the tail_tiles worth splitting.  Needs arrival counters,
    so nothing beyond TILE_COUNTERS tiles: there hip.conv2d_fwd drops the counters for the launch, and the tail with them."""
    return sorted({wgs % cus, wgs % (2 * cus)} - {0}) if cus < wgs <= TILE_COUNTERS else []


def tail_ksplit_ok(ts, nkt, r=0):
    """`ts` K slices for each of `r` tail tiles: two K tiles per slice at least, a bounded number of extra workgroups."""
    return ts * 2 <= nkt and r * ts <= 2048


def workgroup_candidates(M, N, nkt, nseg=1, stem=False, counters=True, act=ACT_RELU, cus=256):
    """Inference, the workgroup kernels: tile x K split x staging family (2 / 3 registers, 22-24 direct-to-LDS ring, 33 / 34 with
    pipelined fragments, 43 / 46 the persistent walker of conv_persist.hip), then per tile the tail splits of a one-segment launch
    with arrival counters (`counters`).  The stem has its 128x64 tile and register staging only."""
    cands = []
    for tm, tn in ([(128, 64)] if stem else [(128, 128), (128, 64), (64, 128), (64, 64)]):
        wgs, small = _tiles(M, N, tm, tn), (tm, tn) == (64, 64)
        for ks in (1, 2, 3, 4, 6, 8, 12, 16, 24):
            if not ksplit_ok(ks, wgs, nkt):
                continue
            stages = [2]
            if (tm, tn) != (128, 128) and nkt // ks >= 3:
                stages.append(3)
            if not stem:
                stages.append(22)
                if nkt // ks >= 3:
                    stages.append(23)
                if small and nkt // ks >= 4:
                    stages.append(24)
                if small and nkt // ks >= 2:
                    stages += [33, 34]
                if small and nseg == 1 and counters and act in (ACT_NONE, ACT_RELU):
                    stages += [43, 46]
            cands += [ConvPlan(tm, tn, ks, 0, st) for st in stages]
        if not stem and nseg == 1 and counters:
            for r in tail_rounds(wgs, cus):
                for ts in (2, 3, 4, 6, 8):
                    if tail_ksplit_ok(ts, nkt, r):
                        deep = (tm, tn) != (128, 128) and nkt // ts >= 3
                        stages = ((2, 3, 22, 23) + ((33, 34) if small else ())) if deep else (2, 22)
                        cands += [ConvPlan(tm, tn, 1, 0, st, r, ts) for st in stages]
    return cands


def wave_candidates(M, N, nkt):
    """The wave kernel (one wave per tile, K split over `kwaves` waves of a workgroup), register staging."""
    cands = []
    for tm, tn in ((32, 32), (64, 32), (32, 64), (64, 64)):
        waves = _tiles(M, N, tm, tn)
        for kwv in (1, 2, 4, 8):
            if (kwv > 1 and (waves >= 4096 or kwv > nkt)) or (kwv == 8 and tm * tn == 4096) or waves * kwv > 65536:
                continue
            cands.append(ConvPlan(tm, tn, 1, kwv))
    return cands


def wave_dma_candidates(M, N, nkt, tail=True, cus=256, rings=(22,), waves_per_wg=(1, 2)):
    """The wave kernel with private DMA rings (conv_wdma_f32; needs Cin % 32 == 0, no pyramid): the K split stays inside the
    workgroup, no K-slice exchange.  Tile x K waves x ring depth `rings` (the ring of 4 exists for the 32x32 tile only), each ring
    also as one- and two-wave workgroups (`waves_per_wg`) where the waves share nothing; then, where `tail` (one segment, arrival
    counters), the tail split of the 32x32 / four-K-wave plan over `cus` CUs."""
    cands = []
    for tm, tn in ((32, 32), (64, 32), (32, 64)):
        for kwv in (1, 2, 4):
            if kwv > nkt:
                continue
            for ring in rings:
                if ring == 24 and (tm, tn) != (32, 32):
                    continue
                cands.append(ConvPlan(tm, tn, 1, kwv, ring))
                cands += [ConvPlan(tm, tn, 1, kwv, ring, grid_wgs=wpb) for wpb in waves_per_wg if wpb >= kwv and kwv < 4]
    tiles32 = _tiles(M, N, 32, 32)
    if tail and cus < tiles32 <= TILE_COUNTERS:
        cands += [ConvPlan(32, 32, 1, 4, 22, tiles32 % cus or cus, ts) for ts in (4, 6, 8) if tail_ksplit_ok(ts, nkt)]
    return cands


def split_bf16(cands):
    """`cands` for the split-bf16 pipes, which stage through registers: one (stages 0) or two (3) register sets for the workgroup
    kernel, the wave kernel as it is (0); de-duplicated and sorted."""
    return sorted({p._replace(stages=st) for p in cands for st in ((0, 3) if not p.wave else (0,))})


def infer_candidates(M, N, nkt, nseg=1, stem=False, counters=True, act=ACT_RELU, cus=256, mma=0, wave_dma=True):
    """Everything InferEngine.autotune times for a shape after the baseline ConvPlan(), in order.  `wave_dma`: the launch can run
    conv_wdma_f32 (Cin % 32 == 0, no pyramid input); `mma` 3 / 6: the split-bf16 rewrite, without the DMA-ring wave kernel."""
    cands = workgroup_candidates(M, N, nkt, nseg, stem, counters, act, cus)
    if not stem:
        cands += wave_candidates(M, N, nkt)
    if mma:
        return split_bf16(cands)
    if not stem and wave_dma:
        cands += wave_dma_candidates(M, N, nkt, nseg == 1 and counters, cus)
    return cands


def train_conv_candidates(M, N, nkt):
    """The inline training sweep of a forward / data-gradient launch, baseline first: fewer K splits and families than inference
    (no 24, the rings of 3 on the 64x64 tile only), tail splits over the whole chip with the two-deep stagings."""
    cands = [ConvPlan()]
    for tm, tn in ((128, 128), (128, 64), (64, 128), (64, 64)):
        wgs = _tiles(M, N, tm, tn)
        for ks in (1, 2, 3, 4, 6, 8, 12, 16):
            if not ksplit_ok(ks, wgs, nkt):
                continue
            deep = (tm, tn) == (64, 64) and nkt // ks >= 3
            cands += [ConvPlan(tm, tn, ks, 0, st) for st in ((2, 22, 3, 23) if deep else (2, 22))]
        cands += [ConvPlan(tm, tn, 1, 0, st, r, ts) for r in tail_rounds(wgs, 256) for ts in (2, 3, 4, 6, 8) if tail_ksplit_ok(ts, nkt, r)
                  for st in (2, 22)]
    return cands


def wgrad_candidates(cout, cout_real, k):
    """Weight gradient of a [cout (padded)][k = KH KW Cin] filter: pixel split x LDS variant.  22 / 23 / 24 are the DMA rings; layers
    with <= 64 output channels have the 32-pixel ring only, at 48 KB = 3 workgroups per CU.  Next to the powers of two, the pixel
    splits that make the grid a whole number of rounds of the chip (2 workgroups of 68 KB LDS per CU = 512 slots, 3 of 34 KB with the
    single-buffer variant = 768): powers of two alone left e.g. 756 workgroups = 1.5 rounds for the layer3 3x3 (msplit 14 -> 504 =
    one round)."""
    tiles = -(-cout // (64 if cout_real <= 64 else 128)) * -(-k // 128)
    cands = []
    for nb, slots in ((2, 512), (1, 768)) + (((22, 512), (23, 768), (24, 512)) if cout_real > 64 else ((22, 768),)):
        half = slots // 2
        fill = {max(1, round(half * j / tiles)) for j in (1, 2, 3, 4, 6, 8, 12, 16)} | {max(1, (half * j) // tiles) for j in (2, 4, 6, 8)}
        cands += [WgradPlan(ms, nb) for ms in sorted({0, 1, 2, 4, 8, 16, 32, 64, 128, 256} | {m for m in fill if m <= 256})]
    return cands


def weight_stationary_candidates(cin):
    """The weight-stationary 1x1 kernel (conv_ws.hip): tile x ring of 2-4, where the filter slice of a tile fits its 64 KB of LDS."""
    return [ConvPlan(tm, tn, 1, 0, st) for tm, tn in ((64, 256), (128, 128), (256, 64)) if tn * cin * 4 <= 64 * 1024 for st in (52, 53, 54)]


# ---- timing ---------------------------------------------------------------------------------------------------------------------


def time_launch(fn, *, iters, reps, warmup, sync_each_rep=False, join=None):
    """Microseconds per call of `fn` on the current stream: `warmup` calls, then the fastest of `reps` runs of `iters` calls between
    two events.  `sync_each_rep`: every run starts on an idle device; `join()` runs before the closing event (side streams)."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(warmup):
        fn()
    best = 1e30
    for _ in range(reps):
        if sync_each_rep:
            torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            fn()
        if join is not None:
            join()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / iters * 1e3)
    return best


def time_conv(d, ws, **timer):
    """time_launch of hip.conv2d_fwd(d, ws), or None where the plan in `d` needs more scratch than `ws` or the library refuses it."""
    from . import hip
    if hip.conv_workspace_bytes(d) > ws.numel():
        return None
    try:
        return time_launch(lambda: hip.conv2d_fwd(d, ws), **timer)
    except RuntimeError:
        return None


def fastest(cands, time_of, best=1e30, plan=None, margin=0.98):
    """(time, plan) after timing `cands` in order: a candidate replaces the incumbent (`best`, `plan`) where it beats it by the
    margin; `time_of(cand)` is None for one that cannot run."""
    for cand in cands:
        t = time_of(cand)
        if t is not None and t < best * margin:
            best, plan = t, cand
    return best, plan


# ---- the inline training sweep --------------------------------------------------------------------------------------------------
_TUNING = os.environ.get('YM_TUNE_TRAIN', '0') == '1'     # sweep unseen shapes inline and remember the winner
_new_entries = {}
_TRAIN_TIMER = dict(iters=5, reps=2, warmup=2)


def tuning():
    """Inline sweeps: tools/autotune_train.py (YM_TUNE_TRAIN=1 at import) or the opt-in tune-on-first-use mode (YM_AUTOTUNE=1, read
    per call like engine.autotune_on)."""
    return _TUNING or os.environ.get('YM_AUTOTUNE', '0') == '1'


def remember(key, hit):
    """A row the inline sweep measured: kept for tools/autotune_train.py (dump_new_entries) and, with YM_AUTOTUNE=1, written through
    to the per-user cache that later processes overlay on the shipped table (engine.tuned_table)."""
    from .engine import record_rows
    _new_entries[key] = hit
    record_rows({key: hit})


def dump_new_entries(path):
    import json
    with open(path, 'w') as f:
        json.dump(_new_entries, f, indent=0, sort_keys=True)


def sweep_train_conv(d, key, ws):
    """Time train_conv_candidates on the forward / data-gradient ConvDesc `d` (scratch `ws`); the winner is remembered as `key`."""
    def time_of(cand):
        cand.apply(d)
        return time_conv(d, ws, **_TRAIN_TIMER)

    plan = fastest(train_conv_candidates(d.B * d.Ho * d.Wo, d.Cout, d.k_pad // 32), time_of, plan=ConvPlan())[1]
    remember(key, plan.to_row())
    return plan


def sweep_wgrad(d, key, ws):
    """Time wgrad_candidates on the WgradDesc `d` (scratch `ws`); the winner is remembered as `key`."""
    import ctypes
    from . import hip

    def launch():
        hip.check(hip.lib().ym_conv2d_wgrad(ctypes.byref(d), ctypes.c_void_p(ws.data_ptr()), ws.numel(), hip.stream_ptr()), 'wgrad')

    def time_of(cand):
        cand.apply(d)
        need = hip.lib().ym_conv2d_wgrad_workspace_bytes(ctypes.byref(d))
        return None if need == 0 or need > ws.numel() else time_launch(launch, **_TRAIN_TIMER)

    plan = fastest(wgrad_candidates(d.Cout, d.Cout_real, d.KH * d.KW * d.Cin), time_of, plan=WgradPlan(0, 2))[1]
    remember(key, plan.to_row())
    return plan
