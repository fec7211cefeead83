"""`--traditional_nms` for a batch: `nms_batch` / `after_nms_batch` / `RequestPipeline` with `cfg.traditional_nms` through
`ym_detect_greedy_nms_batch` (suppression in chunks of 64 sorted candidates).

The contract is the CPU oracle `R.nms(..., traditional=True, stable=True, exp='cr')` per image: ids, scores, boxes and coefs bit for
bit, `None` <-> count 0.  Every case also asserts equality with the per-image `nms()` (the same kernels as a batch of one: image b
of a larger batch against a batch of its own checks the workspace striding) on the same tensors, and that a second call returns the
same bits.  The inputs sit on the edges of the kernel: a class of
exactly one chunk and one just past it, an empty image between two full ones, ties everywhere (also on the max_det cut), a chain
whose suppressed links sit in other chunks than their neighbours, the full 544 px geometry, and classes larger than what the
kernel stages in LDS (4096 candidates) and than what it holds of their scores there (25 600)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import yolact_ref as R
from tests.test_gpu_postproc import _cfg, _check_nms, DEV

pytestmark = pytest.mark.gpu

A128_SCALED = [int(128 / 544 * s) for s in (24, 48, 96, 192, 384)]
SCALES = [24, 48, 96, 192, 384]
_memo = {}


def _memoised(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def _oracle(part, anchors, cfg):
    return R.nms(*part, anchors, score_thre=cfg.nms_score_thre, iou_thre=cfg.nms_iou_thre, top_k=cfg.top_k, max_det=cfg.max_detections,
                 traditional=True, img_size=cfg.img_size, stable=True, exp='cr')


def _class_counts(part, cfg):
    """candidates per foreground class, as the kernel counts them (anchors kept by the score filter, score > threshold)"""
    cls = part[0][0, :, 1:]
    return (cls > cfg.nms_score_thre).sum(0)


def _three_at_128():
    """ONE batch of three 1023-anchor images: a class at exactly one chunk, a class just past the chunk edge, nothing at all."""
    def make():
        parts = [R.synth_head_outputs(1023, proto_hw=32, seed=3, bg_bias=5.0), R.synth_head_outputs(1023, proto_hw=32, seed=5, bg_bias=0.0),
                 R.synth_head_outputs(1023, proto_hw=32, seed=3, bg_bias=30.0)]
        anchors = R.anchors_for(128, A128_SCALED)
        cfg = _cfg(img_size=128, traditional_nms=True)
        assert [int(_class_counts(p, cfg).max()) for p in parts] == [64, 68, 0]
        want = [_oracle(p, anchors, cfg) for p in parts]
        assert [None if w[0] is None else w[0].numel() for w in want] == [100, 100, None]
        return parts, anchors, want
    return _memoised('three128', make)


def _tied(ncls, max_det, levels):
    """the generator of test_gpu_postproc.py::test_nms_class_counts_and_limits: softmax rounded to 1 / levels"""
    gen = torch.Generator().manual_seed(1000 + ncls)
    anchors = R.anchors_for(128, SCALES)
    n = anchors.shape[0]
    logits = torch.randn(1, n, ncls + 1, generator=gen) * 3.0
    logits[..., 0] += 1.0
    cls = torch.round(torch.softmax(logits, -1) * levels) / levels
    box = torch.randn(1, n, 4, generator=gen) * 0.5
    coef = torch.tanh(torch.randn(1, n, 32, generator=gen))
    proto = torch.randn(1, 32, 32, 32, generator=gen)
    return (cls, box, coef, proto), anchors


CHAIN_ROWS = (10, 30, 50)               # rows of the 68 x 68 stride-8 grid, 160 px apart
# (row, phase) blocks of 17 columns (column = 4 x + phase) in score order.  Inside a row a phase-0 column is kept, its right
# neighbour (phase 1) falls to it, phase 2 stands next to that suppressed one and is kept, phase 3 falls to phase 2 -- row 2 takes
# phase 3 before 1 and 2, and the last two blocks alternate, so that every chunk of 64 holds keeps and drops.
CHAIN_BLOCKS = ((0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (0, 2), (2, 3), (1, 2), (0, 3), (2, 1))
CHAIN_TAIL = ((2, 2), (1, 3))


def _chain():
    """box_pred = 0, so the boxes are the anchors: 24 px squares on an 8 px pitch, neighbours overlap 425 / 825 >= 0.5 under the
    + 1 convention, second neighbours 225 / 1025.  Returns the head outputs, the anchors and the anchor index per sorted position."""
    anchors = R.anchors_for(544, SCALES)
    n = anchors.shape[0]
    order = [(CHAIN_ROWS[r] * 68 + 4 * x + ph) * 3 for r, ph in CHAIN_BLOCKS for x in range(17)]
    order += [(CHAIN_ROWS[r] * 68 + 4 * x + ph) * 3 for x in range(17) for r, ph in CHAIN_TAIL]
    assert len(order) == len(set(order)) == 204
    cls = torch.zeros(1, n, 81)
    cls[..., 0] = 1.0
    score = 0.9 - 0.004 * torch.arange(204, dtype=torch.float32)          # strictly decreasing, all > 0.05
    assert bool((score[:-1] > score[1:]).all()) and float(score[-1]) > 0.05
    idx = torch.tensor(order)
    cls[0, idx, 1] = score
    cls[0, idx, 0] = 1.0 - score
    g = torch.Generator().manual_seed(77)
    coef = torch.tanh(torch.randn(1, n, 32, generator=g))
    proto = torch.relu(torch.randn(1, 136, 136, 32, generator=g))
    return (cls, torch.zeros(1, n, 4), coef, proto), anchors, idx


def _few_classes(img_size, ncls, n_cand, seed):
    """a few-class head whose first class has n_cand candidates with random scores; boxes of 0.3 .. 0.6 of the image at random
    centres (box_pred inverts the decode), so that fewer than 128 survive and the output shows the WHOLE kept set, down to the
    last chunk"""
    anchors = R.anchors_for(img_size, SCALES)
    n = anchors.shape[0]
    g = torch.Generator().manual_seed(seed)
    cls = torch.zeros(1, n, ncls + 1)
    pick = torch.randperm(n, generator=g)[:n_cand]
    cls[0, pick, 1] = torch.rand(n_cand, generator=g) * 0.6 + 0.06
    if ncls > 1:
        cls[0, pick[:300], 2] = torch.round(torch.rand(300, generator=g) * 16) / 64 + 0.0625       # a small tied class beside it
    cls[..., 0] = 1.0 - cls[..., 1:].sum(-1)
    centre = torch.rand(n, 2, generator=g) * 0.8 + 0.1
    wh = torch.rand(n, 2, generator=g) * 0.3 + 0.3
    box = torch.cat([(centre - anchors[:, :2]) / (0.1 * anchors[:, 2:]), torch.log(wh / anchors[:, 2:]) / 0.2], 1)[None]
    coef = torch.tanh(torch.randn(1, n, 32, generator=g))
    proto = torch.relu(torch.randn(1, 8, 8, 32, generator=g))
    return (cls, box, coef, proto), anchors


def _to_dev(parts):
    return [torch.cat([p[i] for p in parts], 0).to(DEV) for i in range(4)]


def _check_batch(parts, anchors, cfg, want=None, per_image=True):
    """nms_batch on the parts as ONE batch: twice the same bits, per image the oracle's result and the per-image nms()'s."""
    from yolact_minimal_amd.utils.output_utils import nms, nms_batch
    cls, box, coef, proto = _to_dev(parts)
    a = anchors.to(DEV)
    dets = nms_batch(cls, box, coef, proto, a, cfg)
    again = nms_batch(cls, box, coef, proto, a, cfg)
    counts = dets.counts.tolist()
    assert counts == again.counts.tolist()
    split = dets.split()
    for b, (s, s2) in enumerate(zip(split, again.split())):
        r = want[b] if want is not None else _oracle(parts[b], anchors, cfg)
        assert (r[0] is None) == (counts[b] == 0)
        _check_nms(s, r)
        for x, y in zip(s[:4], s2[:4]):
            assert (x is None and y is None) or torch.equal(x, y), 'a second call returned other bits'
        if per_image:
            one = nms(cls[b:b + 1], box[b:b + 1], coef[b:b + 1], proto[b:b + 1], a, cfg)
            for x, y in zip(s[:4], one[:4]):
                assert (x is None and y is None) or torch.equal(x, y), 'differs from the per-image nms()'
    return dets, counts


def test_chunk_edges_and_an_empty_image_between_two_full_ones():
    parts, anchors, want = _three_at_128()
    cfg = _cfg(img_size=128, traditional_nms=True)
    order = [0, 2, 1]                                    # the empty image in the middle
    dets, counts = _check_batch([parts[i] for i in order], anchors, cfg, [want[i] for i in order])
    assert counts == [100, 0, 100]


@pytest.mark.parametrize('ncls,max_det,levels,most', [(3, 100, 32, 512), (3, 7, 32, 512), (65, 7, 32, 81), (255, 100, 32, 26), (3, 100, 4096, 507)])
def test_ties_everywhere_and_on_the_max_det_cut(ncls, max_det, levels, most):
    part, anchors = _tied(ncls, max_det, levels)
    cfg = _cfg(img_size=128, traditional_nms=True, max_detections=max_det)
    assert int(_class_counts(part, cfg).max()) == most
    want = _oracle(part, anchors, cfg)
    assert want[0].numel() == max_det
    if max_det == 7:
        more = _oracle(part, anchors, _cfg(img_size=128, traditional_nms=True, max_detections=128))[1]
        assert float(more[max_det - 1]) == float(more[max_det]), 'the cut is meant to fall inside a run of equal scores'
    _check_batch([part], anchors, cfg, [want])


def test_a_suppressed_candidate_suppresses_nobody_across_chunk_edges():
    part, anchors, idx = _chain()
    cfg = _cfg(traditional_nms=True, max_detections=128)                  # (102 survive: the output shows every one of them)
    assert _class_counts(part, cfg).tolist() == [204] + [0] * 79
    want = _oracle(part, anchors, cfg)
    fast = R.nms(*part, anchors, max_det=128, stable=True, exp='cr')
    assert not (fast[0].numel() == want[0].numel() and torch.equal(fast[1], want[1])), 'fast_nms must not pass for greedy here'
    # which sorted positions does the oracle keep?
    boxes = R.decode(part[1][0], anchors, 'cr')[idx] * 544.0
    dets = torch.cat([boxes, part[0][0, idx, 1:2]], 1).numpy()
    kept = np.zeros(204, dtype=bool)
    kept[R.greedy_nms(dets, 0.5)] = True
    assert int(kept.sum()) == want[0].numel() < 128
    for k in range(4):
        chunk = kept[64 * k:64 * (k + 1)]
        assert chunk.any() and not chunk.all(), f'chunk {k} of the sorted order must hold keeps and drops'
    # a kept column, its suppressed right neighbour and the kept one beyond it in three different chunks (row 1, x >= 9)
    pos = {int(a): p for p, a in enumerate(idx.tolist())}
    a0 = (CHAIN_ROWS[1] * 68 + 4 * 12) * 3
    p0, p1, p2 = pos[a0], pos[a0 + 3], pos[a0 + 6]
    assert p0 < p1 < p2 and len({p0 // 64, p1 // 64, p2 // 64}) == 3 and kept[p0] and not kept[p1] and kept[p2]
    _check_batch([part], anchors, cfg, [want])


def test_full_size_dense_and_sparse_side_by_side():
    parts = [R.synth_head_outputs(18525, seed=1, bg_bias=4.0), R.synth_head_outputs(18525, seed=2, bg_bias=9.0)]
    cfg = _cfg(traditional_nms=True)
    assert [int(_class_counts(p, cfg).max()) for p in parts] == [879, 279]
    _check_batch(parts, R.anchors_for(544, SCALES), cfg)


@pytest.mark.parametrize('img_size,ncls,n_cand', [(544, 2, 4096), (544, 2, 4097), (648, 1, 25601)])
def test_classes_larger_than_the_staged_form(img_size, ncls, n_cand):
    """4096 candidates are the last count whose sorted boxes live in LDS; from 4097 on the order lives in global memory, and past
    25 600 the scores are read from there too (N = 26 520 anchors at 648 px)."""
    part, anchors = _few_classes(img_size, ncls, n_cand, seed=n_cand)
    cfg = _cfg(img_size=img_size, traditional_nms=True, max_detections=128)
    assert int(_class_counts(part, cfg)[0]) == n_cand
    want = _oracle(part, anchors, cfg)
    assert 50 < want[0].numel() < 128, 'every survivor is meant to be in the output'
    _check_batch([part], anchors, cfg, [want])


def test_after_nms_batch_downstream_dense_and_packed():
    from yolact_minimal_amd.utils.output_utils import nms, after_nms, nms_batch, after_nms_batch
    parts, anchors, _ = _three_at_128()
    cls, box, coef, proto = _to_dev([parts[0], parts[2], parts[1]])
    a = anchors.to(DEV)
    cfg = _cfg(img_size=128, traditional_nms=True)
    cfg.save_lincomb, cfg.no_crop = False, False
    # (every score of these images is above 0.58: 0.3 keeps all 100 rows, 0.8 cuts into them)
    for vt, packed in ((0.3, False), (0.3, True), (0.8, False), (0.8, True)):
        cfg.visual_thre = vt
        got = after_nms_batch(nms_batch(cls, box, coef, proto, a, cfg), 64, 64, cfg, packed=packed)
        assert [g[0] is None for g in got] == [False, True, False]
        for b in range(3):
            r = nms(cls[b:b + 1], box[b:b + 1], coef[b:b + 1], proto[b:b + 1], a, cfg)
            w = after_nms(r[0], r[1], r[2].clone() if r[2] is not None else None, r[3], r[4], 64, 64, cfg, packed=packed)
            assert (w[0] is None) == (got[b][0] is None)
            if w[0] is None:
                continue
            assert (w[0].numel() == 100) if vt == 0.3 else (0 < w[0].numel() < 100)
            for x, y in zip(w[:3], got[b][:3]):
                assert torch.equal(x, y)
            assert torch.equal(w[3].bits, got[b][3].bits) if packed else torch.equal(w[3], got[b][3])


def test_request_pipeline_serves_with_traditional_nms():
    import bench
    from yolact_minimal_amd.pipeline import RequestPipeline
    from yolact_minimal_amd.utils.output_utils import nms, after_nms
    dev = torch.device(DEV)
    net, cfg = bench.build_net('res50_coco', 128, dev)
    cfg.traditional_nms = True
    head = [t.to(dev) for t in _three_at_128()[0][0]]
    img = torch.randn(1, 3, 128, 128, generator=torch.Generator().manual_seed(0)).to(dev)
    pipe = RequestPipeline(net, cfg, 128, 128, dev, depth=2, out_hw=(64, 64), batch=1)
    r = nms(*head, pipe.anchors, cfg)
    want = after_nms(r[0], r[1], r[2].clone(), r[3], r[4], 64, 64, cfg)
    assert want[0].numel() == 100
    pipe.warm_up(img, rounds=0)
    results = [pipe.submit(img, head) for _ in range(4)]
    results = [x for x in results if x is not None] + pipe.drain()
    assert len(results) == 4
    for got in results:
        for x, y in zip(got, want):
            assert torch.equal(x, y)


def _raw_call(head, anchors, ncfg, batch, ws, ws_bytes, counts):
    from yolact_minimal_amd import hip
    md = ncfg.max_det
    out = (torch.empty(batch, md, dtype=torch.int64, device=DEV), torch.empty(batch, md, device=DEV),
           torch.empty(batch, md, 4, device=DEV), torch.empty(batch, md, ncfg.coef_dim, device=DEV))
    rc = hip.lib().ym_detect_greedy_nms_batch(hip.ptr(head[0]), hip.ptr(head[1]), hip.ptr(head[2]), hip.ptr(anchors), ctypes.byref(ncfg), batch,
                                              hip.ptr(counts, torch.int32), hip.ptr(out[0], torch.int64), hip.ptr(out[1]), hip.ptr(out[2]),
                                              hip.ptr(out[3]), ctypes.c_void_p(ws.data_ptr()), ws_bytes, hip.stream_ptr())
    return rc, out


def test_workspace_is_respected_and_checked_before_any_launch():
    from yolact_minimal_amd import hip
    parts, anchors, want = _three_at_128()
    head = _to_dev([parts[0], parts[2], parts[1]])
    a = anchors.to(DEV)
    ncfg = hip.NmsCfg(1023, 81, 32, 200, 100, 0.05, 0.5, 128.0)
    need = hip.lib().ym_greedy_nms_batch_workspace_bytes(ctypes.byref(ncfg), 3)
    assert need > 0
    guard = 4096
    ws = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    counts = torch.full((3,), -1, dtype=torch.int32, device=DEV)
    rc, _ = _raw_call(head, a, ncfg, 3, ws, need - 1, counts)
    torch.cuda.synchronize()
    assert rc == -2, 'YM_ENOSPC'                                            # include/yolact_hip.h
    assert counts.tolist() == [-1, -1, -1]
    assert bool((ws == 0xA5).all()), 'a refused call must not have launched anything'
    rc, out = _raw_call(head, a, ncfg, 3, ws, need, counts)
    hip.check(rc, 'ym_detect_greedy_nms_batch')
    torch.cuda.synchronize()
    assert counts.tolist() == [100, 0, 100]
    assert bool((ws[need:] == 0xA5).all()), 'the call wrote past ym_greedy_nms_batch_workspace_bytes'
    for b, w in ((0, want[0]), (2, want[1])):
        _check_nms(tuple(t[b] for t in out), w)


def test_single_image_entry_workspace_is_respected_and_checked_before_any_launch():
    """`ym_detect_greedy_nms` with `ym_nms_workspace_bytes`: one byte less is refused before anything runs, the stated size is
    enough, and neither the guard behind the workspace nor an output row at or beyond the count is written."""
    from yolact_minimal_amd import hip
    parts, anchors, want = _three_at_128()
    head = [t[0].contiguous() for t in _to_dev([parts[0]])[:3]]
    a = anchors.to(DEV)
    ncfg = hip.NmsCfg(1023, 81, 32, 200, 100, 0.05, 0.5, 128.0)
    need = hip.lib().ym_nms_workspace_bytes(ctypes.byref(ncfg))
    assert need > 0
    guard, md = 4096, 128                                                   # (28 output rows behind the 100 the call may fill)
    ws = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    count = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    out = [torch.full((md * w * 4,), 0x5A, dtype=torch.uint8, device=DEV) for w in (2, 1, 4, 32)]     # ids, scores, boxes, coefs
    patterns = [o.clone() for o in out]

    def call(ws_bytes):
        return hip.lib().ym_detect_greedy_nms(hip.ptr(head[0]), hip.ptr(head[1]), hip.ptr(head[2]), hip.ptr(a), ctypes.byref(ncfg),
                                              hip.ptr(count, torch.int32), *[ctypes.c_void_p(o.data_ptr()) for o in out],
                                              ctypes.c_void_p(ws.data_ptr()), ws_bytes, hip.stream_ptr())

    rc = call(need - 1)
    torch.cuda.synchronize()
    assert rc == -2, 'YM_ENOSPC'                                            # include/yolact_hip.h
    assert count.tolist() == [-1]
    assert bool((ws == 0xA5).all()), 'a refused call must not have launched anything'
    assert all(torch.equal(o, p) for o, p in zip(out, patterns))
    hip.check(call(need), 'ym_detect_greedy_nms')
    torch.cuda.synchronize()
    assert count.tolist() == [100]
    assert bool((ws[need:] == 0xA5).all()), 'the call wrote past ym_nms_workspace_bytes'
    rows = (out[0].view(torch.int64), out[1].view(torch.float32), out[2].view(torch.float32).view(md, 4), out[3].view(torch.float32).view(md, 32))
    _check_nms(tuple(r[:100] for r in rows), want[0])
    for o, p, w in zip(out, patterns, (2, 1, 4, 32)):
        assert torch.equal(o[100 * w * 4:], p[100 * w * 4:]), 'rows at or beyond the count must keep the caller\'s bytes'


def test_a_non_default_stream_has_its_own_scratch():
    from yolact_minimal_amd.utils.output_utils import nms_batch
    parts, anchors, _ = _three_at_128()
    cls, box, coef, proto = _to_dev([parts[0], parts[2], parts[1]])
    a = anchors.to(DEV)
    cfg = _cfg(img_size=128, traditional_nms=True)
    torch.cuda.synchronize()
    first = nms_batch(cls, box, coef, proto, a, cfg)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        second = nms_batch(cls, box, coef, proto, a, cfg)
    torch.cuda.synchronize()
    assert first.counts.tolist() == second.counts.tolist() == [100, 0, 100]
    for b in (0, 2):
        for x, y in zip((first.ids, first.scores, first.boxes, first.coefs), (second.ids, second.scores, second.boxes, second.coefs)):
            assert torch.equal(x[b], y[b])
