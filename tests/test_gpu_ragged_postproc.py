"""GPU: `after_nms_batch` with per-image output sizes (`ym_after_nms_ragged[_packed]`) against the per-image `after_nms`, the uniform
entry and the CPU oracle, what the kernels write outside their rows, and the mixed-size requests of `RequestPipeline` and
`evaluate_pipelined(batch=N)`."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import yolact_ref as R
from yolact_minimal_amd.config import build_cfg

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SMALL_SIZES = [(97, 301), (333, 64), (48, 70), (120, 128), (97, 301)]          # (48, 70): the two-kernel path at a 32 x 32 prototype map
FULL_SIZES = [(480, 640), (640, 480), (427, 640), (240, 320)]                  # (240, 320): the two-kernel path at 136 x 136
COCO_LIKE = [(480, 640), (640, 480), (427, 640), (375, 500), (500, 333), (640, 640)]


def _cfg(size, **kw):
    cfg = build_cfg('res101_coco', 'val', 544)
    cfg.img_size = size
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


@functools.lru_cache(maxsize=None)
def _case(name):
    """(cfg size, sizes, the batch's `nms_batch` result, its per-image split); computed once, never modified (callers copy the boxes)."""
    from yolact_minimal_amd.utils.output_utils import nms_batch
    if name == 'small':
        size, sizes, n_anchors, hp = 128, SMALL_SIZES, 1023, 32
        anchors = R.anchors_for(128, [int(128 / 544 * s) for s in (24, 48, 96, 192, 384)])
        biases = [5.0, 30.0, -2.0, 4.0, 6.0]               # image 1: no detections; image 2: dense enough for max_detections
    else:
        size, sizes, n_anchors, hp = 544, FULL_SIZES, 18525, 136
        anchors = R.anchors_for(544, [24, 48, 96, 192, 384])
        biases = [4.0, 9.0, 7.5, 5.0]
    parts = [R.synth_head_outputs(n_anchors, proto_hw=hp, seed=3 + i, bg_bias=b) for i, b in enumerate(biases)]
    cls, box, coef, proto = (torch.cat([p[i] for p in parts], 0).to(DEV) for i in range(4))
    dets = nms_batch(cls, box, coef, proto, anchors.to(DEV), _cfg(size))
    split = dets.split()
    counts = dets.counts.tolist()
    if name == 'small':
        assert counts[1] == 0 and max(counts) == _cfg(size).max_detections, counts
    assert sum(c > 0 for c in counts) >= len(counts) - 1
    return size, sizes, dets, split


def _fresh(dets):
    from yolact_minimal_amd.utils.output_utils import BatchDetections
    return BatchDetections(dets.counts, dets.ids, dets.scores, dets.boxes.clone(), dets.coefs, dets.proto)


def _words(m):
    return m.bits if hasattr(m, 'bits') else m


def _same(got, want):
    assert (got[0] is None) == (want[0] is None)
    if want[0] is None:
        return
    for a, b in zip(got, want):
        a, b = _words(a), _words(b)
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


@pytest.mark.parametrize('no_crop', [False, True], ids=['crop', 'no_crop'])
@pytest.mark.parametrize('packed', [False, True], ids=['dense', 'packed'])
@pytest.mark.parametrize('name', ['small', 'full'])
def test_equals_the_per_image_path_bit_for_bit(name, packed, no_crop):
    from yolact_minimal_amd.utils.output_utils import PackedMasks, after_nms, after_nms_batch
    size, sizes, dets, split = _case(name)
    cfg = _cfg(size, no_crop=no_crop)
    hs, ws = [s[0] for s in sizes], [s[1] for s in sizes]
    mine = _fresh(dets)
    got = after_nms_batch(mine, hs, ws, cfg, packed=packed)
    assert len(got) == len(sizes)
    for b, (r, (h, w)) in enumerate(zip(split, sizes)):
        boxes = r[2].clone() if r[2] is not None else None
        want = after_nms(r[0], r[1], boxes, r[3], r[4], h, w, cfg, packed=packed)
        _same(got[b], want)
        if want[0] is not None:
            n = want[0].shape[0]
            assert got[b][2].dtype == torch.int32 and tuple(got[b][3].shape) == (n, h, w)
            assert isinstance(got[b][3], PackedMasks) == packed
            assert torch.equal(mine.boxes[b, :n], boxes)                    # the boxes scaled in place, by this image's S
    # the padded form: per-image views of ONE allocation, each at its own size, no host read needed to use them
    ids, scores, box_px, masks, counts = after_nms_batch(_fresh(dets), hs, ws, cfg, sync=False, packed=packed)
    assert isinstance(masks, list) and len(masks) == len(sizes) and counts is dets.counts
    md = dets.ids.shape[1]
    base = _words(masks[0]).untyped_storage().data_ptr()
    for b, (h, w) in enumerate(sizes):
        assert tuple(masks[b].shape) == (md, h, w) and _words(masks[b]).is_contiguous()
        assert _words(masks[b]).untyped_storage().data_ptr() == base and _words(masks[b]).data_ptr() % 256 == 0
        if got[b][0] is not None:
            n = got[b][0].shape[0]
            assert torch.equal(_words(masks[b])[:n], _words(got[b][3])) and torch.equal(box_px[b, :n], got[b][2])


@pytest.mark.parametrize('packed', [False, True], ids=['dense', 'packed'])
@pytest.mark.parametrize('hw', [(300, 200), (480, 640)])
def test_equal_sizes_equal_the_uniform_entry(hw, packed):
    from yolact_minimal_amd.utils.output_utils import after_nms_batch
    h, w = hw
    size, _, dets, _ = _case('full')
    cfg = _cfg(size)
    batch = dets.ids.shape[0]
    a, b = _fresh(dets), _fresh(dets)
    want = after_nms_batch(a, h, w, cfg, packed=packed)
    got = after_nms_batch(b, [h] * batch, [w] * batch, cfg, packed=packed)
    for g_, w_ in zip(got, want):
        _same(g_, w_)
    assert torch.equal(a.boxes, b.boxes)


def test_small_case_against_the_cpu_oracle():
    """Independent of the kernels under test: the oracle's after_nms per image.  Pixels may differ only where the oracle's upsampled
    soft value is within 1e-5 of the threshold (the fused dot product sums in k order), fewer than 1e-5 of them; pixel boxes exactly."""
    from yolact_minimal_amd.utils.output_utils import after_nms_batch
    size, sizes, dets, split = _case('small')
    got = after_nms_batch(_fresh(dets), [s[0] for s in sizes], [s[1] for s in sizes], _cfg(size))
    for g_, r, (h, w) in zip(got, split, sizes):
        if r[0] is None:
            assert g_[0] is None
            continue
        ids, scores, boxes_px, masks, soft, up = R.after_nms(r[0].cpu(), r[1].cpu(), r[2].cpu().clone(), r[3].cpu(), r[4].cpu(), h, w,
                                                              return_soft=True)
        np.testing.assert_array_equal(g_[2].cpu().numpy(), boxes_px.numpy())
        gm = g_[3].cpu()
        assert tuple(gm.shape) == (ids.numel(), h, w) and set(torch.unique(gm).tolist()) <= {0.0, 1.0}
        diff = gm != masks
        if bool(diff.any()):
            assert float((up[diff] - 0.5).abs().max()) < 1e-5, f'{int(diff.sum())} mask pixels of a {h} x {w} image differ away from 0.5'
        assert float(diff.float().mean()) < 1e-5


@pytest.mark.parametrize('packed', [False, True], ids=['dense', 'packed'])
def test_writes_only_what_it_owns(packed):
    """The entries themselves on a flat buffer prefilled with 0xA5, 4096 bytes longer than the layout: rows below the count hold
    masks, and every other byte (rows at or past the count, the alignment gaps, the tail) still holds the fill."""
    from yolact_minimal_amd import hip
    from yolact_minimal_amd.utils.output_utils import ragged_layout
    md, sizes, counts = 7, [(97, 301), (120, 128), (48, 70)], (7, 3, 0)
    esz = 8 if packed else 4
    offsets, total = ragged_layout(sizes, md, packed)
    assert offsets[1] * esz > md * 97 * (5 if packed else 301) * esz           # there IS an alignment gap after the first block
    g = torch.Generator().manual_seed(17)
    proto = torch.relu(torch.randn(3, 32, 32, 32, generator=g)).to(DEV)
    coef = torch.tanh(torch.randn(3, md, 32, generator=g)).to(DEV)
    xy = torch.rand(3, md, 2, generator=g) * 0.5
    boxes = torch.cat([xy, xy + 0.2 + torch.rand(3, md, 2, generator=g) * 0.3], 2).to(DEV)
    boxes_in = boxes.clone()
    cnt = torch.tensor(counts, dtype=torch.int32, device=DEV)
    buf = torch.full((total * esz + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    box_px = torch.empty(3, md, 4, dtype=torch.int32, device=DEV)
    table = (hip.RaggedImage * 3)(*[hip.RaggedImage(h, w, o) for (h, w), o in zip(sizes, offsets)])
    L = hip.lib()
    nbytes = L.ym_after_nms_ragged_workspace_bytes(table, 3, md, 32, 32)
    assert nbytes == md * 32 * 32 * 4                                          # (48, 70) takes the two-kernel path
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    fn = L.ym_after_nms_ragged_packed if packed else L.ym_after_nms_ragged
    hip.check(fn(hip.ptr(proto), hip.ptr(coef), hip.ptr(boxes), hip.ptr(cnt, torch.int32), 3, md, 32, 32, 32, table, 1,
                 ctypes.c_void_p(buf.data_ptr()), hip.ptr(box_px, torch.int32), ctypes.c_void_p(ws.data_ptr()), nbytes, hip.stream_ptr()),
              'ym_after_nms_ragged')
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    owned = np.zeros(host.shape, dtype=bool)
    some = 0
    for (h, w), o, n in zip(sizes, offsets, counts):
        row = h * ((w + 63) // 64 if packed else w)
        lo, hi = o * esz, (o + n * row) * esz
        owned[lo:hi] = True
        if packed:
            words = host[lo:hi].view(np.uint64).reshape(n, h, (w + 63) // 64)
            assert not (words == np.uint64(0xA5A5A5A5A5A5A5A5)).any()
            bits = np.unpackbits(words.view(np.uint8).reshape(n, h, 8 * ((w + 63) // 64)), axis=-1, bitorder='little')
            assert not bits[..., w:].any()                                     # zero bits at x >= img_w
            some += int(bits.sum())
        else:
            vals = host[lo:hi].view(np.float32)
            assert np.isin(vals, (0.0, 1.0)).all()
            some += int(vals.sum())
    assert some > 0                                                            # masks were written, not only zero fill
    assert (host[~owned] == 0xA5).all()
    for b, (h, w) in enumerate(sizes):                                         # boxes: every image by its own S, in place
        s = float(max(h, w))
        assert torch.equal(boxes[b], boxes_in[b] * s) and torch.equal(box_px[b], (boxes_in[b] * s).int())


def _head_batch(n_anchors, num_classes, seeds):
    parts = [R.synth_head_outputs(n_anchors, num_classes=num_classes, proto_hw=32, seed=s, bg_bias=b) for s, b in seeds]
    return [torch.cat([p[i] for p in parts], 0).to(DEV) for i in range(4)]


TRIPLES = [[(97, 301), (333, 64), (48, 70)], [(120, 128), (96, 128), (200, 150)], [(64, 64), (97, 301), (301, 97)],
           [(48, 70), (50, 75), (128, 120)], [(333, 64), (250, 255), (257, 256)], [(100, 100), (99, 101), (480, 640)]]


@pytest.mark.parametrize('mode', ['results', 'packed', 'consumer', 'visual_thre'])
def test_pipeline_requests_with_a_size_per_image(mode):
    """`RequestPipeline(batch=3, depth=2)`: six requests, another size triple each, alternating head outputs; every image of every
    request equals `after_nms` of that image's `nms` result at that image's size."""
    import bench
    from yolact_minimal_amd.pipeline import RequestPipeline
    from yolact_minimal_amd.utils.output_utils import after_nms, nms_batch
    dev = torch.device(DEV)
    net, cfg = bench.build_net('res50_coco', 128, dev)
    packed = mode == 'packed'
    n_anchors = len(net.anchors) // 4
    heads = [_head_batch(n_anchors, cfg.num_classes, [(3, 5.0), (4, 30.0), (5, 3.0)]),
             _head_batch(n_anchors, cfg.num_classes, [(6, 4.0), (7, 6.0), (8, 5.0)])]
    anchors = torch.tensor(net.anchors, dtype=torch.float32).reshape(-1, 4).to(dev)
    splits = [nms_batch(*h, anchors, cfg).split() for h in heads]
    assert [s[0] is None for s in splits[0]] == [False, True, False] and all(s[0] is not None for s in splits[1])
    if mode == 'visual_thre':
        sc = torch.cat([s[1] for s in splits[0] + splits[1] if s[1] is not None])
        cfg.visual_thre = float(sc.sort()[0][sc.numel() // 2])                # the median score: about half survive
    try:
        img = torch.randn(3, 3, 128, 128, generator=torch.Generator().manual_seed(5)).to(dev)
        pipe = RequestPipeline(net, cfg, 128, 128, dev, depth=2, out_hw=(96, 128), batch=3, packed_masks=packed)
        pipe.warm_up(img, rounds=0)
        want = []
        for i, triple in enumerate(TRIPLES):
            want.append([after_nms(r[0], r[1], r[2].clone() if r[2] is not None else None, r[3], r[4], h, w, cfg, packed=packed)
                         for r, (h, w) in zip(splits[i % 2], triple)])

        def keep(ids, scores, boxes_px, masks, counts):
            return ids.clone(), scores.clone(), boxes_px.clone(), [_words(m).clone() for m in masks], counts.clone()

        got = [pipe.submit(img, heads[i % 2], out_hw=triple, consumer=keep if mode == 'consumer' else None)
               for i, triple in enumerate(TRIPLES)]
        got = [r for r in got if r is not None] + pipe.drain()
    finally:
        cfg.visual_thre = 0
        net._engines.clear()
    assert len(got) == len(TRIPLES)
    kept = 0
    for i, (req, exp, triple) in enumerate(zip(got, want, TRIPLES)):
        if mode != 'consumer':
            assert len(req) == 3
            for one, w_ in zip(req, exp):
                _same(one, w_)
                kept += 0 if w_[0] is None else int(w_[0].shape[0])
            continue
        ids, scores, boxes_px, masks, counts = req
        assert counts.tolist() == [0 if s[0] is None else int(s[0].shape[0]) for s in splits[i % 2]]
        for b, ((h, w), w_) in enumerate(zip(triple, exp)):
            assert tuple(masks[b].shape[:2]) == (cfg.max_detections, h)
            if w_[0] is not None:
                n = w_[0].shape[0]
                _same((ids[b, :n], scores[b, :n], boxes_px[b, :n], masks[b][:n]), w_)
    if mode == 'visual_thre':
        total = sum(int(s[0].shape[0]) for i in range(len(TRIPLES)) for s in splits[i % 2] if s[0] is not None)
        assert 0 < kept < total
    if mode != 'consumer':
        assert pipe.detections == kept
    # a single pair still means "all images" (the uniform entry), and a malformed list is refused before the slot is taken
    with pytest.raises(RuntimeError, match='pairs'):
        pipe.submit(img, heads[0], out_hw=[(10, 10), (10, 10)])
    assert pipe.drain() == []


def test_evaluate_pipelined_in_batches_of_four():
    """Six mixed-size samples in requests of four (the second padded with two copies of its last image, never added) against an
    accumulator built here: the same two batches through an engine of the pipeline's mode, `nms_batch`, per-image `after_nms` and
    `DeviceAPData.add`.  (An engine of the slots' mode rather than `net(imgs)`: a depth-2 pipeline reads the throughput-tuned plan
    rows, and another split of a K sum is another rounding -- tests/test_gpu_pipeline.py::_single_path.)"""
    import bench
    from yolact_minimal_amd.engine import InferEngine
    from yolact_minimal_amd.evaluate import IOU_THRES, evaluate_pipelined
    from yolact_minimal_amd.utils.device_metrics import DeviceAPData
    from yolact_minimal_amd.utils.output_utils import after_nms, nms_batch
    from yolact_minimal_amd.utils.synthetic import synth_eval_case
    dev = torch.device(DEV)
    net, cfg, _ = bench.detecting_net('res50_coco', 128, dev)
    nc = len(cfg.class_names)
    g = torch.Generator().manual_seed(23)
    samples = []
    for i, (h, w) in enumerate(COCO_LIKE):
        _, _, _, _, gt, gt_masks, _, _ = synth_eval_case(i + 1, 40, 7, h, w, 10)
        samples.append((torch.randn(1, 3, 128, 128, generator=g).to(dev), gt.to(dev), gt_masks.to(dev), h, w))

    def loader():
        return [(im, gt.clone(), gm, h, w) for im, gt, gm, h, w in samples]

    # the expected accumulator
    want = DeviceAPData(nc, IOU_THRES, dev, max_det=cfg.max_detections)
    eng = InferEngine(net, 4, 128, 128, dev, mode='throughput')
    anchors = torch.tensor(net.anchors, dtype=torch.float32).reshape(-1, 4).to(dev)
    md, rows = cfg.max_detections, 0
    for first in (0, 4):
        real = samples[first:first + 4]
        group = real + [real[-1]] * (4 - len(real))
        eng.run(torch.cat([s[0] for s in group], 0))
        torch.cuda.synchronize()
        dets = nms_batch(*[t.clone() for t in eng.outputs()], anchors, cfg)
        for b, (r, (_, gt, gt_masks, h, w)) in enumerate(zip(dets.split(), real)):   # (zip stops at the real images)
            masks = torch.zeros(md, h, w, device=dev)
            boxes_px = torch.zeros(md, 4, dtype=torch.int32, device=dev)
            if r[0] is not None:
                a = after_nms(r[0], r[1], r[2].clone(), r[3], r[4], h, w, cfg)
                n = a[0].shape[0]
                rows += n
                masks[:n], boxes_px[:n] = a[3], a[2]
            want.add(dets.ids[b], dets.scores[b], boxes_px, masks, dets.counts[b:b + 1], gt.clone(), gt_masks, h, w)
    assert rows >= 12, f'{rows} detections over six images: the network must detect something for this test to mean anything'
    try:
        got, acc = evaluate_pipelined(net, cfg, loader(), depth=2, step=0, batch=4)
    finally:
        net._engines.clear()
    assert acc.images == want.images == 6
    assert torch.equal(acc.gt_count, want.gt_count) and int(acc.gt_count.sum()) == 6 * 7       # the padded copies added no ground truth
    assert torch.equal(acc.class_rows, want.class_rows) and int(acc.class_rows.sum()) > 0     # ... and no log rows

    def points(ap):
        return [(ap[k][t][c].num_gt_positives, list(ap[k][t][c].data_points)) for k in ('box', 'mask') for t in range(len(IOU_THRES))
                for c in range(nc)]
    assert points(acc.to_ap_data()) == points(want.to_ap_data())
    assert got == want.calc_map(0)
