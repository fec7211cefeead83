"""Bit-packed instance masks on the GPU: the producer (`after_nms(..., packed=True)`) and every consumer against the dense path.
The packed path has no arithmetic of its own, so every comparison with the dense path is EXACT; the only tolerance in this file is
the one `tests/test_gpu_postproc.py` already grants the dense masks against the reference's frozen goldens."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import metrics_ref as M
from oracle import yolact_ref as R
from tests import draw_ref as D
from tests.conftest import REPO
from yolact_minimal_amd.config import build_cfg

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
THRES = [x / 100 for x in range(50, 100, 5)]


def _cfg(**kw):
    cfg = build_cfg('res101_coco', 'val', 544)
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _detections(golden_dir, tag):
    """nms() results on the inputs of tests/golden/post_<tag>.npz, built as tests/test_gpu_postproc.py builds them."""
    from yolact_minimal_amd.utils.output_utils import nms
    g = np.load(os.path.join(golden_dir, f'post_{tag}.npz'))
    if tag.endswith('544'):
        seed, bg = {'dense544': (1, 4.0), 'sparse544': (2, 9.0)}[tag]
        cls, box, coef, proto = R.synth_head_outputs(18525, seed=seed, bg_bias=bg)
        anchors, size = R.anchors_for(544, [24, 48, 96, 192, 384]), 544
    else:
        cls, box, coef, proto = (torch.from_numpy(g[k]) for k in ('in_class', 'in_box', 'in_coef', 'in_proto'))
        anchors, size = torch.from_numpy(g['in_anchors']), 128
    out = nms(cls.to(DEV), box.to(DEV), coef.to(DEV), proto.to(DEV), anchors.to(DEV), _cfg(img_size=size))
    assert out[0] is not None
    return g, out, size


def _check_producer(out, h, w, cfg):
    """packed call == dense call: ids, scores, pixel boxes, the in-place box scaling, and the words == pack_reference(dense != 0)."""
    from yolact_minimal_amd.utils.output_utils import PackedMasks, after_nms, pack_reference
    box_d, box_p = out[2].clone(), out[2].clone()
    d = after_nms(out[0], out[1], box_d, out[3], out[4], h, w, cfg)
    p = after_nms(out[0], out[1], box_p, out[3], out[4], h, w, cfg, packed=True)
    n = int(out[0].shape[0])
    assert torch.equal(p[0], d[0]) and torch.equal(p[1], d[1]) and torch.equal(p[2], d[2]) and p[2].dtype == torch.int32
    assert torch.equal(box_p, box_d) and not torch.equal(box_p, out[2])                     # scaled in place, identically
    pm = p[3]
    assert isinstance(pm, PackedMasks) and pm.shape == (n, h, w) and len(pm) == n and pm.device == d[3].device
    assert pm.bits.dtype == torch.int64 and tuple(pm.bits.shape) == (n, h, (w + 63) // 64) and pm.bits.is_contiguous()
    assert pm.nbytes == n * h * ((w + 63) // 64) * 8
    dense = d[3].cpu().numpy()
    np.testing.assert_array_equal(pm.bits.cpu().numpy(), pack_reference(dense != 0))         # word for word, pad bits included
    assert torch.equal(pm.dense(), d[3])
    host = pm.numpy()
    assert host.dtype == np.uint8 and np.array_equal(host, dense.astype(np.uint8))
    return d, p


CASES = [('dense544', [(480, 640), (544, 544), (333, 500), (481, 37), (20, 17)]), ('sparse544', [(300, 200), (333, 500)]),
         ('small128', [(96, 128), (128, 64)]), ('degenerate128', [(64, 64)])]


@pytest.mark.parametrize('no_crop', [False, True], ids=['crop', 'no_crop'])
@pytest.mark.parametrize('tag,sizes', CASES, ids=[c[0] for c in CASES])
def test_producer_equals_dense_and_reference_goldens(golden_dir, tag, sizes, no_crop):
    g, out, size = _detections(golden_dir, tag)
    cfg = _cfg(img_size=size, no_crop=no_crop)
    for h, w in sizes:
        d, p = _check_producer(out, h, w, cfg)
        key = f'masks_{h}x{w}_packed'
        if not no_crop and key in g.files:
            # against the reference's own frozen masks, under the bar the dense path has in tests/test_gpu_postproc.py
            np.testing.assert_array_equal(p[2].cpu().numpy(), g[f'px_boxes_{h}x{w}'])
            msb = np.packbits(p[3].numpy().reshape(-1))
            mism = int(np.unpackbits(msb ^ g[key]).sum())
            numel = int(np.prod(p[3].shape))
            bar = int(1e-5 * numel) if size == 544 else max(2, int(1e-5 * numel))
            print(f'{tag} {h}x{w}: {mism} of {numel} mask pixels differ from the reference golden (bar {bar})')
            assert mism <= bar, f'{mism} mask pixels differ from the reference'
    if not no_crop:
        assert any(f'masks_{h}x{w}_packed' in g.files for h, w in sizes), 'the case must meet a golden'


def test_indexing_and_pack_round_trip():
    from yolact_minimal_amd.utils.output_utils import PackedMasks, pack_reference
    gen = torch.Generator().manual_seed(5)
    for n, h, w in [(6, 9, 1), (6, 7, 63), (5, 3, 64), (5, 4, 65), (4, 11, 500), (3, 480, 640), (0, 8, 70)]:
        m = (torch.rand(n, h, w, generator=gen) > 0.5)
        want = pack_reference(m.numpy())
        for t in (m.float() * 0.5, m.to(torch.uint8) * 7, m):
            pm = PackedMasks.pack(t.to(DEV))
            assert pm.shape == (n, h, w)
            np.testing.assert_array_equal(pm.bits.cpu().numpy(), want)
        assert torch.equal(pm.dense().cpu(), m.float()) and np.array_equal(pm.numpy(), m.numpy().astype(np.uint8))
        assert pm.dense(torch.uint8).dtype == torch.uint8
        if n >= 4:
            keep = torch.tensor([True, False] * (n // 2) + [True] * (n % 2), device=DEV)
            idx = torch.tensor([n - 1, 0], device=DEV)
            for sel in (slice(0, 2), keep, idx):
                sub = pm[sel]
                assert isinstance(sub, PackedMasks) and torch.equal(sub.dense().cpu(), m.float()[sel.cpu() if torch.is_tensor(sel) else sel])
            one = pm[1]
            assert one.shape == (h, w) and torch.equal(one.dense().cpu(), m[1].float())
    with pytest.raises(RuntimeError):
        PackedMasks.pack(torch.zeros(2, 4, 4))


def test_batch_equals_single_image_calls_without_host_reads():
    from yolact_minimal_amd.utils.output_utils import PackedMasks, after_nms, after_nms_batch, nms_batch
    h, w = 333, 500
    cfg = _cfg()
    anchors = R.anchors_for(544, [24, 48, 96, 192, 384]).to(DEV)
    parts = [R.synth_head_outputs(18525, seed=1), R.synth_head_outputs(18525, seed=2, bg_bias=9.0),
             R.synth_head_outputs(18525, seed=4, bg_bias=30.0)]
    cls, box, coef, proto = (torch.cat([p[i] for p in parts], 0).to(DEV) for i in range(4))
    dets = nms_batch(cls, box, coef, proto, anchors, cfg)
    found = dets.counts.tolist()
    assert found[0] >= 50 and found[1] >= 40 and found[2] == 0, found
    counts = [found[0], 37, 0]                                           # three different counts, one of them 0
    dets.counts = torch.tensor(counts, dtype=torch.int32, device=DEV)
    boxes0 = dets.boxes.clone()
    singles = []
    for b, c in enumerate(counts):
        singles.append(None if c == 0 else
                       after_nms(dets.ids[b, :c], dets.scores[b, :c], boxes0[b, :c].clone(), dets.coefs[b, :c], dets.proto[b], h, w, cfg, packed=True))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        ids, scores, box_px, masks, cnt = after_nms_batch(dets, h, w, cfg, sync=False, packed=True)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert isinstance(masks, PackedMasks) and masks.shape == (3, cfg.max_detections, h, w)
    assert tuple(masks.bits.shape) == (3, cfg.max_detections, h, (w + 63) // 64)
    for b, c in enumerate(counts):
        if c:
            assert torch.equal(masks.bits[b, :c], singles[b][3].bits) and torch.equal(box_px[b, :c], singles[b][2]), b
    dets.boxes.copy_(boxes0)
    per_image = after_nms_batch(dets, h, w, cfg, packed=True)
    assert per_image[2] == (None, None, None, None)
    for b in (0, 1):
        r, s = per_image[b], singles[b]
        assert torch.equal(r[0], s[0]) and torch.equal(r[1], s[1]) and torch.equal(r[2], s[2]) and torch.equal(r[3].bits, s[3].bits)


def _eq_nan(a, b):
    return np.array_equal(np.nan_to_num(a, nan=-1.0), np.nan_to_num(b, nan=-1.0))


@pytest.mark.parametrize('n,g,h,w', [(100, 20, 480, 640), (130, 150, 61, 67), (1, 1, 5, 3), (3, 2, 544, 544), (7, 5, 100, 100), (9, 4, 768, 1024)])
def test_mask_iou_packed_is_bit_equal_to_dense(n, g, h, w):
    from yolact_minimal_amd.utils.box_utils import mask_iou
    from yolact_minimal_amd.utils.output_utils import PackedMasks
    gen = torch.Generator().manual_seed(n * 7 + g)
    a = (torch.rand(n, h * w, generator=gen) > 0.6).float()
    b = (torch.rand(g, h * w, generator=gen) > 0.3).float()
    a[0] = 0
    b[-1] = 0
    a_dev, b_dev = a.to(DEV), b.to(DEV)
    want = mask_iou(a_dev, b_dev).numpy()
    pa, pb = PackedMasks.pack(a_dev.reshape(n, h, w)), PackedMasks.pack(b_dev.reshape(g, h, w))
    both = mask_iou(pa, pb)
    assert not both.is_cuda and both.dtype == torch.float32 and _eq_nan(both.numpy(), want)
    assert _eq_nan(mask_iou(pa, b_dev.to(torch.uint8)).numpy(), want)                       # packed x dense uint8 [g, H*W]
    assert _eq_nan(mask_iou(pa, b_dev.to(torch.uint8).reshape(g, h, w)).numpy(), want)      # ... and [g, H, W]
    assert _eq_nan(mask_iou(a_dev, pb).numpy(), want)                                       # dense x packed
    on_dev = mask_iou(pa, pb, to_cpu=False)
    assert on_dev.is_cuda and _eq_nan(on_dev.cpu().numpy(), want)
    assert np.isnan(want[0, -1]) and np.isnan(both.numpy()[0, -1])


@pytest.mark.parametrize('case', [0, 1, 2])
def test_prep_metrics_with_packed_masks_matches_reference_golden(golden_dir, case):
    from yolact_minimal_amd.utils import common_utils as C
    from yolact_minimal_amd.utils.box_utils import mask_iou
    from yolact_minimal_amd.utils.output_utils import PackedMasks
    gold = np.load(os.path.join(golden_dir, 'metrics.npz'))
    n, g, h, w, nc = (int(v) for v in gold[f'c{case}_shape'])
    ids, scores, boxes, masks, gt, gt_masks, h, w = M.synth_eval_case(int(gold[f'c{case}_seed']), n, g, h, w, nc)
    pm = PackedMasks.pack(masks.reshape(n, h, w).to(DEV))
    pg = PackedMasks.pack(gt_masks.reshape(g, h, w).to(DEV))
    assert _eq_nan(mask_iou(pm, pg).numpy(), gold[f'c{case}_mask_iou'])
    gt_px = gt[:, :4] * torch.tensor([w, h, w, h])
    for gt_side in ([gt_masks.to(DEV)] if case else [gt_masks.to(DEV), pg]):                 # once with packed gt masks as well
        ap = {k: [[C.APDataObject() for _ in range(nc)] for _ in THRES] for k in ('box', 'mask')}
        gt_dev = gt.clone().to(DEV)
        C.prep_metrics(ap, ids, scores, boxes.to(DEV), pm, gt_dev, gt_side, h, w, THRES)
        torch.testing.assert_close(gt_dev[:, :4].cpu(), gt_px)
        ref = M.new_ap_data(nc, len(THRES))
        M.prep_metrics(ref, ids, scores, boxes, masks, gt, gt_masks, h, w, THRES)
        rows = []
        for kind in ('box', 'mask'):
            for k in range(len(THRES)):
                for c in range(nc):
                    a, b = ap[kind][k][c], ref[kind][k][c]
                    assert a.num_gt_positives == b.num_gt_positives and list(a.data_points) == list(b.data_points), (kind, k, c)
                    rows.append([a.num_gt_positives, len(a.data_points), sum(1 for p in a.data_points if p[1]), a.get_ap()])
        np.testing.assert_array_equal(np.array(rows, dtype=np.float64), gold[f'c{case}_ap_grid'])
        _, row2, row3 = C.calc_map(ap, THRES, nc, step=0)
        assert row2[1:] == [round(v, 2) for v in gold[f'c{case}_map_box']] and row3[1:] == [round(v, 2) for v in gold[f'c{case}_map_mask']]


def _blob_masks(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    m = torch.zeros(n, h, w)
    for i in range(n):
        for _ in range(1 + i % 3 if min(h, w) > 2 else 0):
            x1, y1 = int(torch.randint(0, w - 2, (1,), generator=g)), int(torch.randint(0, h - 2, (1,), generator=g))
            x2, y2 = int(torch.randint(x1 + 1, w + 1, (1,), generator=g)), int(torch.randint(y1 + 1, h + 1, (1,), generator=g))
            m[i, y1:y2, x1:x2] = 1.0
    return m


@pytest.mark.parametrize('n,h,w', [(100, 480, 640), (7, 61, 67), (7, 33, 47), (3, 544, 544), (2, 1, 1)])
def test_rle_encode_packed_equals_dense_and_oracle(n, h, w):
    from oracle import rle_ref
    from yolact_minimal_amd.utils.common_utils import rle_encode
    from yolact_minimal_amd.utils.output_utils import PackedMasks
    m = _blob_masks(n, h, w, n + h)
    m[0] = 0                                              # empty mask
    m[-1] = 1                                             # full mask
    if n > 2:
        m[1, 0, 0] = 1
    dense = rle_encode(m.to(DEV))
    got = rle_encode(PackedMasks.pack(m.to(DEV)))
    assert got == dense
    for i in range(n):
        assert got[i] == rle_ref.encode(m[i].numpy()), i


def test_rle_encode_packed_grows_buffers_and_add_mask():
    from oracle import rle_ref
    from yolact_minimal_amd.utils.common_utils import rle_encode, MakeJson
    from yolact_minimal_amd.utils.output_utils import PackedMasks
    g = torch.Generator().manual_seed(3)
    m = (torch.rand(2, 120, 160, generator=g) > 0.5).float()          # ~9600 runs each: the retry with larger buffers
    pm = PackedMasks.pack(m.to(DEV))
    got = rle_encode(pm, cap_runs=64)
    assert got == rle_encode(m.to(DEV), cap_runs=64) == [rle_ref.encode(m[i].numpy()) for i in range(2)]
    mj = MakeJson()
    mj.add_mask(7, 0, pm[0], 0.5)
    assert mj.mask_data[0]['segmentation'] == got[0]


FLAG_SETS = [dict(), dict(hide_mask=True), dict(hide_bbox=True), dict(hide_score=True), dict(real_time=True),
             dict(hide_mask=True, hide_bbox=True), dict(hide_mask=True, hide_score=True, real_time=True),
             dict(hide_bbox=True, real_time=True), dict(hide_mask=True, hide_bbox=True, hide_score=True, real_time=True)]


def _draw_both(args, cfg, **kw):
    from yolact_minimal_amd.utils.draw import draw_img
    from yolact_minimal_amd.utils.output_utils import PackedMasks
    ids, scores, boxes, masks, img = args
    d = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (ids, scores, boxes, masks, img)]
    dense = draw_img(d[0], d[1], d[2], d[3], d[4], cfg, **kw)
    packed = draw_img(d[0], d[1], d[2], PackedMasks.pack(d[3]), d[4], cfg, **kw)
    assert packed.is_cuda and packed.dtype == torch.uint8 and torch.equal(packed, dense)
    return packed


@pytest.mark.parametrize('flags', FLAG_SETS, ids=lambda f: '+'.join(sorted(f)) or 'default')
@pytest.mark.parametrize('hw', [(120, 160), (37, 53)])
def test_draw_img_flags(flags, hw):
    args = D.synth(12, hw[0], hw[1], seed=21, wild_boxes=True)
    _draw_both(args, D.make_cfg(**flags), **({'fps': 31.256} if flags.get('real_time') else {}))


@pytest.mark.parametrize('n,hw', [(1, (480, 640)), (7, (480, 640)), (100, (480, 640)), (9, (37, 53)), (9, (1, 1)), (9, (5, 7)), (9, (64, 130))])
def test_draw_img_sizes(n, hw):
    args = D.synth(n, hw[0], hw[1], seed=10 + n, wild_boxes=True)
    got = _draw_both(args, D.make_cfg())
    assert np.array_equal(got.cpu().numpy(), D.draw_ref(*args, D.make_cfg()))
    no_crop = D.synth(15, 120, 160, seed=8, crop=False)
    _draw_both(no_crop, D.make_cfg(no_crop=True))


def test_cutout_mattes_packed():
    from yolact_minimal_amd.utils.draw import cutout_mattes
    from yolact_minimal_amd.utils.output_utils import PackedMasks
    for hw in [(120, 160), (37, 53)]:
        ids, scores, boxes, masks, img = D.synth(8, hw[0], hw[1], seed=13, wild_boxes=True)
        cfg = D.make_cfg(cutout=True)
        d = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (ids, scores, boxes, masks, img)]
        total, objs = cutout_mattes(d[0], d[2], d[3], d[4], cfg)
        ptotal, pobjs = cutout_mattes(d[0], d[2], PackedMasks.pack(d[3]), d[4], cfg)
        assert torch.equal(ptotal, total) and len(pobjs) == len(objs) == 8
        assert all(torch.equal(a, b) for a, b in zip(pobjs, objs))
        total_np, _ = cutout_mattes(d[0], d[2], PackedMasks.pack(d[3]), img, cfg)
        assert isinstance(total_np, np.ndarray) and np.array_equal(total_np, total.cpu().numpy())


def test_draw_batch_packed_with_visual_thre_and_empty_frames():
    from yolact_minimal_amd.utils.output_utils import PackedMasks, after_nms_batch, draw_batch, draw_img, nms_batch
    h, w = 480, 640
    cfg = _cfg(visual_thre=0.3)
    for name in ('hide_mask', 'hide_bbox', 'hide_score', 'real_time', 'cutout'):
        setattr(cfg, name, False)
    anchors = R.anchors_for(544, [24, 48, 96, 192, 384]).to(DEV)
    parts = [R.synth_head_outputs(18525, seed=1), R.synth_head_outputs(18525, seed=2, bg_bias=9.0),
             R.synth_head_outputs(18525, seed=4, bg_bias=30.0), R.synth_head_outputs(18525, seed=5, bg_bias=7.5)]
    cls, box, coef, proto = (torch.cat([p[i] for p in parts], 0).to(DEV) for i in range(4))
    imgs = torch.from_numpy(np.random.default_rng(6).integers(0, 256, (4, h, w, 3)).astype(np.uint8)).to(DEV)
    dets = nms_batch(cls, box, coef, proto, anchors, cfg)
    boxes0 = dets.boxes.clone()
    ids, scores, boxes, masks, counts = after_nms_batch(dets, h, w, cfg, sync=False)
    dets.boxes.copy_(boxes0)
    _, _, pboxes, pmasks, _ = after_nms_batch(dets, h, w, cfg, sync=False, packed=True)
    assert isinstance(pmasks, PackedMasks) and torch.equal(pboxes, boxes)
    counts = torch.tensor([100, 37, 0, 64], dtype=torch.int32, device=DEV)
    scores = scores.clone()
    scores[:, 1::3] *= 0.25
    scores[3, :64] *= 0.1                                   # frame 3: every row under the threshold -> unchanged frame
    want = draw_batch((ids, scores, boxes, masks, counts), imgs, cfg)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        got = draw_batch((ids, scores, boxes, pmasks, counts), imgs, cfg)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.equal(got, want) and torch.equal(got[2], imgs[2]) and torch.equal(got[3], imgs[3]) and not torch.equal(got[0], imgs[0])
    # the per-image call on the filtered rows (PackedMasks indexed by [:n] and by the visual_thre mask)
    keep = scores[1, :37] >= cfg.visual_thre
    one = draw_img(ids[1, :37][keep], scores[1, :37][keep], boxes[1, :37][keep], pmasks[1][:37][keep], imgs[1], cfg)
    assert 0 < int(keep.sum()) < 37 and torch.equal(one, want[1])


def test_pipeline_returns_packed_results_and_holds_less_memory():
    """`RequestPipeline(packed_masks=True)` returns the packing of what the dense pipeline returns, and its peak device memory over
    8 requests is lower by at least ONE dense mask tensor minus one packed one (the least the layout guarantees; with `depth`
    results in flight plus the one the caller holds the measured difference is a multiple of it)."""
    from yolact_minimal_amd.modules.yolact import Yolact
    from yolact_minimal_amd.pipeline import RequestPipeline
    from yolact_minimal_amd.utils.output_utils import PackedMasks, pack_reference
    dev = torch.device(DEV)
    h, w = 480, 640
    cfg = build_cfg('res50_coco', 'val', 544)
    torch.manual_seed(0)
    net = Yolact(cfg).eval().to(dev)
    head = [t.to(dev) for t in R.synth_head_outputs(18525, seed=1, bg_bias=4.0)]             # the post_dense544 head tensors
    img = torch.randn(1, 3, 544, 544, generator=torch.Generator().manual_seed(2)).to(dev)

    def run(packed):
        pipe = RequestPipeline(net, cfg, 544, 544, dev, depth=2, out_hw=(h, w), packed_masks=packed)
        pipe.warm_up(img, head)
        got = [pipe.submit(img, head) for _ in range(3)]
        got = [r for r in got if r is not None] + pipe.drain()
        assert len(got) == 3
        res = [(r[0].cpu(), r[1].cpu(), r[2].cpu(), r[3].bits.cpu().numpy() if packed else pack_reference(r[3].cpu().numpy())) for r in got]
        assert all(isinstance(r[3], PackedMasks) == packed for r in got)
        del got
        torch.cuda.synchronize(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        for _ in range(8):
            pipe.submit(img, head)                                                          # the result is dropped at once
        pipe.drain()
        torch.cuda.synchronize(dev)
        peak = torch.cuda.max_memory_allocated(dev)
        del pipe
        torch.cuda.empty_cache()
        return res, peak

    dense, peak_dense = run(False)
    packed, peak_packed = run(True)
    for a, b in zip(dense, packed):
        assert a[0].numel() == 100
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    md = cfg.max_detections
    least = md * h * w * 4 - md * h * ((w + 63) // 64) * 8
    print(f'peak device memory over 8 requests: dense {peak_dense} B, packed {peak_packed} B, difference {peak_dense - peak_packed} B '
          f'(least guaranteed {least} B)')
    assert peak_dense - peak_packed >= least, (peak_dense, peak_packed, least)


def test_eval_loop_packed_masks_agrees_with_dense(tmp_path):
    code = r'''
import os, sys
sys.path[:0] = [os.path.join(REPO, 'dropin'), REPO]
os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')
import torch
import reference_loops as L
import bench
from yolact_minimal_amd.utils.synthetic import synth_eval_case
dev = torch.device('cuda:0')
net, cfg, img = bench.detecting_net('res50_coco', 256, dev)
h, w = 96, 128
_, _, _, _, gt, gt_masks, _, _ = synth_eval_case(1, 40, 7, h, w, 10)
loader = lambda: [(img, gt.clone(), gt_masks, h, w) for _ in range(2)]
for api in (True, 'device'):
    _, mj_d, seen_d, _ = L.eval_loop(net, cfg, loader(), coco_api=api)
    _, mj_p, seen_p, _ = L.eval_loop(net, cfg, loader(), coco_api=api, packed_masks=True)
    assert seen_d == seen_p == 2 and len(mj_d.mask_data) > 10
    assert mj_d.bbox_data == mj_p.bbox_data and mj_d.mask_data == mj_p.mask_data, api
ap_d, _, _, _ = L.eval_loop(net, cfg, loader(), coco_api=False)
ap_p, _, _, _ = L.eval_loop(net, cfg, loader(), coco_api=False, packed_masks=True)
cells = 0
for kind in ('box', 'mask'):
    for k in range(len(L.IOU_THRES)):
        for c in range(len(cfg.class_names)):
            a, b = ap_d[kind][k][c], ap_p[kind][k][c]
            assert a.num_gt_positives == b.num_gt_positives and list(a.data_points) == list(b.data_points), (kind, k, c)
            cells += bool(a.data_points)
assert cells > 0
print('EVAL_LOOP_PACKED_OK', len(mj_d.mask_data), cells)
'''
    r = subprocess.run([sys.executable, '-c', f'REPO = {REPO!r}\n' + code], cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and 'EVAL_LOOP_PACKED_OK' in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
