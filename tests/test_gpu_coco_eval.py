"""GPU: the device-resident COCO evaluator (`utils/coco_eval.DeviceCOCOeval`: `ym_coco_iou_box`, `ym_coco_iou_mask_packed`,
`ym_coco_match_log`, `ym_coco_accumulate`) against the host restatement of the cocoapi protocol (`tests/coco_eval_ref.py`).  Every
comparison is exact: integers and flags bit for bit, fp64 grids with `np.array_equal`, summary text as strings."""
import functools
import json
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import coco_eval_ref as R
from tests.conftest import REPO

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KINDS = ('bbox', 'segm')


def _feed(scene, nc, max_det, order=None, streams=None, packed=True, pad=True, **kw):
    from yolact_minimal_amd.utils.common_utils import DeviceCOCOeval
    ev = DeviceCOCOeval(nc, DEV, max_det=max_det, **kw)
    args = [R.image_to_device(im, DEV, max_det, packed=packed, pad=pad) for im in scene]
    if order is None:
        for i, a in enumerate(args):
            assert ev.add(*a) == i
        return ev
    cur = torch.cuda.current_stream()
    for s in streams:
        s.wait_stream(cur)                                  # the uploads above ran on the current stream
    for turn, i in enumerate(order):
        with torch.cuda.stream(streams[turn % len(streams)]):
            assert ev.add(*args[i], image_index=i) == i
    for s in streams:
        e = torch.cuda.Event()
        e.record(s)
        cur.wait_event(e)
    return ev


def _assert_equals(ev, ref, scene, nc, max_det):
    """Log (classes, ranks, matched / ignored bits, npig), grids and summary text against the restatement's."""
    cls, rank, flags, npig = ev.log()
    want_cls, want_rank, want_flags, want_npig = R.scene_log(ref, scene, nc, max_det)
    rows = len(scene) * max_det
    assert np.array_equal(cls[:rows], want_cls) and (cls[rows:] == -1).all()
    assert np.array_equal(rank[:rows], want_rank)
    assert np.array_equal(flags[:rows], want_flags)
    assert np.array_equal(npig, want_npig)
    grids = ev.accumulate()
    summary = ev.summarize(grids)
    for kind in KINDS:
        assert np.array_equal(grids[kind][0], ref[kind].eval['precision']), kind
        assert np.array_equal(grids[kind][1], ref[kind].eval['recall']), kind
        want_stats, want_text = ref[kind].summarize()
        assert np.array_equal(summary[kind][0], want_stats) and summary[kind][1] == want_text


@functools.lru_cache(maxsize=None)
def _random_reference():
    return R.evaluate_scene(R.random_sequence(), R.RANDOM_CLASSES)


def test_iou_kernels():
    """37 x 70 masks (two words per row, a ragged tail), n = 5, g = 4: a crowd gt, an empty detection mask, an empty gt mask,
    disjoint boxes and boxes that touch (w == 0); dense and packed detection masks give the same bits."""
    from yolact_minimal_amd import hip
    from yolact_minimal_amd.utils.packed_masks import PackedMasks, pack_reference
    h, w, n, g = 37, 70, 5, 4
    rng = np.random.default_rng(5)
    dm = rng.random((n, h, w)) < 0.5
    gm = rng.random((g, h, w)) < 0.4
    dm[:, :, 64:] |= rng.random((n, h, 6)) < 0.7             # the tail word is busy
    dm[3] = False                                            # an empty detection mask
    gm[2] = False                                            # an empty gt mask
    gm[1] = dm[0] | (rng.random((h, w)) < 0.3)               # the crowd covers detection 0: IoU 1 with it
    crowd = np.array([0, 1, 0, 0], np.uint8)
    dt = np.array([[0, 0, 10, 10], [20, 5, 7.5, 9.25], [0.5, 0.5, 30, 30], [40, 40, 5, 5], [3, 3, 4, 4]], np.float64)
    gt = np.array([[10, 0, 10, 10],                          # touches detection 0: w == 0
                   [0, 0, 50, 50],                           # crowd
                   [100, 100, 5, 5],                         # disjoint from all
                   [2, 2, 9, 11.5]], np.float64)
    want_box, want_mask = R.bbIou(dt, gt, crowd), R.maskIou(list(dm), list(gm), crowd)
    assert want_box[0, 0] == 0 and (want_box[:, 2] == 0).all() and want_mask[0, 1] == 1 and (want_mask[3] == 0).all()
    up = lambda a: torch.from_numpy(a).to(DEV)               # noqa: E731
    d_crowd, d_dt, d_gt = up(crowd), up(dt), up(gt)           # (named: a temporary would be freed once its pointer is taken)
    iou = torch.empty(n, g, dtype=torch.float64, device=DEV)
    hip.check(hip.lib().ym_coco_iou_box(hip.ptr(d_dt, torch.float64), n, hip.ptr(d_gt, torch.float64), g, hip.ptr(d_crowd, torch.uint8),
                                        hip.ptr(iou, torch.float64), hip.stream_ptr()), 'ym_coco_iou_box')
    assert np.array_equal(iou.cpu().numpy(), want_box)
    gbits = PackedMasks.pack(up(gm.astype(np.uint8)))
    from_dense = PackedMasks.pack(up(dm.astype(np.float32)))
    from_words = PackedMasks(up(pack_reference(dm)), h, w)
    assert torch.equal(from_dense.bits, from_words.bits)
    for pm in (from_dense, from_words):
        iou = torch.full((n, g), -7.0, dtype=torch.float64, device=DEV)
        area = torch.full((n,), -7, dtype=torch.int32, device=DEV)
        hip.check(hip.lib().ym_coco_iou_mask_packed(hip.ptr(pm.bits, torch.int64), n, hip.ptr(gbits.bits, torch.int64), g, h * pm.bits.shape[-1],
                                                    hip.ptr(d_crowd, torch.uint8), hip.ptr(iou, torch.float64), hip.ptr(area, torch.int32),
                                                    hip.stream_ptr()), 'ym_coco_iou_mask_packed')
        assert np.array_equal(iou.cpu().numpy(), want_mask)
        assert area.cpu().tolist() == dm.reshape(n, -1).sum(1).tolist()


@pytest.mark.parametrize('name', list('ABCDEFGH'))
def test_known_answers_on_device(name):
    scene, nc = R.known_answer_scenes()[name]
    ref = R.evaluate_scene(scene, nc)
    ev = _feed(scene, nc, 16)
    _assert_equals(ev, ref, scene, nc, 16)


def test_random_sequence():
    scene = R.random_sequence()
    for what, there in R.random_sequence_situations(scene).items():
        assert there, what
    ev = _feed(scene, R.RANDOM_CLASSES, 16)
    _assert_equals(ev, _random_reference(), scene, R.RANDOM_CLASSES, 16)
    # dense detection masks and unpadded rows (counts=None) are the same evaluation
    ev = _feed(scene, R.RANDOM_CLASSES, 16, packed=False, pad=False)
    _assert_equals(ev, _random_reference(), scene, R.RANDOM_CLASSES, 16)


def test_many_rows_in_one_class_walks_several_passes():
    """12 images x 100 detections of one class: 1200 sorted rows, more than one pass of `ym_coco_accumulate` holds; 16 distinct
    scores, so the pass boundary cuts a run of equal scores."""
    from yolact_minimal_amd import hip
    scene = R.many_rows_scene(12, 100)
    assert 12 * 100 > hip.COCO_ROWS_PER_PASS
    ref = R.evaluate_scene(scene, 1)
    ev = _feed(scene, 1, 100, pad=False, capacity_images=16)
    _assert_equals(ev, ref, scene, 1, 100)
    assert len(set(ref['segm'].eval['precision'][:, 50, 0, 0, 2].tolist())) >= 3      # (a live case)


def test_permuted_order_on_two_streams():
    scene = R.random_sequence()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    ev = _feed(scene, R.RANDOM_CLASSES, 16, order=[3, 0, 5, 1, 4, 2], streams=streams)
    _assert_equals(ev, _random_reference(), scene, R.RANDOM_CLASSES, 16)
    with pytest.raises(RuntimeError):
        ev.add(*R.image_to_device(scene[2], DEV, 16), image_index=2)


def test_log_growth():
    scene = R.random_sequence()
    ev = _feed(scene, R.RANDOM_CLASSES, 16, capacity_images=2)
    assert ev.capacity >= 6
    _assert_equals(ev, _random_reference(), scene, R.RANDOM_CLASSES, 16)


@pytest.mark.parametrize('packed', [False, True], ids=['dense', 'packed'])
def test_add_reads_nothing_on_the_host(packed):
    from yolact_minimal_amd.utils.common_utils import DeviceCOCOeval
    scene = R.random_sequence()
    ev = DeviceCOCOeval(R.RANDOM_CLASSES, DEV, max_det=16)
    ev.add(*R.image_to_device(scene[0], DEV, 16, packed=packed))                      # warm-up: library, scratch
    args = R.image_to_device(scene[1], DEV, 16, packed=packed)
    empty = R.image_to_device(scene[4], DEV, 16, packed=packed)                       # (no detections: only its gts count)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        try:
            torch.ones(1, device=DEV).item()
            control = False
        except RuntimeError:
            control = True
        if not control:
            pytest.skip('torch.cuda.set_sync_debug_mode("error") does not flag .item() on this machine')
        ev.add(*args)
        ev.add(*empty)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    part = [scene[0], scene[1], scene[4]]
    _assert_equals(ev, R.evaluate_scene(part, R.RANDOM_CLASSES), part, R.RANDOM_CLASSES, 16)


def test_a_refused_add_consumes_no_image_index():
    from yolact_minimal_amd.utils.coco_eval import COCOGt
    from yolact_minimal_amd.utils.common_utils import DeviceCOCOeval
    scene = R.random_sequence()
    ev = DeviceCOCOeval(R.RANDOM_CLASSES, DEV, max_det=16)
    ids, scores, boxes, masks, counts, gt = R.image_to_device(scene[0], DEV, 16)
    g = 513
    big = COCOGt.from_arrays(np.zeros(g, np.int32), np.zeros(g, np.uint8), np.full(g, 50.0), np.tile([0.0, 0.0, 5.0, 10.0], (g, 1)),
                             torch.ones(g, scene[0]['h'], scene[0]['w'], dtype=torch.uint8), scene[0]['h'], scene[0]['w'], DEV)
    with pytest.raises(RuntimeError, match='512'):
        ev.add(ids, scores, boxes, masks, counts, big)
    for bad in ((ids, scores[:-1], boxes, masks, counts, gt), (ids, scores, boxes[:-1], masks, counts, gt),
                (ids, scores, boxes, masks[:-1], counts, gt)):
        with pytest.raises(RuntimeError):
            ev.add(*bad)
    assert ev.images == 0
    assert ev.add(ids, scores, boxes, masks, counts, gt) == 0
    _assert_equals(ev, R.evaluate_scene(scene[:1], R.RANDOM_CLASSES), scene[:1], R.RANDOM_CLASSES, 16)


def test_score_results_equals_in_memory(tmp_path):
    """The random sequence through `MakeJson.dump` and an annotation file: `score_results` on the files = `DeviceCOCOeval` fed
    directly = the restatement; the bbox file alone gives the bbox half."""
    from yolact_minimal_amd.utils.common_utils import MakeJson, rle_encode, score_results
    scene = R.random_sequence()
    image_ids = [11, 22, 33, 44, 55, 66]
    cat_ids = [3, 7, 11, 20, 42]
    label_map = {c: k + 1 for k, c in enumerate(cat_ids)}
    ann_file, bbox_file, mask_file = (str(tmp_path / n) for n in ('ann.json', 'bbox_detections.json', 'mask_detections.json'))
    with open(ann_file, 'w') as f:
        json.dump(R.scene_annotation_dict(scene, image_ids, cat_ids), f)
    mj = MakeJson(label_map)
    for img_id, im in zip(image_ids, scene):
        ids, scores, boxes, masks, _, _ = R.image_to_device(im, DEV, 16, pad=False)
        if ids is None:
            continue
        rles = rle_encode(masks)
        for j, d in enumerate(im['dets']):                   # eval.py:60-67
            b = d['box']
            if (b[3] - b[1]) * (b[2] - b[0]) > 0:
                mj.add_bbox(img_id, d['cls'], np.array(b), float(d['score']))
                mj.add_mask(img_id, d['cls'], rles[j], float(d['score']))
    mj.dump(bbox_file, mask_file)
    ev = _feed(scene, R.RANDOM_CLASSES, 16)
    grids, summary = ev.accumulate(), ev.summarize()
    got = score_results(ann_file, bbox_file, mask_file, device=DEV)
    alone = score_results(ann_file, bbox_json=bbox_file, device=DEV)
    assert sorted(got) == ['bbox', 'segm'] and sorted(alone) == ['bbox']
    ref = _random_reference()
    for kind, res in [(k, got[k]) for k in KINDS] + [('bbox', alone['bbox'])]:
        assert np.array_equal(res['precision'], grids[kind][0]) and np.array_equal(res['recall'], grids[kind][1])
        assert np.array_equal(res['stats'], summary[kind][0]) and res['text'] == summary[kind][1]
        assert res['text'] == ref[kind].summarize()[1]
    stray = str(tmp_path / 'stray.json')
    with open(stray, 'w') as f:
        json.dump([{'image_id': 77, 'category_id': 3, 'bbox': [0, 0, 5, 5], 'score': 0.5}], f)
    with pytest.raises(AssertionError):
        score_results(ann_file, bbox_json=stray, device=DEV)


_LOOP = r'''
import os, sys, json
sys.path[:0] = [os.path.join(REPO, 'dropin'), REPO]
import numpy as np
import torch
import reference_loops as L
import bench
from tests import coco_eval_ref as R
from yolact_minimal_amd.utils.coco import COCO
from yolact_minimal_amd.utils.synthetic import synth_eval_case
dev = torch.device('cuda:0')
net, cfg, img = bench.detecting_net('res50_coco', 64, dev)
scene = R.random_sequence()[:3]
h, w = scene[0]['h'], scene[0]['w']
image_ids = [30, 10, 20]                                   # not ascending: cocoapi evaluates in ascending image id
cats = {v - 1: k for k, v in cfg.continuous_id.items()}    # class index -> COCO category id
classes = [0, 1, 2, 16, 79]                                # the scene's classes 0..4 as classes of the 80
ann = R.scene_annotation_dict(scene, image_ids, [cats[c] for c in classes])
ann['categories'] = [{'id': k, 'name': str(k)} for k in sorted(cfg.continuous_id)]
ann_file = os.path.join(TMP, 'ann.json')
with open(ann_file, 'w') as f:
    json.dump(ann, f)
coco = COCO(ann_file, device=dev)
_, _, _, _, gt, gt_masks, _, _ = synth_eval_case(1, 40, 7, h, w, 10)
loader = lambda: [(img, gt.clone(), gt_masks, h, w) for _ in image_ids]
ap, none, seen, _ = L.eval_loop(net, cfg, loader())
acc, _, _, _ = L.eval_loop(net, cfg, loader(), device_metrics=True)
assert none is None and seen == 3 and L.table(ap, cfg, step=0) == L.table(acc, cfg, step=0)
_, mj, seen2, _ = L.eval_loop(net, cfg, loader(), image_ids=image_ids, coco_api='device')
assert seen2 == 3 and len(mj.bbox_data) >= 9, len(mj.bbox_data)
_, scorer, seen3, _ = L.eval_loop(net, cfg, loader(), image_ids=image_ids, coco_api='score', coco=coco)
assert seen3 == 3 and scorer.images == 3
want = L.coco_summary(mj, ann_file, label_map=cfg.continuous_id)
got = L.coco_summary(scorer)
for kind in ('bbox', 'segm'):
    assert np.array_equal(got[kind][0], want[kind][0]) and got[kind][1] == want[kind][1], kind
print('COCO_SCORE_OK', len(mj.bbox_data), flush=True)
'''


def test_eval_loop_coco_score(tmp_path):
    """A seeded res50 network at 64 px on a 3-image synthetic dataset, in a child process bound through `dropin/` like
    `dropin/run.py`: `eval_loop(coco_api='score')` = `coco_summary` on the JSONs of `eval_loop(coco_api='device')`, and the default
    loop's table is what it was (= the device accumulator's)."""
    r = subprocess.run([sys.executable, '-c', f'REPO = {REPO!r}\nTMP = {str(tmp_path)!r}\n' + _LOOP], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'COCO_SCORE_OK' in r.stdout, (r.stdout[-2500:], r.stderr[-3000:])
    assert r.stdout.count('Evaluating BBoxes:') == 2 and r.stdout.count('Evaluating Masks:') == 2
    assert r.stdout.count(' Average Recall     (AR) @[ IoU=0.50:0.95 | area= large | maxDets=100 ] = ') == 4
