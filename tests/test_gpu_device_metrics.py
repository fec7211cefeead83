"""GPU: the device-resident mAP accumulator (`utils/device_metrics.DeviceAPData`: `ym_eval_match_log`, `ym_eval_ap`) against the
oracle, the reference goldens and the host `prep_metrics` + `calc_map`, bit for bit; `eval_loop(device_metrics=True)` and
`evaluate_pipelined` against the default loop."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import device_metrics_ref as R
from tests.conftest import REPO

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GOLD = np.load(os.path.join(REPO, 'tests', 'golden', 'metrics.npz'))
THRES = R.THRES
T = len(THRES)
KINDS = ('box', 'mask')


def _cells(ap_data, nc):
    return [ap_data[kind][k][c] for kind in KINDS for k in range(T) for c in range(nc)]


def _points(ap_data, nc):
    return [(a.num_gt_positives, list(a.data_points)) for a in _cells(ap_data, nc)]


def _accumulate(images, nc, max_det=16, order=None, streams=None, **kw):
    from yolact_minimal_amd.utils.common_utils import DeviceAPData
    acc = DeviceAPData(nc, THRES, DEV, max_det=max_det, **kw)
    args = [R.to_device(im, DEV, max_det=max_det) for im in images]
    if order is None:
        for a in args:
            acc.add(*a)
        return acc
    cur = torch.cuda.current_stream()
    for s in streams:
        s.wait_stream(cur)                                  # the uploads above ran on the current stream
    for turn, i in enumerate(order):
        with torch.cuda.stream(streams[turn % len(streams)]):
            assert acc.add(*args[i], image_index=i) == i
    for s in streams:
        ev = torch.cuda.Event()
        ev.record(s)
        cur.wait_event(ev)
    return acc


@functools.lru_cache(maxsize=None)
def _sequence_reference():
    """The six-image sequence through the HOST path on the same inputs: (points in push order, points after get_ap's sort, APs,
    table text); computed once."""
    from yolact_minimal_amd.utils import common_utils as C
    nc = R.SEQUENCE_CLASSES
    ap = {k: [[C.APDataObject() for _ in range(nc)] for _ in THRES] for k in KINDS}
    for ids, scores, boxes, masks, gt, gt_masks, h, w in R.sequence_images():
        C.prep_metrics(ap, ids, scores, boxes.to(DEV), masks.to(DEV), gt.clone().to(DEV), gt_masks.to(DEV), h, w, THRES)
    pushed = _points(ap, nc)
    aps = [a.get_ap() for a in _cells(ap, nc)]
    return pushed, _points(ap, nc), aps, C.calc_map(ap, THRES, nc, step=0)


def _assert_equals_sequence(acc):
    nc = R.SEQUENCE_CLASSES
    pushed, sorted_pts, aps, table = _sequence_reference()
    got = acc.to_ap_data()
    assert _points(got, nc) == pushed
    grid, empty = acc.ap_grid()
    assert [a.get_ap() for a in _cells(got, nc)] == aps
    assert _points(got, nc) == sorted_pts                   # identical after get_ap's in-place stable sort
    flat = grid.reshape(-1).tolist()
    assert flat == [float(v) for v in aps] and not empty.any()
    assert acc.calc_map(step=0) == table


@pytest.mark.parametrize('packed', [False, True], ids=['dense', 'packed'])
@pytest.mark.parametrize('case', [0, 1, 2])
def test_golden_cases(case, packed):
    """Padded to max_det = 128 rows with NaN scores, class 3 and all-ones masks past the count: the cells equal the oracle's, the
    AP grid equals the reference's `c*_ap_grid` with ==, the calc_map rows equal the golden rows."""
    from yolact_minimal_amd.utils.common_utils import DeviceAPData
    images, nc = R.golden_images(GOLD, case)
    acc = DeviceAPData(nc, THRES, DEV, max_det=128, capacity_images=2)
    acc.add(*R.to_device(images[0], DEV, max_det=128, packed=packed))
    got, ref = acc.to_ap_data(), R.oracle_accumulate(images, nc)
    assert _points(got, nc) == _points(ref, nc)
    grid, empty = acc.ap_grid()
    rows = [[a.num_gt_positives, len(a.data_points), sum(1 for p in a.data_points if p[1]), v]
            for a, v in zip(_cells(got, nc), grid.reshape(-1).tolist())]
    assert np.array_equal(np.array(rows, dtype=np.float64), GOLD[f'c{case}_ap_grid'])
    assert empty.tolist() == [a.is_empty() for a in ref['box'][0]]
    _, row2, row3 = acc.calc_map(step=0)
    assert row2[1:] == [round(v, 2) for v in GOLD[f'c{case}_map_box']] and row3[1:] == [round(v, 2) for v in GOLD[f'c{case}_map_mask']]


def test_sequence_equals_host_path_and_an_image_without_detections_counts_nothing():
    images = R.sequence_images()
    acc = _accumulate(images, R.SEQUENCE_CLASSES)
    _assert_equals_sequence(acc)
    # a seventh image whose count is 0 and whose gt is not empty: eval.py:53-54 skips it before prep_metrics
    args = list(R.to_device(images[1], DEV, max_det=16))
    args[4] = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert acc.add(*args) == 6 and acc.images == 7
    _assert_equals_sequence(acc)


def test_permuted_order_on_two_streams():
    images = R.sequence_images()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    acc = _accumulate(images, R.SEQUENCE_CLASSES, order=[3, 0, 5, 1, 4, 2], streams=streams)
    _assert_equals_sequence(acc)
    with pytest.raises(RuntimeError):
        acc.add(*R.to_device(images[2], DEV, max_det=16), image_index=2)


def test_log_growth():
    acc = _accumulate(R.sequence_images(), R.SEQUENCE_CLASSES, capacity_images=2)
    assert acc.capacity >= 6
    _assert_equals_sequence(acc)


def _many_rows_case(n_img, md, g, last):
    """`n_img` images of 8 x 8 pixels with `md` detection rows each: 6 x 6 ground-truth squares, predictions = a square moved and
    shrunk by 0 / 1 pixel (IoUs spread over the thresholds), every other mask without its corner pixel (mask IoU != box IoU);
    scores from 16 values, descending within an image like after_nms' rows; the last image has `last` rows, its last one of class 1."""
    rng = np.random.default_rng(7)
    rect = rng.integers(0, 3, (n_img, g, 2))
    gt = np.zeros((n_img, g, 5), np.float32)
    gt_masks = np.zeros((n_img, g, 8, 8), np.float32)
    for i in range(n_img):
        for j in range(g):
            x, y = rect[i, j]
            gt[i, j] = [x / 8, y / 8, (x + 6) / 8, (y + 6) / 8, 0 if j < 3 else 1]
            gt_masks[i, j, y:y + 6, x:x + 6] = 1
    pick = rng.integers(0, g, (n_img, md))
    move = rng.integers(0, 2, (n_img, md, 4))
    boxes = np.zeros((n_img, md, 4), np.int32)
    masks = np.zeros((n_img, md, 8, 8), np.float32)
    for i in range(n_img):
        for r in range(md):
            x, y = rect[i, pick[i, r]] + move[i, r, :2]
            x2, y2 = min(x + 6 - move[i, r, 2], 8), min(y + 6 - move[i, r, 3], 8)
            boxes[i, r] = [x, y, x2, y2]
            masks[i, r, y:y2, x:x2] = 1
            if r % 2:
                masks[i, r, y, x] = 0
    scores = -np.sort(-((rng.integers(0, 16, (n_img, md)) + 0.5) / 16).astype(np.float32), axis=1)
    ids = np.zeros((n_img, md), np.int64)
    ids[-1, last - 1] = 1
    counts = np.full((n_img, 1), md, np.int32)
    counts[-1] = last
    return ids, scores, boxes, masks, counts, gt, gt_masks


def test_many_rows_in_one_class_walks_several_passes():
    """3 * EVAL_AP_ROWS_PER_PASS + 37 rows of class 0 (and one of class 1) from small images; 16 distinct scores, so every pass
    boundary of the sorted class cuts a run of equal scores.  All cells against the host `APDataObject.get_ap` of `to_ap_data()`."""
    from yolact_minimal_amd import hip
    from yolact_minimal_amd.utils.common_utils import DeviceAPData
    rpp, md, g = hip.EVAL_AP_ROWS_PER_PASS, 100, 4
    want_rows = 3 * rpp + 37
    n_img = -(-(want_rows + 1) // md)
    last = want_rows + 1 - (n_img - 1) * md                  # rows of the last image: the rest of class 0 and the one row of class 1
    ids, scores, boxes, masks, counts, gt, gt_masks = _many_rows_case(n_img, md, g, last)
    dev = [torch.from_numpy(a).to(DEV) for a in (ids, scores, boxes, masks, counts, gt, gt_masks)]
    acc = DeviceAPData(2, THRES, DEV, max_det=md, capacity_images=8)
    for i in range(n_img):
        acc.add(dev[0][i], dev[1][i], dev[2][i], dev[3][i], dev[4][i], dev[5][i], dev[6][i], 8, 8)
    got = acc.to_ap_data()
    pts = got['box'][0][0].data_points
    assert len(pts) == want_rows and len(got['mask'][3][1].data_points) == 1
    ranked = sorted(p[0] for p in pts)[::-1]
    for b in (rpp, 2 * rpp, 3 * rpp):
        assert ranked[b - 1] == ranked[b]                    # the pass boundary lies inside a tie run
    grid, empty = acc.ap_grid()
    want = [a.get_ap() for a in _cells(got, 2)]
    assert grid.reshape(-1).tolist() == [float(v) for v in want] and not empty.any()
    assert len(set(want[0::2])) >= 10                         # (a live case: class 0's cells differ from one another)


@pytest.mark.parametrize('packed', [False, True], ids=['dense', 'packed'])
def test_add_reads_nothing_on_the_host(packed):
    from yolact_minimal_amd.utils.common_utils import DeviceAPData
    images = R.sequence_images()
    acc = DeviceAPData(R.SEQUENCE_CLASSES, THRES, DEV, max_det=16)
    acc.add(*R.to_device(images[0], DEV, max_det=16, packed=packed))          # warm-up: library, thresholds, scratch
    args = R.to_device(images[1], DEV, max_det=16, packed=packed)
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
        acc.add(*args)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    ref = R.oracle_accumulate(images[:2], R.SEQUENCE_CLASSES)
    assert _points(acc.to_ap_data(), R.SEQUENCE_CLASSES) == _points(ref, R.SEQUENCE_CLASSES)


def test_a_refused_add_consumes_no_image_index():
    from yolact_minimal_amd.utils.common_utils import DeviceAPData
    images = R.sequence_images()
    acc = DeviceAPData(R.SEQUENCE_CLASSES, THRES, DEV, max_det=16)
    ids, scores, boxes, masks, counts, gt, gt_masks, h, w = R.to_device(images[0], DEV, max_det=16)
    for bad in ((ids, scores[:-1], boxes, masks, counts, gt, gt_masks, h, w), (ids, scores, boxes, masks, counts, gt[:, :4], gt_masks, h, w),
                (ids, scores, boxes, masks, counts, gt, gt_masks[:-1], h, w)):
        with pytest.raises(RuntimeError):
            acc.add(*bad)
    assert acc.images == 0
    assert acc.add(ids, scores, boxes, masks, counts, gt, gt_masks, h, w) == 0          # (gt was not scaled by the refused calls)
    ref = R.oracle_accumulate(images[:1], R.SEQUENCE_CLASSES)
    assert _points(acc.to_ap_data(), R.SEQUENCE_CLASSES) == _points(ref, R.SEQUENCE_CLASSES)


_LOOPS = r'''
import os, sys
sys.path[:0] = [os.path.join(REPO, 'dropin'), REPO]
assert os.environ['GPU_MAX_HW_QUEUES'] == '8'
import torch
import reference_loops as L
import bench
from yolact_minimal_amd.evaluate import eval_pipeline, evaluate_pipelined
from yolact_minimal_amd.pipeline import RequestPipeline
from yolact_minimal_amd.utils.synthetic import synth_eval_case
from utils.output_utils import nms, after_nms
dev = torch.device('cuda:0')
net, cfg, img = bench.detecting_net('res50_coco', 256, dev)
nc = len(cfg.class_names)
samples = []
for i in range(6):
    h, w = (96, 128) if i % 2 == 0 else (80, 112)
    _, _, _, _, gt, gt_masks, _, _ = synth_eval_case(i + 1, 40, 7, h, w, 10)
    samples.append((img, gt, gt_masks, h, w))
loader = lambda: [(im, gt.clone(), gm, h, w) for im, gt, gm, h, w in samples]
def points(ap):
    return [(ap[k][t][c].num_gt_positives, list(ap[k][t][c].data_points)) for k in ('box', 'mask') for t in range(10) for c in range(nc)]
ap, _, seen, _ = L.eval_loop(net, cfg, loader())
acc, _, seen2, _ = L.eval_loop(net, cfg, loader(), device_metrics=True)
assert seen == seen2 == 6 and sum(len(a.data_points) for a in ap['box'][0]) > 60
dev_pts = points(acc.to_ap_data())
assert dev_pts == points(ap)
want = L.table(ap, cfg, step=0)
assert L.table(acc, cfg, step=0) == want
print('EVAL_LOOP_DEVICE_OK', seen, flush=True)
for packed in (True, False):
    got, acc2 = evaluate_pipelined(net, cfg, loader(), depth=4, packed_masks=packed, step=0)
    assert got == want, (got, want)
    assert points(acc2.to_ap_data()) == dev_pts
shared = eval_pipeline(net, cfg, img, 96, 128, depth=4)              # one pipeline, two sample sets: nothing of the first is left
for _ in range(2):
    got, acc3 = evaluate_pipelined(net, cfg, loader(), step=0, pipe=shared)
    assert got == want, (got, want)
    assert points(acc3.to_ap_data()) == dev_pts
print('PIPELINED_OK', flush=True)
pipe = RequestPipeline(net, cfg, 256, 256, dev, depth=2, out_hw=(96, 128))
pipe.warm_up(img, rounds=0)
assert pipe.submit(img) is None
(res,) = pipe.drain()
with torch.no_grad():
    o = net(img)
ref = after_nms(*nms(*o, net.anchors, cfg), 96, 128)
assert all(torch.equal(a, b) for a, b in zip(res, ref))
pipe.vt = 0.3                                                        # (cfg.visual_thre as the pipeline read it)
try:
    pipe.submit(img, consumer=lambda *r: None)
    raise AssertionError('a consumer would have seen rows under cfg.visual_thre')
except RuntimeError as e:
    assert 'visual_thre' in str(e)
assert pipe.drain() == []
print('SUBMIT_UNCHANGED_OK', flush=True)
'''


@functools.lru_cache(maxsize=None)
def _loops_output():
    """Both loops on one detecting network in ONE child process, started with GPU_MAX_HW_QUEUES=8 in its environment (whatever this
    process inherited): a queue per slot of the depth-4 pipeline, as serving sets it."""
    r = subprocess.run([sys.executable, '-c', f'REPO = {REPO!r}\n' + _LOOPS], cwd=REPO, capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, GPU_MAX_HW_QUEUES='8'))
    return r.stdout + '\n--- stderr ---\n' + r.stderr[-3000:]


def test_eval_loop_device_metrics_gives_the_default_table():
    assert 'EVAL_LOOP_DEVICE_OK 6' in _loops_output(), _loops_output()


def test_evaluate_pipelined_gives_the_loop_table_and_submit_is_unchanged():
    out = _loops_output()
    assert 'PIPELINED_OK' in out and 'SUBMIT_UNCHANGED_OK' in out, out
