"""The batched COCO metric stage on the GPU: `DeviceCOCOeval.add_batch` (`ym_eval_coco_add_ragged_packed`) writes, bit for bit, what
`DeviceCOCOeval.add` writes image by image -- and what the host restatement of the cocoapi protocol (`tests/coco_eval_ref.py`) says --
at the word, chunk, group, batch-size and padding edges; `coco_gt_batch` equals `COCOGtBatch.from_gts`;
`evaluate_coco_pipelined(batched_metrics=True)` gives the per-image loop's evaluator.  Every comparison is exact: the logs, `npig` and
`class_rows` are integers, the grids fp64 quotients of integers.  Rows past an image's count carry NaN scores, the valid class 0, a
full box and all-ones masks, so a kernel that looks past the count is caught."""
import functools
import json

import numpy as np
import pytest
import torch

from tests import coco_eval_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KINDS = ('bbox', 'segm')
MD = 16


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _image(seed, h, w, n_det, n_gt, nc=3, crowd=0.2):
    """One scene image of h x w: `n_gt` gts (rectangles with a notch; `area` = the mask's pixels; about a fifth crowds) and `n_det`
    detections, most of them a gt moved by a pixel or two, scores in sixteenths, in score-descending row order."""
    rng = np.random.default_rng(seed)

    def box(lo):
        bw, bh = int(rng.integers(min(lo, w), w + 1)), int(rng.integers(min(lo, h), h + 1))
        return int(rng.integers(0, w - bw + 1)), int(rng.integers(0, h - bh + 1)), bw, bh

    gts = []
    for _ in range(n_gt):
        x, y, bw, bh = box(2)
        m = R._rect_mask(h, w, x, y, x + bw, y + bh)
        m[y:y + bh // 4, x:x + bw // 4] = False
        gts.append({'cls': int(rng.integers(0, nc)), 'bbox': [float(x), float(y), float(bw), float(bh)], 'area': int(m.sum()),
                    'iscrowd': int(rng.random() < crowd), 'mask': m})
    dets = []
    for _ in range(n_det):
        if gts and rng.random() < 0.8:
            q = gts[int(rng.integers(0, len(gts)))]
            x, y, bw, bh = (int(v) for v in q['bbox'])
            j = rng.integers(-1, 2, 4)
            x1, y1 = min(max(x + j[0], 0), w - 1), min(max(y + j[1], 0), h - 1)
            x2, y2 = min(max(x + bw + j[2], x1 + 1), w), min(max(y + bh + j[3], y1 + 1), h)
            cls = q['cls'] if rng.random() < 0.85 else int(rng.integers(0, nc))
        else:
            x, y, bw, bh = box(1)
            x1, y1, x2, y2, cls = x, y, x + bw, y + bh, int(rng.integers(0, nc))
        m = R._rect_mask(h, w, x1, y1, x2, y2)
        m[y2 - (y2 - y1) // 5:y2, x2 - (x2 - x1) // 5:x2] = False
        dets.append({'cls': cls, 'score': np.float32(int(rng.integers(1, 17)) / 16), 'box': (x1, y1, x2, y2), 'mask': m})
    dets.sort(key=lambda d: -float(d['score']))
    return {'h': h, 'w': w, 'gts': gts, 'dets': dets}


@functools.lru_cache(maxsize=None)
def _six_images():
    """5x3 (one word, one chunk); 33x70 (66 words: the last chunk has 6 of 20); 40x65 (two words per row, 63 pad bits) with an all-zero
    detection mask against an all-zero gt mask of its class (i == 0 -> 0, no NaN); 48x64 without detections: only npig moves; an image
    without ground truth whose detections are 20 x 20 px; an image whose count is max_det."""
    zero = _image(23, 40, 65, 9, 5)
    zero = {**zero, 'dets': [dict(d) for d in zero['dets']], 'gts': [dict(q) for q in zero['gts']]}
    j = 0                                                       # (a gt of detection 0's class)
    zero['gts'][j]['cls'] = zero['dets'][0]['cls']
    zero['dets'][0]['mask'] = np.zeros((40, 65), bool)
    zero['gts'][j]['mask'] = np.zeros((40, 65), bool)
    h, w = 40, 56
    lone = {'h': h, 'w': w, 'gts': [], 'dets': [R._det(h, w, k % 3, (8 - k) / 8, (3 * k, 2 * k, 3 * k + 20, 2 * k + 20)) for k in range(5)]}
    return [_image(21, 5, 3, 6, 3), _image(22, 33, 70, 12, 4), zero, _image(24, 48, 64, 0, 3), lone, _image(26, 33, 47, MD, 6)]


SIX_INDEX = [3, 5, 0, 1, 4, 2]


# ---- scenes as device inputs ----------------------------------------------------------------------------------------------------
def _rows(im, max_det):
    """`image_to_device(pad=True)`, also for an image without detections: sentinel rows and a count of 0."""
    from yolact_minimal_amd.utils.packed_masks import PackedMasks
    a = R.image_to_device(im, DEV, max_det)
    if a[0] is not None:
        return a
    h, w = im['h'], im['w']
    return (torch.zeros(max_det, dtype=torch.int64, device=DEV), torch.full((max_det,), float('nan'), device=DEV),
            torch.tensor([0, 0, w, h], dtype=torch.int32, device=DEV).repeat(max_det, 1),
            PackedMasks.pack(torch.ones(max_det, h, w, device=DEV)), torch.zeros(1, dtype=torch.int32, device=DEV), a[5])


def _ragged_views(packed_list, sizes, max_det):
    """The per-image `PackedMasks` as views of ONE `ragged_layout` allocation (what `after_nms_batch(..., packed=True)` returns);
    the words between the blocks are all ones."""
    from yolact_minimal_amd.utils.output_utils import ragged_layout
    from yolact_minimal_amd.utils.packed_masks import PackedMasks
    offsets, total = ragged_layout(sizes, max_det, True)
    flat = torch.full((total,), -1, dtype=torch.int64, device=DEV)
    views = []
    for pm, (h, w), o in zip(packed_list, sizes, offsets):
        wq = (w + 63) // 64
        view = flat[o:o + max_det * h * wq].view(max_det, h, wq)
        view.copy_(pm.bits)
        views.append(PackedMasks(view, h, w))
    return views


def _batch_args(images, max_det, pad=()):
    """(per-image `add` arguments, `add_batch`'s tensors).  `pad`: entries that `add_batch` is told to skip: NaN scores, class 0,
    all-ones masks and a full count."""
    args = [_rows(im, max_det) for im in images]
    sizes = [(im['h'], im['w']) for im in images]
    ids, scores, boxes = (torch.stack([a[k] for a in args]) for k in (0, 1, 2))
    counts = torch.cat([a[4] for a in args])
    packed = [a[3] for a in args]
    for b in pad:
        ids[b], scores[b], counts[b] = 0, float('nan'), max_det
        packed[b].bits.fill_(-1)
    return args, (ids, scores, boxes, _ragged_views(packed, sizes, max_det), counts)


def _run_both(images, index, nc, max_det=MD, pad=(), kinds=KINDS, prefill=False):
    """`images` through `add` one by one and through ONE `add_batch` -> (evaluator of add, evaluator of add_batch)."""
    from yolact_minimal_amd.utils.coco_eval import COCOGtBatch, DeviceCOCOeval
    one = DeviceCOCOeval(nc, DEV, max_det=max_det, kinds=kinds, capacity_images=4)
    many = DeviceCOCOeval(nc, DEV, max_det=max_det, kinds=kinds, capacity_images=4)
    args, (ids, scores, boxes, views, counts) = _batch_args(images, max_det, pad)
    if prefill:
        for ev in (one, many):
            ev._grow(16)
            ev.score.fill_(-7.0), ev.cls.fill_(77), ev.rank.fill_(55), ev.flags.fill_(0x5a5a5a5a)
    for b, a in enumerate(args):
        if b not in pad:
            assert one.add(*a, image_index=index[b]) == index[b]
    segm = 'segm' in kinds
    gts = [a[5] for a in args]
    if not segm:                                                # (an IoU type that is off needs none of its inputs)
        for gt in gts:
            gt.masks = None
    got = many.add_batch(ids, scores, boxes, views if segm else None, counts, COCOGtBatch.from_gts(gts),
                         [None if b in pad else index[b] for b in range(len(args))])
    assert got == [index[b] for b in range(len(args)) if b not in pad]
    torch.cuda.synchronize()
    return one, many


def _assert_same(one, many):
    assert one.images == many.images and one.capacity == many.capacity
    for name in ('score', 'cls', 'rank', 'flags', 'npig', 'class_rows'):
        assert torch.equal(getattr(one, name), getattr(many, name)), name


def _assert_reference(ev, images, index, nc, max_det=MD, kinds=KINDS):
    """Log, counters and grids against the restatement's, for images whose indices are a permutation of 0 .. len - 1."""
    scene = [None] * len(images)
    for im, i in zip(images, index):
        scene[i] = im
    ref = R.evaluate_scene(scene, nc, kinds)
    cls, rank, flags, npig = ev.log()
    want_cls, want_rank, want_flags, want_npig = R.scene_log(ref, scene, nc, max_det)
    rows = len(scene) * max_det
    assert np.array_equal(cls[:rows], want_cls) and (cls[rows:] == -1).all()
    assert np.array_equal(rank[:rows], want_rank)
    assert np.array_equal(flags[:rows], want_flags)
    assert np.array_equal(npig, want_npig)
    grids = ev.accumulate()
    for kind in kinds:
        assert np.array_equal(grids[kind][0], ref[kind].eval['precision']), kind
        assert np.array_equal(grids[kind][1], ref[kind].eval['recall']), kind
    return ref


# ---- tests ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list('ABCDEFGH'))
def test_known_answers_in_one_add_batch(name):
    """The scene sizes are 100x200, 10x220, 16x16, 128x128, 50x720 (a 12-word row) and 64x128."""
    scene, nc = R.known_answer_scenes()[name]
    index = list(range(len(scene)))
    one, many = _run_both(scene, index, nc)
    _assert_same(one, many)
    _assert_reference(many, scene, index, nc)


def test_all_known_answer_scenes_as_one_ragged_request():
    """The ten images of A .. H in ONE call: six different sizes side by side."""
    images = [im for name in 'ABCDEFGH' for im in R.known_answer_scenes()[name][0]]
    assert len({(im['h'], im['w']) for im in images}) == 6
    index = list(range(len(images)))
    one, many = _run_both(images, index, 1)
    _assert_same(one, many)
    _assert_reference(many, images, index, 1)


@pytest.mark.parametrize('kinds', [KINDS, ('bbox',), ('segm',)], ids=['both', 'bbox', 'segm'])
def test_random_sequence_with_permuted_indices(kinds):
    scene = R.random_sequence()
    index = [3, 0, 5, 1, 4, 2]
    one, many = _run_both(scene, index, R.RANDOM_CLASSES, kinds=kinds)
    assert many.images == 6 and many.capacity == 8
    _assert_same(one, many)
    _assert_reference(many, scene, index, R.RANDOM_CLASSES, kinds=kinds)
    assert int(many.flags.count_nonzero()) > 0


def test_word_and_chunk_edges():
    images = _six_images()
    zero = images[2]
    assert not zero['dets'][0]['mask'].any() and any(q['cls'] == zero['dets'][0]['cls'] and not q['mask'].any() for q in zero['gts'])
    assert len(images[3]['dets']) == 0 and len(images[4]['gts']) == 0 and len(images[5]['dets']) == MD
    one, many = _run_both(images, SIX_INDEX, 3)
    assert many.images == 6 and many.capacity == 8
    _assert_same(one, many)
    _assert_reference(many, images, SIX_INDEX, 3)
    cls, rank, flags, npig = many.log()
    # the image without ground truth: 20 x 20 px detections are 'small', so their 'medium' and 'large' words carry the ignore bit of
    # every threshold and nothing else -- for both IoU types: the areas were computed without any gt
    at = SIX_INDEX[4] * MD
    assert (cls[at:at + 5] >= 0).all() and (cls[at + 5:at + MD] == -1).all()
    ignored = np.uint32(0x3ff << 16)
    for word in (2, 3, 6, 7):
        assert (flags[at:at + 5, word] == ignored).all(), word
    for word in (0, 1, 4, 5):
        assert (flags[at:at + 5, word] == 0).all(), word
    # the image without detections: only npig moved
    at = SIX_INDEX[3] * MD
    assert (cls[at:at + MD] == -1).all() and (flags[at:at + MD] == 0).all()
    assert not np.isnan(many.accumulate()['segm'][0]).any()


@pytest.mark.parametrize('images, max_det', [
    (lambda: [_image(31, 16, 16, 20, 129), _image(32, 16, 16, 20, 512)], 24),      # g crosses MAXR = 128; g at the limit
    (lambda: [_image(33, 16, 16, 130, 5), _image(34, 16, 16, 3, 2)], 130),         # the detection-row pass crosses 128
], ids=['g129_g512', 'count130'])
def test_group_edges(images, max_det):
    images = images()
    one, many = _run_both(images, [1, 0], 3, max_det=max_det)
    _assert_same(one, many)
    assert int(many.flags.count_nonzero()) > 0 and int(many.class_rows.sum()) > 0


def test_a_batch_of_one_equals_add():
    images = [_six_images()[1]]
    one, many = _run_both(images, [0], 3)
    _assert_same(one, many)
    _assert_reference(many, images, [0], 3)


def test_a_batch_of_32_with_padding_entries():
    pool = [_image(41, 16, 16, 5, 3), _image(42, 5, 3, 8, 4), _image(43, 9, 65, 0, 2), _image(44, 16, 16, 8, 0)]
    images = [pool[b % 4] for b in range(32)]
    index = [(b * 7) % 32 for b in range(32)]                   # (a permutation)
    pad = (5, 17, 31)
    one, many = _run_both(images, index, 3, max_det=8, pad=pad)
    assert many.images == 29
    _assert_same(one, many)
    assert int(many.flags.count_nonzero()) > 0


def test_writes_only_its_own_log_rows():
    images = _six_images()[:3]
    index = [3, 11, 1]
    one, many = _run_both(images, index, 3, prefill=True)
    _assert_same(one, many)
    own = torch.zeros(many.capacity * MD, dtype=torch.bool)
    for i in index:
        own[i * MD:(i + 1) * MD] = True
    other = ~own.to(DEV)
    assert int(other.sum()) == 13 * MD
    assert bool((many.score[other] == -7.0).all()) and bool((many.cls[other] == 77).all()) and bool((many.rank[other] == 55).all())
    assert bool((many.flags[other] == 0x5a5a5a5a).all())
    assert bool((many.cls[own.to(DEV)] != 77).all()) and bool((many.flags[own.to(DEV)] != 0x5a5a5a5a).all())


def test_two_add_batch_calls_on_two_streams_with_one_log_growth():
    from yolact_minimal_amd.utils.coco_eval import COCOGtBatch, DeviceCOCOeval
    scene = R.random_sequence()
    nc = R.RANDOM_CLASSES
    serial = DeviceCOCOeval(nc, DEV, max_det=MD, capacity_images=4)
    for i, im in enumerate(scene):
        serial.add(*_rows(im, MD), image_index=i)
    ev = DeviceCOCOeval(nc, DEV, max_det=MD, capacity_images=4)
    halves = [([0, 2, 1], _batch_args([scene[i] for i in (0, 2, 1)], MD)), ([5, 3, 4], _batch_args([scene[i] for i in (5, 3, 4)], MD))]
    bundles = [COCOGtBatch.from_gts([a[5] for a in args]) for _, (args, _) in halves]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    cur = torch.cuda.current_stream()
    for s in streams:
        s.wait_stream(cur)                                      # the uploads above ran on the current stream
    for s, (index, (_, tensors)), bundle in zip(streams, halves, bundles):
        with torch.cuda.stream(s):
            assert ev.add_batch(*tensors, bundle, index) == index
    assert ev.capacity == 8 and serial.capacity == 8            # (grown once, for index 5, on the second stream)
    for s in streams:
        cur.wait_stream(s)
    torch.cuda.synchronize()
    _assert_same(serial, ev)
    _assert_reference(ev, scene, list(range(6)), nc)


def test_ground_truth_bundles_agree(tmp_path):
    """`coco_gt_batch` (annotation file -> ragged rasteriser -> one ragged packing launch) = `COCOGtBatch.from_gts` of the per-image
    `coco_gt` = the scene's arrays, for six images of five sizes, one of them without annotations."""
    from yolact_minimal_amd.utils.coco import COCO
    from yolact_minimal_amd.utils.coco_eval import COCOGtBatch, coco_gt, coco_gt_batch
    scene = _six_images()
    image_ids, cat_ids = [11, 66, 22, 55, 33, 44], [3, 7, 11]
    label_map = {c: k + 1 for k, c in enumerate(cat_ids)}
    ann_file = str(tmp_path / 'ann.json')
    with open(ann_file, 'w') as f:
        json.dump(R.scene_annotation_dict(scene, image_ids, cat_ids), f)
    coco = COCO(ann_file, device=DEV)
    a = coco_gt_batch(coco, image_ids, label_map, DEV)
    b = COCOGtBatch.from_gts([coco_gt(coco, i, label_map, DEV) for i in image_ids])
    torch.cuda.synchronize()
    assert a.sizes == b.sizes == [(im['h'], im['w']) for im in scene]
    assert a.first == b.first == list(np.cumsum([0] + [len(im['gts']) for im in scene]))
    assert a.offsets == b.offsets and all(o * 8 % 256 == 0 for o in a.offsets)
    for name in ('cls', 'crowd', 'area', 'bbox'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    gts = [q for im in scene for q in im['gts']]
    assert a.cls.cpu().tolist() == [q['cls'] for q in gts] and a.crowd.cpu().tolist() == [q['iscrowd'] for q in gts]
    assert a.area.cpu().tolist() == [float(q['area']) for q in gts] and a.bbox.cpu().tolist() == [q['bbox'] for q in gts]
    from yolact_minimal_amd.utils.packed_masks import PackedMasks
    for k, im in enumerate(scene):
        if not im['gts']:
            assert a.masks(k) is None and b.masks(k) is None
            continue
        assert torch.equal(a.masks(k).bits, b.masks(k).bits), k
        want = PackedMasks.pack(torch.from_numpy(np.stack([q['mask'] for q in im['gts']]).astype(np.uint8)).to(DEV))
        assert torch.equal(a.masks(k).bits, want.bits), k
    no_masks = coco_gt_batch(coco, image_ids, label_map, DEV, masks=False)
    assert no_masks.table is None and no_masks.bits is None and torch.equal(no_masks.bbox, a.bbox)


def test_coco_gt_batch_padding_entries_bring_their_size_only(tmp_path):
    from yolact_minimal_amd.utils.coco import COCO
    from yolact_minimal_amd.utils.coco_eval import coco_gt_batch
    scene = _six_images()[:3]
    image_ids, cat_ids = [5, 9, 7], [3, 7, 11]
    label_map = {c: k + 1 for k, c in enumerate(cat_ids)}
    ann_file = str(tmp_path / 'ann.json')
    with open(ann_file, 'w') as f:
        json.dump(R.scene_annotation_dict(scene, image_ids, cat_ids), f)
    coco = COCO(ann_file, device=DEV)
    full = coco_gt_batch(coco, image_ids + [7], label_map, DEV)
    padded = coco_gt_batch(coco, image_ids + [7], label_map, DEV, live=[True, True, True, False])
    g = [len(im['gts']) for im in scene]
    assert padded.sizes == full.sizes and padded.first == list(np.cumsum([0] + g + [0])) and full.first[-1] == sum(g) + g[2]
    for name in ('cls', 'crowd', 'area', 'bbox'):
        assert torch.equal(getattr(padded, name), getattr(full, name)[:sum(g)]), name
    assert padded.masks(3) is None and all(torch.equal(padded.masks(k).bits, full.masks(k).bits) for k in range(3))
    with pytest.raises(RuntimeError, match='live flags'):
        coco_gt_batch(coco, image_ids, label_map, DEV, live=[True])


@pytest.mark.parametrize('ev_dev, gt_dev', [('cuda', 'cuda:0'), ('cuda:0', 'cuda')])
def test_cuda_and_cuda0_name_the_same_device(ev_dev, gt_dev, tmp_path):
    """An evaluator on 'cuda' takes bundles on 'cuda:0' and the other way round, from `from_gts` and from `coco_gt_batch`."""
    from yolact_minimal_amd.utils.coco import COCO
    from yolact_minimal_amd.utils.coco_eval import COCOGtBatch, DeviceCOCOeval, coco_gt_batch
    scene = R.random_sequence()[:2]
    nc = R.RANDOM_CLASSES
    ann_file = str(tmp_path / 'ann.json')
    with open(ann_file, 'w') as f:
        json.dump(R.scene_annotation_dict(scene, [1, 2], list(range(1, nc + 1))), f)
    coco = COCO(ann_file, device=gt_dev)
    label_map = {c: c for c in range(1, nc + 1)}
    args, tensors = _batch_args(scene, MD)
    with torch.cuda.device(0):
        ev = DeviceCOCOeval(nc, ev_dev, max_det=MD)
        assert ev.add_batch(*tensors, coco_gt_batch(coco, [1, 2], label_map, gt_dev), [0, 1]) == [0, 1]
        ev2 = DeviceCOCOeval(nc, ev_dev, max_det=MD)
        gts = [R.image_to_device(im, gt_dev, MD)[5] for im in scene]
        assert ev2.add_batch(*tensors, COCOGtBatch.from_gts(gts), [0, 1]) == [0, 1]
    torch.cuda.synchronize()
    _assert_same(ev, ev2)
    _assert_reference(ev, scene, [0, 1], nc)


def test_segm_alone_without_pixel_boxes():
    """kinds = ('segm',) with `boxes_px=None`: every row below its count is a detection.  The six images have no empty pixel box, so
    the log is the one `add` leaves with the boxes, and the restatement's."""
    from yolact_minimal_amd.utils.coco_eval import COCOGtBatch, DeviceCOCOeval
    images = _six_images()
    assert all((d['box'][2] - d['box'][0]) * (d['box'][3] - d['box'][1]) > 0 for im in images for d in im['dets'])
    one, with_boxes = _run_both(images, SIX_INDEX, 3, kinds=('segm',))
    ev = DeviceCOCOeval(3, DEV, max_det=MD, kinds=('segm',), capacity_images=4)
    args, (ids, scores, _, views, counts) = _batch_args(images, MD)
    assert ev.add_batch(ids, scores, None, views, counts, COCOGtBatch.from_gts([a[5] for a in args]), SIX_INDEX) == SIX_INDEX
    torch.cuda.synchronize()
    _assert_same(one, ev)
    _assert_same(with_boxes, ev)
    _assert_reference(ev, images, SIX_INDEX, 3, kinds=('segm',))
    with pytest.raises(RuntimeError, match='boxes_px'):
        DeviceCOCOeval(3, DEV, max_det=MD).add_batch(ids, scores, None, views, counts, COCOGtBatch.from_gts([a[5] for a in args]), SIX_INDEX)


def test_add_batch_reads_nothing_on_the_host():
    from yolact_minimal_amd.utils.coco_eval import COCOGtBatch, DeviceCOCOeval
    scene = R.random_sequence()
    ev = DeviceCOCOeval(R.RANDOM_CLASSES, DEV, max_det=MD)
    args, tensors = _batch_args(scene[:2], MD)
    ev.add_batch(*tensors, COCOGtBatch.from_gts([a[5] for a in args]), [0, 1])          # warm-up: library, scratch
    args, tensors = _batch_args(scene[2:], MD)                                          # (scene[4] has no detections)
    bundle = COCOGtBatch.from_gts([a[5] for a in args])
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
        ev.add_batch(*tensors, bundle, [2, 3, 4, 5])
    finally:
        torch.cuda.set_sync_debug_mode('default')
    _assert_reference(ev, scene, list(range(6)), R.RANDOM_CLASSES)


def test_a_refused_add_batch_consumes_no_index():
    from yolact_minimal_amd.utils.coco_eval import COCOGt, COCOGtBatch, DeviceCOCOeval
    scene = R.random_sequence()[:3]
    h, w = scene[0]['h'], scene[0]['w']
    ev = DeviceCOCOeval(R.RANDOM_CLASSES, DEV, max_det=MD)
    args, tensors = _batch_args(scene, MD)
    gts = [a[5] for a in args]
    g = 513
    big = COCOGt.from_arrays(np.zeros(g, np.int32), np.zeros(g, np.uint8), np.full(g, 50.0), np.tile([0.0, 0.0, 5.0, 10.0], (g, 1)),
                             torch.ones(g, h, w, dtype=torch.uint8), h, w, DEV)
    ev.add_batch(tensors[0][:1], tensors[1][:1], tensors[2][:1], tensors[3][:1], tensors[4][:1], COCOGtBatch.from_gts(gts[:1]), [0])
    log = [t.clone() for t in (ev.score, ev.cls, ev.rank, ev.flags, ev.npig, ev.class_rows)]
    with pytest.raises(RuntimeError, match='512'):
        ev.add_batch(*tensors, COCOGtBatch.from_gts([gts[0], big, gts[2]]), [3, 1, 2])
    with pytest.raises(RuntimeError, match='added before'):
        ev.add_batch(*tensors, COCOGtBatch.from_gts(gts), [1, 0, 2])
    with pytest.raises(RuntimeError, match='repeated'):
        ev.add_batch(*tensors, COCOGtBatch.from_gts(gts), [1, 2, 1])
    with pytest.raises(RuntimeError, match='packed masks only'):
        dense = [torch.ones(MD, h, w, device=DEV) for _ in scene]
        ev.add_batch(tensors[0], tensors[1], tensors[2], dense, tensors[4], COCOGtBatch.from_gts(gts), [1, 2, 3])
    torch.cuda.synchronize()
    assert ev.images == 1
    for was, now in zip(log, (ev.score, ev.cls, ev.rank, ev.flags, ev.npig, ev.class_rows)):
        assert torch.equal(was, now)
    assert ev.add_batch(tensors[0][1:], tensors[1][1:], tensors[2][1:], tensors[3][1:], tensors[4][1:], COCOGtBatch.from_gts(gts[1:]),
                        [1, 2]) == [1, 2] and ev.images == 3
    _assert_reference(ev, scene, [0, 1, 2], R.RANDOM_CLASSES)


def test_evaluate_coco_pipelined_with_batched_metrics_equals_the_per_image_loop(tmp_path):
    """res50 at 128 px with seeded weights, 7 synthetic images of mixed output sizes in an annotation file whose image ids are not
    ascending, depth 2, requests of four (the second padded with one copy): one `add_batch` per request against one `add` per image
    on one pipeline."""
    import bench
    from yolact_minimal_amd.evaluate import eval_pipeline, evaluate_coco_pipelined
    from yolact_minimal_amd.utils.coco import COCO
    dev = torch.device(DEV)
    net, cfg, _ = bench.detecting_net('res50_coco', 128, dev)
    sizes = [(48, 64), (64, 48), (40, 56), (37, 50), (50, 33), (64, 64), (33, 70)]
    scene = [_image(60 + k, h, w, 0, 5, nc=5) for k, (h, w) in enumerate(sizes)]
    image_ids = [70, 10, 30, 20, 60, 50, 40]
    cats = {v - 1: k for k, v in cfg.continuous_id.items()}    # class index -> COCO category id
    ann = R.scene_annotation_dict(scene, image_ids, [cats[c] for c in (0, 1, 2, 16, 79)])
    ann['categories'] = [{'id': k, 'name': str(k)} for k in sorted(cfg.continuous_id)]
    ann_file = str(tmp_path / 'ann.json')
    with open(ann_file, 'w') as f:
        json.dump(ann, f)
    coco = COCO(ann_file, device=dev)
    g = torch.Generator().manual_seed(23)
    samples = [(torch.randn(1, 3, 128, 128, generator=g).to(dev), None, None, h, w) for h, w in sizes]
    try:
        pipe = eval_pipeline(net, cfg, samples[0][0], 48, 64, depth=2, packed_masks=True, batch=4)      # (one capture for both runs)
        want_summary, want = evaluate_coco_pipelined(net, cfg, list(samples), coco, image_ids, pipe=pipe, batched_metrics=False)
        got_summary, got = evaluate_coco_pipelined(net, cfg, list(samples), coco, image_ids, pipe=pipe, batched_metrics=True)
    finally:
        net._engines.clear()
    assert got.images == want.images == 7 and got._seen == set(range(7))     # (the padded entry was not added)
    assert int(want.class_rows.sum()) >= 7, 'the network must detect something for this test to mean anything'
    assert int(got.npig[0].sum()) == sum(1 for im in scene for q in im['gts'] if not q['iscrowd'])
    _assert_same(want, got)
    a, b = got.accumulate(), want.accumulate()
    for kind in KINDS:
        assert np.array_equal(a[kind][0], b[kind][0]) and np.array_equal(a[kind][1], b[kind][1]), kind
        assert np.array_equal(got_summary[kind][0], want_summary[kind][0]) and got_summary[kind][1] == want_summary[kind][1]
