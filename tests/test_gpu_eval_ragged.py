"""The batched metric stage on the GPU: `DeviceAPData.add_batch` (`ym_eval_add_ragged_packed`) writes, bit for bit, what
`DeviceAPData.add` writes image by image -- and what the CPU oracle's `prep_metrics` says -- at the chunk, group, batch-size and
padding edges; `ym_pack_masks_ragged` equals `ym_pack_masks` per block; `evaluate_pipelined(batched_metrics=True)` gives the
per-image loop's accumulator.  The inputs come from `device_metrics_ref.to_device(..., max_det=, packed=True)`: rows past the count
carry NaN scores, the valid class 3 and all-ones masks, so a kernel that looks past the count is caught."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import metrics_ref as M
from tests import device_metrics_ref as R
from yolact_minimal_amd import hip

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NC = 5


def _empty_gt(image):
    ids, scores, boxes, masks, _, _, h, w = image
    return ids, scores, boxes, masks, torch.zeros(0, 5), torch.zeros(0, h, w), h, w


@functools.lru_cache(maxsize=None)
def _case(seed, n, g, h, w):
    ids, scores, boxes, masks, gt, gt_masks, h, w = M.synth_eval_case(seed, n, max(g, 1), h, w, NC)
    image = (ids[:n], R.quantise(scores[:n]), boxes[:n], masks[:n], gt, gt_masks, h, w)
    return _empty_gt(image) if g == 0 else image


def _oracle_rows(image, max_det):
    """(score, class, flags) of one image slot and its gt counts, from the CPU oracle; the two cases `prep_metrics` is never given
    (no detection: nothing; no ground truth: data points without a match) are written down here."""
    ids, scores, _, _, gt, _, _, _ = image
    if len(ids) and len(gt):
        return R.oracle_log([image], NC, max_det)
    score, cls = np.zeros(max_det, dtype=np.float32), np.full(max_det, -1, dtype=np.int32)
    score[:len(ids)], cls[:len(ids)] = np.asarray(scores, dtype=np.float32), ids
    return score, cls, np.zeros(max_det, dtype=np.uint32), np.zeros(NC, dtype=np.int64)


def _ragged_views(packed_list, sizes, max_det, dev):
    """The per-image `PackedMasks` as views of ONE `ragged_layout` allocation (what `after_nms_batch(..., packed=True)` returns);
    the words between the blocks are all ones."""
    from yolact_minimal_amd.utils.output_utils import ragged_layout
    from yolact_minimal_amd.utils.packed_masks import PackedMasks
    offsets, total = ragged_layout(sizes, max_det, True)
    flat = torch.full((total,), -1, dtype=torch.int64, device=dev)
    views = []
    for pm, (h, w), o in zip(packed_list, sizes, offsets):
        wq = (w + 63) // 64
        view = flat[o:o + max_det * h * wq].view(max_det, h, wq)
        view.copy_(pm.bits)
        views.append(PackedMasks(view, h, w))
    return views


def _run_both(images, index, max_det, pad=(), prefill=False):
    """`images` through `add` one by one and through ONE `add_batch` -> (accumulator of add, accumulator of add_batch, the gts as
    add_batch was given them, their clones from before).  `pad`: entries whose index is None for add_batch and which `add` never
    sees; their device rows are NaN scores, class 3, all-ones masks and a full count."""
    from yolact_minimal_amd.utils.device_metrics import DeviceAPData
    dev = torch.device(DEV)
    one = DeviceAPData(NC, R.THRES, dev, max_det=max_det, capacity_images=4)
    many = DeviceAPData(NC, R.THRES, dev, max_det=max_det, capacity_images=4)
    args = [R.to_device(im, dev, max_det=max_det, packed=True) for im in images]
    sizes = [(a[7], a[8]) for a in args]
    ids, scores, boxes = (torch.stack([a[k] for a in args]) for k in (0, 1, 2))
    counts = torch.cat([a[4] for a in args])
    for b in pad:
        ids[b], scores[b], counts[b] = 3, float('nan'), max_det
        args[b][3].bits.fill_(-1)
    views = _ragged_views([a[3] for a in args], sizes, max_det, dev)
    gts = [a[5] for a in args]
    before = [g.clone() for g in gts]
    if prefill:
        for acc in (one, many):
            acc._grow(16)
            acc.score.fill_(-7.0), acc.cls.fill_(77), acc.flags.fill_(0x5a5a5a5a)
    for b, a in enumerate(args):
        if b not in pad:
            one.add(a[0], a[1], a[2], a[3], a[4], a[5].clone(), a[6], a[7], a[8], image_index=index[b])
    got = many.add_batch(ids, scores, boxes, views, counts, gts, [a[6] for a in args], sizes,
                         [None if b in pad else index[b] for b in range(len(args))])
    assert got == [index[b] for b in range(len(args)) if b not in pad]
    torch.cuda.synchronize()
    return one, many, gts, before


def _assert_same(one, many):
    assert one.images == many.images and one.capacity == many.capacity
    for name in ('score', 'cls', 'flags', 'gt_count', 'class_rows'):
        assert torch.equal(getattr(one, name), getattr(many, name)), name


def _assert_oracle(acc, images, index, max_det, pad=()):
    score, cls = np.zeros(acc.capacity * max_det, dtype=np.float32), np.full(acc.capacity * max_det, -1, dtype=np.int32)
    flags, gt_count = np.zeros(acc.capacity * max_det, dtype=np.uint32), np.zeros(NC, dtype=np.int64)
    for b, im in enumerate(images):
        if b in pad:
            continue
        s, c, f, g = _oracle_rows(im, max_det)
        at = slice(index[b] * max_det, (index[b] + 1) * max_det)
        score[at], cls[at], flags[at] = s, c, f
        gt_count += g
    assert np.array_equal(acc.score.cpu().numpy(), score)
    assert np.array_equal(acc.cls.cpu().numpy(), cls)
    assert np.array_equal(acc.flags.cpu().numpy().view(np.uint32), flags)
    assert np.array_equal(acc.gt_count.cpu().numpy(), gt_count)
    assert np.array_equal(acc.class_rows.cpu().numpy(), np.bincount(cls[cls >= 0], minlength=NC))


MD = 16


@functools.lru_cache(maxsize=None)
def _six_images():
    """5x3 (one word, one chunk); 33x70 (66 words: the last chunk has 6 of 20) with gt 1 a copy of gt 0 -- equal IoUs, the first must
    win; 40x65 (two words per row, 63 pad bits) with an all-zero detection mask against an all-zero gt mask of its class (NaN IoU);
    48x64 without detections, whose gt must not be counted; an image without ground truth; an image whose count is max_det."""
    tiny = _case(21, 6, 3, 5, 3)
    ids, scores, boxes, masks, gt, gt_masks, h, w = _case(22, 12, 4, 33, 70)
    gt, gt_masks = gt.clone(), gt_masks.clone()
    gt[1], gt_masks[1] = gt[0], gt_masks[0]
    twins = (ids, scores, boxes, masks, gt, gt_masks, h, w)
    ids, scores, boxes, masks, gt, gt_masks, h, w = _case(23, 9, 5, 40, 65)
    masks, gt_masks = masks.clone(), gt_masks.clone()
    j = [int(c) for c in gt[:, 4].tolist()].index(ids[0])      # (a gt of detection 0's class)
    masks[0], gt_masks[j] = 0, 0
    nan = (ids, scores, boxes, masks, gt, gt_masks, h, w)
    return [tiny, twins, nan, _case(24, 0, 3, 48, 64), _case(25, 7, 0, 40, 56), _case(26, MD, 6, 33, 47)]


SIX_INDEX = [7, 2, 0, 9, 4, 3]


def test_six_mixed_images_equal_add_and_the_oracle():
    images = _six_images()
    assert any(c == images[2][0][0] for c in images[2][4][:, 4].int().tolist())
    one, many, _, _ = _run_both(images, SIX_INDEX, MD)
    assert many.images == 6 and many.capacity == 16             # (grown once, for index 9)
    _assert_same(one, many)
    _assert_oracle(many, images, SIX_INDEX, MD)
    assert int(many.flags.count_nonzero()) > 0
    # the NaN pair exists and matched nothing on the mask side; the twin gts gave detection 0 of image 1 at most one match
    from yolact_minimal_amd.utils.packed_masks import PackedMasks, mask_iou_packed
    dev = torch.device(DEV)
    iou = mask_iou_packed(PackedMasks.pack(images[2][3].to(dev)), PackedMasks.pack(images[2][5].to(dev)))
    assert bool(torch.isnan(iou[0]).any())


@pytest.mark.parametrize('images, max_det', [
    (lambda: [_case(31, 20, 129, 16, 16), _case(32, 20, 512, 16, 16)], 24),      # g crosses MAXR = 128; g at the limit
    (lambda: [_case(33, 130, 5, 16, 16), _case(34, 3, 2, 16, 16)], 130),         # the detection-row pass crosses 128
], ids=['g129_g512', 'count130'])
def test_group_edges(images, max_det):
    images = images()
    one, many, _, _ = _run_both(images, [1, 0], max_det)
    _assert_same(one, many)
    _assert_oracle(many, images, [1, 0], max_det)
    assert int(many.flags.count_nonzero()) > 0


def test_a_batch_of_one_equals_add():
    images = [_six_images()[1]]
    one, many, _, _ = _run_both(images, [2], MD)
    _assert_same(one, many)
    _assert_oracle(many, images, [2], MD)


def test_a_batch_of_32_with_padding_entries():
    pool = [_case(41, 5, 3, 16, 16), _case(42, 8, 4, 5, 3), _case(43, 0, 2, 9, 65), _case(44, 8, 0, 16, 16)]
    images = [pool[b % 4] for b in range(32)]
    index = [(b * 7) % 32 for b in range(32)]                   # (a permutation)
    pad = (5, 17, 31)
    one, many, _, _ = _run_both(images, index, 8, pad=pad)
    assert many.images == 29
    _assert_same(one, many)
    _assert_oracle(many, images, index, 8, pad=pad)


def test_writes_only_its_own_log_rows_and_leaves_the_gts_alone():
    images = _six_images()[:3]
    index = [3, 11, 1]
    one, many, gts, before = _run_both(images, index, MD, prefill=True)
    _assert_same(one, many)
    for g, b in zip(gts, before):
        assert torch.equal(g, b)                                # NOT scaled in place (`add` got clones)
    own = torch.zeros(many.capacity * MD, dtype=torch.bool)
    for i in index:
        own[i * MD:(i + 1) * MD] = True
    other = ~own.to(DEV)
    assert int(other.sum()) == 13 * MD
    assert bool((many.score[other] == -7.0).all()) and bool((many.cls[other] == 77).all()) and bool((many.flags[other] == 0x5a5a5a5a).all())
    assert bool((many.cls[own.to(DEV)] != 77).all())


@pytest.mark.parametrize('dtype', [torch.uint8, torch.float32], ids=['uint8', 'fp32'])
def test_pack_masks_ragged_equals_pack_masks_per_block(dtype):
    from yolact_minimal_amd.utils.packed_masks import PackedMasks
    dev = torch.device(DEV)
    sizes, rows = [(5, 3), (33, 70), (7, 9), (40, 65)], [3, 4, 0, 5]
    g = torch.Generator().manual_seed(5)
    src = [(torch.rand(r, h, w, generator=g) < 0.4).to(dtype).mul(3).to(dev) for r, (h, w) in zip(rows, sizes)]
    it = iter(rows)
    offsets, total = hip.aligned_layout('test', sizes, 8, lambda h, w: next(it) * h * ((w + 63) // 64))
    bits = torch.full((total + 40,), 0x5a5a5a5a5a5a5a5a, dtype=torch.int64, device=dev)
    hip.check(hip.lib().ym_pack_masks_ragged((ctypes.c_void_p * 4)(*[m.data_ptr() for m in src]), int(dtype == torch.uint8),
                                             (ctypes.c_int32 * 4)(*rows), hip.ragged_table(sizes, offsets), 4,
                                             hip.ptr(bits, torch.int64), hip.stream_ptr()), 'ym_pack_masks_ragged')
    torch.cuda.synchronize()
    owned = torch.zeros(total + 40, dtype=torch.bool, device=dev)
    for m, r, (h, w), o in zip(src, rows, sizes, offsets):
        n = r * h * ((w + 63) // 64)
        owned[o:o + n] = True
        if r:
            assert torch.equal(bits[o:o + n], PackedMasks.pack(m).bits.reshape(-1)), (h, w)
    assert int((~owned).sum()) > 40 and bool((bits[~owned] == 0x5a5a5a5a5a5a5a5a).all())     # the gaps and the tail keep the sentinel


def test_gt_masks_may_arrive_packed_dense_or_mixed():
    from yolact_minimal_amd.utils.device_metrics import DeviceAPData
    from yolact_minimal_amd.utils.packed_masks import PackedMasks
    dev = torch.device(DEV)
    images, index = _six_images()[:3], [2, 0, 1]
    args = [R.to_device(im, dev, max_det=MD, packed=True) for im in images]
    sizes = [(a[7], a[8]) for a in args]
    ids, scores, boxes = (torch.stack([a[k] for a in args]) for k in (0, 1, 2))
    counts = torch.cat([a[4] for a in args])
    views = _ragged_views([a[3] for a in args], sizes, MD, dev)
    logs = []
    for form in ('dense', 'packed', 'mixed', 'uint8'):
        gm = [a[6] for a in args]
        if form == 'uint8':
            gm = [m.to(torch.uint8) for m in gm]
        elif form != 'dense':
            gm = [PackedMasks.pack(m) if form == 'packed' or b == 1 else m for b, m in enumerate(gm)]
        acc = DeviceAPData(NC, R.THRES, dev, max_det=MD, capacity_images=4)
        acc.add_batch(ids, scores, boxes, views[0], counts, [a[5] for a in args], gm, sizes, index,
                      mask_table=hip.ragged_table(sizes, [(v.bits.data_ptr() - views[0].bits.data_ptr()) // 8 for v in views]))
        torch.cuda.synchronize()
        logs.append(acc)
    _assert_oracle(logs[0], images, index, MD)
    for acc in logs[1:]:
        _assert_same(logs[0], acc)


def test_a_refused_add_batch_consumes_no_index():
    from yolact_minimal_amd.utils.device_metrics import DeviceAPData
    dev = torch.device(DEV)
    good, big = _case(34, 3, 2, 16, 16), _case(51, 3, 513, 16, 16)
    acc = DeviceAPData(NC, R.THRES, dev, max_det=4, capacity_images=4)

    def call(images, index):
        args = [R.to_device(im, dev, max_det=4, packed=True) for im in images]
        sizes = [(a[7], a[8]) for a in args]
        return acc.add_batch(torch.stack([a[0] for a in args]), torch.stack([a[1] for a in args]), torch.stack([a[2] for a in args]),
                             _ragged_views([a[3] for a in args], sizes, 4, dev), torch.cat([a[4] for a in args]), [a[5] for a in args],
                             [a[6] for a in args], sizes, index)

    call([good], [0])
    log = [t.clone() for t in (acc.score, acc.cls, acc.flags, acc.gt_count, acc.class_rows)]
    with pytest.raises(RuntimeError, match='512'):
        call([good, big], [1, 2])
    with pytest.raises(RuntimeError, match='added before'):
        call([good, good], [1, 0])
    with pytest.raises(RuntimeError, match='packed masks only'):
        a = R.to_device(good, dev, max_det=4)
        acc.add_batch(a[0][None], a[1][None], a[2][None], [a[3]], a[4], [a[5]], [a[6]], [(16, 16)], [1])
    torch.cuda.synchronize()
    assert acc.images == 1
    for was, now in zip(log, (acc.score, acc.cls, acc.flags, acc.gt_count, acc.class_rows)):
        assert torch.equal(was, now)
    assert call([good, good], [1, 2]) == [1, 2] and acc.images == 3


def test_evaluate_pipelined_with_batched_metrics_equals_the_per_image_loop():
    """The six-sample mixed-size recipe of tests/test_gpu_ragged_postproc.py::test_evaluate_pipelined_in_batches_of_four (res50 at
    128 px, depth 2, requests of four, the second padded with two copies): one `add_batch` per request against one `add` per image,
    in the same process."""
    import bench
    from yolact_minimal_amd.evaluate import eval_pipeline, evaluate_pipelined
    from yolact_minimal_amd.utils.synthetic import synth_eval_case
    dev = torch.device(DEV)
    net, cfg, _ = bench.detecting_net('res50_coco', 128, dev)
    nc = len(cfg.class_names)
    g = torch.Generator().manual_seed(23)
    samples = []
    for i, (h, w) in enumerate([(480, 640), (640, 480), (427, 640), (375, 500), (500, 333), (640, 640)]):
        _, _, _, _, gt, gt_masks, _, _ = synth_eval_case(i + 1, 40, 7, h, w, 10)
        samples.append((torch.randn(1, 3, 128, 128, generator=g).to(dev), gt.to(dev), gt_masks.to(dev), h, w))

    def loader():
        return [(im, gt.clone(), gm, h, w) for im, gt, gm, h, w in samples]

    try:
        pipe = eval_pipeline(net, cfg, samples[0][0], 480, 640, depth=2, packed_masks=True, batch=4)     # (one capture for both runs)
        want_table, want = evaluate_pipelined(net, cfg, loader(), step=0, pipe=pipe, batched_metrics=False)
        got_table, got = evaluate_pipelined(net, cfg, loader(), step=0, pipe=pipe, batched_metrics=True)
    finally:
        net._engines.clear()
    assert got.images == want.images == 6
    assert int(want.class_rows.sum()) >= 12, 'the network must detect something for this test to mean anything'
    assert torch.equal(got.gt_count, want.gt_count) and int(got.gt_count.sum()) == 6 * 7
    assert torch.equal(got.class_rows, want.class_rows)
    for name in ('score', 'cls', 'flags'):
        assert torch.equal(getattr(got, name), getattr(want, name)), name
    a, b = got.to_ap_data(), want.to_ap_data()
    for kind in ('box', 'mask'):
        for k in range(len(a[kind])):
            for c in range(nc):
                assert a[kind][k][c].data_points == b[kind][k][c].data_points
                assert a[kind][k][c].num_gt_positives == b[kind][k][c].num_gt_positives
    assert got_table == want_table
