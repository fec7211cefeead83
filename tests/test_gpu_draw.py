"""The device renderer (csrc/draw.hip through utils/draw.py) against the numpy oracle tests/draw_ref.py on the downloaded inputs.
Everything is integer arithmetic: all comparisons are exact (torch.equal / array_equal on uint8)."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

from tests import draw_ref as R
from tests.conftest import REPO
from tests.test_draw_cpu import KNOWN

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _to_dev(ids, scores, boxes, masks, img=None):
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (ids, scores, boxes, masks)]
    return t if img is None else t + [torch.from_numpy(img).to(DEV)]


def _draw(args, cfg, **kw):
    from yolact_minimal_amd.utils.draw import draw_img
    ids, scores, boxes, masks, img = args
    d = _to_dev(ids, scores, boxes, masks, img)
    out = draw_img(d[0], d[1], d[2], d[3], d[4], cfg, **kw)
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == img.shape
    assert torch.equal(d[4], torch.from_numpy(img).to(DEV)), 'the input frame was modified'
    return out.cpu().numpy()


def _check(args, cfg, **kw):
    got = _draw(args, cfg, **kw)
    want = R.draw_ref(*args, cfg, **kw)
    bad = np.argwhere((got != want).any(axis=2))
    assert bad.size == 0, f'{len(bad)} pixels differ, first (y, x) = {bad[0].tolist()}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}'
    return got


@pytest.mark.parametrize('case', KNOWN, ids=lambda f: f.__name__)
def test_known_answers(case):
    args, cfg, want = case()
    assert np.array_equal(_draw(args, cfg), want)


@pytest.mark.parametrize('n', [1, 7, 100])
def test_synthetic_480x640(n):
    got = _check(R.synth(n, 480, 640, seed=10 + n, wild_boxes=True), R.make_cfg())
    assert got.any()


@pytest.mark.parametrize('hw', [(37, 53), (1, 1), (5, 7), (64, 130)])
def test_row_tails_and_unaligned_rows(hw):
    _check(R.synth(9, hw[0], hw[1], seed=3, wild_boxes=True), R.make_cfg())


def test_boxes_outside_reversed_and_clipped_plates():
    h, w = 96, 128
    ids, scores, boxes, masks, img = R.synth(10, h, w, seed=5, wild_boxes=True)
    boxes[6] = (w - 1, h - 1, w - 1, h - 1)
    boxes[7] = (-500, -500, -400, -450)
    boxes[8] = (-5, -14, 20, 3)                    # the label's lower rows reach into the frame from above
    boxes[9] = (w - 30, 0, 10, h - 1)              # reversed in x only, plate clipped at the right edge
    _check((ids, scores, boxes, masks, img), R.make_cfg())


FLAG_SETS = [dict(hide_mask=True), dict(hide_bbox=True), dict(hide_score=True), dict(real_time=True),
             dict(hide_mask=True, hide_bbox=True), dict(hide_mask=True, hide_score=True, real_time=True),
             dict(hide_bbox=True, real_time=True), dict(hide_mask=True, hide_bbox=True, hide_score=True, real_time=True)]


@pytest.mark.parametrize('flags', FLAG_SETS, ids=lambda f: '+'.join(sorted(f)))
@pytest.mark.parametrize('hw', [(120, 160), (37, 53)])
def test_flags(flags, hw):
    args = R.synth(12, hw[0], hw[1], seed=21, wild_boxes=True)
    _check(args, R.make_cfg(**flags), **({'fps': 31.256} if flags.get('real_time') else {}))


def test_no_crop_masks_outside_their_boxes():
    args = R.synth(15, 120, 160, seed=8, crop=False)
    ids, _, boxes, masks, _ = args
    outside = masks[0].copy()
    x1, y1, x2, y2 = boxes[0]
    outside[y1:y2 + 1, x1:x2 + 1] = 0
    assert outside.any(), 'the case needs mask pixels outside the box'
    _check(args, R.make_cfg(no_crop=True))
    _check(args, R.make_cfg(no_crop=True, hide_bbox=True))


def test_cutout_mattes():
    from yolact_minimal_amd.utils.draw import cutout_mattes, draw_img
    for hw in [(120, 160), (37, 53)]:
        args = R.synth(8, hw[0], hw[1], seed=13, wild_boxes=True)
        ids, scores, boxes, masks, img = args
        cfg = R.make_cfg(cutout=True)
        assert boxes.min() < 0
        d = _to_dev(ids, scores, boxes, masks, img)
        total, objs = cutout_mattes(d[0], d[2], d[3], d[4], cfg)
        want_total, want_objs = R.cutout_ref(ids, boxes, masks, img, cfg)
        assert np.array_equal(total.cpu().numpy(), want_total) and len(objs) == len(want_objs)
        for o, w in zip(objs, want_objs):
            assert tuple(o.shape) == w.shape and np.array_equal(o.cpu().numpy(), w)
        total_np, objs_np = cutout_mattes(d[0], d[2], d[3], img, cfg)
        assert isinstance(total_np, np.ndarray) and np.array_equal(total_np, want_total)
        assert all(np.array_equal(a, b) for a, b in zip(objs_np, want_objs))
        assert np.array_equal(draw_img(d[0], d[1], d[2], d[3], img, cfg), R.draw_ref(*args, cfg))     # cutout does not change the frame
    assert cutout_mattes(None, None, None, img, cfg) == (None, [])


def test_score_labels_are_pythons_format():
    vals = np.array([0.125, 0.375, 0.995, 0.9999, 1.0, 0.0, 0.005, 0.015, 0.625, 0.0049999], dtype=np.float32)
    n = len(vals)
    h, w = 24 * n, 200
    rng = np.random.default_rng(2)
    ids = rng.integers(0, 80, n).astype(np.int64)
    boxes = np.array([[2, 24 * i + 1, 190, 24 * i + 22] for i in range(n)], dtype=np.int32)
    img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    args = (ids, vals, boxes, np.zeros((n, h, w), dtype=np.float32), img)
    cfg = R.make_cfg()
    labels = [f'{cfg.class_names[int(i)]}: {v:.2f}' for i, v in zip(ids, vals)]           # Python's own format of the float32
    assert [t.split(': ')[1] for t in labels[:6]] == ['0.12', '0.38', '1.00', '1.00', '1.00', '0.00']      # float32(0.995) = 0.99500000476...
    got = _draw(args, cfg)
    assert np.array_equal(got, R.draw_ref(*args, cfg, labels=labels))
    # and a wrong digit would be seen: the same frame with one label changed differs
    wrong = list(labels)
    wrong[0] = wrong[0][:-1] + '3'
    assert not np.array_equal(got, R.draw_ref(*args, cfg, labels=wrong))


def test_long_and_non_ascii_class_names():
    names = ('a' * 60, 'café ☃', 'x')
    ids = np.array([0, 1, 2], dtype=np.int64)
    scores = np.array([0.5, 0.25, 0.75], dtype=np.float32)
    boxes = np.array([[1, 1, 600, 20], [1, 30, 300, 50], [1, 60, 100, 80]], dtype=np.int32)
    img = np.full((90, 640, 3), 90, dtype=np.uint8)
    _check((ids, scores, boxes, np.zeros((3, 90, 640), dtype=np.float32), img), R.make_cfg(class_names=names))


def test_none_returns_the_input_object_and_numpy_round_trip():
    from yolact_minimal_amd.utils.draw import draw_img
    args = R.synth(7, 120, 160, seed=4)
    ids, scores, boxes, masks, img = args
    cfg = R.make_cfg()
    assert draw_img(None, None, None, None, img, cfg) is img
    dimg = torch.from_numpy(img).to(DEV)
    assert draw_img(None, None, None, None, dimg, cfg) is dimg
    d = _to_dev(ids, scores, boxes, masks)
    out_np = draw_img(*d, img, cfg)
    assert isinstance(out_np, np.ndarray) and out_np.dtype == np.uint8 and out_np.shape == img.shape
    out_dev = draw_img(*d, dimg, cfg)
    assert torch.is_tensor(out_dev) and out_dev.is_cuda and np.array_equal(out_dev.cpu().numpy(), out_np)
    assert np.array_equal(out_np, R.draw_ref(*args, cfg))
    with pytest.raises(RuntimeError):
        draw_img(d[0].cpu(), d[1].cpu(), d[2].cpu(), d[3].cpu(), img, cfg)


def test_end_to_end_net_nms_after_nms_draw():
    from yolact_minimal_amd.config import build_cfg, norm_mean, norm_std
    from yolact_minimal_amd.modules.yolact import Yolact
    from yolact_minimal_amd.utils.output_utils import nms, after_nms, draw_img
    cfg = build_cfg('res50_coco', 'val', 544)
    torch.manual_seed(0)
    net = Yolact(cfg).eval().to(DEV)
    frame = np.random.default_rng(11).integers(0, 256, (544, 544, 3)).astype(np.uint8)
    x = torch.from_numpy(((frame.astype(np.float32) - norm_mean) / norm_std).transpose(2, 0, 1)[None].copy()).to(DEV)
    with torch.no_grad():
        cls, box, coef, proto = net(x)
    for thre in (0.05, 0.02, 0.01, 0.005, 0.002, 0.0005, 0.0):
        cfg.nms_score_thre = thre
        r = nms(cls, box, coef, proto, net.anchors, cfg)
        if r[0] is not None and r[0].numel() >= 20:
            break
    assert r[0] is not None and r[0].numel() >= 20, 'the end-to-end case needs at least 20 detections'
    ids, scores, boxes, masks = after_nms(*r, 544, 544, cfg)
    assert ids is not None and ids.numel() >= 20
    for name in ('hide_mask', 'hide_bbox', 'hide_score', 'real_time', 'cutout'):
        setattr(cfg, name, False)
    out = draw_img(ids, scores, boxes, masks, frame, cfg)
    want = R.draw_ref(ids.cpu().numpy(), scores.cpu().numpy(), boxes.cpu().numpy(), masks.cpu().numpy(), frame, cfg)
    assert np.array_equal(out, want) and not np.array_equal(out, frame)


def test_draw_batch_equals_per_image_without_host_reads():
    from oracle import yolact_ref as O
    from yolact_minimal_amd.config import build_cfg
    from yolact_minimal_amd.utils.output_utils import nms_batch, after_nms_batch, draw_img, draw_batch
    h, w = 480, 640
    cfg = build_cfg('res101_coco', 'val', 544)
    for name in ('hide_mask', 'hide_bbox', 'hide_score', 'real_time', 'cutout'):
        setattr(cfg, name, False)
    cfg.visual_thre = 0.3
    anchors = O.anchors_for(544, [24, 48, 96, 192, 384]).to(DEV)
    parts = [O.synth_head_outputs(18525, seed=1), O.synth_head_outputs(18525, seed=2, bg_bias=9.0),
             O.synth_head_outputs(18525, seed=4, bg_bias=30.0), O.synth_head_outputs(18525, seed=5, bg_bias=7.5)]
    cls, box, coef, proto = (torch.cat([p[i] for p in parts], 0).to(DEV) for i in range(4))
    imgs = torch.from_numpy(np.random.default_rng(6).integers(0, 256, (4, h, w, 3)).astype(np.uint8)).to(DEV)
    dets = nms_batch(cls, box, coef, proto, anchors, cfg)
    ids, scores, boxes, masks, counts = after_nms_batch(dets, h, w, cfg, sync=False)
    assert counts.tolist() == [100, 100, 0, 100]
    # different counts per frame and scores on both sides of visual_thre (the synthetic heads score everything above 0.8)
    counts = torch.tensor([100, 37, 0, 64], dtype=torch.int32, device=DEV)
    scores = scores.clone()
    scores[:, 1::3] *= 0.25
    scores[3, :64] *= 0.1                                   # frame 3: every row under the threshold -> unchanged frame
    padded = (ids, scores, boxes, masks, counts)
    per_image, kept = [], []
    for b, n in enumerate(counts.tolist()):
        keep = scores[b, :n] >= cfg.visual_thre             # after_nms's filter
        kept.append(int(keep.sum()))
        if kept[-1] == 0:
            per_image.append(draw_img(None, None, None, None, imgs[b], cfg))
        else:
            per_image.append(draw_img(ids[b, :n][keep], scores[b, :n][keep], boxes[b, :n][keep], masks[b, :n][keep], imgs[b], cfg))
    assert kept[2] == 0 and kept[3] == 0 and 0 < kept[1] < 37 and 37 < kept[0] < 100, kept
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        out = draw_batch(padded, imgs, cfg)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert out.is_cuda and out.shape == imgs.shape
    for b in range(4):
        assert torch.equal(out[b], per_image[b]), b
    assert torch.equal(out[2], imgs[2]) and torch.equal(out[3], imgs[3]) and not torch.equal(out[0], imgs[0])


def _uniform_batch(hw, counts, max_det, seed):
    """-> (per-image numpy inputs of tests.draw_ref.synth, the padded device tensors ids / scores / boxes / masks [B, max_det, H, W] /
    counts, the frames [B, H, W, 3]).  Rows past counts[b] hold garbage: NaN scores, huge boxes, all-ones masks."""
    h, w = hw
    batch = len(counts)
    per_image = [R.synth(n, h, w, seed=seed + b) for b, n in enumerate(counts)]
    ids = torch.full((batch, max_det), 1 << 40, dtype=torch.int64)
    scores = torch.full((batch, max_det), float('nan'))
    boxes = torch.full((batch, max_det, 4), 1 << 30, dtype=torch.int32)
    boxes[:, :, :2] = -(1 << 30)
    masks = torch.ones(batch, max_det, h, w)
    for b, n in enumerate(counts):
        i, s, bx, m, _ = per_image[b]
        if n:
            ids[b, :n], scores[b, :n], boxes[b, :n], masks[b, :n] = (torch.from_numpy(a) for a in (i, s, bx, m))
    imgs = torch.from_numpy(np.stack([p[4] for p in per_image]))
    return per_image, [t.to(DEV) for t in (ids, scores, boxes, masks, torch.tensor(counts, dtype=torch.int32))], imgs.to(DEV)


def _check_uniform_batch(hw, counts, max_det, seed, packed):
    """`draw_batch` on a uniform batch, byte for byte against the host oracle and against `draw_img` per image -> the oracle's frames."""
    from yolact_minimal_amd.utils.draw import draw_batch, draw_img
    from yolact_minimal_amd.utils.packed_masks import PackedMasks
    cfg = R.make_cfg()
    per_image, (ids, scores, boxes, masks, cnt), imgs = _uniform_batch(hw, counts, max_det, seed)
    before = imgs.clone()
    out = draw_batch((ids, scores, boxes, PackedMasks.pack(masks) if packed else masks, cnt), imgs, cfg)
    assert out.is_cuda and out.dtype == torch.uint8 and out.shape == imgs.shape and torch.equal(imgs, before)
    want = []
    for b, n in enumerate(counts):
        i, s, bx, m, img = per_image[b]
        want.append(R.draw_ref(i, s, bx, m, img, cfg) if n else img)
        single = draw_img(ids[b, :n], scores[b, :n], boxes[b, :n], masks[b, :n], imgs[b], cfg) if n else imgs[b]
        assert np.array_equal(out[b].cpu().numpy(), want[b]), f'frame {b} differs from the oracle'
        assert torch.equal(out[b], single), f'frame {b} differs from draw_img'
        assert n or torch.equal(out[b], imgs[b]), f'frame {b} has no detection and must come back unchanged'
    return want, [p[4] for p in per_image]


@pytest.mark.parametrize('packed', [False, True], ids=['dense', 'packed'])
@pytest.mark.parametrize('hw', [(6, 7), (8, 8)], ids=['6x7_elementwise', '8x8_16byte'])
def test_uniform_draw_batch_drops_the_rows_past_the_counts(hw, packed):
    want, frames = _check_uniform_batch(hw, [3, 0, 1], 3, 71, packed)
    assert not np.array_equal(want[0], frames[0]) and not np.array_equal(want[2], frames[2])


def test_uniform_draw_batch_of_33_frames():
    """One frame more than a ragged batch may hold (and than the bits of its per-launch image set): every frame is drawn."""
    want, frames = _check_uniform_batch((4, 8), [1] * 33, 1, 83, False)
    assert all(not np.array_equal(w, f) for w, f in zip(want, frames)), 'a frame came back undrawn'
    assert len({w.tobytes() for w in want}) == 33, 'the 33 frames differ in content'


def test_dropin_draw_img_draws_without_a_checkout(tmp_path):
    code = textwrap.dedent('''
        import numpy as np, torch
        from utils.output_utils import nms, after_nms, draw_img
        from tests import draw_ref as R
        args = R.synth(5, 60, 80, seed=2)
        cfg = R.make_cfg()
        d = [torch.from_numpy(a).cuda() for a in args[:4]]
        out = draw_img(d[0], d[1], d[2], d[3], args[4], cfg, img_name='x.jpg')
        assert isinstance(out, np.ndarray) and np.array_equal(out, R.draw_ref(*args, cfg))
        assert draw_img(None, None, None, None, args[4], cfg) is args[4]
        print('DROPIN_DRAW_OK')
    ''')
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(REPO, 'dropin'), REPO]))
    r = subprocess.run([sys.executable, '-c', code], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'DROPIN_DRAW_OK' in r.stdout, r.stderr[-2000:]
