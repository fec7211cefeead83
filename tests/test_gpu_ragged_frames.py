"""GPU: the two ends of a mixed-size request.  `val_aug_batch` (`ym_val_preprocess_batch`) against `val_aug` per frame (bit for bit: one
kernel) and the CPU oracle; the ragged `draw_batch` (`ym_draw_detections_ragged[_packed]`) against `draw_img` per image and the numpy
oracle tests/draw_ref.py (byte for byte), with guard bytes around every frame; `RequestPipeline.submit_frames` against the per-image
stages and against `submit`."""
import functools

import numpy as np
import pytest
import torch

from oracle import yolact_ref as O
from tests import draw_ref as R
from yolact_minimal_amd.config import build_cfg

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# ---- 1. val_aug_batch ------------------------------------------------------------------------------------------------------------
# (64, 64) is the identity at S = 64; (128, 40) tall, (40, 128) wide; (200, 301) scales down, width % 4 != 0
VA_SIZES = [(1, 1), (5, 7), (37, 53), (64, 64), (128, 40), (40, 128), (200, 301)]


def _raw_frames(sizes, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.uint8:
        return [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8) for h, w in sizes]
    return [torch.rand(h, w, 3, generator=g) * 255.0 for h, w in sizes]


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize('size', [64, 128])
@pytest.mark.parametrize('dtype', [torch.uint8, torch.float32], ids=['uint8', 'float32'])
def test_val_aug_batch_equals_val_aug_bit_for_bit(dtype, size):
    from yolact_minimal_amd.utils.augmentations import val_aug, val_aug_batch
    from yolact_minimal_amd.utils.frames import FrameBatch
    raw = _raw_frames(VA_SIZES, dtype, 7)
    dev = [f.to(DEV) for f in raw]
    batch = len(raw)
    out = torch.full((batch + 1, 3, size, size), float('nan'), device=DEV)
    got = val_aug_batch(dev, size, out=out)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (batch, 3, size, size)
    for b in range(batch):
        single = val_aug(dev[b], size)
        assert torch.equal(_bits(got[b]), _bits(single)), VA_SIZES[b]
        torch.testing.assert_close(got[b].cpu(), O.val_aug(raw[b], size), rtol=1e-5, atol=1e-5)
    assert bool(torch.isnan(out[batch]).all()), 'the row behind the batch was written'
    assert not bool(torch.isnan(got).any())
    # the same through a FrameBatch, into a tensor of its own
    fb = FrameBatch.from_tensors(dev)
    assert fb.dtype == dtype and all(torch.equal(v, d) for v, d in zip(fb.frames, dev))
    assert torch.equal(_bits(val_aug_batch(fb, size)), _bits(got))


def test_val_aug_batch_of_one_of_32_and_of_33():
    from yolact_minimal_amd.utils.augmentations import val_aug, val_aug_batch
    from yolact_minimal_amd.utils.frames import FrameBatch
    one = _raw_frames([(37, 53)], torch.uint8, 3)[0].to(DEV)
    assert torch.equal(_bits(val_aug_batch([one], 64)[0]), _bits(val_aug(one, 64)))
    many = [f.to(DEV) for f in _raw_frames([(9, 11)] * 32, torch.uint8, 4)]
    got = val_aug_batch(many, 64)
    assert tuple(got.shape) == (32, 3, 64, 64)
    for b in (0, 1, 17, 31):
        assert torch.equal(_bits(got[b]), _bits(val_aug(many[b], 64))), b
    assert not torch.equal(got[0], got[31])
    with pytest.raises(RuntimeError):
        val_aug_batch(many + [one], 64)
    # from_numpy: one pinned buffer, one copy; numpy() brings the frames back
    arrays = [f.numpy() for f in _raw_frames(VA_SIZES, torch.uint8, 5)]
    fb = FrameBatch.from_numpy(arrays, DEV)
    assert fb.sizes == VA_SIZES and all(np.array_equal(a, b) for a, b in zip(fb.numpy(), arrays))
    assert torch.equal(_bits(val_aug_batch(fb, 64)[6]), _bits(val_aug(torch.from_numpy(arrays[6]).to(DEV), 64)))


# ---- 2. the ragged draw_batch ----------------------------------------------------------------------------------------------------
DRAW_CASES = [((1, 1), 3), ((5, 7), 9), ((37, 53), 0), ((64, 130), 16), ((97, 301), 21), ((120, 128), 1)]
DRAW_SIZES = [s for s, _ in DRAW_CASES]
MAX_DET = 21
GUARD = 0xA5
TAIL = 512               # guard bytes behind the last frame


@functools.lru_cache(maxsize=None)
def _draw_inputs():
    """-> (per-image numpy inputs of tests.draw_ref.synth, the padded device tensors ids / scores / boxes / counts, the dense mask
    views in ragged_layout order).  Rows past counts[b] hold garbage: NaN scores, huge boxes, all-ones masks.  Never modified."""
    from yolact_minimal_amd.utils.output_utils import ragged_layout
    batch = len(DRAW_CASES)
    per_image = [R.synth(n, h, w, seed=41 + b, wild_boxes=True) for b, ((h, w), n) in enumerate(DRAW_CASES)]
    ids = torch.full((batch, MAX_DET), 1 << 40, dtype=torch.int64)
    scores = torch.full((batch, MAX_DET), float('nan'))
    boxes = torch.full((batch, MAX_DET, 4), 1 << 30, dtype=torch.int32)
    boxes[:, :, :2] = -(1 << 30)
    offsets, total = ragged_layout(DRAW_SIZES, MAX_DET)
    flat = torch.ones(total)
    for b, ((h, w), n) in enumerate(DRAW_CASES):
        i, s, bx, m, _ = per_image[b]
        if n:
            ids[b, :n], scores[b, :n], boxes[b, :n] = torch.from_numpy(i), torch.from_numpy(s), torch.from_numpy(bx)
            flat[offsets[b]:offsets[b] + n * h * w] = torch.from_numpy(m).reshape(-1)
    flat = flat.to(DEV)
    masks = [flat[o:o + MAX_DET * h * w].view(MAX_DET, h, w) for (h, w), o in zip(DRAW_SIZES, offsets)]
    counts = torch.tensor([n for _, n in DRAW_CASES], dtype=torch.int32)
    return per_image, ids.to(DEV), scores.to(DEV), boxes.to(DEV), counts.to(DEV), masks


@functools.lru_cache(maxsize=None)
def _packed_views():
    """The same masks as `PackedMasks` views of one allocation in the packed ragged_layout."""
    from yolact_minimal_amd.utils.output_utils import ragged_layout
    from yolact_minimal_amd.utils.packed_masks import PackedMasks
    dense = _draw_inputs()[5]
    offsets, total = ragged_layout(DRAW_SIZES, MAX_DET, packed=True)
    flat = torch.zeros(total, dtype=torch.int64, device=DEV)
    views = []
    for m, (h, w), o in zip(dense, DRAW_SIZES, offsets):
        wq = (w + 63) // 64
        view = flat[o:o + MAX_DET * h * wq].view(MAX_DET, h, wq)
        view.copy_(PackedMasks.pack(m).bits)
        views.append(PackedMasks(view, h, w))
    return views


def _frame_batch():
    from yolact_minimal_amd.utils.frames import FrameBatch
    return FrameBatch.from_numpy([p[4] for p in _draw_inputs()[0]], DEV)


def _guarded_like(fb):
    from yolact_minimal_amd.utils.frames import FrameBatch, frame_layout
    _, total = frame_layout(fb.sizes)
    return FrameBatch(torch.full((total + TAIL,), GUARD, dtype=torch.uint8, device=DEV), fb.sizes)


def _assert_guards(dst):
    host = dst.data.cpu().numpy()
    outside = np.ones(host.shape, dtype=bool)
    for (h, w), o in zip(dst.sizes, dst.offsets):
        outside[o:o + h * w * 3] = False
    assert outside.sum() >= TAIL and (host[outside] == GUARD).all(), 'bytes outside the frames were written'


def _expected(cfg, fps, thre):
    """Per image: `draw_img` on the device on the unpadded (and, with `thre`, filtered) rows, checked against the numpy oracle."""
    from yolact_minimal_amd.utils.draw import draw_img
    per_image, ids, scores, boxes, _, masks = _draw_inputs()
    single = R.make_cfg(**{k: v for k, v in vars(cfg).items() if k != 'visual_thre'})          # (after_nms filters, draw_img does not)
    want, survivors = [], []
    for b, (_, n) in enumerate(DRAW_CASES):
        i_np, s_np, b_np, m_np, img = per_image[b]
        keep = np.ones(n, dtype=bool) if thre <= 0 else s_np >= np.float32(thre)
        survivors.append(int(keep.sum()))
        frame = torch.from_numpy(img).to(DEV)
        if survivors[-1] == 0:
            want.append(img)
            continue
        k = torch.from_numpy(keep).to(DEV)
        got = draw_img(ids[b, :n][k], scores[b, :n][k], boxes[b, :n][k], masks[b][:n][k], frame, single, fps=fps).cpu().numpy()
        ref = R.draw_ref(i_np[keep], s_np[keep], b_np[keep], m_np[keep], img, single, **({'fps': fps} if fps is not None else {}))
        assert np.array_equal(got, ref), f'draw_img differs from the oracle on image {b}'
        want.append(ref)
    return want, survivors


FLAG_SETS = [dict(), dict(hide_mask=True), dict(hide_bbox=True), dict(hide_score=True, real_time=True), dict(visual_thre=0.5)]


@pytest.mark.parametrize('packed', [False, True], ids=['dense', 'packed'])
@pytest.mark.parametrize('flags', FLAG_SETS, ids=lambda f: '+'.join(sorted(f)) or 'default')
def test_ragged_draw_batch_equals_draw_img_and_the_oracle(flags, packed):
    from yolact_minimal_amd.utils.draw import draw_batch
    from yolact_minimal_amd.utils.frames import FrameBatch
    cfg = R.make_cfg(**flags)
    fps = 31.256 if flags.get('real_time') else None
    want, survivors = _expected(cfg, fps, cfg.visual_thre)
    counts_host = [n for _, n in DRAW_CASES]
    if cfg.visual_thre > 0:
        # the case's point: besides the frame without detections, a frame whose rows ALL fall under the threshold, and a partly filtered one
        assert any(s == 0 and n > 0 for s, n in zip(survivors, counts_host)), survivors
        assert any(0 < s < n for s, n in zip(survivors, counts_host)), survivors
    else:
        assert survivors == counts_host
    _, ids, scores, boxes, counts, dense = _draw_inputs()
    masks = _packed_views() if packed else dense
    padded = (ids, scores, boxes, masks, counts)
    imgs = _frame_batch()
    before = imgs.data.clone()
    dst = _guarded_like(imgs)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')                       # no host read, no synchronisation
    try:
        out = draw_batch(padded, imgs, cfg, fps=fps, _out=dst)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert out is dst and isinstance(out, FrameBatch) and out.sizes == DRAW_SIZES
    got = out.numpy()
    for b, (g, w) in enumerate(zip(got, want)):
        bad = np.argwhere((g != w).any(axis=2))
        assert bad.size == 0, f'image {b} {DRAW_SIZES[b]}: {len(bad)} pixels differ, first (y, x) = {bad[0].tolist()}'
    for b, s in enumerate(survivors):
        if s == 0:
            assert np.array_equal(got[b], _draw_inputs()[0][b][4]), f'frame {b} has no surviving row and must come back unchanged'
    assert not np.array_equal(got[4], _draw_inputs()[0][4][4])
    _assert_guards(dst)
    assert torch.equal(imgs.data, before), 'the input frames were modified'
    # without a destination: a new FrameBatch with the same frames
    fresh = draw_batch(padded, imgs, cfg, fps=fps)
    assert fresh is not imgs and fresh.data.data_ptr() != imgs.data.data_ptr()
    assert all(np.array_equal(a, b) for a, b in zip(fresh.numpy(), want))
    # in place
    same = draw_batch(padded, imgs, cfg, fps=fps, _out=imgs)
    assert same is imgs and all(np.array_equal(a, b) for a, b in zip(imgs.numpy(), want))


def test_ragged_draw_batch_refuses_mismatched_tables():
    from yolact_minimal_amd.utils.draw import draw_batch
    _, ids, scores, boxes, counts, dense = _draw_inputs()
    imgs, cfg = _frame_batch(), R.make_cfg()
    other_size = list(dense)
    other_size[3] = torch.zeros(MAX_DET, 64, 128, device=DEV)                    # frame 3 is 64 x 130
    with pytest.raises(RuntimeError, match='do not fit'):
        draw_batch((ids, scores, boxes, other_size, counts), imgs, cfg)
    elsewhere = list(dense)
    elsewhere[2] = dense[2].clone()                                              # right shape, another allocation
    with pytest.raises(RuntimeError, match='not at its place'):
        draw_batch((ids, scores, boxes, elsewhere, counts), imgs, cfg)
    mixed = list(dense)
    mixed[1] = _packed_views()[1]
    with pytest.raises(RuntimeError):
        draw_batch((ids, scores, boxes, mixed, counts), imgs, cfg)
    with pytest.raises(RuntimeError):
        draw_batch((ids, scores, boxes, dense[:5], counts), imgs, cfg)
    with pytest.raises(RuntimeError):                                            # a destination of other sizes
        draw_batch((ids, scores, boxes, dense, counts), imgs, cfg, _out=_guarded_like(_frame_batch_of([(4, 4)] * 6)))
    # with hide_mask the masks are ignored altogether
    out = draw_batch((ids, scores, boxes, None, counts), imgs, R.make_cfg(hide_mask=True))
    want, _ = _expected(R.make_cfg(hide_mask=True), None, 0.0)
    assert all(np.array_equal(a, b) for a, b in zip(out.numpy(), want))


def _frame_batch_of(sizes):
    from yolact_minimal_amd.utils.frames import FrameBatch
    return FrameBatch.from_numpy([np.zeros((h, w, 3), np.uint8) for h, w in sizes], DEV)


# ---- 3. RequestPipeline.submit_frames --------------------------------------------------------------------------------------------
TRIPLES = [[(97, 301), (333, 64), (48, 70)], [(120, 128), (96, 128), (200, 150)]]


@functools.lru_cache(maxsize=None)
def _net():
    """res50_coco at 128 px, the random-init recipe of tests/test_gpu_pipeline.py."""
    from yolact_minimal_amd.modules.yolact import Yolact
    cfg = build_cfg('res50_coco', 'val', 128)
    for name in ('hide_mask', 'hide_bbox', 'hide_score', 'real_time', 'cutout'):
        setattr(cfg, name, False)
    torch.manual_seed(0)
    net = Yolact(cfg).eval()
    sd = net.state_dict()
    O.randomize_bn_(sd, 1)
    O.randomize_bias_(sd, 2)
    net.load_state_dict(sd)
    return net.to(DEV), cfg


def _head_batch(n_anchors, num_classes, seeds):
    parts = [O.synth_head_outputs(n_anchors, num_classes=num_classes, proto_hw=32, seed=s, bg_bias=b) for s, b in seeds]
    return [torch.cat([p[i] for p in parts], 0).to(DEV) for i in range(4)]


def _heads(net, cfg):
    n_anchors = len(net.anchors) // 4
    return [_head_batch(n_anchors, cfg.num_classes, [(3, 5.0), (4, 30.0), (5, 3.0)]),          # image 1: no detections
            _head_batch(n_anchors, cfg.num_classes, [(6, 4.0), (7, 6.0), (8, 5.0)])]


def _triple_frames(k):
    from yolact_minimal_amd.utils.frames import FrameBatch
    rng = np.random.default_rng(20 + k)
    return FrameBatch.from_numpy([rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for h, w in TRIPLES[k]], DEV)


def _words(m):
    return m.bits if hasattr(m, 'bits') else m


def _same(got, want):
    assert (got[0] is None) == (want[0] is None)
    if want[0] is None:
        return
    for a, b in zip(got, want):
        a, b = _words(a), _words(b)
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


@pytest.mark.parametrize('packed', [False, True], ids=['dense', 'packed'])
@pytest.mark.parametrize('thre', [0.0, 0.3], ids=['all_rows', 'visual_thre'])
def test_submit_frames_draws_what_the_per_image_stages_draw(thre, packed):
    from yolact_minimal_amd.pipeline import RequestPipeline
    from yolact_minimal_amd.utils.frames import FrameBatch
    from yolact_minimal_amd.utils.output_utils import after_nms, draw_img, nms
    net, cfg = _net()
    dev = torch.device(DEV)
    heads = _heads(net, cfg)
    frames = [_triple_frames(0), _triple_frames(1)]
    cfg.visual_thre = thre
    try:
        want, counts = [], []
        for k in range(2):
            for b, (h, w) in enumerate(TRIPLES[k]):
                r = nms(*[t[b:b + 1] for t in heads[k]], net.anchors, cfg)
                counts.append(0 if r[0] is None else int(r[0].shape[0]))
                want.append(draw_img(*after_nms(*r, h, w, cfg), frames[k].frames[b], cfg))
        assert counts[1] == 0 and min(counts[:1] + counts[2:]) > 0, counts
        pipe = RequestPipeline(net, cfg, 128, 128, dev, depth=2, batch=3, packed_masks=packed)
        pipe.warm_up(torch.zeros(3, 3, 128, 128, device=dev), rounds=0)
        got = [pipe.submit_frames(frames[k], heads[k], draw=True) for k in range(2)]
        assert got == [None, None]
        got = pipe.drain()
        # a plain consumer keeps the refusal under visual_thre; drawing does not go with a consumer
        if thre > 0:
            with pytest.raises(RuntimeError, match='visual_thre'):
                pipe.submit_frames(frames[0], heads[0], consumer=lambda *r: None)
        with pytest.raises(RuntimeError):
            pipe.submit_frames(frames[0], heads[0], draw=True, consumer=lambda *r: None)
        assert pipe.drain() == []
    finally:
        cfg.visual_thre = 0
        net._engines.clear()
    assert len(got) == 2 and all(isinstance(g, FrameBatch) for g in got)
    for k in range(2):
        assert got[k].sizes == TRIPLES[k]
        for b in range(3):
            assert torch.equal(got[k].frames[b], want[3 * k + b]), (k, b)
    assert torch.equal(got[0].frames[1], frames[0].frames[1]), 'the frame without detections comes back unchanged'
    assert not torch.equal(got[0].frames[0], frames[0].frames[0])


def test_submit_frames_differs_from_submit_in_the_input_path_only():
    from yolact_minimal_amd.pipeline import RequestPipeline
    from yolact_minimal_amd.utils.augmentations import val_aug_batch
    net, cfg = _net()
    dev = torch.device(DEV)
    frames = _triple_frames(0)
    try:
        pipe = RequestPipeline(net, cfg, 128, 128, dev, depth=1, with_post=False, batch=3)
        outs = []
        for _ in range(2):                       # the first request runs before the engine's graph exists, the second after
            assert pipe.submit_frames(frames) is None
            outs.append(pipe.drain()[0])
        assert pipe.submit(val_aug_batch(frames, 128)) is None
        ref = pipe.drain()[0]
        with pytest.raises(RuntimeError):
            pipe.submit_frames(frames, draw=True)                       # nothing to draw without post-processing
    finally:
        net._engines.clear()
    assert len(ref) == 4
    for out in outs:
        for a, b in zip(out, ref):
            assert a.shape == b.shape and torch.equal(_bits(a), _bits(b))
    assert float(ref[0].abs().max()) > 0


@pytest.mark.parametrize('batch', [3, 1])
def test_submit_frames_without_draw_equals_submit_with_out_hw(batch):
    from yolact_minimal_amd.pipeline import RequestPipeline
    from yolact_minimal_amd.utils.augmentations import val_aug_batch
    from yolact_minimal_amd.utils.frames import FrameBatch
    from yolact_minimal_amd.utils.output_utils import after_nms, nms
    net, cfg = _net()
    dev = torch.device(DEV)
    heads = [t[:batch] if batch == 1 else t for t in _heads(net, cfg)[1]]
    full = _triple_frames(1)
    frames = full if batch == 3 else FrameBatch.from_tensors(full.frames[:1])
    try:
        pipe = RequestPipeline(net, cfg, 128, 128, dev, depth=2, batch=batch)
        pipe.warm_up(torch.zeros(batch, 3, 128, 128, device=dev), rounds=0)
        assert pipe.submit_frames(frames, heads) is None
        got = pipe.drain()[0]
        if batch == 3:
            assert pipe.submit(val_aug_batch(frames, 128), heads, out_hw=frames.sizes) is None
            want = pipe.drain()[0]
        else:                                    # (submit takes a list of sizes with batch > 1 only: the per-image stage instead)
            h, w = frames.sizes[0]
            want = after_nms(*nms(*heads, net.anchors, cfg), h, w, cfg)
            got, want = [got], [want]
    finally:
        net._engines.clear()
    assert len(got) == batch
    for g, w_, (h, w) in zip(got, want, frames.sizes):
        assert g[0] is not None and tuple(g[3].shape[1:]) == (h, w)
        _same(g, w_)
