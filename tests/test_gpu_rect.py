"""GPU: rectangular inference ("window mode", yolact_minimal_amd/utils/rect.py; include/yolact_hip.h "window mode").

  1. `val_aug(frame, S, window)` against the existing square kernel's top-left crop, bit for bit.
  2. `Yolact.forward` on H != W inputs against the CPU oracle and against the real reference's own rectangular forward.
  3. `after_nms(window=True)` -- single, batch, ragged; dense, packed; fused and two-kernel path -- against tests/rect_ref.py.
  4. nms + after_nms through the window against the existing square path on the same detections: everything equal.
  5. `RequestPipeline` in window mode against the per-call window functions.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from oracle import yolact_ref as R
from tests import rect_ref
from tests.test_oracle_golden import make_net
from yolact_minimal_amd.config import build_cfg

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _bits(t):
    return t.contiguous().view(torch.int32)


def _frame(h, w, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.uint8:
        return torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8)
    return torch.rand(h, w, 3, generator=g) * 255.0


# ---- 1. pre-processing ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.uint8, torch.float32], ids=['uint8', 'float32'])
@pytest.mark.parametrize('h,w,size', [(30, 80, 64), (80, 30, 64), (32, 64, 64), (480, 640, 544)])
def test_val_aug_window_is_the_top_left_of_the_square_output(h, w, size, dtype):
    from yolact_minimal_amd import rect_window
    from yolact_minimal_amd.utils.augmentations import val_aug
    frame = _frame(h, w, dtype, 5).to(DEV)
    hn, wn = rect_window([(h, w)], size)
    assert (hn, wn) != (size, size)
    square = val_aug(frame, size)
    got = val_aug(frame, size, window=(hn, wn))
    assert tuple(got.shape) == (3, hn, wn) and got.is_contiguous()
    assert torch.equal(_bits(got), _bits(square[:, :hn, :wn]))
    # what the window drops is padding: norm_mean blended with norm_mean, normalised: 0 up to the rounding of the blend (a few ulp of
    # ~120, divided by ~57)
    rest = square.clone()
    rest[:, :hn, :wn] = 0
    assert float(rest.abs().max()) < 1e-5
    # a window smaller than the picture is still the same crop (the caller's business), one outside the square is refused
    assert torch.equal(_bits(val_aug(frame, size, window=(16, 24))), _bits(square[:, :16, :24]))
    with pytest.raises(RuntimeError):
        val_aug(frame, size, window=(size + 32, size))


@pytest.mark.parametrize('dtype', [torch.uint8, torch.float32], ids=['uint8', 'float32'])
def test_val_aug_batch_window_equals_the_single_calls_and_old_entries_keep_their_output(dtype):
    from yolact_minimal_amd import rect_window
    from yolact_minimal_amd.utils.augmentations import val_aug, val_aug_batch
    sizes = [(30, 80), (32, 64), (17, 80)]
    frames = [_frame(h, w, dtype, 11 + i).to(DEV) for i, (h, w) in enumerate(sizes)]
    win = rect_window(sizes, 64)
    assert win == (32, 64)
    out = torch.full((4, 3, *win), float('nan'), device=DEV)
    got = val_aug_batch(frames, 64, out=out, window=win)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (3, 3, *win)
    for b, f in enumerate(frames):
        assert torch.equal(_bits(got[b]), _bits(val_aug(f, 64, window=win))), b
        assert torch.equal(_bits(got[b]), _bits(val_aug(f, 64)[:, :win[0], :win[1]])), b
    assert bool(torch.isnan(out[3]).all()), 'the row behind the batch was written'
    # the old entries are the Hn = Wn = S case: window=None, and the window entry at the square, give the same bits; the values are
    # the oracle's (the bar of tests/test_gpu_ragged_frames.py)
    old = val_aug_batch(frames, 64)
    assert torch.equal(_bits(old), _bits(val_aug_batch(frames, 64, window=(64, 64))))
    for b, f in enumerate(frames):
        assert torch.equal(_bits(old[b]), _bits(val_aug(f, 64)))
        assert torch.equal(_bits(old[b]), _bits(val_aug(f, 64, window=(64, 64))))
        torch.testing.assert_close(old[b].cpu(), R.val_aug(f.cpu(), 64), rtol=1e-5, atol=1e-5)
    with pytest.raises(RuntimeError):
        val_aug_batch(frames, 64, out=torch.empty(3, 3, 64, 64, device=DEV), window=win)      # out has the window's shape


# ---- 2. forward ----------------------------------------------------------------------------------------------------------------------
def _close(got, want, name, atol=1e-4, rtol=1e-4):
    # the bars of tests/test_gpu_forward.py
    got, want = got.cpu(), want.cpu() if torch.is_tensor(want) else torch.from_numpy(want)
    assert got.shape == want.shape, f'{name}: {tuple(got.shape)} vs {tuple(want.shape)}'
    err = (got - want).abs()
    bound = atol + rtol * want.abs()
    assert bool((err <= bound).all()), f'{name}: max err {err.max().item():.3e} (max |ref| {want.abs().max().item():.3e})'


def _swin_net(size, seed):
    from oracle.make_golden_swin import randomize_swin_
    from yolact_minimal_amd.modules.yolact import Yolact
    cfg = build_cfg('swin_tiny_coco', 'val', size)
    torch.manual_seed(seed)
    net = Yolact(cfg).eval()
    sd = net.state_dict()
    randomize_swin_(sd, seed + 100)
    R.randomize_bias_(sd, seed + 200)
    net.load_state_dict(sd)
    return net, cfg


@pytest.mark.parametrize('name,h,w,batch,graph', [
    ('res50_coco', 64, 96, 1, '0'), ('res50_coco', 64, 96, 1, '1'), ('res50_coco', 96, 64, 2, '1'), ('res101_coco', 96, 128, 1, '1'),
    ('swin_tiny_coco', 96, 128, 2, '1')])
def test_forward_on_a_rectangular_input_matches_the_oracle(name, h, w, batch, graph, monkeypatch):
    from yolact_minimal_amd import rect_anchor_index
    monkeypatch.setenv('YM_GRAPH', graph)
    seed = 40 + batch
    net, cfg = (_swin_net if name.startswith('swin') else functools.partial(make_net, name))(max(h, w), seed)
    img = torch.randn(batch, 3, h, w, generator=torch.Generator().manual_seed(seed + 300))
    with torch.no_grad():
        want = R.forward_eval_any(img, net.state_dict())
    net = net.to(DEV)
    with torch.no_grad():
        out = net(img.to(DEV))
        out2 = net(img.to(DEV))                  # graph replay / buffer reuse
    torch.cuda.synchronize()
    n = rect_anchor_index(cfg, h, w).numel()
    assert tuple(out[0].shape) == (batch, n, cfg.num_classes) and tuple(out[3].shape) == (batch, h // 4, w // 4, 32)
    assert tuple(net.anchors_for(h, w).shape) == (n, 4)          # one anchor per prediction row
    for a, b in zip(out, out2):
        assert torch.equal(a, b)
    for t, ref, key in zip(out, want, ('class_pred', 'box_pred', 'coef_pred', 'proto_out')):
        _close(t, ref, f'{name} {h}x{w} {key}')


def test_forward_on_a_rectangular_input_matches_the_reference(golden_dir):
    """The real reference's own forward on the same 64 x 96 tensor (tools/make_golden_rect.py)."""
    g = np.load(os.path.join(golden_dir, 'forward_res50_coco_rect_64x96_b2.npz'))
    seed = int(g['seed'])
    net, cfg = make_net('res50_coco', int(g['size']), seed)
    img = torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(seed + 300))
    d = img.double()
    np.testing.assert_allclose([d.sum().item(), d.abs().sum().item(), (d * d).sum().item()], g['img_digest'], rtol=1e-12)
    net = net.to(DEV)
    with torch.no_grad():
        out = net(img.to(DEV))
    for t, key in zip(out, ('class_pred', 'box_pred', 'coef_pred', 'proto_out')):
        _close(t, g[key], key + ' vs the reference on 64 x 96')


# ---- 3. after_nms, window rule -------------------------------------------------------------------------------------------------------
# P = 32.  Landscape: the map is the top 24 rows (y < 0.75 of the square); portrait: the left 24 columns (the boxes transposed).
#   0: inside the window          1: ends below the window (y2 = 0.9)      2: wholly below it (y1 * 32 - 1 >= 24)
#   3: x1 > x2 (the crop sorts)   4: covers everything
BOXES = torch.tensor([[0.10, 0.08, 0.55, 0.60], [0.30, 0.40, 0.80, 0.90], [0.20, 0.82, 0.70, 0.97], [0.90, 0.10, 0.35, 0.70],
                      [-0.2, -0.1, 1.3, 1.2]])
FILL = 7.0


@functools.lru_cache(maxsize=None)
def _window_case(portrait, seed, batch=3):
    """(proto [B, Hp, Wp, 32], coefs [B, 5, 32], boxes [B, 5, 4]) on the CPU; built once, never modified."""
    g = torch.Generator().manual_seed(seed)
    hp, wp = (32, 24) if portrait else (24, 32)
    proto = torch.relu(torch.randn(batch, hp, wp, 32, generator=g))
    coefs = torch.tanh(torch.randn(batch, 5, 32, generator=g))
    boxes = BOXES[:, [1, 0, 3, 2]] if portrait else BOXES
    boxes = boxes.unsqueeze(0).repeat(batch, 1, 1) + (torch.rand(batch, 5, 4, generator=g) - 0.5) * 0.02
    assert float(boxes[:, 2, [0, 2] if portrait else [1, 3]].min()) * 32 - 1 >= 24      # detection 2 stays outside the window
    return proto, coefs, boxes.contiguous()


@functools.lru_cache(maxsize=None)
def _window_want(portrait, seed, b, h, w):
    """tests/rect_ref.py for image b at h x w: computed once per case, shared by every entry that is checked against it."""
    proto, coefs, boxes = _window_case(portrait, seed)
    px, masks, up = rect_ref.after_nms_window(boxes[b], coefs[b], proto[b], h, w)
    band = rect_ref.threshold_band(up)
    assert band < 1e-3, f'seed {seed}: {band:.2e} of the reference pixels lie within 1e-4 of the threshold'
    assert float(masks[2].sum()) == 0 and float(masks[[0, 1, 3, 4]].sum(dim=(1, 2)).min()) > 0      # the case is what the table above says
    return px, masks, up


def _check_masks(got_px, got_masks, want, n=5):
    px, masks, up = want
    assert got_px.dtype == torch.int32
    np.testing.assert_array_equal(got_px.cpu().numpy()[:n], px.numpy()[:n])
    gm = got_masks.cpu()[:n]
    assert tuple(gm.shape) == tuple(masks[:n].shape)
    assert set(torch.unique(gm).tolist()) <= {0.0, 1.0}
    diff = gm != masks[:n]
    if bool(diff.any()):        # the rule of tests/test_gpu_postproc.py::_check_after
        assert float((up[:n][diff] - 0.5).abs().max()) < 1e-4, f'{int(diff.sum())} mask pixels differ away from 0.5'
    assert float(diff.float().mean()) < 1e-4


def _dense(m):
    from yolact_minimal_amd.utils.packed_masks import PackedMasks
    return m.dense() if isinstance(m, PackedMasks) else m


# (portrait, h, w): slack below the picture; exact fit (the last rows blend with the clamp row); portrait; strong down-scale
WINDOW_OUT = [(False, 90, 128), (False, 96, 128), (True, 128, 90), (False, 20, 30)]


@pytest.mark.parametrize('packed', [False, True], ids=['dense', 'packed'])
@pytest.mark.parametrize('portrait,h,w', WINDOW_OUT)
def test_after_nms_window_single_image(portrait, h, w, packed):
    from yolact_minimal_amd import hip
    from yolact_minimal_amd.utils.output_utils import after_nms
    proto, coefs, boxes = _window_case(portrait, 3)
    hp, wp = proto.shape[1:3]
    nbytes = hip.lib().ym_after_nms_window_workspace_bytes(hip.ragged_table([(h, w)], [0]), 1, 5, hp, wp, 32)
    assert (nbytes > 0) == ((h, w) == (20, 30)), 'only 20 x 30 takes the two-kernel path'
    if (h, w) == (96, 128):
        # exact fit: the last output row's second source row is row 24 of the virtual map = the clamp row
        assert 0.25 * (95 + 0.5) - 0.5 > 23 and hp == 24
    ids = torch.arange(5, device=DEV)
    scores = torch.linspace(0.9, 0.5, 5).to(DEV)
    box_d = boxes[0].to(DEV)
    got = after_nms(ids, scores, box_d, coefs[0].to(DEV), proto[0].to(DEV), h, w, packed=packed, window=True)
    assert got[0] is ids and got[1] is scores
    want = _window_want(portrait, 3, 0, h, w)
    _check_masks(got[2], _dense(got[3]), want)
    assert torch.equal(box_d.cpu(), boxes[0] * max(h, w)), 'boxes are scaled in place by max(h, w), as before'


@pytest.mark.parametrize('packed', [False, True], ids=['dense', 'packed'])
def test_after_nms_window_batch_and_ragged(packed):
    """The batch entry at one size (ints) and at per-image sizes (a fused image, the exact fit, a two-kernel image in ONE call),
    counts on the device: rows at or past a count are not written."""
    from yolact_minimal_amd.utils.output_utils import BatchDetections, after_nms_batch
    proto, coefs, boxes = _window_case(False, 3)
    counts = [5, 3, 0]

    def dets():
        return BatchDetections(torch.tensor(counts, dtype=torch.int32, device=DEV), torch.zeros(3, 5, dtype=torch.int64, device=DEV),
                               torch.full((3, 5), 0.5, device=DEV), boxes.to(DEV), coefs.to(DEV), proto.to(DEV))
    for hs, ws in ((96, 128), ([90, 96, 20], [128, 128, 30])):
        out = after_nms_batch(dets(), hs, ws, packed=packed, window=True)
        assert out[2] == (None,) * 4
        for b in (0, 1):
            h, w = (hs, ws) if isinstance(hs, int) else (hs[b], ws[b])
            assert out[b][0].shape[0] == counts[b]
            _check_masks(out[b][2], _dense(out[b][3]), _window_want(False, 3, b, h, w), n=counts[b])
    # window=True against window=False on the same tensors: they differ (the per-axis rule stretches 24 rows over the square)
    a = after_nms_batch(dets(), [96] * 3, [128] * 3, packed=packed, window=False)
    b = after_nms_batch(dets(), [96] * 3, [128] * 3, packed=packed, window=True)
    assert not torch.equal(_dense(a[0][3]), _dense(b[0][3]))


@pytest.mark.parametrize('packed', [False, True], ids=['dense', 'packed'])
@pytest.mark.parametrize('portrait,sizes', [(False, [(90, 128), (20, 30), (96, 128)]), (True, [(128, 90), (128, 96), (30, 20)])])
def test_after_nms_window_entry_writes_its_rows_only(portrait, sizes, packed):
    """The C entry on buffers of our own: rows past each count, the alignment gaps between the blocks and a guard block behind the
    last keep their fill; boxes past the count are scaled all the same (as in the ragged entry); the written rows are rect_ref's."""
    from yolact_minimal_amd import hip
    from yolact_minimal_amd.utils.output_utils import ragged_layout
    from yolact_minimal_amd.utils.packed_masks import PackedMasks
    proto, coefs, boxes = _window_case(portrait, 3)
    hp, wp = proto.shape[1:3]
    counts = [3, 5, 2]
    offsets, total = ragged_layout(sizes, 5, packed)
    table = hip.ragged_table(sizes, offsets)
    L = hip.lib()
    nbytes = L.ym_after_nms_window_workspace_bytes(table, 3, 5, hp, wp, 32)
    assert nbytes == 5 * hp * wp * 4
    guard = 1024
    if packed:
        masks = torch.full((total + guard,), -1, dtype=torch.int64, device=DEV)
    else:
        masks = torch.full((total + guard,), FILL, dtype=torch.float32, device=DEV)
    before = masks.clone()
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    box_d, px = boxes.to(DEV), torch.full((3, 5, 4), -7, dtype=torch.int32, device=DEV)
    fn = L.ym_after_nms_window_packed if packed else L.ym_after_nms_window
    proto_d, coefs_d, counts_d = proto.to(DEV), coefs.to(DEV), torch.tensor(counts, dtype=torch.int32, device=DEV)     # (kept alive)
    hip.check(fn(hip.ptr(proto_d), hip.ptr(coefs_d), hip.ptr(box_d), hip.ptr(counts_d, torch.int32),
                 3, 5, hp, wp, 32, table, 32, 1, hip.ptr(masks, masks.dtype), hip.ptr(px, torch.int32), ctypes.c_void_p(ws.data_ptr()), nbytes,
                 hip.stream_ptr()), 'ym_after_nms_window')
    torch.cuda.synchronize()
    written = torch.zeros(total + guard, dtype=torch.bool)
    for b, ((h, w), o) in enumerate(zip(sizes, offsets)):
        row = h * ((w + 63) // 64 if packed else w)
        written[o:o + counts[b] * row] = True
        block = masks[o:o + 5 * row]
        dense = PackedMasks._wrap(block.view(5, h, -1), h, w).dense() if packed else block.view(5, h, w)
        _check_masks(px[b], dense, _window_want(portrait, 3, b, h, w), n=counts[b])
        np.testing.assert_array_equal(px[b].cpu().numpy(), (boxes[b] * max(h, w)).int().numpy())
    assert torch.equal(masks.cpu()[~written], before.cpu()[~written]), 'something outside the rows below the counts was written'
    # Pv below the map's own extent, or the window entry without one, is refused before any launch
    for pv in (0, 24):
        assert fn(hip.ptr(proto_d), hip.ptr(coefs_d), hip.ptr(box_d), None, 3, 5, hp, wp, 32, table, pv, 1, hip.ptr(masks, masks.dtype),
                  hip.ptr(px, torch.int32), ctypes.c_void_p(ws.data_ptr()), nbytes, hip.stream_ptr()) != 0


# ---- 4. the window path against the square path, end to end ----------------------------------------------------------------------------
@pytest.mark.parametrize('packed', [False, True], ids=['dense', 'packed'])
def test_window_postprocessing_equals_the_square_path_on_the_same_detections(packed):
    """544 px, a 480 x 640 frame (window 416 x 544).  Square run: every anchor outside the window is background.  Window run: the
    gathered rows, the prototype map cut to 104 x 136.  Class ids, scores, boxes, pixel boxes and every mask bit are EQUAL: the window
    rule is the square geometry on the part of the map that exists, and the frame ends two prototype rows above the cut."""
    from yolact_minimal_amd import rect_anchor_index, rect_window
    from yolact_minimal_amd.utils.output_utils import after_nms, nms
    cfg = build_cfg('res101_coco', 'val', 544)
    h, w = 480, 640
    hn, wn = rect_window([(h, w)], 544)
    assert (hn, wn) == (416, 544)
    hp, wp, pv = hn // 4, wn // 4, 544 // 4
    # the last output row's source rows: floor(136 / 640 * (479 + .5) - .5) = 101 and 102 < 104: the clamp row is never read
    last = pv / max(h, w) * (h - 1 + 0.5) - 0.5
    assert int(last) + 1 == 102 and int(last) + 1 <= hp - 2
    cls, box, coef, proto = R.synth_head_outputs(18525, seed=1, bg_bias=4.0)
    anchors = R.anchors_for(544, cfg.scales)
    idx = rect_anchor_index(cfg, hn, wn)
    outside = torch.ones(18525, dtype=torch.bool)
    outside[idx] = False
    cls = cls.clone()
    cls[0, outside] = 0
    cls[0, outside, 0] = 1
    sq = nms(cls.to(DEV), box.to(DEV), coef.to(DEV), proto.to(DEV), anchors.to(DEV), cfg)
    net_anchors = anchors[idx].contiguous()
    wi = nms(cls[:, idx].to(DEV), box[:, idx].to(DEV), coef[:, idx].to(DEV), proto[:, :hp, :wp].contiguous().to(DEV), net_anchors.to(DEV), cfg)
    assert sq[0] is not None and sq[0].shape[0] > 10
    for a, b, what in zip(sq[:4], wi[:4], ('class ids', 'scores', 'boxes', 'coefs')):
        assert torch.equal(a, b), what
    assert tuple(wi[4].shape) == (hp, wp, 32)
    a = after_nms(sq[0], sq[1], sq[2].clone(), sq[3], sq[4], h, w, cfg, packed=packed)
    b = after_nms(wi[0], wi[1], wi[2].clone(), wi[3], wi[4], h, w, cfg, packed=packed, window=True)
    assert torch.equal(a[2], b[2]), 'pixel boxes'
    ma, mb = (a[3].bits, b[3].bits) if packed else (a[3], b[3])
    assert ma.shape == mb.shape and torch.equal(ma, mb), 'mask bits'
    assert float(_dense(b[3]).sum()) > 0


# ---- 5. serving ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _net128():
    net, cfg = make_net('res50_coco', 128, 9)
    return net.to(DEV), cfg


def _heads128(net, seed):
    """Synthetic head outputs of a 96 x 128 window forward at 128 px (a random-init net's own detections are degenerate)."""
    n = net.anchors_for(96, 128).shape[0]
    cls, box, coef, proto = R.synth_head_outputs(n, proto_hw=32, seed=seed, bg_bias=5.0)
    return tuple(t.to(DEV) for t in (cls, box, coef, proto[:, :24].contiguous()))


@pytest.mark.parametrize('packed', [False, True], ids=['dense', 'packed'])
def test_window_pipeline_serves_what_the_per_call_window_functions_return(packed):
    """`for_frames` picks 96 x 128 for 90 x 128 frames.  `submit_frames(draw=True)`: the drawn frames of the per-call stages
    (draw_batch, RLE, packed masks and the metrics take frame-sized outputs: nothing in them knows about the window).  Without
    drawing: the detections of `nms_batch` + `after_nms_batch(window=True)`; without post-processing: the network outputs of
    `net(val_aug_batch(frames, window=...))`."""
    from yolact_minimal_amd.pipeline import RequestPipeline
    from yolact_minimal_amd.utils.augmentations import val_aug_batch
    from yolact_minimal_amd.utils.frames import FrameBatch
    from yolact_minimal_amd.utils.output_utils import after_nms_batch, draw_batch, nms_batch
    net, cfg = _net128()
    dev = torch.device(DEV)
    frames = [FrameBatch.from_tensors([_frame(90, 128, torch.uint8, 20 + k).to(DEV)]) for k in range(2)]
    heads = [_heads128(net, 5 + k) for k in range(2)]
    anchors = net.anchors_for(96, 128, dev)
    try:
        pipe = RequestPipeline.for_frames(net, cfg, [(90, 128)], dev, depth=2, packed_masks=packed)
        assert pipe.window == (96, 128) and (pipe.engines[0].H, pipe.engines[0].W) == (96, 128)
        assert torch.equal(pipe.anchors, anchors)
        pipe.warm_up(torch.zeros(1, 3, 96, 128, device=dev), rounds=0)
        want_drawn, want_dets = [], []
        for k in range(2):
            r = after_nms_batch(nms_batch(*heads[k], anchors, cfg), [90], [128], cfg, sync=False, packed=packed, window=True)
            want_drawn.append(draw_batch(r, frames[k], cfg))
            want_dets.append(after_nms_batch(nms_batch(*heads[k], anchors, cfg), [90], [128], cfg, packed=packed, window=True)[0])
        assert [pipe.submit_frames(frames[k], heads[k], draw=True) for k in range(2)] == [None, None]
        drawn = pipe.drain()
        assert [pipe.submit_frames(frames[k], heads[k]) for k in range(2)] == [None, None]
        dets = pipe.drain()
        # a frame batch whose picture does not fit the window: refused before anything is launched or counted
        submitted = pipe.submitted
        for bad in ((128, 128), (128, 90), (100, 128)):
            with pytest.raises(RuntimeError, match=r'96 x 128') as e:
                pipe.submit_frames(FrameBatch.from_tensors([_frame(*bad, torch.uint8, 1).to(DEV)]), heads[0], draw=True)
            assert '128 x 128' in str(e.value) or '128 x 96' in str(e.value)
        assert pipe.submitted == submitted and pipe.pending == [None, None] and pipe.drain() == []
        # the forward itself, through the slot's engine (the throughput plan: fp32 summation order may differ from net()'s)
        fwd = RequestPipeline.for_frames(net, cfg, [(90, 128)], dev, depth=1, with_post=False)
        assert fwd.submit_frames(frames[0]) is None
        outs = fwd.drain()[0]
        with torch.no_grad():
            ref = net(val_aug_batch(frames[0], 128, window=(96, 128)))
    finally:
        net._engines.clear()
    for k in range(2):
        assert isinstance(drawn[k], FrameBatch) and drawn[k].sizes == [(90, 128)]
        assert torch.equal(drawn[k].frames[0], want_drawn[k].frames[0]), k
        assert not torch.equal(drawn[k].frames[0], frames[k].frames[0]), 'nothing was drawn'
        assert dets[k][0] is not None and dets[k][0].shape[0] > 0
        for a, b in zip(dets[k], want_dets[k]):
            a, b = (a.bits, b.bits) if packed and not torch.is_tensor(a) else (a, b)
            assert a.shape == b.shape and torch.equal(a, b)
        assert tuple(_dense(dets[k][3]).shape[1:]) == (90, 128)
    for a, b, key in zip(outs, ref, ('class', 'box', 'coef', 'proto')):
        _close(a, b, f'window pipeline forward {key}')
    assert tuple(outs[3].shape) == (1, 24, 32, 32)


def test_for_frames_gives_the_square_pipeline_for_square_or_mixed_frames_and_it_serves_as_before():
    """`height == width` is the path it was: no window, the square anchors, results equal to the square per-call functions."""
    from yolact_minimal_amd.pipeline import RequestPipeline
    from yolact_minimal_amd.utils.frames import FrameBatch
    from yolact_minimal_amd.utils.output_utils import after_nms, nms
    net, cfg = _net128()
    dev = torch.device(DEV)
    n = len(net.anchors) // 4
    heads = tuple(t.to(DEV) for t in R.synth_head_outputs(n, proto_hw=32, seed=4, bg_bias=5.0))
    frames = FrameBatch.from_tensors([_frame(90, 128, torch.uint8, 2).to(DEV)])
    try:
        for hw in ([(100, 100)], [(90, 128), (128, 90)]):
            pipe = RequestPipeline.for_frames(net, cfg, hw, dev, depth=2)
            assert pipe.window is None and (pipe.engines[0].H, pipe.engines[0].W) == (128, 128)
            assert tuple(pipe.anchors.shape) == (n, 4)
        pipe.warm_up(torch.zeros(1, 3, 128, 128, device=dev), rounds=0)
        assert pipe.submit_frames(frames, heads) is None
        got = pipe.drain()[0]
        want = after_nms(*nms(*heads, net.anchors, cfg), 90, 128, cfg)
    finally:
        net._engines.clear()
    assert got[0] is not None
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
