"""Rectangular inference ("window mode"), the host side: window and anchor geometry, and the C-ABI surface.  No GPU."""
import inspect
import re
import os

import pytest
import torch

from oracle import yolact_ref as R
from tests.conftest import REPO
from yolact_minimal_amd.config import build_cfg


@pytest.mark.parametrize('h,w,size,want', [
    (480, 640, 544, (416, 544)), (1080, 1920, 544, (320, 544)), (640, 480, 544, (544, 416)), (500, 500, 544, (544, 544)),
    (32, 64, 64, (32, 64)), (30, 80, 64, (32, 64))])
def test_rect_window(h, w, size, want):
    from yolact_minimal_amd import rect_window
    assert rect_window([(h, w)], size) == want
    assert rect_window((h, w), size) == want                   # one pair
    assert size in rect_window([(h, w)], size)                 # one of the two is always the square's side


def test_rect_window_of_a_mixed_batch():
    from yolact_minimal_amd import rect_window
    assert rect_window([(480, 640), (640, 480)], 544) == (544, 544)            # landscape + portrait -> the square
    assert rect_window([(480, 640), (1080, 1920)], 544) == (416, 544)          # the larger of the two windows
    assert rect_window([(90, 128), (96, 128)], 128) == (96, 128)
    with pytest.raises(RuntimeError):
        rect_window([], 544)
    with pytest.raises(RuntimeError):
        rect_window([(0, 5)], 544)


def test_rect_anchor_index_counts():
    from yolact_minimal_amd import rect_anchor_index
    from yolact_minimal_amd.utils.rect import rect_level_shapes
    cfg = build_cfg('res50_coco', 'val', 64)
    idx = rect_anchor_index(cfg, 32, 64)
    assert idx.dtype == torch.int64 and idx.numel() == 3 * (32 + 8 + 2 + 1 + 1) == 132
    assert len(R.anchors_for(64, cfg.scales)) == 258
    assert rect_level_shapes(416, 544) == [(52, 68), (26, 34), (13, 17), (7, 9), (4, 5)]
    cfg = build_cfg('res101_coco', 'val', 544)
    idx = rect_anchor_index(cfg, 416, 544)
    assert idx.numel() == 3 * (52 * 68 + 26 * 34 + 13 * 17 + 7 * 9 + 4 * 5)
    with pytest.raises(RuntimeError):
        rect_anchor_index(cfg, 416, 576)                       # wider than the square
    with pytest.raises(RuntimeError):
        rect_anchor_index(cfg, 408, 544)                       # not a multiple of 32


@pytest.mark.parametrize('size,hn,wn', [(64, 32, 64), (64, 64, 32), (128, 96, 128), (544, 416, 544), (544, 544, 320)])
def test_rect_anchors_are_rows_of_the_square_list(size, hn, wn):
    from yolact_minimal_amd import rect_anchor_index
    from yolact_minimal_amd.modules.yolact import Yolact
    cfg = build_cfg('res50_coco', 'val', size)
    net = Yolact(cfg).eval()
    before = list(net.anchors)
    idx = rect_anchor_index(cfg, hn, wn)
    assert bool((idx[1:] > idx[:-1]).all())                    # strictly increasing: the square list's order, thinned
    square = R.anchors_for(size, cfg.scales)
    got = net.anchors_for(hn, wn)
    assert got.dtype == torch.float32 and tuple(got.shape) == (idx.numel(), 4)
    assert torch.equal(got, square[idx])
    assert net.anchors_for(hn, wn) is got                      # cached per shape
    assert net.anchors == before                               # net.anchors itself stays as it is
    # the kept rows are exactly the anchors whose cell lies inside the window: centre < window / size on both axes
    inside = (square[:, 0] * size < wn) & (square[:, 1] * size < hn)
    keep = torch.zeros(len(square), dtype=torch.bool)
    keep[idx] = True
    strides = torch.cat([torch.full((3 * (-(-size // s)) ** 2,), s) for s in (8, 16, 32, 64, 128)])
    assert torch.equal(keep[strides <= 32], inside[strides <= 32])      # (the two ceil'ed levels may keep a cell that straddles the edge)


@pytest.mark.parametrize('size', [64, 544])
def test_square_window_keeps_every_anchor(size):
    from yolact_minimal_amd import rect_anchor_index
    cfg = build_cfg('res50_coco', 'val', size)
    n = len(R.anchors_for(size, cfg.scales))
    win = -(-size // 32) * 32
    if win == size:
        assert torch.equal(rect_anchor_index(cfg, size, size), torch.arange(n))


def _declared():
    text = open(os.path.join(REPO, 'include', 'yolact_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return text


NEW = ('ym_val_preprocess_window', 'ym_after_nms_window_workspace_bytes', 'ym_after_nms_window', 'ym_after_nms_window_packed')


def test_new_symbols_are_declared_bound_and_exported():
    import ctypes
    from yolact_minimal_amd import hip
    text = _declared()
    for name in NEW:
        assert name in hip.ABI_SYMBOLS and re.search(r'\b' + name + r'\s*\(', text), name
    lib = hip.lib()
    for name in NEW:
        assert hasattr(lib, name), name
    # the window entries are the ragged ones plus `int Pv` behind the table; the preprocess entry plus `int Hn, int Wn` behind S
    i32 = ctypes.c_int
    rag = list(lib.ym_after_nms_ragged.argtypes)
    assert list(lib.ym_after_nms_window.argtypes) == rag[:10] + [i32] + rag[10:]
    assert list(lib.ym_after_nms_window_packed.argtypes) == list(lib.ym_after_nms_window.argtypes)
    assert list(lib.ym_after_nms_window_workspace_bytes.argtypes) == list(lib.ym_after_nms_ragged_workspace_bytes.argtypes) + [i32]
    pre = list(lib.ym_val_preprocess_batch.argtypes)
    assert list(lib.ym_val_preprocess_window.argtypes) == pre[:5] + [i32, i32] + pre[5:]


def test_old_signatures_are_unchanged():
    """The entries that existed before window mode keep their C signatures (header text) and their ctypes bindings."""
    import ctypes
    from yolact_minimal_amd import hip
    text = re.sub(r'\s+', ' ', _declared())
    for decl in (
            'int ym_val_preprocess(const void* img_hwc_bgr, int is_uint8, int H, int W, int S, const float* mean_bgr, const float* std_bgr, float* out_chw_rgb, ym_stream_t s);',
            'int ym_val_preprocess_batch(const void* frames, int is_uint8, const ym_ragged_image* images, int B, int S, const float* mean_bgr, const float* std_bgr, float* out, ym_stream_t s);',
            'size_t ym_after_nms_batch_workspace_bytes(int max_det, int Hp, int Wp, int img_h, int img_w);',
            'size_t ym_after_nms_ragged_workspace_bytes(const ym_ragged_image* images, int B, int max_det, int Hp, int Wp);',
            'int ym_after_nms_ragged(const float* proto, const float* coefs, float* boxes, const int32_t* counts, int B, int max_det, int Hp, int Wp, int K, const ym_ragged_image* images, int do_crop, float* masks, int32_t* boxes_px, void* workspace, size_t workspace_bytes, ym_stream_t s);',
            'int ym_mask_assemble(const float* proto, const float* coefs, const float* boxes, int n, int Hp, int Wp, int K, int do_crop, float* out, ym_stream_t s);',
            'int ym_mask_resize_binarize(const float* masks, int n, int Hp, int Wp, int img_h, int img_w, float* out, ym_stream_t s);'):
        assert decl in text, decl
    lib = hip.lib()
    vp, i32, sz, fp = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(ctypes.c_float)
    tab = ctypes.POINTER(hip.RaggedImage)
    assert list(lib.ym_val_preprocess.argtypes) == [vp, i32, i32, i32, i32, fp, fp, vp, vp]
    assert list(lib.ym_val_preprocess_batch.argtypes) == [vp, i32, tab, i32, i32, fp, fp, vp, vp]
    assert list(lib.ym_after_nms_batch.argtypes) == [vp] * 4 + [i32] * 8 + [vp, vp, vp, sz, vp]
    assert list(lib.ym_after_nms_batch_packed.argtypes) == list(lib.ym_after_nms_batch.argtypes)
    assert list(lib.ym_after_nms_ragged.argtypes) == [vp] * 4 + [i32] * 5 + [tab, i32, vp, vp, vp, sz, vp]
    assert list(lib.ym_after_nms_ragged_workspace_bytes.argtypes) == [tab, i32, i32, i32, i32]
    assert list(lib.ym_mask_assemble.argtypes) == [vp, vp, vp, i32, i32, i32, i32, i32, vp, vp]
    assert list(lib.ym_mask_resize_binarize.argtypes) == [vp, i32, i32, i32, i32, i32, vp, vp]


def test_python_surface():
    from yolact_minimal_amd.pipeline import RequestPipeline
    from yolact_minimal_amd.utils.augmentations import val_aug, val_aug_batch
    from yolact_minimal_amd.utils.output_utils import after_nms, after_nms_batch
    for fn in (val_aug, val_aug_batch):
        assert inspect.signature(fn).parameters['window'].default is None
    for fn in (after_nms, after_nms_batch):
        assert inspect.signature(fn).parameters['window'].default is False
    assert callable(RequestPipeline.for_frames)


def test_window_workspace_query_follows_the_virtual_extent():
    """Which path an image takes is a host decision on Pv / max(h, w) (both axes), not on the physical map."""
    from yolact_minimal_amd import hip
    L = hip.lib()
    tab = hip.ragged_table([(20, 30)], [0])
    assert L.ym_after_nms_window_workspace_bytes(tab, 1, 5, 24, 32, 32) == 5 * 24 * 32 * 4      # 30 px from a 32-wide extent: two kernels
    tab = hip.ragged_table([(96, 128)], [0])
    assert L.ym_after_nms_window_workspace_bytes(tab, 1, 5, 24, 32, 32) == 0                    # fused
    assert L.ym_after_nms_window_workspace_bytes(tab, 1, 5, 24, 32, 0) == L.ym_after_nms_ragged_workspace_bytes(tab, 1, 5, 24, 32)
