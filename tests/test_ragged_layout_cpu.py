"""Mixed-size batches without a GPU: `ragged_layout` (256-byte aligned, disjoint blocks), the argument errors of
`after_nms_batch` with per-image sizes, and the C-ABI surface of `ym_after_nms_ragged[_packed]`."""
import ctypes
import os
import re

import pytest
import torch

from tests.conftest import REPO
from yolact_minimal_amd import hip
from yolact_minimal_amd.utils.output_utils import BatchDetections, after_nms_batch, ragged_layout

NEW_SYMBOLS = ('ym_after_nms_ragged_workspace_bytes', 'ym_after_nms_ragged', 'ym_after_nms_ragged_packed')
COCO_LIKE = [(480, 640), (640, 480), (427, 640), (375, 500), (500, 333), (640, 640)]


def _block(h, w, max_det, packed):
    return max_det * h * ((w + 63) // 64 if packed else w)


@pytest.mark.parametrize('packed', [False, True], ids=['dense', 'packed'])
@pytest.mark.parametrize('max_det,sizes', [
    (7, [(97, 301), (120, 128)]),                          # 7 * 97 * 301 floats: the unpadded second offset would be odd
    (7, [(97, 301), (120, 128), (48, 70)]),
    (100, COCO_LIKE + COCO_LIKE[:2]),
    (1, [(1, 1)] * 32),
    (3, [(5, 63), (5, 64), (5, 65), (1, 1), (333, 64)]),
])
def test_layout_is_aligned_disjoint_and_covered(packed, max_det, sizes):
    offsets, total = ragged_layout(sizes, max_det, packed)
    esz = 8 if packed else 4
    assert len(offsets) == len(sizes) and offsets[0] == 0
    end = 0
    for (h, w), o in zip(sizes, offsets):
        assert isinstance(o, int) and (o * esz) % 256 == 0
        assert o >= end                                     # in order, so disjoint
        assert o - end < 256 // esz                         # and no more padding than the alignment asks for
        end = o + _block(h, w, max_det, packed)
    assert total == end                                     # the total covers the last block


def test_the_unpadded_offset_would_be_misaligned():
    assert (7 * 97 * 301) % 2 == 1
    offsets, _ = ragged_layout([(97, 301), (120, 128)], 7, False)
    assert offsets[1] > 7 * 97 * 301 and offsets[1] % 64 == 0


def _fake_dets(batch, md=7, hp=8):
    z = torch.zeros
    return BatchDetections(z(batch, dtype=torch.int32), z(batch, md, dtype=torch.int64), z(batch, md), z(batch, md, 4), z(batch, md, 32),
                           z(batch, hp, hp, 32))


def test_argument_errors_raise_before_any_launch():
    for bad in ([], [(10, 10)] * 33, [(0, 10)], [(10, -1)]):
        with pytest.raises(RuntimeError):
            ragged_layout(bad, 7)
    with pytest.raises(RuntimeError):
        ragged_layout([(10, 10)], 0)
    # (CPU tensors: every one of these must raise on the arguments, not reach the device)
    with pytest.raises(RuntimeError, match='heights'):
        after_nms_batch(_fake_dets(3), [10, 10], [10, 10, 10])              # length mismatch
    with pytest.raises(RuntimeError, match='heights'):
        after_nms_batch(_fake_dets(3), [10, 10, 10], 10)                    # a sequence and an int
    with pytest.raises(RuntimeError, match='output size'):
        after_nms_batch(_fake_dets(2), [10, 0], [10, 10])
    with pytest.raises(RuntimeError, match='output size'):
        after_nms_batch(_fake_dets(2), [10, 10], [-3, 10], packed=True)
    with pytest.raises(RuntimeError, match='images per call'):
        after_nms_batch(_fake_dets(33), [10] * 33, [10] * 33)
    with pytest.raises(RuntimeError, match='no CPU path'):
        after_nms_batch(_fake_dets(2), [10, 12], [10, 12])                  # valid arguments: the loud CPU failure


def _header():
    text = open(os.path.join(REPO, 'include', 'yolact_hip.h')).read()
    return re.sub(r'/\*.*?\*/', '', text, flags=re.S)


def test_header_binding_and_library_agree_on_the_ragged_symbols():
    text = _header()
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    raw = ctypes.CDLL(hip.LIB_PATH)
    L = hip.lib()
    for name in NEW_SYMBOLS:
        m = re.search(r'\b' + name + r'\s*\(([^)]*)\)', text)
        assert m, name + ' is not declared in include/yolact_hip.h'
        assert name in hip.ABI_SYMBOLS and hasattr(raw, name), name
        assert len(getattr(L, name).argtypes) == len(m.group(1).split(',')), name
    assert int(re.search(r'#define\s+YM_RAGGED_MAX_IMAGES\s+(\d+)', text).group(1)) == hip.RAGGED_MAX_IMAGES == 32
    assert int(re.search(r'#define\s+YM_RAGGED_ALIGN_BYTES\s+(\d+)', text).group(1)) == hip.RAGGED_ALIGN_BYTES == 256
    assert ctypes.sizeof(hip.RaggedImage) == 16 and hip.RaggedImage.offset.offset == 8
    assert raw.ym_abi_version() == 1


def test_library_refuses_bad_tables_without_a_gpu():
    """The entry checks its table before it touches the device: too many images, a misaligned or overlapping block."""
    L = hip.lib()
    one = ctypes.c_void_p(256)                                               # (never dereferenced: the checks come first)

    def call(entries, packed=False, md=7):
        tab = (hip.RaggedImage * len(entries))(*[hip.RaggedImage(*e) for e in entries])
        fn = L.ym_after_nms_ragged_packed if packed else L.ym_after_nms_ragged
        return fn(one, one, one, one, len(entries), md, 32, 32, 32, tab, 1, one, one, None, 0, None)

    assert call([(10, 10, 64 * i * 7 * 2) for i in range(33)]) == -1
    assert b'images per call' in L.ym_last_error()
    assert call([(10, 10, 0), (10, 10, 7 * 100 + 1)]) == -1
    assert b'multiple of 256' in L.ym_last_error()
    assert call([(10, 10, 0), (10, 10, 64)]) == -1
    assert b'overlap' in L.ym_last_error()
    assert call([(10, 0, 0)], packed=True) == -1
    tab = (hip.RaggedImage * 2)(hip.RaggedImage(480, 640, 0), hip.RaggedImage(48, 70, 1 << 30))
    assert L.ym_after_nms_ragged_workspace_bytes(tab, 2, 7, 32, 32) == 7 * 32 * 32 * 4          # (48, 70) needs the two-kernel path
    assert L.ym_after_nms_ragged_workspace_bytes(tab, 1, 7, 32, 32) == 0
    assert L.ym_after_nms_ragged_workspace_bytes(tab, 2, 100, 136, 136) == 100 * 136 * 136 * 4
