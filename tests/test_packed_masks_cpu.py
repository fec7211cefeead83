"""Bit-packed instance masks without a GPU: the layout (`pack_reference` / `unpack_reference` state it in numpy), the golden
fixtures' own packed masks through it, the C-ABI surface, and the loud failure on CPU tensors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.conftest import REPO
from yolact_minimal_amd.utils.output_utils import PackedMasks, after_nms, pack_reference, unpack_reference

NEW_SYMBOLS = ('ym_after_nms_batch_packed', 'ym_pack_masks', 'ym_unpack_masks', 'ym_mask_iou_packed_workspace_bytes',
               'ym_mask_iou_packed', 'ym_rle_encode_packed', 'ym_draw_detections_batch_packed', 'ym_draw_cutout_objects_packed')


@pytest.mark.parametrize('w', [1, 63, 64, 65, 500, 640])
def test_reference_pair_round_trips_and_pads_with_zeros(w):
    rng = np.random.default_rng(w)
    m = (rng.random((3, 5, w)) < 0.5).astype(np.uint8)
    m[0, 0, :] = 1                                                    # a full row: every pad bit would show
    bits = pack_reference(m)
    wq = (w + 63) // 64
    assert bits.dtype == np.int64 and bits.shape == (3, 5, wq) and bits.flags['C_CONTIGUOUS']
    back = unpack_reference(bits, w)
    assert back.dtype == np.uint8 and back.shape == m.shape
    np.testing.assert_array_equal(back, m)
    # bit k of word j is pixel 64 j + k, spelled out with python integers
    u = bits.view(np.uint64)
    for j in range(wq):
        for k in range(64):
            x = 64 * j + k
            got = (u[..., j] >> np.uint64(k)) & np.uint64(1)
            want = m[..., x] if x < w else np.zeros(m.shape[:2], dtype=np.uint8)          # pad bits are zero
            np.testing.assert_array_equal(got.astype(np.uint8), want)
    # the host view documented in include/yolact_hip.h
    view = np.unpackbits(bits.view(np.uint8).reshape(3, 5, wq * 8), axis=-1, bitorder='little')[..., :w]
    np.testing.assert_array_equal(view, m)
    # float masks pack like their != 0
    np.testing.assert_array_equal(pack_reference(m.astype(np.float32) * 0.25), bits)


def test_golden_packed_masks_survive_the_layout(golden_dir):
    g = np.load(os.path.join(golden_dir, 'post_small128.npz'))
    n = int(g['n'])
    gold = g['masks_96x128_packed']                                     # MSB-first np.packbits of the flat [n, 96, 128] tensor
    dense = np.unpackbits(gold)[:n * 96 * 128].reshape(n, 96, 128)
    assert dense.any()
    bits = pack_reference(dense)
    assert bits.shape == (n, 96, 2)
    back = unpack_reference(bits, 128)
    np.testing.assert_array_equal(np.packbits(back.reshape(-1)), gold)


def test_header_declares_and_library_exports_the_packed_symbols():
    from yolact_minimal_amd import hip
    text = open(os.path.join(REPO, 'include', 'yolact_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = set(re.findall(r'\b(ym_[a-z0-9_]+)\s*\(', text))
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in hip.ABI_SYMBOLS, name
        assert hasattr(lib, name), name


def test_cpu_tensors_fail_loudly():
    with pytest.raises(RuntimeError):
        PackedMasks.pack(torch.zeros(2, 8, 8))
    with pytest.raises(RuntimeError):
        PackedMasks(torch.zeros(2, 8, 1, dtype=torch.int64), 8, 8)
    n = 3
    with pytest.raises(RuntimeError):
        after_nms(torch.zeros(n, dtype=torch.int64), torch.ones(n), torch.rand(n, 4), torch.zeros(n, 32), torch.zeros(8, 8, 32), 16, 16,
                  packed=True)
