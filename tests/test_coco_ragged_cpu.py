"""The ragged annotation rasteriser without a GPU: `ym_ann_to_mask_ragged` / `ym_ann_to_mask_ragged_workspace_bytes` are declared,
exported and bound; every refusal of the entry comes before any HIP call; the workspace size function; the host packer
`pack_annotations` on a hand-written input."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.conftest import REPO
from yolact_minimal_amd import hip

NAMES = ('ym_ann_to_mask_ragged_workspace_bytes', 'ym_ann_to_mask_ragged')
I32P = ctypes.POINTER(ctypes.c_int32)

_MEM = torch.zeros(4096, dtype=torch.uint8)                         # a non-null pointer; a refused call never follows it
_P = _MEM.data_ptr() + (-_MEM.data_ptr()) % 16


def test_the_entries_are_declared_exported_and_bound():
    text = open(os.path.join(REPO, 'include', 'yolact_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    lib = hip.lib()
    for name in NAMES:
        assert re.search(r'\b' + name + r'\s*\(', text), name
        assert name in hip.ABI_SYMBOLS and hasattr(lib, name) and getattr(lib, name).argtypes is not None
    assert lib.ym_ann_to_mask_ragged_workspace_bytes.restype is ctypes.c_size_t
    assert lib.ym_abi_version() == 1


def _first(values):
    return (ctypes.c_int32 * len(values))(*values)


def _call(sizes=((48, 64), (37, 53)), offsets=(0, 6400), first=(0, 2, 3), batch=None, null_images=False, null_first=False,
          masks=_P, item_off=_P, ann_off=_P, ann_kind=_P, workspace=None, workspace_bytes=0):
    lib = hip.lib()
    table = hip.ragged_table(sizes, offsets)
    rc = lib.ym_ann_to_mask_ragged(ctypes.c_void_p(_P), ctypes.c_void_p(_P), ctypes.c_void_p(item_off) if item_off else None,
                                   ctypes.c_void_p(ann_off) if ann_off else None, ctypes.c_void_p(ann_kind) if ann_kind else None,
                                   None if null_images else table, None if null_first else ctypes.cast(_first(first), I32P),
                                   len(sizes) if batch is None else batch, ctypes.c_void_p(masks) if masks else None,
                                   workspace, workspace_bytes, None)
    return rc, lib.ym_last_error().decode()


@pytest.mark.parametrize('kw,text', [
    ({'batch': 0}, '1 .. 32 images per call, got 0'),
    ({'batch': -1}, '1 .. 32 images per call, got -1'),
    ({'batch': 33}, '1 .. 32 images per call, got 33'),
    ({'null_images': True}, 'null image table'),
    ({'null_first': True}, 'null ann_first table'),
    ({'sizes': ((48, 0), (37, 53))}, 'image 0 is 48 x 0'),
    ({'sizes': ((48, 64), (-1, 53))}, 'image 1 is -1 x 53'),
    ({'sizes': ((4, 4097), (37, 53)), 'offsets': (0, 65536)}, 'image 0 is 4 x 4097: need 0 < W <= 4096'),
    ({'sizes': ((1 << 19, 4096), (37, 53)), 'first': (0, 0, 1)}, 'H*W < 2^31'),
    ({'first': (1, 2, 3)}, 'ann_first[0] = 1, not 0'),
    ({'first': (0, 2, 1)}, 'ann_first decreases at image 1 (1 after 2)'),
    ({'offsets': (0, 6200)}, 'image 1: block offset 6200 is not a multiple of 256 bytes'),
    ({'offsets': (0, 6144)}, 'the blocks of images 0 and 1 overlap'),               # image 0 holds 2 * 48 * 64 = 6144 bytes
    ({'offsets': (0, 5888)}, 'the blocks of images 0 and 1 overlap'),
    ({'masks': _P + 2}, 'masks must be 4-byte aligned'),
    ({'item_off': None}, '3 annotations with a null'),
    ({'ann_off': None}, '3 annotations with a null'),
    ({'ann_kind': None}, '3 annotations with a null'),
    ({'masks': None}, '3 annotations with a null'),
])
def test_the_entry_refuses_before_any_hip_call(kw, text):
    if kw.get('offsets') == (0, 6144):
        kw = dict(kw, first=(0, 3, 4))                             # three masks in image 0: 9216 bytes, past the next block's start
    rc, err = _call(**kw)
    assert rc == -1 and err.startswith('ann_to_mask_ragged:') and text in err, (rc, err)


def test_a_short_workspace_is_enospc_and_no_annotations_a_no_op():
    sizes, offsets, first = ((48, 64), (900, 1100)), (0, 3072), (0, 1, 3)
    need = hip.lib().ym_ann_to_mask_ragged_workspace_bytes(hip.ragged_table(sizes, offsets), ctypes.cast(_first(first), I32P), 2)
    assert need > 0
    for ws, nbytes in ((None, need), (ctypes.c_void_p(_P), need - 1), (None, 0)):
        rc, err = _call(sizes=sizes, offsets=offsets, first=first, workspace=ws, workspace_bytes=nbytes)
        assert rc == -2 and f'ann_to_mask_ragged: workspace < {need} bytes' in err, (rc, err)
    # n == 0: nothing to do, null device arrays and a null `masks` are fine -- but the tables are still checked
    assert _call(first=(0, 0, 0), masks=None, item_off=None, ann_off=None, ann_kind=None)[0] == 0
    assert _call(first=(0, 0, 0), offsets=(0, 100))[0] == -1


def _ws(sizes, counts):
    from yolact_minimal_amd.utils.coco import _mask_block_layout
    offsets, _ = _mask_block_layout(list(sizes), list(counts))
    first = np.concatenate([[0], np.cumsum(counts)]).tolist()
    return hip.lib().ym_ann_to_mask_ragged_workspace_bytes(hip.ragged_table(sizes, offsets), ctypes.cast(_first(first), I32P), len(sizes))


def test_workspace_size_is_the_sum_of_the_large_images_slices():
    lib = hip.lib()
    assert _ws([(640, 640), (48, 64)], [5, 7]) == 0
    one = lib.ym_ann_to_mask_workspace_bytes(1, 900, 1100)
    assert one > 0
    for n_big in (1, 3):
        assert _ws([(640, 640), (900, 1100), (48, 64)], [5, n_big, 7]) == n_big * one == lib.ym_ann_to_mask_workspace_bytes(n_big, 900, 1100)
    assert _ws([(640, 640), (900, 1100), (48, 64)], [5, 0, 7]) == 0             # a large image without annotations needs nothing
    assert _ws([(900, 1100), (48, 64), (1000, 1000)], [2, 1, 3]) == 2 * one + lib.ym_ann_to_mask_workspace_bytes(3, 1000, 1000)
    # arguments the entry would refuse: 0
    table, first = hip.ragged_table([(900, 1100)], [0]), ctypes.cast(_first([0, 2]), I32P)
    assert lib.ym_ann_to_mask_ragged_workspace_bytes(table, first, 1) == 2 * one
    assert lib.ym_ann_to_mask_ragged_workspace_bytes(None, first, 1) == 0
    assert lib.ym_ann_to_mask_ragged_workspace_bytes(table, None, 1) == 0
    assert lib.ym_ann_to_mask_ragged_workspace_bytes(table, first, 0) == 0
    assert lib.ym_ann_to_mask_ragged_workspace_bytes(table, first, 33) == 0
    assert lib.ym_ann_to_mask_ragged_workspace_bytes(table, ctypes.cast(_first([0, -1]), I32P), 1) == 0
    assert lib.ym_ann_to_mask_ragged_workspace_bytes(hip.ragged_table([(900, 1100)], [100]), first, 1) == 0
    assert lib.ym_ann_to_mask_ragged_workspace_bytes(hip.ragged_table([(9, 5000)], [0]), first, 1) == 0


def test_pack_annotations_on_a_hand_written_batch():
    from oracle import rle_ref as R
    from yolact_minimal_amd.utils.coco import pack_annotations
    tri, quad, odd = [1.0, 2.0, 6.0, 2.0, 6.0, 7.0], [0, 0, 0, 5, 4, 5, 4, 0], [2, 3, 5, 3, 5, 8, 9.5]     # odd: 3 vertices + a stray value
    dense = np.zeros((10, 12), np.uint8)
    dense[2:5, 3:7] = 1
    runs = R.rle_counts(dense)
    segs = [[[tri, quad], {'size': [10, 12], 'counts': runs}, [], {'size': [10, 12], 'counts': R.rle_to_string(runs)}],      # mixed
            [],                                                                                                          # no annotation
            [[odd]]]
    sizes = [(10, 12), (37, 53), (9, 7)]
    pk = pack_annotations(segs, sizes)
    nr = len(runs)
    assert pk.ann_first == [0, 4, 4, 5] and pk.sizes == sizes
    np.testing.assert_array_equal(pk.ann_kind, [0, 1, 0, 1, 0])
    # entries: [tri, quad, end] [runs, end] [end] [runs, end] [odd, end]
    np.testing.assert_array_equal(pk.ann_off, [0, 3, 5, 6, 8, 10])
    np.testing.assert_array_equal(pk.item_off, [0, 3, 7, 0, nr, 7, nr, 2 * nr, 7, 10])
    np.testing.assert_array_equal(pk.xy, np.array(tri + quad + odd[:6], np.float64))
    np.testing.assert_array_equal(pk.counts, np.array(list(runs) * 2, np.uint32))
    assert [a.dtype for a in (pk.xy, pk.counts, pk.item_off, pk.ann_off, pk.ann_kind)] == \
        [np.float64, np.uint32, np.int32, np.int32, np.int32]
    # the masks: [4, 10, 12] at 0, nothing for image 1 (its offset is still aligned), [1, 9, 7] behind
    assert pk.block_offsets == [0, 512, 512] and pk.total_bytes == 512 + 63
    assert all(o % hip.RAGGED_ALIGN_BYTES == 0 for o in pk.block_offsets)
    # one host buffer, every array at an 8-byte aligned offset, in the order of the entry's arguments, not overlapping
    assert pk.buffer.dtype == np.uint8 and pk.buffer.ndim == 1
    names = ('xy', 'counts', 'item_off', 'ann_off', 'ann_kind')
    assert tuple(pk.array_offsets) == names and all(pk.array_offsets[n] % 8 == 0 for n in names)
    end = 0
    for name in names:
        arr = getattr(pk, name)
        assert pk.array_offsets[name] >= end and arr.base is not None
        assert arr.ctypes.data == pk.buffer.ctypes.data + pk.array_offsets[name]
        end = pk.array_offsets[name] + arr.nbytes
    assert end <= pk.buffer.nbytes


def test_pack_annotations_spans_more_than_one_launch_and_refuses_bad_input():
    from yolact_minimal_amd.utils.coco import pack_annotations
    sizes = [((9, 1), (1, 9), (33, 4))[i % 3] for i in range(33)]
    pk = pack_annotations([[[[0, 0, 1, 0, 1, 1]]] for _ in sizes], sizes)
    assert pk.ann_first == list(range(34)) and pk.block_offsets == [256 * i for i in range(33)] and pk.total_bytes == 256 * 32 + 132
    empty = pack_annotations([], [])
    assert empty.ann_first == [0] and empty.block_offsets == [] and empty.total_bytes == 0 and empty.ann_off.tolist() == [0]
    with pytest.raises(ValueError, match='RLE annotation of size'):
        pack_annotations([[[[0, 0, 4, 0, 4, 4]]], [{'size': [11, 12], 'counts': [120]}]], [(8, 8), (10, 12)])
    with pytest.raises(ValueError, match='2 annotation lists for 1 image sizes'):
        pack_annotations([[], []], [(8, 8)])
    with pytest.raises(RuntimeError, match='output size 0 x 8'):
        pack_annotations([[]], [(0, 8)])


def test_anns_to_masks_batch_needs_a_device():
    from yolact_minimal_amd.utils.coco import anns_to_masks_batch
    with pytest.raises(RuntimeError, match='a CUDA/HIP device is required'):
        anns_to_masks_batch([[[[0, 0, 4, 0, 4, 4]]]], [(8, 8)], device='cpu')
