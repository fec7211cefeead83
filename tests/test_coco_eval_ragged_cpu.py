"""The batched COCO metric stage without a GPU: `ym_eval_coco_add_ragged_packed` is exported and bound, refuses bad arguments on the
host before any HIP call (a 4 KB host buffer stands for every device pointer: a refused call never follows it), and its workspace
query is a host function of the sizes."""
import ctypes

import pytest
import torch

from yolact_minimal_amd import hip

EINVAL, ENOSPC = -1, -2           # YM_EINVAL, YM_ENOSPC
ALIGN = hip.RAGGED_ALIGN_BYTES // 8
NAME = 'eval_coco_add_ragged_packed:'
POINTERS = ('ids', 'scores', 'boxes', 'counts', 'det_bits', 'gt_class', 'gt_crowd', 'gt_area', 'gt_xywh', 'gt_bits', 'thr', 'area_rng',
            'score', 'cls', 'rank', 'flags', 'npig', 'class_rows', 'ws')


def _words(h, w):
    return h * ((w + 63) // 64)


def _layout(sizes, rows):
    """Blocks of rows[b] x h x ceil(w / 64) words, each at the next multiple of 256 bytes (any number of images)."""
    offsets, end = [], 0
    for (h, w), r in zip(sizes, rows):
        offsets.append(-(-end // ALIGN) * ALIGN)
        end = offsets[-1] + r * _words(h, w)
    return offsets


def _first(g):
    first = [0]
    for v in g:
        first.append(first[-1] + v)
    return first


def _call(sizes=((8, 70), (5, 3)), g=(2, 3), index=(0, 1), max_det=4, batch=None, thresholds=10, log_rows=64, det_off=None,
          gt_off=None, gt_sizes=None, gt_first=None, short=0, null=(), kinds=3, tables=True):
    lib = hip.lib()
    sizes = list(sizes)
    n = len(sizes)
    mem = torch.zeros(4096, dtype=torch.uint8)                      # a non-null pointer; a refused call never follows it
    p = ctypes.c_void_p(mem.data_ptr())
    det = hip.ragged_table(sizes, _layout(sizes, [max_det] * n) if det_off is None else det_off) if tables else None
    gtt = hip.ragged_table(sizes if gt_sizes is None else list(gt_sizes), _layout(sizes, g) if gt_off is None else gt_off) if tables else None
    first_c = (ctypes.c_int32 * (n + 1))(*(_first(g) if gt_first is None else gt_first))
    index_c = (ctypes.c_int64 * n)(*index)
    b = n if batch is None else batch
    ws = lib.ym_eval_coco_add_ragged_workspace_bytes(det, first_c, b, max_det, kinds)
    a = {k: (None if k in null else p) for k in POINTERS}
    rc = lib.ym_eval_coco_add_ragged_packed(
        a['ids'], a['scores'], a['boxes'], a['counts'], b, max_det, a['det_bits'], det, a['gt_class'], a['gt_crowd'], a['gt_area'],
        a['gt_xywh'], first_c, a['gt_bits'], gtt, index_c, a['thr'], thresholds, a['area_rng'], 5, 100, kinds, a['score'], a['cls'],
        a['rank'], a['flags'], log_rows, a['npig'], a['class_rows'], a['ws'], ws - short if short else max(ws, 1 << 20), None)
    return rc, lib.ym_last_error().decode(), ws


def test_the_two_symbols_are_exported_and_bound():
    lib = hip.lib()
    for name in ('ym_eval_coco_add_ragged_workspace_bytes', 'ym_eval_coco_add_ragged_packed'):
        assert name in hip.ABI_SYMBOLS
        assert not name.startswith('ym_coco_')                      # (tests/test_coco_eval_cpu.py pins that list)
        assert getattr(lib, name).argtypes is not None
    assert lib.ym_eval_coco_add_ragged_workspace_bytes.restype is ctypes.c_size_t
    assert lib.ym_eval_coco_add_ragged_packed.restype is ctypes.c_int


@pytest.mark.parametrize('kw, text', [
    (dict(sizes=[(4, 4)] * 33, g=[1] * 33, index=list(range(33)), log_rows=4096), 'images per call'),                  # B = 33
    (dict(batch=0), 'images per call'),
    (dict(max_det=0), 'max_det'),
    (dict(max_det=1025, log_rows=1 << 20), 'max_det'),
    (dict(thresholds=0), 'thresholds'),
    (dict(thresholds=17), 'thresholds'),
    (dict(kinds=0), 'kinds'),
    (dict(kinds=4), 'kinds'),
    (dict(g=(2, 513)), '513 gt annotations'),                                                                           # g_b = 513
    (dict(gt_first=[0, 3, 2]), 'not ascending'),
    (dict(gt_sizes=[(8, 70), (5, 4)]), 'gt masks of 5 x 4'),
    (dict(det_off=[0, ALIGN * 2 + 1]), 'not a multiple of 256 bytes'),                                                  # misaligned
    (dict(gt_off=[0, ALIGN + 3]), 'not a multiple of 256 bytes'),
    (dict(det_off=[0, 0]), 'overlap'),                                                                                  # overlapping
    (dict(gt_off=[ALIGN, ALIGN]), 'overlap'),
    (dict(sizes=[(1 << 20, 1024), (5, 3)]), '2^24 words'),
    (dict(index=(0, 16), log_rows=64), 'past the 64 rows of the log'),                                                  # past log_rows
    (dict(index=(3, 3)), 'twice'),                                                                                      # duplicate
    (dict(null=('ids',)), 'null pointer'),
    (dict(null=('rank',)), 'null pointer'),
    (dict(null=('gt_class',)), 'null pointer'),
    (dict(null=('ws',)), 'null pointer'),
    (dict(null=('boxes',)), 'bbox needs boxes_px'),                                                                     # an enabled kind
    (dict(null=('gt_xywh',)), 'bbox needs gt_xywh'),
    (dict(null=('det_bits',)), 'segm needs det_bits'),
    (dict(null=('gt_bits',)), 'segm needs gt_bits'),
    (dict(tables=False), 'segm needs det_bits and both tables'),
])
def test_refusals_happen_on_the_host_and_name_the_entry(kw, text):
    rc, msg, _ = _call(**kw)
    assert rc == EINVAL, msg
    assert msg.startswith(NAME) and text in msg, msg


def test_an_iou_type_that_is_off_needs_none_of_its_inputs():
    """The checks pass (padding only: nothing is launched, so the host buffer is never followed)."""
    rc, msg, ws = _call(index=(-1, -1), kinds=1, tables=False, null=('det_bits', 'gt_bits'))
    assert rc == 0 and ws > 0, msg
    rc, msg, ws = _call(index=(-1, -1), kinds=2, null=('gt_xywh', 'boxes'))
    assert rc == 0 and ws > 0, msg
    # ... and a live entry is still refused for what its own kind misses
    rc, msg, _ = _call(kinds=2, null=('gt_bits',))
    assert rc == EINVAL and 'segm needs gt_bits' in msg
    rc, msg, _ = _call(kinds=1, tables=False, null=('gt_xywh',))
    assert rc == EINVAL and 'bbox needs gt_xywh' in msg


def test_a_workspace_one_byte_short_is_enospc_and_padding_alone_launches_nothing():
    rc, msg, ws = _call(short=1)
    assert ws > 0 and rc == ENOSPC and msg.startswith(NAME) and 'workspace' in msg
    # (two padding entries both carry -1: no duplicate, nothing past the log, and a call of padding alone launches nothing)
    rc, msg, _ = _call(index=(-1, -1), log_rows=0)
    assert rc == 0, msg


def test_workspace_is_a_host_function_that_grows_with_batch_gt_and_chunks():
    lib = hip.lib()

    def ws(sizes, g, max_det=100, kinds=3):
        first = _first(g)
        return lib.ym_eval_coco_add_ragged_workspace_bytes(hip.ragged_table(sizes, _layout(sizes, [max_det] * len(sizes))),
                                                           (ctypes.c_int32 * len(first))(*first), len(sizes), max_det, kinds)

    one = ws([(48, 64)], [7])
    # two fp64 IoU matrices and the box areas; 48 words = 3 chunks of partials and the mask areas
    assert one >= (2 * 100 * 7 + 100) * 8 + (3 * (100 * 7 + 107) + 100) * 4
    assert ws([(48, 64)] * 2, [7, 7]) > one                           # B
    assert ws([(48, 64)], [8]) > one                                  # g
    assert ws([(49, 64)], [7]) == one and ws([(61, 64)], [7]) > one   # words: 49 rows are still 3 chunks of 20, 61 are 4
    assert ws([(48, 65)], [7]) > one                                  # (a 65th column is a second word per row)
    assert ws([(48, 64)], [7], kinds=1) < one and ws([(48, 64)], [7], kinds=2) < one
    assert ws([(48, 64)], [513]) == 0 and ws([(1 << 20, 1024)], [1]) == 0 and ws([(48, 64)], [7], max_det=1025) == 0
    assert ws([(48, 64)], [7], kinds=0) == 0 and ws([(48, 64)], [7], kinds=4) == 0
    # without segm the sizes are not looked at
    first = (ctypes.c_int32 * 2)(0, 7)
    assert lib.ym_eval_coco_add_ragged_workspace_bytes(None, first, 1, 100, 1) == ws([(48, 64)], [7], kinds=1)
    assert lib.ym_eval_coco_add_ragged_workspace_bytes(None, first, 1, 100, 3) == 0


def test_an_image_without_ground_truth_keeps_room_for_its_area_partials():
    lib = hip.lib()

    def ws(words_h, kinds):
        return lib.ym_eval_coco_add_ragged_workspace_bytes(hip.ragged_table([(words_h, 64)], [0]), (ctypes.c_int32 * 2)(0, 0), 1, 100, kinds)

    # segm on: chunks x max_det area partials and max_det mask areas; bbox on: max_det box areas
    assert ws(48, 2) >= (3 * 100 + 100) * 4 and ws(61, 2) - ws(48, 2) == 100 * 4
    assert ws(48, 1) >= 100 * 8 and ws(61, 1) == ws(48, 1)
    assert ws(48, 3) >= 100 * 8 + (3 * 100 + 100) * 4


def test_evaluate_coco_pipelined_refuses_dense_masks_before_anything_runs():
    from yolact_minimal_amd.evaluate import evaluate_coco_pipelined

    def samples():
        raise AssertionError('the samples were read')
        yield

    with pytest.raises(RuntimeError, match='packed'):
        evaluate_coco_pipelined(torch.nn.Linear(1, 1), None, samples(), None, [], batch=4, packed_masks=False, batched_metrics=True)
    with pytest.raises(RuntimeError, match='packed'):
        evaluate_coco_pipelined(torch.nn.Linear(1, 1), None, samples(), None, [], packed_masks=False, batched_metrics=True)
