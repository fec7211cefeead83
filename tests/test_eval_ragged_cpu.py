"""The batched metric stage without a GPU: `ym_eval_add_ragged_packed` / `ym_pack_masks_ragged` are exported and bound, refuse bad
arguments on the host before any HIP call (a 4 KB host buffer stands for every device pointer: a refused call never follows it), and
the workspace query is a host function of the sizes."""
import ctypes

import pytest
import torch

from yolact_minimal_amd import hip

EINVAL, ENOSPC = -1, -2           # YM_EINVAL, YM_ENOSPC
ALIGN = hip.RAGGED_ALIGN_BYTES // 8


def _words(h, w):
    return h * ((w + 63) // 64)


def _layout(sizes, rows):
    """Blocks of rows[b] x h x ceil(w / 64) words, each at the next multiple of 256 bytes (any number of images)."""
    offsets, end = [], 0
    for (h, w), r in zip(sizes, rows):
        offsets.append(-(-end // ALIGN) * ALIGN)
        end = offsets[-1] + r * _words(h, w)
    return offsets


def _call(sizes=((8, 70), (5, 3)), g=(2, 3), index=(0, 1), max_det=4, batch=None, thresholds=10, log_rows=64, det_off=None,
          gt_off=None, gt_sizes=None, gt_first=None, short=0, null=()):
    lib = hip.lib()
    sizes = list(sizes)
    n = len(sizes)
    mem = torch.zeros(4096, dtype=torch.uint8)                      # a non-null pointer; a refused call never follows it
    p = ctypes.c_void_p(mem.data_ptr())
    det = hip.ragged_table(sizes, _layout(sizes, [max_det] * n) if det_off is None else det_off)
    gtt = hip.ragged_table(sizes if gt_sizes is None else list(gt_sizes), _layout(sizes, g) if gt_off is None else gt_off)
    first = [0]
    for v in g:
        first.append(first[-1] + v)
    first_c = (ctypes.c_int32 * (n + 1))(*(first if gt_first is None else gt_first))
    index_c = (ctypes.c_int64 * n)(*index)
    b = n if batch is None else batch
    ws = lib.ym_eval_add_ragged_workspace_bytes(det, first_c, b, max_det)
    a = {k: p for k in ('ids', 'scores', 'boxes', 'counts', 'det_bits', 'gt', 'gt_bits', 'thr', 'score', 'cls', 'flags', 'gt_count',
                        'class_rows', 'ws')}
    for k in null:
        a[k] = None
    rc = lib.ym_eval_add_ragged_packed(a['ids'], a['scores'], a['boxes'], a['counts'], b, max_det, a['det_bits'], det, a['gt'], first_c,
                                       a['gt_bits'], gtt, index_c, a['thr'], thresholds, 5, a['score'], a['cls'], a['flags'], log_rows,
                                       a['gt_count'], a['class_rows'], a['ws'], ws - short if short else max(ws, 1 << 20), None)
    return rc, lib.ym_last_error().decode(), ws


def test_the_three_symbols_are_exported_and_bound():
    lib = hip.lib()
    for name in ('ym_eval_add_ragged_workspace_bytes', 'ym_eval_add_ragged_packed', 'ym_pack_masks_ragged'):
        assert name in hip.ABI_SYMBOLS
        assert getattr(lib, name).argtypes is not None
    assert lib.ym_eval_add_ragged_workspace_bytes.restype is ctypes.c_size_t


@pytest.mark.parametrize('kw, text', [
    (dict(sizes=[(4, 4)] * 33, g=[1] * 33, index=list(range(33)), log_rows=4096), 'images per call'),                  # B = 33
    (dict(batch=0), 'images per call'),
    (dict(max_det=0), 'max_det'),
    (dict(max_det=1025, log_rows=1 << 20), 'max_det'),
    (dict(thresholds=0), 'thresholds'),
    (dict(thresholds=17), 'thresholds'),
    (dict(g=(2, 513)), '513 gt instances'),                                                                             # g_b = 513
    (dict(gt_first=[0, 3, 2]), 'not ascending'),
    (dict(gt_sizes=[(8, 70), (5, 4)]), 'gt masks of 5 x 4'),
    (dict(det_off=[0, ALIGN * 2 + 1]), 'not a multiple of 256 bytes'),                                                  # misaligned
    (dict(gt_off=[0, ALIGN + 3]), 'not a multiple of 256 bytes'),
    (dict(det_off=[0, 0]), 'overlap'),                                                                                  # overlapping
    (dict(gt_off=[ALIGN, ALIGN]), 'overlap'),
    (dict(sizes=[(4096, 4096), (5, 3)]), '2^18 words'),
    (dict(index=(0, 16), log_rows=64), 'past the 64 rows of the log'),                                                  # past log_rows
    (dict(index=(3, 3)), 'twice'),                                                                                      # duplicate
    (dict(null=('ids',)), 'null pointer'),
    (dict(null=('gt_bits',)), 'null pointer'),
    (dict(null=('ws',)), 'null pointer'),
])
def test_refusals_happen_on_the_host_and_name_the_entry(kw, text):
    rc, msg, _ = _call(**kw)
    assert rc == EINVAL, msg
    assert msg.startswith('eval_add_ragged_packed:') and text in msg, msg


def test_a_workspace_one_byte_short_is_enospc_and_padding_may_repeat_its_index():
    rc, msg, ws = _call(short=1)
    assert ws > 0 and rc == ENOSPC and msg.startswith('eval_add_ragged_packed:') and 'workspace' in msg
    # (two padding entries both carry -1: no duplicate, nothing past the log, and a call of padding alone launches nothing)
    rc, msg, _ = _call(index=(-1, -1), log_rows=0)
    assert rc == 0, msg


def test_workspace_is_a_host_function_that_grows_with_batch_gt_and_words():
    lib = hip.lib()

    def ws(sizes, g, max_det=100):
        first = [0]
        for v in g:
            first.append(first[-1] + v)
        return lib.ym_eval_add_ragged_workspace_bytes(hip.ragged_table(sizes, _layout(sizes, [max_det] * len(sizes))),
                                                      (ctypes.c_int32 * len(first))(*first), len(sizes), max_det)

    one = ws([(48, 64)], [7])
    assert one >= (3 * (100 * 7 + 107) + 2 * 100 * 7) * 4            # 48 words = 3 chunks of partials, then two IoU matrices
    assert ws([(48, 64)] * 2, [7, 7]) > one                           # B
    assert ws([(48, 64)], [8]) > one                                  # g
    assert ws([(49, 64)], [7]) == one and ws([(61, 64)], [7]) > one   # words: 49 rows are still 3 chunks of 20, 61 are 4
    assert ws([(48, 65)], [7]) > one                                  # (a 65th column is a second word per row)
    assert ws([(48, 64)], [0]) == 256                                 # no ground truth: no pair
    assert ws([(48, 64)], [513]) == 0 and ws([(4096, 4096)], [1]) == 0 and ws([(48, 64)], [7], max_det=1025) == 0


def _pack_call(sizes, rows, offsets=None, batch=None, null_src=None):
    lib = hip.lib()
    mem = torch.zeros(4096, dtype=torch.uint8)
    n = len(sizes)
    src = (ctypes.c_void_p * n)(*[None if b == null_src else mem.data_ptr() for b in range(n)])
    table = hip.ragged_table(sizes, _layout(sizes, rows) if offsets is None else offsets)
    rc = lib.ym_pack_masks_ragged(src, 1, (ctypes.c_int32 * n)(*rows), table, n if batch is None else batch,
                                  ctypes.c_void_p(mem.data_ptr()), None)
    return rc, lib.ym_last_error().decode()


@pytest.mark.parametrize('kw, text', [
    (dict(sizes=[(4, 4)] * 33, rows=[1] * 33), 'images per call'),
    (dict(sizes=[(8, 70), (5, 3)], rows=[2, 3], offsets=[0, 5]), 'not a multiple of 256 bytes'),
    (dict(sizes=[(8, 70), (5, 3)], rows=[2, 3], offsets=[0, 0]), 'overlap'),
    (dict(sizes=[(8, 70), (5, 3)], rows=[2, -1]), 'rows'),
    (dict(sizes=[(8, 70), (5, 3)], rows=[2, 3], null_src=1), 'rows'),
    (dict(sizes=[(8, 70), (0, 3)], rows=[2, 3], offsets=[0, ALIGN]), 'image 1 is 0 x 3'),
])
def test_pack_masks_ragged_refuses_on_the_host(kw, text):
    rc, msg = _pack_call(**kw)
    assert rc == EINVAL, msg
    assert msg.startswith('pack_masks_ragged:') and text in msg, msg


def test_pack_masks_ragged_without_rows_launches_nothing():
    rc, msg = _pack_call([(8, 70), (5, 3)], [0, 0], offsets=[0, 0])
    assert rc == 0, msg


def test_evaluate_pipelined_refuses_dense_masks_before_anything_runs():
    from yolact_minimal_amd.evaluate import evaluate_pipelined

    def samples():
        raise AssertionError('the samples were read')
        yield

    with pytest.raises(RuntimeError, match='packed'):
        evaluate_pipelined(torch.nn.Linear(1, 1), None, samples(), batch=4, packed_masks=False, batched_metrics=True)
