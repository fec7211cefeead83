"""CPU: the host model of the device-resident mAP accumulator (tests/device_metrics_ref.py) against the oracle
(oracle/metrics_ref.py) and the reference goldens, and the properties of the six-image sequence the GPU tests rely on."""
import os
import re

import numpy as np

from oracle import metrics_ref as M
from tests import device_metrics_ref as R
from tests.conftest import REPO

GOLD = np.load(os.path.join(REPO, 'tests', 'golden', 'metrics.npz'))
T = len(R.THRES)


def test_constants_match_the_header():
    from yolact_minimal_amd import hip
    text = open(os.path.join(REPO, 'include', 'yolact_hip.h')).read()
    for name in ('EVAL_MAX_DET', 'EVAL_MAX_THRESHOLDS', 'EVAL_AP_ROWS_PER_PASS'):
        assert int(re.search(rf'#define YM_{name} (\d+)', text).group(1)) == getattr(hip, name), name
    assert 2 * hip.EVAL_MAX_THRESHOLDS <= 32


def test_model_reproduces_the_reference_goldens():
    for case, shape in enumerate([(40, 7, 48, 64, 6), (100, 15, 120, 160, 10), (9, 3, 33, 47, 4)]):
        assert tuple(int(v) for v in GOLD[f'c{case}_shape']) == shape
        images, nc = R.golden_images(GOLD, case)
        log = R.oracle_log(images, nc, max_det=128)
        assert np.array_equal(R.log_grid_rows(*log, nc), GOLD[f'c{case}_ap_grid'])
        assert np.array_equal(R.log_grid_rows(*log, nc, cell=lambda b, g: R.ap_cell_passes(b, g, 16)), GOLD[f'c{case}_ap_grid'])
        assert np.array_equal(R.grid_rows(R.oracle_accumulate(images, nc), nc), GOLD[f'c{case}_ap_grid'])


def _sequence():
    images = R.sequence_images()
    nc = R.SEQUENCE_CLASSES
    return images, nc, R.oracle_accumulate(images, nc), R.oracle_log(images, nc, max_det=16)


def test_sequence_model_equals_oracle_and_ties_decide():
    images, nc, ref, log = _sequence()
    score, cls, flags, gt_count = log
    assert int((cls >= 0).sum()) == 53
    for s in score[cls >= 0]:
        assert float(np.float32(s)) == float(s) and (float(s) * 16) % 2 == 1          # k/8 + 1/16: exact in fp32
    ap, empty = R.ap_grid(score, cls, flags, gt_count, T, nc)
    for cell in (R.ap_cell, lambda b, g: R.ap_cell_passes(b, g, 4)):
        got, _ = R.ap_grid(score, cls, flags, gt_count, T, nc, cell)
        for b in range(2 * T):
            for c in range(nc):
                assert got[b // T, b % T, c] == ref['box' if b < T else 'mask'][b % T][c].get_ap(), (b, c)
    assert not empty.any()
    # points that share their score with another point of their class: none in class 0 (3 points), 5 / 7 / 18 / 8 in the others, and
    # in each of those a tie run spans several images -- the stable order across images is what decides
    tied_per_class, repeats_per_class = [], []
    for c in range(nc):
        mine = np.nonzero(cls == c)[0]
        vals, counts = np.unique(score[mine], return_counts=True)
        tied_per_class.append(int(counts[counts > 1].sum()))
        repeats_per_class.append(len(mine) - len(vals))
        assert c == 0 or any(len({i // 16 for i in mine[score[mine] == v]}) > 1 for v in vals), c
    assert tied_per_class == [0, 5, 7, 18, 8]
    # the "3 to 12 tied scores per class" of the sequence's description counts the points whose score repeats an earlier point's of
    # their class (points minus distinct scores): 3 to 12 in the four classes that have ties
    assert repeats_per_class == [0, 3, 4, 12, 5]
    # ... ties taken in reverse push order give another AP in 59 of the 100 cells
    rev, _ = R.ap_grid(score[::-1], cls[::-1], flags[::-1], gt_count, T, nc)
    assert int((rev != ap).sum()) == 59
    m = M.calc_map(ref, R.THRES, nc)
    assert abs(m['box'][0] - 7.2617) < 1e-4 and abs(m['mask'][0] - 10.6439) < 1e-4


def test_model_edge_cells():
    # gt and no points: 0.0, not empty; points and no gt: the reference returns the int 0 and the class is not empty
    score, cls = np.array([0.5, 0.25], np.float32), np.array([1, 1], np.int32)
    flags, gt_count = np.array([1, 0], np.uint32), np.array([3, 0, 0], np.int64)
    ap, empty = R.ap_grid(score, cls, flags, gt_count, 1, 3)
    assert ap[0, 0, 0] == 0.0 and ap[0, 0, 1] == 0.0 and empty.tolist() == [False, False, True]
    a = M.APData()
    a.data_points = [(0.5, True), (0.25, False)]
    assert a.get_ap() == 0 and isinstance(a.get_ap(), int) and not a.is_empty()
    # recall never reaches 1.0: 2 of 4 gt found -> grid values above 0.5 sample 0
    for bits, num_gt in (([1, 0, 1], 4), ([1], 1), ([0], 2), ([1], 3), ([0, 0, 1, 1, 0, 1, 0], 3), ([1] * 7 + [0] * 6, 9)):
        a = M.APData()
        a.num_gt_positives = num_gt
        a.data_points = [(1.0 - 0.01 * i, bool(b)) for i, b in enumerate(bits)]
        want = a.get_ap()
        assert R.ap_cell(bits, num_gt) == want
        for rpp in (1, 2, 3, 64):
            assert R.ap_cell_passes(bits, num_gt, rpp) == want, (bits, num_gt, rpp)
    # ... by hand: precision 1, 1/2, 2/3 -> envelope 1, 2/3, 2/3; recall 1/4, 1/4, 2/4 -> grid values 0 .. 0.25 sample 1.0,
    # 0.26 .. 0.50 sample 2/3, the other 50 sample 0; summed left to right
    by_hand = 0.0
    for k in range(101):
        by_hand += 1.0 if k <= 25 else 2 / 3 if k <= 50 else 0.0
    assert R.ap_cell([1, 0, 1], 4) == by_hand / 101


def test_pass_walk_equals_the_whole_class_walk():
    rng = np.random.default_rng(5)
    for trial in range(60):
        n = int(rng.integers(1, 400))
        bits = (rng.random(n) < rng.random()).astype(np.int64)
        num_gt = int(bits.sum()) + int(rng.integers(0, 50)) + (trial % 2)
        a = M.APData()
        a.num_gt_positives = num_gt
        a.data_points = [(0.0, bool(b)) for b in bits]              # (equal scores: the stable sort keeps the order)
        want = a.get_ap()
        assert R.ap_cell(bits, num_gt) == want
        assert R.ap_cell_passes(bits, num_gt, int(rng.integers(1, 70))) == want


def test_calc_map_shares_its_arithmetic():
    """`common_utils.calc_map` is `map_table` over the host cells; the rows still equal the goldens'."""
    from yolact_minimal_amd.utils import common_utils as C
    images, nc = R.golden_images(GOLD, 0)
    ref = R.oracle_accumulate(images, nc)
    ap = {k: [[C.APDataObject() for _ in range(nc)] for _ in R.THRES] for k in ('box', 'mask')}
    for kind in ap:
        for k in range(T):
            for c in range(nc):
                ap[kind][k][c].data_points = list(ref[kind][k][c].data_points)
                ap[kind][k][c].num_gt_positives = ref[kind][k][c].num_gt_positives
    text, row2, row3 = C.calc_map(ap, R.THRES, nc, step=0)
    assert row2[1:] == [round(v, 2) for v in GOLD['c0_map_box']] and row3[1:] == [round(v, 2) for v in GOLD['c0_map_mask']]
    cells = lambda kind, k, c: None if ap[kind][k][c].is_empty() else ap[kind][k][c].get_ap()       # noqa: E731
    assert C.map_table(cells, R.THRES, nc, 0) == (text, row2, row3)
    assert C.DeviceAPData.__module__ == 'yolact_minimal_amd.utils.device_metrics'
