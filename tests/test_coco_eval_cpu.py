"""No GPU: hand-derived known answers for the COCO-protocol restatement (`tests/coco_eval_ref.py`), and the host-only parts of
`yolact_minimal_amd/utils/coco_eval.py` (summary, annotation records, ABI constants and symbols).

Notation of the derivations: e = np.spacing(1); a cell of `precision` is the 101 samples q[r] = envelope(pr)[first i with rc[i] >=
recThrs[r]] (0 when there is none), pr = tp / (fp + tp + e), rc = tp / npig; 51 of the recThrs are <= .5 (0, .01, ..., .5) and 50
are above.  1 / (1 + e) is not 1, hence the 1e-12 comparisons.  All scenes use integer rectangles whose masks are the filled boxes,
so `bbox` and `segm` have the same answers."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import coco_eval_ref as R
from tests.conftest import REPO

E = np.spacing(1)
ONE = 1 / (1 + E)
TOL = 1e-12
KINDS = ('bbox', 'segm')
SCENES = R.known_answer_scenes()


def _run(name):
    scene, nc = SCENES[name]
    return R.evaluate_scene(scene, nc)


def _close(got, want):
    assert np.allclose(np.asarray(got, float), np.asarray(want, float), rtol=0, atol=TOL), (got, want)


@pytest.mark.parametrize('kind', KINDS)
def test_A_hit_miss_hit(kind):
    """2 gts (area 2500: medium), detections .9 hit, .8 miss, .7 hit at every threshold (IoU 1): tp = 1 1 2, fp = 0 1 1, npig = 2,
    rc = .5 .5 1, pr = 1/(1+e), 1/(2+e), 2/(3+e), envelope = 1/(1+e), 2/(3+e), 2/(3+e).  recThrs <= .5 -> index 0, above -> index 2:
    AP = (51 / (1+e) + 50 * 2/(3+e)) / 101 = .83498...  maxDets = 1 keeps the .9 row only: recall .5; 10 and 100: recall 1."""
    ev = _run('A')[kind]
    prec, rec = ev.eval['precision'], ev.eval['recall']
    for t in range(10):
        _close(prec[t, :51, 0, 0, 2], [ONE] * 51)
        _close(prec[t, 51:, 0, 0, 2], [2 / (3 + E)] * 50)
    ap = (51 * ONE + 50 * 2 / (3 + E)) / 101
    stats, text = ev.summarize()
    _close(stats, [ap, ap, ap, -1, ap, -1, .5, 1, 1, -1, 1, -1])
    assert abs(ap - .835) < 5e-4
    assert text.split('\n')[0] == ' Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 0.835'
    assert text.split('\n')[6] == ' Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ] = 0.500'
    assert text.split('\n')[3] == ' Average Precision  (AP) @[ IoU=0.50:0.95 | area= small | maxDets=100 ] = -1.000'
    _close(rec[:, 0, 0, :], [[.5, 1, 1]] * 10)


@pytest.mark.parametrize('kind', KINDS)
def test_B_two_detections_inside_one_crowd(kind):
    """A regular gt (hit by the .9 row) and a crowd region [100, 0, 100, 100]; the .8 and .7 rows lie inside the crowd: IoU with a
    crowd is i / |d| = 1.  Both match the SAME crowd gt (a crowd is not used up) and inherit its ignore flag, so the only counted
    row is the true positive: npig = 1, tp = 1, fp = 0 -> every sample 1/(1+e), AP ~ 1."""
    ev = _run('B')[kind]
    crowd_id = 2                                              # the second annotation
    img = [e for e in ev.evalImgs if e is not None and e['aRng'] == ev.params.areaRng[0]][0]
    assert img['dtMatches'][:, 1].tolist() == [crowd_id] * 10 and img['dtMatches'][:, 2].tolist() == [crowd_id] * 10
    assert img['dtIgnore'][:, 1:].all() and not img['dtIgnore'][:, 0].any()
    _close(ev.eval['precision'][:, :, 0, 0, 2], np.full((10, 101), ONE))
    _close(ev.summarize()[0][:3], [ONE] * 3)


@pytest.mark.parametrize('kind', KINDS)
def test_C_the_stop_rule(kind):
    """Detection (0,0)-(60,10), 600 px; regular gt [0,0,100,10]: i = 600, u = 1000, IoU .6; crowd [6,0,200,10]: i = 540, IoU =
    540/600 = .9.  The gts are walked regular first.  t <= .6: the regular gt is taken (IoU >= t), then the crowd is an ignored gt
    behind a regular match: STOP -> true positive.  t = .65 .. .9 (iouThrs[8] = .8999999999999999 <= .9): the regular gt fails,
    the crowd matches -> ignored, not a false positive.  t = .95: nothing matches and the area 600 lies inside `all` and `small`:
    a false positive there.  npig = 1 (the crowd never counts): AP cells are 1/(1+e) for the first three thresholds and 0 after."""
    ev = _run('C')[kind]
    img = [e for e in ev.evalImgs if e is not None and e['aRng'] == ev.params.areaRng[0]][0]
    assert img['dtMatches'][:, 0].tolist() == [1, 1, 1, 2, 2, 2, 2, 2, 2, 0]
    assert img['dtIgnore'][:, 0].tolist() == [False] * 3 + [True] * 6 + [False]
    _close(ev.eval['precision'][:, 0, 0, 0, 2], [ONE] * 3 + [0] * 7)
    _close(ev.eval['recall'][:, 0, 0, 2], [1] * 3 + [0] * 7)
    _close(ev.summarize()[0][:3], [3 * ONE / 10, ONE, 0])


@pytest.mark.parametrize('kind', KINDS)
def test_D_iou_exactly_at_the_threshold(kind):
    """gt [0,0,10,10] vs detection (0,0)-(10,5): i = 50, u = 100, IoU exactly .5 = iouThrs[0]: `iou < min(t, 1 - 1e-10)` is false at
    .5 (a match) and true from .55 up."""
    ev = _run('D')[kind]
    img = [e for e in ev.evalImgs if e is not None and e['aRng'] == ev.params.areaRng[0]][0]
    assert img['dtMatches'][:, 0].tolist() == [1] + [0] * 9
    _close(ev.summarize()[0][:3], [ONE / 10, ONE, 0])


@pytest.mark.parametrize('kind', KINDS)
def test_E_area_ranges(kind):
    """gt of area exactly 1024 = 32^2: inside `small` [0, 1024] AND `medium` [1024, 9216] (both ends inclusive), outside `large`.
    Detections: .95 unmatched, 20 x 20 = 400 px; .9 the gt's box.  all / small: the 400 px row is a false positive ahead of the hit:
    tp = 0 1, fp = 1 1, pr = 0, 1/(2+e) -> envelope 1/(2+e) everywhere, rc = 0 1: AP = 1/(2+e) = .5.  medium: the 400 px row is
    ignored (unmatched, area outside): AP = 1/(1+e).  large: the gt is ignored, npig = 0: -1.  maxDets = 1 keeps the .95 row only:
    AR@1 = 0."""
    ev = _run('E')[kind]
    half = 1 / (2 + E)
    _close(ev.summarize()[0], [half, half, half, half, ONE, -1, 0, 1, 1, 1, 1, -1])
    by_rng = {tuple(e['aRng']): e for e in ev.evalImgs if e is not None}
    rng = ev.params.areaRng
    assert not by_rng[tuple(rng[0])]['dtIgnore'][:, 0].any() and not by_rng[tuple(rng[1])]['dtIgnore'][:, 0].any()
    assert by_rng[tuple(rng[2])]['dtIgnore'][:, 0].all() and by_rng[tuple(rng[3])]['dtIgnore'][:, 0].all()
    assert by_rng[tuple(rng[1])]['gtIgnore'].tolist() == [0] and by_rng[tuple(rng[2])]['gtIgnore'].tolist() == [0]
    assert by_rng[tuple(rng[3])]['gtIgnore'].tolist() == [1]


@pytest.mark.parametrize('kind', KINDS)
def test_F_max_dets(kind):
    """12 gts, 12 detections of one class in one image, row i hits gt i (IoU 1), scores descending: the rows of rank < maxDet are
    all hits: AR@1 = 1/12, AR@10 = 10/12, AR@100 = 12/12; AP (maxDets 100) ~ 1."""
    stats = _run('F')[kind].summarize()[0]
    _close(stats[6:9], [1 / 12, 10 / 12, 1])
    assert stats[6] < stats[7] < stats[8]
    _close(stats[0], ONE)


@pytest.mark.parametrize('kind', KINDS)
def test_G_equal_scores_across_images_keep_image_order(kind):
    """Two images, one gt each, one detection of score .5 each: image 0's misses, image 1's hits.  The mergesort keeps image 0's row
    first: tp = 0 1, fp = 1 1, npig = 2, rc = 0 .5, pr = 0, 1/(2+e) -> envelope 1/(2+e); recThrs <= .5 -> 1/(2+e), above -> none -> 0:
    AP = 51 / (2+e) / 101 = .2525.  (The other order would give 51 / (1+e) / 101 = .505.)"""
    stats = _run('G')[kind].summarize()[0]
    _close(stats[0], 51 / (2 + E) / 101)
    _close(stats[8], .5)


@pytest.mark.parametrize('kind', KINDS)
def test_H_an_image_without_detections_lowers_recall(kind):
    """Image 0: a gt and its hit; image 1: a gt and no detection.  npig = 2: rc = .5, pr = 1/(1+e): recThrs <= .5 -> 1/(1+e), above ->
    0: AP = 51 / (1+e) / 101 = .505, AR = .5.  Without image 1 both would be 1."""
    stats = _run('H')[kind].summarize()[0]
    _close(stats[0], 51 * ONE / 101)
    _close(stats[6:9], [.5, .5, .5])


def test_random_sequence_holds_every_situation():
    for what, there in R.random_sequence_situations(R.random_sequence()).items():
        assert there, what


# ---- the package's host-only parts ----------------------------------------------------------------------------------------------
def test_package_summarize_equals_the_restatement():
    from yolact_minimal_amd.utils.coco_eval import CocoParams, summarize_grids
    p, q = CocoParams(), R.Params()
    assert np.array_equal(p.iouThrs, q.iouThrs) and np.array_equal(p.recThrs, q.recThrs) and p.maxDets == q.maxDets
    assert p.areaRng == q.areaRng and p.areaRngLbl == q.areaRngLbl and p.eps == np.spacing(1)
    assert np.array_equal(p.recThrs, np.linspace(0, 1, 101)) and np.array_equal(p.iouThrs, np.linspace(.5, .95, 10))
    runs = [_run(name) for name in 'ACE'] + [R.evaluate_scene(R.random_sequence(), R.RANDOM_CLASSES)]
    for evs in runs:
        for kind in KINDS:
            want_stats, want_text = evs[kind].summarize()
            stats, text = summarize_grids(evs[kind].eval['precision'], evs[kind].eval['recall'])
            assert np.array_equal(stats, want_stats) and text == want_text


def test_coco_gt_records():
    from yolact_minimal_amd.utils.coco import COCO
    from yolact_minimal_amd.utils.coco_eval import coco_gt_records
    coco = COCO()
    coco.dataset = {
        'images': [{'id': 7, 'height': 20, 'width': 30}, {'id': 9, 'height': 20, 'width': 30}],
        'categories': [{'id': 3}, {'id': 18}, {'id': 44}],
        'annotations': [
            {'id': 1, 'image_id': 7, 'category_id': 18, 'bbox': [1, 2.5, 10, 4], 'area': 33.5, 'iscrowd': 0, 'segmentation': [[1, 2, 11, 2, 11, 6]]},
            {'id': 2, 'image_id': 9, 'category_id': 3, 'bbox': [0, 0, 5, 5], 'area': 25, 'iscrowd': 0, 'segmentation': [[0, 0, 5, 0, 5, 5]]},
            {'id': 3, 'image_id': 7, 'category_id': 3, 'bbox': [0, 0, 30, 20], 'area': 600, 'iscrowd': 1,
             'segmentation': {'size': [20, 30], 'counts': [0, 600]}},
            {'id': 4, 'image_id': 7, 'category_id': 44, 'bbox': [0, 0, 2, 2], 'area': 4, 'iscrowd': 0, 'segmentation': [[0, 0, 2, 0, 2, 2]]}]}
    coco.createIndex()
    label_map = {3: 1, 18: 2}                                  # 44 is no evaluated category
    rec = coco_gt_records(coco, 7, label_map)
    assert [(r['cls'], r['iscrowd'], r['area'], r['bbox']) for r in rec] == [(1, 0, 33.5, [1.0, 2.5, 10.0, 4.0]), (0, 1, 600.0, [0.0, 0.0, 30.0, 20.0])]
    assert rec[1]['segmentation'] == {'size': [20, 30], 'counts': [0, 600]} and all(isinstance(v, float) for v in rec[0]['bbox'])
    assert coco_gt_records(coco, 11, label_map) == []


def test_constants_match_the_header():
    from yolact_minimal_amd import hip
    text = open(os.path.join(REPO, 'include', 'yolact_hip.h')).read()
    macro = lambda name: int(re.search(rf'#define {name} (\d+)', text).group(1))     # noqa: E731
    assert (macro('YM_COCO_MAX_GT'), macro('YM_COCO_AREAS'), macro('YM_COCO_WORDS_PER_ROW'), macro('YM_COCO_ROWS_PER_PASS')) == \
        (hip.COCO_MAX_GT, hip.COCO_AREAS, hip.COCO_WORDS_PER_ROW, hip.COCO_ROWS_PER_PASS)
    assert hip.COCO_WORDS_PER_ROW == 2 * hip.COCO_AREAS


def test_library_exports_the_coco_symbols():
    from yolact_minimal_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(hip.LIB_PATH)
    names = [n for n in hip.ABI_SYMBOLS if n.startswith('ym_coco_')]
    assert sorted(names) == ['ym_coco_accumulate', 'ym_coco_accumulate_workspace_bytes', 'ym_coco_iou_box', 'ym_coco_iou_mask_packed',
                             'ym_coco_match_log']
    for name in names:
        assert hasattr(lib, name), name
