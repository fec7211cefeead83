"""The device renderer's contract, as far as it can be checked without a GPU: the three arithmetic identities behind "exact", the font
table, hand-derived known answers (also replayed on the device by tests/test_gpu_draw.py) and the numpy oracle against them."""
import os
import re

import numpy as np
import pytest

from tests import draw_ref as R
from tests.conftest import REPO
from yolact_minimal_amd import hip
from yolact_minimal_amd.config import COLORS, COCO_CLASSES, CUSTOM_CLASSES
from yolact_minimal_amd.utils import draw, font  # noqa: F401  (the module under test must import without a GPU)


# ---- arithmetic identities -------------------------------------------------------------------------------------------------
def test_blend_is_addweighted_for_all_pairs():
    """(4c + 6v + 5) // 10 == round(0.4 c + 0.6 v) in float32, in float64 and with a single rounding: 0.4 c + 0.6 v = (2c + 3v) / 5
    never ends in .5, so neither the rounding mode nor the float type matters."""
    c, v = np.meshgrid(np.arange(256), np.arange(256), indexing='ij')
    want = (4 * c + 6 * v + 5) // 10
    f32 = np.float32(0.4) * c.astype(np.float32) + np.float32(0.6) * v.astype(np.float32)
    f64 = 0.4 * c.astype(np.float64) + 0.6 * v.astype(np.float64)
    exact = (2 * c + 3 * v) / 5.0                                   # one rounding
    assert not np.any((2 * c + 3 * v) % 5 * 2 == 5)                 # no fractional part of one half (trivially: 5 is odd)
    for name, x in (('float32', f32), ('float64', f64), ('single rounding', exact)):
        assert np.array_equal(np.rint(x).astype(np.int64), want), name
        assert np.array_equal(np.floor(x.astype(np.float64) + 0.5).astype(np.int64), want), name + ' (half up)'


def test_shadow_is_float32_times_06_for_all_values():
    v = np.arange(256)
    assert np.array_equal((v.astype(np.float32) * np.float32(0.6)).astype(np.uint8), (3 * v) // 5)
    assert np.array_equal((v.astype(np.float32) * 0.6).astype(np.uint8), (3 * v) // 5)      # numpy promotes the python scalar weakly or not


TIES = (0.125, 0.375, 0.625, 0.875, 0.005, 0.015, 0.025, 0.995, 0.9999, 1.0, 0.0, 0.5, 0.045, 0.055, 0.105, 0.115)


def test_score_text_is_pythons_format():
    rng = np.random.default_rng(7)
    sample = np.concatenate([rng.random(20000).astype(np.float32), (np.arange(1001) / 1000).astype(np.float32),
                             np.array(TIES, dtype=np.float32), np.array([-0.001, -0.125, 1.5, 12.345, 99.995], dtype=np.float32)])
    for v in sample:
        assert R.score_text(v) == f'{np.float32(v):.2f}', float(v)
    assert R.score_text(np.float32(0.125)) == '0.12' and R.score_text(np.float32(0.375)) == '0.38'
    assert R.score_text(np.float32('nan')) == 'nan' and R.score_text(np.float32('-inf')) == '-inf'


# ---- font ------------------------------------------------------------------------------------------------------------------
def test_font_table():
    assert font.FONT.shape == (95, font.HEIGHT) and font.FONT.dtype == np.uint16
    assert not font.FONT[0].any()                                   # 0x20 is empty
    for code in range(0x21, 0x7F):
        rows = font.FONT[code - 0x20]
        assert rows.any(), hex(code)
        assert not np.any(rows >> font.ADVANCE), hex(code)          # nothing outside the cell
    assert len({font.FONT[c - 0x20].tobytes() for c in range(0x20, 0x7F)}) == 95     # all glyphs differ
    assert font.sanitize('aé\tb\x7f') == 'a??b?'
    assert abs(font.HEIGHT - 13) <= 1                               # next to Hershey Duplex at scale 0.6


def test_font_constants_match_the_header():
    text = open(os.path.join(REPO, 'include', 'yolact_hip.h')).read()
    c = {k: int(v) for k, v in re.findall(r'#define YM_DRAW_([A-Z_]+) (\d+)', text)}
    assert (c['FONT_ADVANCE'], c['FONT_HEIGHT']) == (font.ADVANCE, font.HEIGHT) == (hip.DRAW_FONT_ADVANCE, hip.DRAW_FONT_HEIGHT)
    assert (c['NAME_STRIDE'], c['LABEL_MAX'], c['MAX_DET']) == (hip.DRAW_NAME_STRIDE, hip.DRAW_LABEL_MAX, hip.DRAW_MAX_DET)
    assert (c['NAME_STRIDE'] - 1, c['LABEL_MAX']) == (R.NAME_MAX, R.LABEL_MAX)
    assert (c['HIDE_MASK'], c['HIDE_BBOX'], c['HIDE_SCORE'], c['REAL_TIME']) == \
        (hip.DRAW_HIDE_MASK, hip.DRAW_HIDE_BBOX, hip.DRAW_HIDE_SCORE, hip.DRAW_REAL_TIME)


def test_coco_labels_fit_their_plates():
    """Every glyph pixel of a label with baseline-left (x1, y1 + 15) lies inside the plate x1..x1+text_w, y1..y1+text_h+5."""
    for name in COCO_CLASSES:
        for cents in range(101):
            text = R.label_text(name, np.float32(cents / 100), False)
            assert len(text) <= R.LABEL_MAX and text.startswith(name + ': ')
            text_w, text_h = font.text_size(text)
            bm = font.text_bitmap(text)
            ys, xs = np.nonzero(bm)
            top = 15 - (font.HEIGHT - 1)
            assert xs.min() >= 0 and xs.max() <= text_w and ys.min() + top >= 0 and ys.max() + top <= text_h + 5


# ---- hand-derived known answers (shared with the GPU test) -----------------------------------------------------------------------
P1, P3 = (84, 84, 242), (9, 199, 120)        # COLORS[1], COLORS[3] (pinned below)


def known_single_mask_and_box():
    """8 x 8 frame of (100, 150, 200); one detection, class 0, mask rows 2..4 x columns 2..4, box given with reversed corners
    (5, 6) - (1, 1).  Every pixel is first blended: uncovered (0 + 6 v + 5) // 10 = (60, 90, 120); covered with P[1] = (84, 84, 242):
    (336 + 600 + 5) // 10 = 94, (336 + 900 + 5) // 10 = 124, (968 + 1200 + 5) // 10 = 217.  Outline in P[1]: rows 1 and 6 for
    x = 1..5, columns 1 and 5 for y = 1..6.  Plate from (5, 6): x 5..7, y 6..7 (clipped).  The text's first row is y = 8: outside."""
    img = np.empty((8, 8, 3), dtype=np.uint8)
    img[:] = (100, 150, 200)
    masks = np.zeros((1, 8, 8), dtype=np.float32)
    masks[0, 2:5, 2:5] = 1
    d, m, o = (60, 90, 120), (94, 124, 217), P1
    rows = ['dddddddd',
            'dooooodd',
            'dommmodd',
            'dommmodd',
            'dommmodd',
            'dodddodd',
            'dooooooo',
            'dddddooo']
    want = np.array([[{'d': d, 'm': m, 'o': o}[ch] for ch in row] for row in rows], dtype=np.uint8)
    args = (np.array([0], dtype=np.int64), np.array([0.9], dtype=np.float32), np.array([[5, 6, 1, 1]], dtype=np.int32), masks, img)
    return args, R.make_cfg(), want


def known_overlap_modulo():
    """4 x 6 frame of (10, 20, 30), nc = 5, ids 0 and 2 (weights 1 and 3), no boxes.  Columns 0-1: s = 1 -> P[1]; columns 2-3:
    s = 4 mod 4 = 0 -> the background colour, i.e. only darkened: (65 // 10, 125 // 10, 185 // 10) = (6, 12, 18); columns 4-5: s = 3 ->
    P[3] = (9, 199, 120): (36 + 60 + 5) // 10 = 10, (796 + 120 + 5) // 10 = 92, (480 + 180 + 5) // 10 = 66."""
    img = np.empty((4, 6, 3), dtype=np.uint8)
    img[:] = (10, 20, 30)
    masks = np.zeros((2, 4, 6), dtype=np.float32)
    masks[0, :, 0:4] = 1
    masks[1, :, 2:6] = 1
    want = np.empty((4, 6, 3), dtype=np.uint8)
    want[:, 0:2] = ((336 + 60 + 5) // 10, (336 + 120 + 5) // 10, (968 + 180 + 5) // 10)
    want[:, 2:4] = (6, 12, 18)
    want[:, 4:6] = (10, 92, 66)
    args = (np.array([0, 2], dtype=np.int64), np.array([0.8, 0.7], dtype=np.float32), np.zeros((2, 4), dtype=np.int32), masks, img)
    return args, R.make_cfg(class_names=CUSTOM_CLASSES, hide_bbox=True), want


def known_draw_order():
    """Two detections whose plates overlap, masks hidden: detection 0 ('dog', P[1]) at (4, 3), detection 1 ('bear', P[3]) at (10, 9).
    The reference paints 1 first and 0 over it, so wherever both touch a pixel detection 0 shows — also where 1 has a glyph pixel."""
    h, w = 40, 72
    img = np.full((h, w, 3), 7, dtype=np.uint8)
    ids = np.array([0, 2], dtype=np.int64)
    boxes = np.array([[4, 3, 30, 35], [10, 9, 60, 38]], dtype=np.int32)
    cfg = R.make_cfg(class_names=CUSTOM_CLASSES, hide_mask=True, hide_score=True)
    want = img.copy()
    for i in (1, 0):
        x1, y1, x2, y2 = boxes[i]
        colour = (P1, P3)[i]
        text = ('dog', 'bear')[i]
        want[y1, x1:x2 + 1] = colour
        want[y2, x1:x2 + 1] = colour
        want[y1:y2 + 1, x1] = colour
        want[y1:y2 + 1, x2] = colour
        want[y1:y1 + font.HEIGHT + 5 + 1, x1:x1 + len(text) * font.ADVANCE + 1] = colour
        bm = font.text_bitmap(text)
        patch = want[y1 + 2:y1 + 2 + font.HEIGHT, x1:x1 + bm.shape[1]]
        patch[bm] = 255
    args = (ids, np.array([0.9, 0.8], dtype=np.float32), boxes, np.zeros((2, h, w), dtype=np.float32), img)
    return args, cfg, want


KNOWN = (known_single_mask_and_box, known_overlap_modulo, known_draw_order)


def test_palette_entries_the_known_answers_use():
    assert tuple(COLORS[0]) == (0, 0, 0) and tuple(COLORS[1]) == P1 and tuple(COLORS[3]) == P3


def test_draw_order_known_answer_shows_detection_zero_on_top():
    (ids, scores, boxes, masks, img), cfg, want = known_draw_order()
    # pixels of detection 0's plate (x 4..40, y 3..22) where 'bear' (text rows 11..24 from x = 10) has a glyph pixel and 'dog' (text rows
    # 5..18 from x = 4) has none: they must show detection 0's plate colour
    dog, bear = font.text_bitmap('dog'), font.text_bitmap('bear')
    both = [(y, x) for y in range(11, 23) for x in range(10, 41)
            if bear[y - 11, x - 10] and not (y <= 18 and x - 4 < dog.shape[1] and dog[y - 5, x - 4])]
    assert both, 'the case must contain a pixel where only the lower label has a glyph'
    for y, x in both:
        assert tuple(want[y, x]) == P1
    assert tuple(want[9, 50]) == P3 and tuple(want[3, 20]) == P1 and tuple(want[0, 0]) == (7, 7, 7)


@pytest.mark.parametrize('case', KNOWN, ids=lambda f: f.__name__)
def test_oracle_agrees_with_the_known_answers(case):
    (ids, scores, boxes, masks, img), cfg, want = case()
    got = R.draw_ref(ids, scores, boxes, masks, img, cfg)
    assert got.dtype == np.uint8 and np.array_equal(got, want)


def test_oracle_conventions():
    ids, scores, boxes, masks, img = R.synth(6, 37, 53, seed=1, wild_boxes=True)
    cfg = R.make_cfg()
    assert R.draw_ref(None, None, None, None, img, cfg) is img
    a = R.draw_ref(ids, scores, boxes, masks, img, cfg)
    b = R.draw_ref(ids, scores, boxes, masks, img, R.make_cfg(real_time=True), fps=31.256)
    th, tw = font.HEIGHT, len('fps: 31.26') * font.ADVANCE
    assert np.array_equal(a[th + 8:], b[th + 8:]) and np.array_equal(a[:, tw + 8:], b[:, tw + 8:]) and not np.array_equal(a, b)
    total, objs = R.cutout_ref(ids, boxes, masks, img, cfg)
    assert total.shape == img.shape and len(objs) == 6
    assert objs[0].shape == img[boxes[0][1]:boxes[0][3], boxes[0][0]:boxes[0][2]].shape        # python slice rules, negative corners


def test_renderer_refuses_host_detections():
    import torch
    cfg = R.make_cfg()
    img = np.zeros((8, 8, 3), dtype=np.uint8)
    assert draw.draw_img(None, None, None, None, img, cfg) is img
    with pytest.raises(RuntimeError):
        draw.draw_img(torch.zeros(1, dtype=torch.int64), torch.zeros(1), torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, 8, 8), img, cfg)
    with pytest.raises(RuntimeError):
        draw.draw_img(np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.float32), np.zeros((1, 4), dtype=np.int32),
                      np.zeros((1, 8, 8), dtype=np.float32), img, cfg)
