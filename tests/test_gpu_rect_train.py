"""Window training on the GPU (yolact_minimal_amd/utils/rect.py): the mask-loss kernel with a virtual extent, the augmentation into a
window, one whole training step on a window against fp64 autograd, and the accuracy a window-trained detector reaches through the
window serving path.  The fp64 references are tests/rect_train_ref.py, pinned against the oracle in tests/test_rect_train_cpu.py."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from oracle import yolact_ref as R
from tests import rect_train_ref as W
from yolact_minimal_amd.config import build_cfg
from yolact_minimal_amd.modules.yolact import Yolact

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

COUNTS = (0, 1, 37, 128)                       # positives per image


@pytest.fixture(autouse=True)
def _restore_switch():
    """The accuracy test trains with `Trainer(deterministic=True)`, a process-wide switch: the tests after it see the default again."""
    from yolact_minimal_amd import loss, train_engine as T
    before = T._DETERMINISTIC
    gens = {k: g.get_state() for k, g in loss._mask_generators.items()}      # (the kernel tests re-seed the sub-sampling generator)
    yield
    T._DETERMINISTIC = before
    T.tuned_table_changed()
    for k in list(loss._mask_generators):
        if k in gens:
            loss._mask_generators[k].set_state(gens[k])
        else:
            del loss._mask_generators[k]


def _cfg128():
    cfg = build_cfg('res50_coco', 'train', 128)
    cfg.masks_to_train = 128                   # all 128 positives of the last image are trained (the kernel's capacity), no sub-sampling
    return cfg


def _gpu_mask_loss(cfg, case, virtual, seed=0):
    from yolact_minimal_amd.loss import lincomb_mask_loss, mask_generator
    proto, coef, pos, anchor_gt, anchor_box, masks = case
    pg, cg = proto.to(DEV).requires_grad_(), coef.to(DEV).requires_grad_()
    mask_generator(DEV).manual_seed(seed)      # the visiting order of the positives comes from this generator
    got = lincomb_mask_loss(cfg, pos.to(DEV), anchor_gt.to(DEV), cg, pg, [m.to(DEV) for m in masks], anchor_box.to(DEV), virtual=virtual)
    got.backward()
    torch.cuda.synchronize()
    return got.detach().cpu(), pg.grad.cpu(), cg.grad.cpu()


@pytest.mark.parametrize('hp,wp', [(24, 32), (32, 24), (17, 24)])
def test_window_mask_loss_kernel_matches_fp64_restatement(hp, wp):
    """`ym_mask_loss_batch_window` on maps that are the top-left of a 32 x 32 one: boxes inside, reaching the cut exactly and
    extending past it (clamped), 0 / 1 / 37 / 128 positives per image; 17 x 24 = 408 pixels is no multiple of the 32-pixel tile.
    Bars of test_mask_loss_kernel_matches_oracle_autograd."""
    pv = 32
    case = W.rect_case(hp, wp, pv, COUNTS, seed=hp)
    proto, coef, pos, anchor_gt, anchor_box, masks = case
    pr, cf = proto.double().requires_grad_(), coef.double().requires_grad_()
    ref = W.window_mask_loss(pos, anchor_gt, cf, pr, [m.double() for m in masks], anchor_box.double(), pv)
    ref.backward()
    got, dproto, dcoef = _gpu_mask_loss(_cfg128(), case, pv)
    print(f'window mask loss {hp}x{wp} of {pv}: gpu {float(got):.7f} fp64 {float(ref.detach()):.7f}  '
          f'max|dproto err| / max {float((dproto.double() - pr.grad).abs().max() / pr.grad.abs().max()):.2e}  '
          f'max|dcoef err| / max {float((dcoef.double() - cf.grad).abs().max() / cf.grad.abs().max()):.2e}')
    np.testing.assert_allclose(float(got), float(ref.detach()), rtol=2e-5)
    torch.testing.assert_close(dproto.double(), pr.grad, rtol=1e-4, atol=1e-5 * float(pr.grad.abs().max()))
    torch.testing.assert_close(dcoef.double(), cf.grad, rtol=1e-4, atol=1e-5 * float(cf.grad.abs().max()))
    assert float(dproto[0].abs().max()) == 0.0 and float(dcoef[0].abs().max()) == 0.0      # the image without positives
    # the case holds positives whose crop window (box * Pv + padding) passes the map's edge: pixels there do not exist, so what the
    # comparison above pins for them is the scaling by Pv, not the kernel's clamp of the window to the map (which changes no pixel)
    assert float(ref.detach()) > 0 and bool((anchor_box[pos][:, 3] * pv + 1 > hp).any() or (anchor_box[pos][:, 2] * pv + 1 > wp).any())

    # the one-image entry (gathered operands) is the same kernel with one item
    from yolact_minimal_amd import hip
    i = 2
    idx = torch.nonzero(pos[i]).flatten().to(DEV)
    ds = torch.empty(4, hp, wp, device=DEV)
    hip.gt_masks_downsample(masks[i].to(DEV).contiguous(), hp, wp, ds)
    coeff = 6.125 / pv / pv / int(pos.sum())
    one_dproto, one_dcoef = torch.zeros(hp, wp, 32, device=DEV), torch.zeros(coef.shape[1], 32, device=DEV)
    acc = torch.zeros(1, dtype=torch.float64, device=DEV)
    ws = torch.empty(hip.lib().ym_mask_loss_workspace_bytes(), dtype=torch.uint8, device=DEV)
    proto_i, coef_i = proto[i].to(DEV).contiguous(), coef[i].to(DEV)[idx].contiguous()
    box_i, gt_i = anchor_box[i].to(DEV)[idx].contiguous(), anchor_gt[i].to(DEV)[idx].to(torch.int32).contiguous()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())                                         # noqa: E731
    hip.check(hip.lib().ym_mask_loss_fwd_bwd_window(
        hip.ptr(proto_i), hip.ptr(coef_i), hip.ptr(box_i), hip.ptr(gt_i, torch.int32), hip.ptr(ds), hip.ptr(idx, torch.int64),
        idx.shape[0], hp, wp, pv, 1.0, float(coeff), vp(acc), hip.ptr(one_dproto), hip.ptr(one_dcoef), vp(ws), ws.numel(),
        hip.stream_ptr()), 'ym_mask_loss_fwd_bwd_window')
    torch.cuda.synchronize()
    for got_t, ref_t in ((one_dproto.cpu().double(), pr.grad[i]), (one_dcoef.cpu().double(), cf.grad[i])):
        torch.testing.assert_close(got_t, ref_t, rtol=1e-4, atol=1e-5 * float(ref_t.abs().max()))
    # a virtual extent smaller than the map is refused before any launch
    assert hip.lib().ym_mask_loss_fwd_bwd_window(
        hip.ptr(proto_i), hip.ptr(coef_i), hip.ptr(box_i), hip.ptr(gt_i, torch.int32), hip.ptr(ds), hip.ptr(idx, torch.int64),
        idx.shape[0], hp, wp, max(hp, wp) - 1, 1.0, float(coeff), vp(acc), hip.ptr(one_dproto), hip.ptr(one_dcoef), vp(ws), ws.numel(),
        hip.stream_ptr()) != 0


def _sha(t):
    import hashlib
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


@pytest.mark.parametrize('hp,wp,pv', [(24, 32, 32), (17, 24, 32), (34, 34, 34)])
def test_pv_0_returns_the_bits_recorded_before_the_window_entries_existed(golden_dir, monkeypatch, hp, wp, pv):
    """`Pv = 0` means per-axis extents, today's rule.  tests/golden/rect_train_mask_loss_pv0.json holds the sha256 of the loss and
    both gradients that the library returned for these cases BEFORE the window entries existed (recorded from a build of the
    parent commit, repeatable run to run: no sub-sampling, ordered partial sums).  `ym_mask_loss_batch` -- now the Pv = 0 instance
    of the window kernels -- and `ym_mask_loss_batch_window(Pv = 0)` both return those bits."""
    import json
    from yolact_minimal_amd import hip
    want = json.load(open(os.path.join(golden_dir, 'rect_train_mask_loss_pv0.json')))[f'{hp}x{wp}']
    case = W.rect_case(hp, wp, pv, COUNTS, seed=3)
    cfg = _cfg128()
    old = _gpu_mask_loss(cfg, case, None, seed=7)
    assert float(old[0]) == want['loss_value'] > 0
    assert {'loss': _sha(old[0]), 'dproto': _sha(old[1]), 'dcoef': _sha(old[2])} == {k: want[k] for k in ('loss', 'dproto', 'dcoef')}
    L = hip.lib()
    calls = []

    def through_window(items, b, h, w, *rest):
        calls.append((h, w))
        return L.ym_mask_loss_batch_window(items, b, h, w, 0, *rest)
    monkeypatch.setattr(L, 'ym_mask_loss_batch', through_window)
    new = _gpu_mask_loss(cfg, case, None, seed=7)
    assert calls == [(hp, wp)]
    assert {'loss': _sha(new[0]), 'dproto': _sha(new[1]), 'dcoef': _sha(new[2])} == {k: want[k] for k in ('loss', 'dproto', 'dcoef')}


# ---- augmentation into a window --------------------------------------------------------------------------------------------------
def _plan(final_mode, mirror, h, w, window, k):
    from yolact_minimal_amd.utils.augmentations import AugPlan
    p = AugPlan()
    p.brightness, p.contrast, p.saturation, p.hue = 12.5, 1.1, 0.9, 7.0
    p.mirror = mirror
    p.crop = (2, 3, w - 5, h - 4)
    cw, ch = w - 5, h - 4
    p.square = max(cw, ch)
    p.pad = (0, 3) if ch < cw else (4, 0)
    p.size = 64
    p.final_pad = p.final_crop = None
    if final_mode == 0:
        p.resize = 64
    elif final_mode == 1:
        p.resize, p.final_pad = 32, (9, 21)
    else:
        p.resize, p.final_crop = 96, (17, 5)
    p.boxes, p.labels = np.zeros((k, 4)), np.zeros(k)
    p.keep = np.arange(k)[::-1].copy()
    p.window = window
    return p


@pytest.mark.parametrize('window', [(32, 64), (64, 32), (32, 32)])
@pytest.mark.parametrize('dtype', [torch.uint8, torch.float32])
def test_train_aug_window_is_the_cut_of_the_square_result(window, dtype):
    """Image rows and kept mask rows of `apply_train_aug_batch(window=)` equal the square result's `[:Hn, :Wn]` bit for bit: final_mode
    0 / 1 / 2, mirror on and off, 37 x 53 and 53 x 37 sources, B = 1 and B = 17 (two launches per entry)."""
    from yolact_minimal_amd.utils.augmentations import apply_train_aug, apply_train_aug_batch
    hn, wn = window
    g = torch.Generator().manual_seed(hn * 100 + wn)
    imgs, masks, plans = [], [], []
    for b in range(17):
        h, w = (37, 53) if b % 2 == 0 else (53, 37)
        k = 0 if b % 4 == 3 else 1 + b % 2        # kept masks: independent of the final mode (b % 3); sample 0 keeps one
        img = torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8)
        m = (torch.rand(max(k, 1), h, w, generator=g) > 0.5).to(torch.uint8)
        imgs.append(img.to(dtype).to(DEV))
        masks.append(m.to(dtype).to(DEV))
        plans.append(_plan(b % 3, bool((b // 3) % 2), h, w, None, k))
    assert {(int(p.final_pad is not None) + 2 * int(p.final_crop is not None), p.mirror) for p in plans} == {(m, f) for m in (0, 1, 2) for f in (False, True)}
    # every final mode keeps mask rows with and without mirror, and one sample of each mode keeps none
    modes = {}
    for p in plans:
        modes.setdefault((int(p.final_pad is not None) + 2 * int(p.final_crop is not None), p.mirror), []).append(len(p.keep))
    assert all(max(ks) >= 1 for ks in modes.values()) and all(0 in modes[(m, False)] + modes[(m, True)] for m in (0, 1, 2)), modes
    # B = 1 for a sample of each final mode (each keeps mask rows), then B = 17
    for sel in ([0], [1], [2], list(range(17))):
        batch = len(sel)
        bi, bm, bp = [imgs[i] for i in sel], [masks[i] for i in sel], [plans[i] for i in sel]
        sq_img, sq_masks = apply_train_aug_batch(bi, bm, bp)
        win_img, win_masks = apply_train_aug_batch(bi, bm, bp, window=window)
        torch.cuda.synchronize()
        assert tuple(win_img.shape) == (batch, 3, hn, wn) and tuple(sq_img.shape) == (batch, 3, 64, 64)
        assert torch.equal(win_img, sq_img[:, :, :hn, :wn])
        assert float(win_img.abs().max()) > 0
        rows = lit = 0
        for a, b, p in zip(win_masks, sq_masks, bp):
            assert a.shape[0] == len(p.keep) and tuple(a.shape) == (b.shape[0], hn, wn) and torch.equal(a, b[:, :hn, :wn])
            rows += a.shape[0]
            lit += int((a.flatten(1).sum(1) > 0).sum())
        assert rows == sum(len(p.keep) for p in bp) >= 1 and lit == rows, (sel, rows, lit)      # mask pixels were compared, none blank
    # the one-sample call and plans drawn for the window take the same path
    p = _plan(2, True, 37, 53, window, 2)
    one_img, one_masks = apply_train_aug(imgs[0], masks[0].repeat(2, 1, 1), p)
    p.window = None
    ref_img, ref_masks = apply_train_aug(imgs[0], masks[0].repeat(2, 1, 1), p)
    assert torch.equal(one_img, ref_img[:, :hn, :wn]) and torch.equal(one_masks, ref_masks[:, :hn, :wn])
    with pytest.raises(RuntimeError):
        apply_train_aug_batch(imgs[:1], masks[:1], plans[:1], window=(hn, 96))


# ---- one training step on a window ---------------------------------------------------------------------------------------------
def _window_targets(size, hn, wn, seed):
    """`R.synth_targets` of the square, cut to the window: boxes clipped to it (they stay in 0..1 of the square), masks cut; boxes
    that keep less than 5 % of the square's side inside are dropped."""
    boxes, masks = R.synth_targets(2, size, seed=seed)
    out_b, out_m = [], []
    for bx, m in zip(boxes, masks):
        bx = bx.clone()
        bx[:, 2].clamp_(max=wn / size)
        bx[:, 3].clamp_(max=hn / size)
        keep = ((bx[:, 2] - bx[:, 0]) > 0.05) & ((bx[:, 3] - bx[:, 1]) > 0.05)
        assert bool(keep.any())
        out_b.append(bx[keep].contiguous())
        out_m.append(m[keep][:, :hn, :wn].contiguous())
    return out_b, out_m


def _window_oracle_grads(net, sd0, img, boxes, masks, anchors, size, dtype):
    params = {k: (v.clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd0.items()}
    names = [k for k, _ in net.named_parameters()]
    for k in names:
        params[k].requires_grad_(True)
    out = R.TrainNet(params).forward(img.to(dtype))
    torch.set_default_dtype(dtype)
    try:
        losses = W.window_compute_loss(*out, [b.to(dtype) for b in boxes], [m.to(dtype) for m in masks], anchors.to(dtype), size)
    finally:
        torch.set_default_dtype(torch.float32)
    sum(losses).backward()
    return [float(l.detach()) for l in losses], {k: params[k].grad.double() for k in names}


def _rel_err(a, b):
    return ((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30)).item()


@pytest.mark.parametrize('window', [(64, 96), (96, 64)])
def test_window_train_step_matches_fp64_autograd(window):
    """res50_coco on a 2 x 3 x Hn x Wn window of S = 96: the four losses and every parameter gradient against fp64 autograd through
    `R.TrainNet` and the `R` loss functions with the window's anchors (the restatement for the mask and semantic terms).  Bars of
    test_train_step_matches_reference_golden: losses 2e-4, the gradient error judged against the CPU fp32 oracle's own distance
    from fp64 (a random-init net at this size amplifies fp32 rounding by ~1e5 in the backbone)."""
    from yolact_minimal_amd.utils.rect import rect_anchor_index
    size, (hn, wn), seed = 96, window, 21
    cfg = build_cfg('res50_coco', 'train', size)
    torch.manual_seed(seed)
    net = Yolact(cfg).train()
    sd0 = {k: v.clone() for k, v in net.state_dict().items()}
    img = torch.randn(2, 3, size, size, generator=torch.Generator().manual_seed(seed + 300))[:, :, :hn, :wn].contiguous()
    boxes, masks = _window_targets(size, hn, wn, seed)
    anchors = torch.tensor(net.anchors).reshape(-1, 4)[rect_anchor_index(cfg, hn, wn)]
    l32, g32 = _window_oracle_grads(net, sd0, img, boxes, masks, anchors, size, torch.float32)
    l64, g64 = _window_oracle_grads(net, sd0, img, boxes, masks, anchors, size, torch.float64)

    net = net.to(DEV)
    losses = net(img.to(DEV), [b.to(DEV) for b in boxes], [m.to(DEV) for m in masks])
    sum(losses).backward()
    torch.cuda.synchronize()
    got = np.array([float(l.detach()) for l in losses])
    e_gpu = np.array([_rel_err(p.grad.cpu(), g64[k]) for k, p in net.named_parameters()])
    e_cpu = np.array([_rel_err(g32[k], g64[k]) for k, _ in net.named_parameters()])
    print(f'window step {hn}x{wn} of {size}: losses gpu {got.tolist()} fp64 {l64} cpu fp32 {l32}')
    print(f'  gradient error vs fp64, gpu / cpu fp32: median {np.median(e_gpu):.3e} / {np.median(e_cpu):.3e}  '
          f'q90 {np.quantile(e_gpu, 0.9):.3e} / {np.quantile(e_cpu, 0.9):.3e}  max {e_gpu.max():.3e} / {e_cpu.max():.3e}')
    assert all(v > 0 for v in l64)
    np.testing.assert_allclose(got, np.array(l64), rtol=2e-4)
    assert np.median(e_gpu) <= 4 * np.median(e_cpu) + 1e-5, (np.median(e_gpu), np.median(e_cpu))
    assert np.quantile(e_gpu, 0.9) <= 4 * np.quantile(e_cpu, 0.9) + 1e-4, (np.quantile(e_gpu, 0.9), np.quantile(e_cpu, 0.9))
    assert e_gpu.max() <= 10 * e_cpu.max() + 1e-4, (e_gpu.max(), e_cpu.max())


def test_window_forward_refuses_bad_shapes_and_swin_before_any_launch():
    cfg = build_cfg('res50_coco', 'train', 96)
    net = Yolact(cfg).train().to(DEV)
    boxes, masks = _window_targets(96, 64, 96, 21)
    for shape in ((2, 3, 64, 128), (2, 3, 48, 96), (2, 3, 64, 80)):
        with pytest.raises(RuntimeError):
            net(torch.zeros(shape, device=DEV), [b.to(DEV) for b in boxes], [m.to(DEV) for m in masks])
    swin = Yolact(build_cfg('swin_tiny_coco', 'train', 96)).train().to(DEV)
    with pytest.raises(RuntimeError, match='Swin'):
        swin(torch.zeros(2, 3, 64, 96, device=DEV), [b.to(DEV) for b in boxes], [m.to(DEV) for m in masks])


# ---- accuracy -------------------------------------------------------------------------------------------------------------------
# The yardstick: the square recipe on the same cut pictures (tools/overfit_demo.py --size 128 --steps 600 --window 96 128
# --window-recipe square --deterministic, seed 0), scored through the square path; measured once, recorded in
# profiles/rect_training.md.  [box mAP all, box mAP@50], [mask mAP all, mask mAP@50]
YARDSTICK_PROFILE = 'profiles/rect_training.md'
YARDSTICK_BOX = (52.3, 57.01)
YARDSTICK_MASK = (0.0, 0.0)        # (the mask branch died in the yardstick's trajectory: see the profile)


def test_window_trained_detector_scores_like_the_square_recipe_through_the_window_path():
    """600 steps of the overfit recipe on the pictures cut to 96 x 128 of S = 128, trained on [8, 3, 96, 128] and scored through
    `anchors_for` + `after_nms(window=True)`, against the square recipe on the same cut pictures (YARDSTICK_*, from
    profiles/rect_training.md).  The bar is the project's own for one trajectory of this recipe (tests/test_gpu_overfit.py): no more
    than 15 points under on mAP "all" and 12 under on mAP@50, box and mask, one-sided.  A square-trained detector through the window
    path is printed beside it, not asserted: that is the situation profiles/rect_serving.md records.
    Measured (deterministic mode, repeats to the digit): window-trained through the window path box 65.36 / 71.72, mask 55.99 / 71.72;
    square-trained through the square path 52.30 / 57.01, 0.00 / 0.00 (its mask branch died), through the window path 21.70 / 53.66.
    With that yardstick the mask half of this bar cannot fail; the test after this one binds on masks at a seed whose yardstick lives."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tools'))
    from overfit_demo import run
    args = dict(window=(96, 128), size=128, steps=600, batch=8, cfg_name='res50_custom', seed=0, deterministic=True,
                log=lambda *_: None, log_every=50)
    got = run(**args)
    print(f"window-trained, window path: box {got['box_map'][:2]} mask {got['mask_map'][:2]}  (square path: box "
          f"{got['paths']['square']['box_map'][:2]} mask {got['paths']['square']['mask_map'][:2]})  last losses {got['losses'][-1][1]}")
    print(f'yardstick ({YARDSTICK_PROFILE}): box {YARDSTICK_BOX} mask {YARDSTICK_MASK}')
    sq = run(window_recipe='square', **args)
    print(f"square-trained, square path: box {sq['box_map'][:2]} mask {sq['mask_map'][:2]};  through the window path: box "
          f"{sq['paths']['window']['box_map'][:2]} mask {sq['paths']['window']['mask_map'][:2]}")
    assert got['window'] == [96, 128] and got['window_recipe'] == 'window' and all(np.isfinite(sum(v)) for _, v in got['losses'])
    assert got['box_map'][0] >= YARDSTICK_BOX[0] - 15 and got['mask_map'][0] >= YARDSTICK_MASK[0] - 15, (got['box_map'], got['mask_map'])
    assert got['box_map'][1] >= YARDSTICK_BOX[1] - 12 and got['mask_map'][1] >= YARDSTICK_MASK[1] - 12, (got['box_map'], got['mask_map'])


# The seed-0 yardstick's mask branch is dead, so the test above binds on boxes only.  A second yardstick binds on masks: the square
# recipe on the cut pictures was run once at seeds 0, 1, 2, 3 (profiles/rect_training.md lists all four); the rule looks at the
# square recipe's own runs only: the FIRST seed whose square trajectory ends with a live mask branch (last mask loss < 1).
# That is seed 2 (seeds 0, 1 and 3 end at mask loss 7.8, 6.8, 8.5 with mask mAP 0).
LIVE_SEED = 2
LIVE_YARDSTICK_BOX = (83.9, 97.32)
LIVE_YARDSTICK_MASK = (76.4, 97.32)


def test_window_trained_masks_hold_against_a_live_square_trajectory():
    """The same recipe and the same bar at seed 2, where the square recipe's mask branch lives: the window-trained detector through
    the window path against the square recipe on the same cut pictures through the square path, box AND mask, 15 points on mAP
    "all" and 12 on mAP@50, one-sided.  Measured: window-trained 81.03 / 100.0 box, 75.31 / 100.0 mask against 83.90 / 97.32 and
    76.40 / 97.32."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tools'))
    from overfit_demo import run
    got = run(window=(96, 128), size=128, steps=600, batch=8, cfg_name='res50_custom', seed=LIVE_SEED, deterministic=True,
              log=lambda *_: None, log_every=50)
    print(f"seed {LIVE_SEED}: window-trained, window path: box {got['box_map'][:2]} mask {got['mask_map'][:2]}  last losses "
          f"{got['losses'][-1][1]};  yardstick ({YARDSTICK_PROFILE}): box {LIVE_YARDSTICK_BOX} mask {LIVE_YARDSTICK_MASK}")
    assert LIVE_YARDSTICK_MASK[0] > 50                                     # the yardstick itself has working masks
    assert got['box_map'][0] >= LIVE_YARDSTICK_BOX[0] - 15 and got['mask_map'][0] >= LIVE_YARDSTICK_MASK[0] - 15, (got['box_map'], got['mask_map'])
    assert got['box_map'][1] >= LIVE_YARDSTICK_BOX[1] - 12 and got['mask_map'][1] >= LIVE_YARDSTICK_MASK[1] - 12, (got['box_map'], got['mask_map'])
