"""Rectangular inference ("window mode"): the geometry, host only.

The reference pads a frame to a square with `norm_mean` at the top-left, resizes the square to `img_size` and runs all of it
(`utils/augmentations.py:138-165,219-227`).  The padding normalises to exactly 0.0 and lies below / right of the picture, so the
network input that matters is the top-left `Hn x Wn` WINDOW of the square one, and everything the network says about it lives in
the square's coordinate frame: boxes in 0..1 of the `img_size` square, masks on the `img_size / 4` prototype grid.  Window mode
runs only that window: `val_aug(..., window=)`, `Yolact.anchors_for`, `after_nms(..., window=True)`, `RequestPipeline` with
`height != width`.  It is an opt-in approximation (at the window's edge the convolutions see a zero border where the square run
sees the activations of the padded region), not a parity path.
"""
import torch

FPN_STRIDES = (8, 16, 32, 64, 128)


def _ceil_div(a, b):
    return -(-a // b)


def rect_window(sizes, img_size):
    """The network input shape `(Hn, Wn)` that holds the picture of every frame of `sizes` = [(h, w), ...] (or one pair) after the
    reference's pad-to-square + resize to `img_size`: `Hn = ceil32(max_i ceil(S * h_i / L_i))`, `L_i = max(h_i, w_i)`, likewise
    `Wn`.  One of the two is always `img_size` (rounded up to 32); a square frame, or a mix of landscape and portrait, gives the
    square.  Integer arithmetic."""
    s = int(img_size)
    if len(sizes) == 2 and not hasattr(sizes[0], '__len__'):
        sizes = [sizes]
    if s < 1 or not len(sizes):
        raise RuntimeError(f'rect_window: img_size = {s}, {len(sizes)} frames')
    hn = wn = 0
    for h, w in sizes:
        h, w = int(h), int(w)
        if h < 1 or w < 1:
            raise RuntimeError(f'rect_window: frame size {h} x {w}')
        side = max(h, w)
        hn, wn = max(hn, _ceil_div(s * h, side)), max(wn, _ceil_div(s * w, side))
    return _ceil_div(hn, 32) * 32, _ceil_div(wn, 32) * 32


def rect_level_shapes(hn, wn):
    """The five FPN level shapes [(h_l, w_l)] of an `hn x wn` input: /8, /16, /32, then two stride-2 3x3 convolutions (ceil)."""
    hn, wn = int(hn), int(wn)
    if hn < 32 or wn < 32 or hn % 32 or wn % 32:
        raise RuntimeError(f'window {hn} x {wn}: both sides are positive multiples of 32')
    shapes = [(hn // 8, wn // 8), (hn // 16, wn // 16), (hn // 32, wn // 32)]
    for _ in range(2):
        h, w = shapes[-1]
        shapes.append((_ceil_div(h, 2), _ceil_div(w, 2)))
    return shapes


def rect_anchor_index(cfg, hn, wn):
    """int64 indices into the square anchor list (`Yolact.anchors`, level-major, then row, column, aspect ratio) of the anchors an
    `hn x wn` window keeps: per level the rows `j < h_l` and columns `i < w_l` of the square `n_l x n_l` grid, in the same order --
    which is the order the heads of an `hn x wn` forward write their predictions in."""
    s = int(cfg.img_size)
    na = len(cfg.aspect_ratios)
    out, base = [], 0
    for stride, (h, w) in zip(FPN_STRIDES, rect_level_shapes(hn, wn)):
        n = _ceil_div(s, stride)
        if h > n or w > n:
            raise RuntimeError(f'window {hn} x {wn} is not inside the {s} x {s} input (level /{stride}: {h} x {w} of {n} x {n})')
        cell = torch.arange(h, dtype=torch.int64).view(h, 1) * n + torch.arange(w, dtype=torch.int64).view(1, w)
        out.append((base + cell.reshape(-1, 1) * na + torch.arange(na, dtype=torch.int64).view(1, na)).reshape(-1))
        base += n * n * na
    return torch.cat(out)
