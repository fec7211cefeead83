"""CPU restatement of window-mode `after_nms` (include/yolact_hip.h, "window mode") from the pieces of oracle/yolact_ref.py.

`proto` is the top-left `[Hp, Wp]` window of the square `P x P` prototype map (`P = max(Hp, Wp)`) that the square run would have
produced.  The reference's `after_nms` on that square map, with what lies past the window taken from the window's last row /
column (replicate padding), restricted to what the window holds:
    soft = sigmoid(proto @ coef^T)                       [Hp, Wp, n]
    crop with the window of `crop_window(boxes, P, P)`   (box -> prototype pixels through P on BOTH axes)
    F.pad(mode='replicate') to P x P
    F.interpolate to (L, L), L = max(img_h, img_w), bilinear, align_corners=False
    > 0.5, slice to img_h x img_w
Not a test module.
"""
import torch
import torch.nn.functional as F

from oracle import yolact_ref as R


def after_nms_window(boxes, coefs, proto, img_h, img_w, do_crop=True):
    """-> (boxes_px int32 [n, 4], masks f32 [n, img_h, img_w] in {0, 1}, up f32 [n, img_h, img_w]: the interpolated soft masks).
    `boxes` is not mutated."""
    hp, wp, _ = proto.shape
    p = max(hp, wp)
    soft = torch.sigmoid(torch.matmul(proto, coefs.t()))                         # [Hp, Wp, n]
    if do_crop:
        x1, x2, y1, y2 = R.crop_window(boxes, p, p)
        xs = torch.arange(wp, dtype=x1.dtype).view(1, -1, 1)
        ys = torch.arange(hp, dtype=x1.dtype).view(-1, 1, 1)
        inside = (xs >= x1.view(1, 1, -1)) & (xs < x2.view(1, 1, -1)) & (ys >= y1.view(1, 1, -1)) & (ys < y2.view(1, 1, -1))
        soft = soft * inside.float()
    soft = soft.permute(2, 0, 1).contiguous().unsqueeze(0)                       # [1, n, Hp, Wp]
    soft = F.pad(soft, (0, p - wp, 0, p - hp), mode='replicate')
    size = max(img_h, img_w)
    up = F.interpolate(soft, (size, size), mode='bilinear', align_corners=False).squeeze(0)[:, :img_h, :img_w]
    return (boxes * size).int(), (up > 0.5).float(), up


def threshold_band(up, tol=1e-4):
    """Fraction of pixels whose interpolated value is within `tol` of the 0.5 threshold (where two fp32 evaluations may disagree)."""
    return float(((up - 0.5).abs() < tol).float().mean())
