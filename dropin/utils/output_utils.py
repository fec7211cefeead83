"""`utils.output_utils` for the reference scripts: `nms` / `after_nms` are the HIP path, and so is `draw_img` whenever its
detections are device tensors (what `after_nms` returns): masks, boxes and labels are drawn on the device and only the finished
frame comes back.  With numpy detections (the ONNX / TensorRT scripts) `draw_img`, and always `draw_lincomb`, are the checkout's
own cv2 code (`utils/output_utils.py:276-369`), loaded from there on first use."""
import importlib.util
import os
import sys

import torch

from yolact_minimal_amd.utils.output_utils import nms, after_nms  # noqa: F401
from yolact_minimal_amd.utils.draw import draw_img as _device_draw_img, draw_batch, cutout_mattes  # noqa: F401

_host = None


def _checkout_module():
    global _host
    if _host is None:
        here = os.path.dirname(os.path.abspath(__file__))
        for p in sys.path:
            cand = os.path.join(p or os.getcwd(), 'utils', 'output_utils.py')
            if os.path.isfile(cand) and os.path.dirname(os.path.abspath(cand)) != here:
                spec = importlib.util.spec_from_file_location('_reference_output_utils', cand)
                mod = importlib.util.module_from_spec(spec)
                spec.loader.exec_module(mod)      # needs the checkout's own dependencies (cv2, cython_nms)
                _host = mod
                break
        else:
            raise ImportError('draw_img / draw_lincomb are the reference checkout\'s host-side cv2 helpers: run from inside a '
                              'Yolact_minimal checkout (its utils/output_utils.py was not found on sys.path)')
    return _host


def draw_img(ids_p, class_p, box_p, mask_p, img_origin, cfg, img_name=None, fps=None):
    if ids_p is None:
        return img_origin
    if not (torch.is_tensor(ids_p) and ids_p.is_cuda):
        return _checkout_module().draw_img(ids_p, class_p, box_p, mask_p, img_origin, cfg, img_name, fps)
    if getattr(cfg, 'cutout', False) and not getattr(cfg, 'hide_mask', False):
        _write_cutouts(ids_p, box_p, mask_p, img_origin, cfg, img_name)
    return _device_draw_img(ids_p, class_p, box_p, mask_p, img_origin, cfg, img_name, fps)


def _write_cutouts(ids_p, box_p, mask_p, img_origin, cfg, img_name):
    """The files of the reference's cfg.cutout branch (`:346-358`); the mattes come from the device, cv2 only encodes them."""
    try:
        import cv2
    except ImportError:
        return                      # no encoder on this machine: cutout_mattes() still gives the arrays
    total, objs = cutout_mattes(ids_p, box_p, mask_p, img_origin, cfg)
    as_np = (lambda a: a) if not torch.is_tensor(total) else (lambda a: a.cpu().numpy())
    cv2.imwrite(f'results/images/{img_name}_total_obj.jpg', as_np(total))
    for i, obj in enumerate(objs):
        cv2.imwrite(f'results/images/{img_name}_{i}.jpg', as_np(obj))


def draw_lincomb(*args, **kwargs):
    return _checkout_module().draw_lincomb(*args, **kwargs)
