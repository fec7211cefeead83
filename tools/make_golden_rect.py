"""Writes tests/golden/forward_res50_coco_rect_64x96_b2.npz: the REAL reference's eval forward on a rectangular tensor.

The reference's network is fully convolutional, so `net(img)` accepts H != W as it is; only its anchors assume the square.  The
fixture pins the rectangular forward of this project (tests/test_gpu_rect.py) against the reference's own outputs, not only
against the restatement in oracle/yolact_ref.py.  Run from the repository root with the reference checkout present:

    python tools/make_golden_rect.py

Data only: seed, the four output tensors, a digest of the input.
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import yolact_ref as R  # noqa: E402
from oracle.make_golden import import_reference, ref_cfg, tensor_digest  # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden')
NAME, SIZE, H, W, BATCH, SEED = 'res50_coco', 96, 64, 96, 2, 27


def main():
    ref_config, ref_yolact, _, _ = import_reference()
    cfg = ref_cfg(ref_config, NAME, SIZE)
    torch.manual_seed(SEED)
    net = ref_yolact.Yolact(cfg).eval()
    sd = net.state_dict()
    R.randomize_bn_(sd, SEED + 100)
    R.randomize_bias_(sd, SEED + 200)
    net.load_state_dict(sd)
    img = torch.randn(BATCH, 3, H, W, generator=torch.Generator().manual_seed(SEED + 300))
    with torch.no_grad():
        ref = net(img)
        mine = R.forward_eval_any(img, sd)
    for a, b, key in zip(ref, mine, ('class', 'box', 'coef', 'proto')):
        print(f'{key}: {tuple(a.shape)}  max|reference - restatement| = {(a - b).abs().max().item():.3e}')
    path = os.path.join(OUT, f'forward_{NAME}_rect_{H}x{W}_b{BATCH}.npz')
    np.savez_compressed(path, seed=np.array(SEED), size=np.array(SIZE), class_pred=ref[0].numpy(), box_pred=ref[1].numpy(),
                        coef_pred=ref[2].numpy(), proto_out=ref[3].numpy(), img_digest=tensor_digest(img))
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
