"""bench.py's result line and `--dump-outputs`: a plain run prints the headline alone, and the arrays it writes are what the last
timed step computed (float32 / float64, large ones as a fixed seeded sample)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.conftest import REPO


def test_dump_outputs_writes_float_arrays_and_samples_large_ones(tmp_path):
    import bench
    arrays = dict(small=torch.arange(6, dtype=torch.float16).reshape(2, 3), ids=torch.tensor([3, 1, 2]),
                  big=torch.arange(100, dtype=torch.float32).reshape(2, 50), f64=torch.tensor([0.5], dtype=torch.float64))
    names = bench.dump_outputs(str(tmp_path / 'a'), arrays, max_elems=16)
    assert names == ['big_rowsum', 'big_sample', 'f64', 'ids', 'small']
    got = {n: np.load(tmp_path / 'a' / f'{n}.npy') for n in names}
    assert got['small'].dtype == np.float32 and np.array_equal(got['small'], np.arange(6).reshape(2, 3))
    assert got['ids'].dtype == np.float64 and np.array_equal(got['ids'], [3, 1, 2])
    assert got['f64'].dtype == np.float64 and got['f64'][0] == 0.5
    assert got['big_rowsum'].dtype == np.float64 and np.array_equal(got['big_rowsum'], [sum(range(50)), sum(range(50, 100))])
    s = got['big_sample']
    assert s.dtype == np.float32 and s.shape == (16,) and np.all(np.diff(s) >= 0) and s.min() >= 0 and s.max() < 100
    # the sample is fixed: a second run writes the same files
    bench.dump_outputs(str(tmp_path / 'b'), arrays, max_elems=16)
    for n in names:
        assert np.array_equal(np.load(tmp_path / 'b' / f'{n}.npy'), got[n]), n
    with pytest.raises(ValueError):
        bench.dump_outputs(str(tmp_path / 'c'), arrays, max_elems=16, limit_bytes=64)
    assert not (tmp_path / 'c').exists()


@pytest.mark.gpu
def test_plain_bench_prints_the_headline_only_and_dumps_the_last_step(tmp_path):
    """`bench.py --steps K --warmup W --dump-outputs DIR` without `--full`: one JSON line with the headline fields only, K timed
    steps, and the dumped detections equal to the post-processing of the step's inputs recomputed here."""
    import bench
    from yolact_minimal_amd.utils.output_utils import nms, after_nms
    out_dir = tmp_path / 'out'
    cmd = [sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1', '--steps', '6', '--warmup', '2', '--cfg', 'res50_coco',
           '--img_size', '256', '--dump-outputs', str(out_dir)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert {'metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'} <= set(d)
    assert not {'extra', 'roofline', 'cpu_baseline'} & set(d)
    assert d['steps'] == 6 and d['warmup'] == 2 and d['unit'] == 'img/s' and d['higher_is_better'] and d['dtype'] == 'f32'
    assert d['value'] > 0 and abs(d['value'] * d['ms_per_step'] / 1e3 - 1.0) < 0.01          # one image per step

    files = {f[:-4]: np.load(out_dir / f) for f in os.listdir(out_dir)}
    assert {'class_pred', 'box_pred', 'coef_pred', 'proto_out', 'detections_per_image', 'ids', 'scores', 'boxes_px', 'masks_sample',
            'masks_rowsum'} == set(files)
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    n = int(files['detections_per_image'].sum())
    assert n > 0 and files['ids'].shape == (n,) and files['masks_rowsum'].shape == (n,)

    # the same seeded inputs in this process, one request at a time
    dev = torch.device('cuda', 0)
    net, cfg = bench.build_net('res50_coco', 256, dev)
    w = bench.Workload(net, cfg, 1, 256, dev, with_post=True, inflight=1)
    r = nms(*w.head, w.anchors, cfg)
    ids, scores, boxes, masks = after_nms(r[0], r[1], r[2], r[3], r[4], 480, 640, cfg)
    assert np.array_equal(files['ids'], ids.cpu().double().numpy())
    assert np.array_equal(files['scores'], scores.cpu().numpy())
    assert np.array_equal(files['boxes_px'], boxes.cpu().double().numpy())
    assert np.array_equal(files['masks_rowsum'], masks.reshape(n, -1).sum(dim=1, dtype=torch.float64).cpu().numpy())
    w.engine.run(w.img)
    for name, t in zip(('class_pred', 'box_pred', 'coef_pred', 'proto_out'), w.engine.outputs()):
        np.testing.assert_allclose(files[name], t.cpu().numpy(), rtol=1e-4, atol=1e-5, err_msg=name)
