"""`ym_greedy_nms_batch_workspace_bytes` without a GPU: it answers on the host, refuses what `check_cfg` refuses, is linear in the
batch size, and for one image equals `ym_nms_workspace_bytes`, the one size that serves both single-image entries."""
import ctypes

import pytest


def _cfg(n=18525, c=81, top_k=200, max_det=100):
    from yolact_minimal_amd import hip
    return hip.NmsCfg(n, c, 32, top_k, max_det, 0.05, 0.5, 544.0)


def _bytes(cfg, batch):
    from yolact_minimal_amd import hip
    return hip.lib().ym_greedy_nms_batch_workspace_bytes(ctypes.byref(cfg), batch)


def test_zero_for_a_bad_batch_or_cfg():
    from yolact_minimal_amd import hip
    assert _bytes(_cfg(), 1) > 0
    assert _bytes(_cfg(), 0) == 0 and _bytes(_cfg(), -3) == 0
    for bad in (_cfg(n=0), _cfg(c=1), _cfg(c=257), _cfg(top_k=257), _cfg(max_det=129), _cfg(max_det=0), _cfg(n=1 << 24, c=256)):
        assert _bytes(bad, 1) == 0
        assert hip.lib().ym_nms_workspace_bytes(ctypes.byref(bad)) == 0


@pytest.mark.parametrize('n,c', [(18525, 81), (1023, 81), (4096, 3), (4097, 3), (26520, 2)])
def test_linear_in_the_batch(n, c):
    one = _bytes(_cfg(n, c), 1)
    assert one > 0 and one % 256 == 0
    for batch in (2, 3, 8, 65535):
        assert _bytes(_cfg(n, c), batch) == batch * one


@pytest.mark.parametrize('n,c', [(18525, 81), (1023, 81), (4096, 3), (4097, 3), (26520, 2)])
def test_the_single_image_size_still_fits_the_fast_entry(n, c):
    from yolact_minimal_amd import hip
    cfg = _cfg(n, c)
    assert hip.lib().ym_nms_workspace_bytes(ctypes.byref(cfg)) >= hip.lib().ym_nms_batch_workspace_bytes(ctypes.byref(cfg), 1) > 0


def test_the_single_image_greedy_workspace_is_the_batch_of_one():
    from yolact_minimal_amd import hip
    cfg = _cfg()
    old = hip.lib().ym_nms_workspace_bytes(ctypes.byref(cfg))
    new = _bytes(cfg, 1)
    assert 0 < new == old
    # the floor the header states: stage A + the candidate lists (4 bytes) + one kept byte per (class, anchor); the order by rank
    # (4 more bytes) exists only where a class can outgrow what the kernel stages in LDS (N > 4096)
    stage_a = hip.lib().ym_nms_batch_workspace_bytes(ctypes.byref(cfg), 1)
    cn = 80 * 18525
    assert stage_a + 9 * cn <= new < stage_a + 9 * cn + 8 * 256
    small = _cfg(n=1023)
    cn = 80 * 1023
    stage_a = hip.lib().ym_nms_batch_workspace_bytes(ctypes.byref(small), 1)
    assert stage_a + 5 * cn <= _bytes(small, 1) < stage_a + 5 * cn + 8 * 256
