"""Host-side pins of the ordered BatchNorm sums (no GPU): the descriptor field sits in what was trailing padding, the new entry points
are declared, bound and exported, and the switches exist where the tools expect them."""
import ctypes
import inspect
import os
import re
import sys

from tests.conftest import REPO

NEW_SYMBOLS = ('ym_conv2d_bn_partial_rows', 'ym_bn_partials_finish', 'ym_unordered_sum_launches', 'ym_bn_train_fwd_workspace_bytes')


def test_bn_ordered_fills_the_trailing_padding_of_the_descriptor():
    from yolact_minimal_amd import hip
    f = hip.ConvDesc
    assert f.bn_ordered.size == 4
    assert f.bn_ordered.offset == f.grid_wgs.offset + f.grid_wgs.size          # right behind grid_wgs
    assert f.bn_ordered.offset + 4 == ctypes.sizeof(f)                          # ... and nothing behind it
    # the size tests/test_abi.py pins (its formula: ... 6 bnb_* pointers, grid_wgs + what was 4 bytes of padding)
    assert ctypes.sizeof(f) == 40 + 13 * 4 + 4 + 3 * 32 + 6 * 4 + 16 + 8 + 44 + 8 + 4 + 4 + 4 + 6 * 8 + 8
    assert hip.lib().ym_sizeof_conv_desc() == ctypes.sizeof(f)
    d = f()
    assert d.bn_ordered == 0                                                    # default: the atomics, as before


def test_header_declares_the_field_behind_grid_wgs():
    text = open(os.path.join(REPO, 'include', 'yolact_hip.h')).read()
    body = re.sub(r'/\*.*?\*/', '', text[:text.index('} ym_conv_desc;')], flags=re.S)
    fields = re.findall(r'\b(\w+)(?:\[\d+\])?;', body)
    assert fields[-2:] == ['grid_wgs', 'bn_ordered']
    assert re.search(r'int32_t\s+bn_ordered;', body)


def test_new_entry_points_are_declared_bound_and_exported():
    from yolact_minimal_amd import hip
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'yolact_hip.h')).read(), flags=re.S)
    lib = hip.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r'\b' + name + r'\s*\(', text), name
        assert name in hip.ABI_SYMBOLS, name
        assert hasattr(lib, name), name


def test_counter_and_workspace_query_answer_on_the_host():
    from yolact_minimal_amd import hip
    L = hip.lib()
    a = L.ym_unordered_sum_launches()
    assert a >= 0 and L.ym_unordered_sum_launches() == a                        # monotonic, and reading it does not move it
    # 16*C for the sums + one [2][C] fp64 row per workgroup of the statistics pass (16 rows of y per row lane, at most 1024)
    assert L.ym_bn_train_fwd_workspace_bytes(338, 64) == 16 * 64 + -(-338 // (16 * 16)) * 16 * 64
    assert L.ym_bn_train_fwd_workspace_bytes(5000, 256) == 16 * 256 + -(-5000 // (4 * 16)) * 16 * 256
    assert L.ym_bn_train_fwd_workspace_bytes(10 ** 7, 256) == 16 * 256 + 1024 * 16 * 256
    assert L.ym_bn_train_fwd_workspace_bytes(5000, 256) == L.ym_bn_train_bwd_workspace_bytes(5000, 256)


def test_switches_exist(monkeypatch):
    from yolact_minimal_amd import train_engine as T
    from yolact_minimal_amd.trainer import Trainer
    assert isinstance(T._DETERMINISTIC, bool)                                   # tools/train_ab.py --set x:_DETERMINISTIC=1 casts by type
    before = T._DETERMINISTIC
    try:
        assert T.set_deterministic(None) is before                              # None: leave it
        assert T.set_deterministic(True) is True and T._DETERMINISTIC is True
        assert T.set_deterministic(False) is False and T._DETERMINISTIC is False
    finally:
        T._DETERMINISTIC = before
    assert inspect.signature(Trainer.__init__).parameters['deterministic'].default is None
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    import overfit_demo
    assert inspect.signature(overfit_demo.run).parameters['deterministic'].default is False
    assert callable(overfit_demo.state_digest)


def test_environment_sets_the_default():
    import subprocess
    code = 'from yolact_minimal_amd import train_engine as T; print(int(T._DETERMINISTIC))'
    for val, want in (('1', '1'), (None, '0')):
        env = {k: v for k, v in os.environ.items() if k != 'YM_DETERMINISTIC'}
        if val is not None:
            env['YM_DETERMINISTIC'] = val
        out = subprocess.run([sys.executable, '-c', code], cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        assert out.stdout.strip().splitlines()[-1] == want
