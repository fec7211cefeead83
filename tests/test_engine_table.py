"""CPU: the tuned-table plumbing of the inference engine (no GPU, no kernel launch)."""
import json
import os

import pytest


def test_throughput_mode_reads_tp_entries_first(monkeypatch):
    """`InferEngine(mode='throughput')` (the slots of a RequestPipeline with several requests in flight) reads `<sig>_tp` before
    `<sig>`; the default mode never sees the `_tp` rows."""
    from yolact_minimal_amd import engine as E
    table = {'M1_N1_C32_k1_s1_seg1_r0': [64, 64, 3, 0, 2, 0, 0], 'M1_N1_C32_k1_s1_seg1_r0_tp': [32, 32, 1, 4, 22, 0, 0],
             'M2_N1_C32_k1_s1_seg1_r0': [128, 64, 1, 0, 22, 8, 3]}
    monkeypatch.setattr(E, '_tuned', table)
    monkeypatch.setattr(E, '_build_mode', ['latency'])
    assert E._entry('M1_N1_C32_k1_s1_seg1_r0') == [64, 64, 3, 0, 2, 0, 0]
    monkeypatch.setattr(E, '_build_mode', ['throughput'])
    assert E._entry('M1_N1_C32_k1_s1_seg1_r0') == [32, 32, 1, 4, 22, 0, 0]
    assert E._entry('M2_N1_C32_k1_s1_seg1_r0') == [128, 64, 1, 0, 22, 8, 3]          # no _tp row: the latency choice
    assert E._entry('unknown') is None


def test_conv_plan_from_row_validates_grid_wgs():
    from yolact_minimal_amd.conv_plan import ConvPlan

    def grid(row):
        return ConvPlan.from_row(row).grid_wgs

    assert grid([64, 64, 1, 0, 43, 0, 0, 768]) == 768 and grid([32, 32, 1, 1, 22, 0, 0, 1]) == 1
    assert grid([64, 64, 1, 0, 2, 0, 0]) == 0
    with pytest.raises(ValueError):
        grid([64, 64, 1, 0, 43, 0, 0, 12.5])           # an old autotune detail row: a timing where grid_wgs belongs
    with pytest.raises(ValueError):
        grid([32, 32, 1, 4, 22, 0, 0, 768])            # a persistent-kernel grid on a wave-DMA row (there: waves per workgroup)
    with pytest.raises(ValueError):
        grid([32, 32, 1, 4, 22, 40, 4, 2])             # the wave kernel's tail split needs four-wave workgroups
    assert grid([32, 32, 1, 4, 22, 40, 4, 4]) == 4 and grid([32, 32, 1, 2, 23, 0, 0, 2]) == 2


def test_committed_table_is_well_formed():
    """Every row of yolact_minimal_amd/tuned_gfx950.json: conv rows have 7 or 8 integer fields (tile, ksplit, kwaves, stages, tail,
    [grid_wgs / waves per workgroup]), wave-kernel rows with DMA rings name a tile the kernel has, `_tp` rows shadow an existing
    shape, weight-gradient rows have two fields; every row reads back as the plan it names (conv_plan.py).  Pyramid rows (`_L<n>`)
    name no persistent or weight-stationary kernel: those are the stages the pyramid planner reads."""
    from yolact_minimal_amd import engine as E
    from yolact_minimal_amd.conv_plan import ConvPlan, WgradPlan
    table = json.load(open(E.TUNED_PATH))
    assert len(table) > 400
    for key, row in table.items():
        assert all(isinstance(v, int) and not isinstance(v, bool) for v in row), (key, row)
        if key.startswith('W_'):
            assert len(row) == 2 and WgradPlan.from_row(row).to_row() == row, (key, row)
            continue
        assert len(row) in (5, 7, 8), (key, row)
        p = ConvPlan.from_row(row)
        assert p.to_row() == row, (key, row)
        if '_L' in key:
            assert not (p.persistent or p.weight_stationary), (key, row)
        if len(row) >= 7 and p.wave_dma:                                              # conv_wdma_f32
            assert (p.tile_m, p.tile_n) in ((32, 32), (64, 32), (32, 64)) and p.kwaves in (1, 2, 4), (key, row)
            wpb = p.grid_wgs
            assert wpb in (0, 1, 2, 4) and (wpb == 0 or wpb >= p.kwaves), (key, row)
            # (K waves, ring depth, waves per workgroup) must be an instantiation csrc/conv_wave.hip builds (dispatch_dma)
            built = {(kw, ns, 4) for kw in (1, 2, 4) for ns in (2, 3)} | {(1, 2, 1), (1, 3, 1), (1, 2, 2), (1, 3, 2), (2, 2, 2), (2, 3, 2)}
            if (p.tile_m, p.tile_n) == (32, 32):
                built |= {(1, 4, 4), (2, 4, 4), (4, 4, 4), (1, 4, 1), (1, 4, 2)}
            assert (p.kwaves, p.ring, wpb or 4) in built, (key, row)
            if p.tail_tiles or p.tail_ksplit:                                        # tail split: 32x32 tile, four K waves, <= 8 slices
                assert (p.tile_m, p.tile_n, p.kwaves) == (32, 32, 4) and 2 <= p.tail_ksplit <= 8 and wpb in (0, 4), (key, row)
        if key.endswith('_tp'):
            assert key[:-3] in table or key[:-3].startswith('M'), key


def test_pipeline_checks_the_hardware_queue_count(monkeypatch):
    from yolact_minimal_amd.pipeline import hw_queues_ok
    monkeypatch.setenv('GPU_MAX_HW_QUEUES', '8')
    assert hw_queues_ok(4) and hw_queues_ok(7) and not hw_queues_ok(8)
    monkeypatch.delenv('GPU_MAX_HW_QUEUES')
    assert hw_queues_ok(3) and not hw_queues_ok(4)              # ROCm's default: 4 hardware queues
    monkeypatch.setenv('GPU_MAX_HW_QUEUES', 'x')
    assert not hw_queues_ok(4)


def _desc_from_key(key, row):
    """A descriptor with the GEMM shape a forward-conv key names (M = B Ho Wo: any factorisation gives the same plan) and the
    row's tiling; pointers are placeholders (the planner never dereferences them)."""
    import re
    from yolact_minimal_amd.conv_plan import ConvPlan
    from yolact_minimal_amd.hip import ConvDesc
    m = re.match(r'M(\d+)_N(\d+)_C(\d+)_k(\d+)_s(\d+)_seg(\d+)_r(\d+)', key)
    M, N, C, k, s, nseg, res = map(int, m.groups())
    ho = max(h for h in range(1, 1200) if M % (h * h) == 0)
    d = ConvDesc()
    d.inp = d.weight = 0x1000
    d.residual = 0x1000 if res else None
    d.B, d.H, d.W, d.Cin, d.Cout = M // (ho * ho), ho * s, ho * s, C, N
    d.KH = d.KW = k
    d.stride, d.pad, d.Ho, d.Wo = s, k // 2, ho, ho
    d.k_pad = -(-(k * k * C) // 32) * 32
    cuts = [0, N] if nseg == 1 else [0, N - N // 3 - 12, N - N // 3, N][:nseg + 1]
    d.nseg = nseg
    for i in range(nseg):
        d.seg[i].n_begin, d.seg[i].n_end = cuts[i], cuts[i + 1]
        d.seg[i].out, d.seg[i].pitch, d.seg[i].batch_stride = 0x2000, cuts[i + 1] - cuts[i], ho * ho * (cuts[i + 1] - cuts[i])
    ConvPlan.from_row(row).apply(d)
    d.tile_counters = 0x3000
    return d


def test_planner_accepts_every_forward_row_of_the_committed_table():
    """`ym_conv2d_workspace_bytes` / `ym_conv2d_tile_counters` run on the host: every inference row of the table (latency and
    throughput choices) must be a plan the C-ABI accepts for its shape -- a stale or mistyped row fails here, not on the GPU box.
    Rows for the segmented head (3 outputs) and the pyramid launch (`_L<n>`) are planned by the engine with their real segment
    tables and are covered by the GPU forward tests."""
    import ctypes
    import re
    from yolact_minimal_amd import engine as E, hip
    from yolact_minimal_amd.conv_plan import ConvPlan
    lib = hip.lib()
    table = json.load(open(E.TUNED_PATH))
    pat = re.compile(r'^M\d+_N\d+_C\d+_k\d+_s\d+_seg1_r[01](_tp)?$')
    checked = wave = split = 0
    for key, row in table.items():
        if not pat.match(key) or '_C4_' in key:                                   # (the 7x7 stem on the 4-channel image: its own mode)
            continue
        d = _desc_from_key(key, row)
        lib.ym_conv2d_workspace_bytes(None)                                        # plants a known message in ym_last_error()
        sentinel = lib.ym_last_error()
        nb = lib.ym_conv2d_workspace_bytes(ctypes.byref(d))
        assert lib.ym_last_error() == sentinel, (key, row, lib.ym_last_error())
        tiles = lib.ym_conv2d_tile_counters(ctypes.byref(d))
        assert 0 <= tiles <= hip.TILE_COUNTERS, (key, row, tiles)
        p = ConvPlan.from_row(row)
        if p.tile_m > 0 and p.ksplit > 0:              # (0 = the planner's own choice) scratch exactly when K slices meet in memory
            tail = p.tail_tiles > 0
            in_workgroup = p.wave                         # kwaves: the K split stays inside the workgroup
            assert (nb > 0) == (tail or (p.ksplit > 1 and not in_workgroup)), (key, row, nb)
        if p.wave_dma:
            assert d.Cin % 32 == 0, (key, row)
            wave += 1
        split += int(nb > 0)
        checked += 1
    assert checked > 150 and wave >= 15 and split > 50, (checked, wave, split)


def test_tuner_rows_reach_the_table_only_through_the_reference_digest_gate(tmp_path):
    """tools/table_gate.py: rows a tuner proposes (`tune_forward.py --inflight N --write` writes `<sig>_tp` rows) are merged into the
    table only after the 544 px reference-digest tests have run green against the CANDIDATE table; a red or missing run leaves
    the table as it was."""
    from tools import table_gate as G
    path = tmp_path / 'table.json'
    base = {'M1156_N256_C1024_k1_s1_seg1_r0': [32, 32, 1, 4, 22, 40, 4]}
    path.write_text(json.dumps(base))
    rows = {'M1156_N256_C1024_k1_s1_seg1_r0_tp': [32, 32, 1, 4, 22, 0, 0]}
    seen, narrowed = [], []

    def red(candidate):
        seen.append(json.load(open(candidate)))
        narrowed.append(os.environ.get(G.KEYS_ENV))
        return 1

    with pytest.raises(G.GateRefused):
        G.merge_rows(rows, str(path), runner=red)
    assert json.loads(path.read_text()) == base                         # untouched
    assert seen[0] == {**base, **rows}                                  # the tests saw the candidate, not the committed table
    assert narrowed == [','.join(sorted(rows))] and G.KEYS_ENV not in os.environ      # ... and the per-row test only the merged keys
    assert not list(tmp_path.parent.glob('tuned_candidate_*'))
    merged = G.merge_rows(rows, str(path), runner=lambda candidate: 0)
    assert merged == {**base, **rows} and json.loads(path.read_text()) == merged
    # the gate's test list names tests that exist, parametrised over both plan modes
    import ast
    src = open(os.path.join(G.REPO, 'tests', 'test_gpu_forward.py')).read()
    names = {n.name for n in ast.walk(ast.parse(src)) if isinstance(n, ast.FunctionDef)}
    rowsrc = open(os.path.join(G.REPO, 'tests', 'test_gpu_forward_fullsize.py')).read()
    in_file = {'tests/test_gpu_forward.py': names,
               'tests/test_gpu_forward_fullsize.py': {n.name for n in ast.walk(ast.parse(rowsrc)) if isinstance(n, ast.FunctionDef)}}
    for t in G.GATE_TESTS:                                              # each in the file its id names
        assert t.split('::')[1] in in_file[t.split('::')[0]], t
    assert sum(t.startswith('tests/test_gpu_forward.py::') for t in G.GATE_TESTS) >= 2         # the digests stay in the gate
    assert "'throughput'" in src
    # every forward row, of any image size, is launched at its own shape against fp64 under the candidate table: the per-row test is
    # part of the gate, reads the table through the engine (YM_TUNED_PATH) and the gate's key list
    assert 'tests/test_gpu_forward_fullsize.py::test_every_tuned_forward_launch_at_full_size' in G.GATE_TESTS
    assert 'tuned_table()' in rowsrc and 'tuned_gfx950.json\'' not in rowsrc and f"KEYS_ENV = '{G.KEYS_ENV}'" in rowsrc
    # and the tuner goes through it
    tool = open(os.path.join(G.REPO, 'tools', 'tune_forward.py')).read()
    assert 'merge_rows' in tool and 'json.dump(table, open(E.TUNED_PATH' not in tool


def test_every_forward_key_of_the_committed_table_resolves_to_a_layer():
    """tests/conv_geometry.py, the geometry rule of tests/test_gpu_forward_fullsize.py: every forward key of the table is a layer of
    some model at an image size that is a multiple of 32 from 128 to 864 and a batch of 1 / 2 / 4 / 8 / 16; strided keys get a
    consistent input side, `_L5` keys five levels; and every row names a kernel variant that exists for its shape (no quiet
    fall-back inside ym_conv2d_fwd).  A new row for a size outside the rule fails here, before anyone needs a GPU."""
    from tests import conv_geometry as CG
    from yolact_minimal_amd import engine as E
    table = json.load(open(E.TUNED_PATH))
    keys = CG.forward_keys(table)
    assert len(keys) > 1000 and all(not k.startswith(('T_', 'W_')) for k in keys)
    assert len(keys) + sum(k.startswith(('T_', 'W_')) for k in table) == len(table)        # nothing is neither
    pyramids = 0
    for key in keys:
        g = CG.resolve(key)
        assert g is not None, f'{key}: no layer of any model / image size / batch has this shape'
        if g.levels:
            pyramids += 1
            assert len(g.levels) == 5 and g.batch * sum(s * s for s in g.levels) == g.M and g.stride == 1, g.describe()
            assert list(g.levels) == CG.resnet_chain(g.size)[3:], g.describe()
        else:
            assert g.batch * g.ho * g.ho == g.M and (g.h + 2 * g.pad - g.k) // g.stride + 1 == g.ho, g.describe()
            if g.stride > 1:
                assert g.h in CG.resnet_chain(g.size) and g.h > g.ho, g.describe()
            if g.C == 4:
                assert g.h == g.size and (g.k, g.stride, g.pad) in ((7, 2, 3), (4, 4, 0)), g.describe()
        assert g.batch in (1, 2, 4, 8, 16) and g.size % 32 == 0 and 128 <= g.size <= 864, g.describe()
        plan, mma = CG.launch_plan(g, table[key])
        assert CG.silent_fallback(g, plan, mma) is None, (g.describe(), table[key], CG.silent_fallback(g, plan, mma))
    assert pyramids >= 30
    # the rule refuses what it should: a size that is no multiple of 32, a side no chain has, a pyramid of another depth
    assert CG.resolve('M10201_N256_C256_k3_s1_seg1_r0') is None                 # 101 x 101: a side of 808 px, no multiple of 32
    assert CG.resolve('M10000_N256_C256_k3_s1_seg1_r0')[-5:] == (1, 800, 100, 100, None)
    assert CG.resolve('M1156_N256_C256_k3_s2_seg1_r0')[-5:] == (1, 544, 68, 34, None)
    assert CG._input_side(544, 9, 3, 2, 256) == (17, 1) and CG._input_side(544, 9, 3, 2, 4) is None      # (an odd input side)
    assert CG.resolve('M1364_N256_C256_k3_s1_seg1_r0_L4') is None
    assert CG.resolve('T_M1156_N256_C256_k3_s1') is None
