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
    from yolact_minimal_amd import conv_launch, plan_transfer
    from yolact_minimal_amd.conv_plan import ConvPlan
    _, M, N, C, k, s, nseg, res, _, _ = plan_transfer.parse_key(key)
    ho = max(h for h in range(1, 1200) if M % (h * h) == 0)
    cuts = [0, N] if nseg == 1 else [0, N - N // 3 - 12, N - N // 3, N][:nseg + 1]
    segs = [(n0, n1, 0x2000, ho * ho * (n1 - n0), n1 - n0, 0) for n0, n1 in zip(cuts, cuts[1:])]
    d = conv_launch.conv_desc(M // (ho * ho), ho * s, ho * s, C, N, k, k, s, k // 2, ho, ho, -(-(k * k * C) // 32) * 32, segs)
    d.inp = d.weight = 0x1000
    d.residual = 0x1000 if res else None
    ConvPlan.from_row(row).apply(d)
    d.tile_counters = 0x3000
    return d


def test_planner_accepts_every_forward_row_of_the_committed_table():
    """`ym_conv2d_workspace_bytes` / `ym_conv2d_tile_counters` run on the host: every inference row of the table (latency and
    throughput choices) must be a plan the C-ABI accepts for its shape -- a stale or mistyped row fails here, not on the GPU box.
    Rows for the segmented head (3 outputs) and the pyramid launch (`_L<n>`) are planned by the engine with their real segment
    tables and are covered by the GPU forward tests."""
    import ctypes
    from yolact_minimal_amd import engine as E, hip, plan_transfer
    from yolact_minimal_amd.conv_plan import ConvPlan
    lib = hip.lib()
    table = json.load(open(E.TUNED_PATH))
    checked = wave = split = 0
    for key, row in table.items():
        f = plan_transfer.parse_key(key)
        if f.prefix or f.nseg != 1 or f.levels or f.suffix not in ('', '_tp') or f.C == 4:     # (the stem on the 4-channel image: its own mode)
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


def _launch_desc(g, plan, mma):
    """The descriptor tests/test_gpu_forward_fullsize.py (`Launch`) builds for a row, with placeholder pointers (16-byte aligned where
    its tensors are; the planner looks at nullness and alignment only): folded BatchNorm + ReLU, for an `_st` row the raw output + its
    BatchNorm sums, for the three-segment head a bias and tanh on the third segment; arrival counters always."""
    from yolact_minimal_amd import conv_launch
    b, N, C, k = g.batch, g.N, g.C, g.k
    sides = [(s, s) for s in g.levels] if g.levels else [(g.h, g.ho)]
    pix = sum(ho * ho for _, ho in sides)
    if g.nseg == 1:
        segs = [(0, N, 0x10000, 0 if g.levels else g.ho * g.ho * N, N, 0 if g.suffix == '_st' else 1)]
    else:
        cuts, na, n_total = (0, 243, 255, 351), 3, 37 + pix * 3 + 29
        segs = [(n0, n1, 0x10000 * (i + 1) + 37 * ((n1 - n0) // na) * 4, n_total * ((n1 - n0) // na), n1 - n0, 2 * (i == 2))
                for i, (n0, n1) in enumerate(zip(cuts, cuts[1:]))]
    d = conv_launch.conv_desc(b, sides[0][0], sides[0][0], C, N, k, k, g.stride, g.pad, sides[0][1], sides[0][1], (k * k * C + 31) // 32 * 32,
                              segs, levels=sides if g.levels else None)
    d.inp, d.weight, d.tile_counters = 0x1000, 0x2000, 0x3000
    d.scale = 0x4000 if g.nseg == 1 and g.suffix != '_st' else None
    d.shift = 0x5000 if g.suffix != '_st' else None
    d.residual = 0x6000 if g.residual else None
    if g.suffix == '_st':
        d.bn_sum, d.bn_sumsq = 0x7000, 0x8000
    plan.apply(d)
    d.mma = mma
    return d


def test_every_forward_key_of_the_committed_table_resolves_to_a_layer():
    """tests/conv_geometry.py, the geometry rule of tests/test_gpu_forward_fullsize.py: every forward key of the table is a layer of
    some model at an image size that is a multiple of 32 from 128 to 864 and a batch of 1 / 2 / 4 / 8 / 16; strided keys get a
    consistent input side, `_L5` keys five levels; and the library runs every row of the table as the row says -- the plan
    ym_conv2d_effective_plan reports for the row's launch is the requested one -- but for the rows of conv_geometry.KNOWN_FALLBACKS,
    which resolve to exactly the plan listed there.  A new row for a size outside the rule, or one that names a kernel variant its
    shape does not have, fails here, before anyone needs a GPU."""
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
        CG.check_effective(g, table[key], plan, mma, _launch_desc(g, plan, mma))
    assert pyramids >= 30 and set(CG.KNOWN_FALLBACKS) <= set(keys)
    # the rule refuses what it should: a size that is no multiple of 32, a side no chain has, a pyramid of another depth
    assert CG.resolve('M10201_N256_C256_k3_s1_seg1_r0') is None                 # 101 x 101: a side of 808 px, no multiple of 32
    assert CG.resolve('M10000_N256_C256_k3_s1_seg1_r0')[-5:] == (1, 800, 100, 100, None)
    assert CG.resolve('M1156_N256_C256_k3_s2_seg1_r0')[-5:] == (1, 544, 68, 34, None)
    assert CG._input_side(544, 9, 3, 2, 256) == (17, 1) and CG._input_side(544, 9, 3, 2, 4) is None      # (an odd input side)
    assert CG.resolve('M1364_N256_C256_k3_s1_seg1_r0_L4') is None
    assert CG.resolve('T_M1156_N256_C256_k3_s1') is None


SIDES = (8, 10, 13, 16, 20, 23, 26, 32, 40, 46, 50, 64, 80, 92, 100, 128, 160, 184, 200)    # as in test_plan_transfer.py
POLICY = {      # configuration -> (cases, sha256 of the canonical result list), recorded at the commit before conv_launch.py existed
    'infer latency mma0 nearest=1': (2214, '2a20ec2c7ed65fa824cdbdc2573632d254d0eedd5630daa31a7c9f50aafa68d6'),
    'infer latency mma0 nearest=only': (2214, '971d267760c8cfdc3093cccd3732cfa70f099967137fa0beeeb81788e5e3c6c8'),
    'infer latency mma0 nearest=0': (2214, 'e2bf2fd0e223229345a81e66c1b70e115a1d62477305949c0b584c22eaea0a8e'),
    'infer latency mma3 nearest=1': (2214, '1342834748066fdbb083b62327d978fd875b0c65121d62761d1cf0e134e63695'),
    'infer latency mma3 nearest=only': (2214, 'a6c7c80b1d143766ff6faee289ddc478693e26505476926e054b7b91272e957a'),
    'infer latency mma3 nearest=0': (2214, 'b10a54f175c372a2696238d70778520b1e98bfd749228ff86caddbc0d036d752'),
    'infer latency mma6 nearest=1': (2214, 'bd03dead7e4191f431875a71c301987b1814f5cf5b84a1f59ed658c67fa9409f'),
    'infer latency mma6 nearest=only': (2214, 'e6852a2666dc5c55e67fc6a0b856b0e82980ba545002195bec671d5b265ddec7'),
    'infer latency mma6 nearest=0': (2214, '45f0f7c5eeb63f26fb9238a979bc3baee0a74e54b5dcc6162f98fd1f44f981ef'),
    'infer throughput mma0 nearest=1': (2214, 'f59c6a11c74b8f9c5bccde3725f6ef6dda21d4c578bdd6013e63f60de6c32d18'),
    'infer throughput mma0 nearest=only': (2214, '971d267760c8cfdc3093cccd3732cfa70f099967137fa0beeeb81788e5e3c6c8'),
    'infer throughput mma0 nearest=0': (2214, '6150a061bf1c34fa84a057bea8267cedaa2ce70eeda63a6256649e217c81e656'),
    'infer throughput mma3 nearest=1': (2214, '1342834748066fdbb083b62327d978fd875b0c65121d62761d1cf0e134e63695'),
    'infer throughput mma3 nearest=only': (2214, 'a6c7c80b1d143766ff6faee289ddc478693e26505476926e054b7b91272e957a'),
    'infer throughput mma3 nearest=0': (2214, 'b10a54f175c372a2696238d70778520b1e98bfd749228ff86caddbc0d036d752'),
    'infer throughput mma6 nearest=1': (2214, '02039c8ec571aa7926fd3200999231f016566b3f1b7511c87d60378037a3af3c'),
    'infer throughput mma6 nearest=only': (2214, 'e6852a2666dc5c55e67fc6a0b856b0e82980ba545002195bec671d5b265ddec7'),
    'infer throughput mma6 nearest=0': (2214, '3a777ef16996e01870119a81ec97dfd879409c189aea3c51ab027d65b8fadae3'),
    'infer latency mma3 nearest=1 no_tuned': (2214, 'a350180249fa5ddbd8c65f25412be03559ac38d268ae90d7c2e6064065dfd828'),
    'train mma0 nearest=1': (6226, 'd926dc18df4c5772cbc5295f1185a82ead41dfe66dc6a1d076bb82f249017004'),
    'train mma0 nearest=only': (6226, '1e120195359da1c5d8958fa97ea223b47be527f4cb34af87f90970985dd07bb6'),
    'train mma0 nearest=0': (6226, '2065c0bd4973668142cbf8d6dfd158553c76769324861a212cb9e648dccbbc63'),
    'train mma3 nearest=1': (6226, '49a5f5ef8f05cd6c0336e8139db55067df465c2fc9db574f09de26c814324892'),
    'train mma3 nearest=only': (6226, '6a88a180a9fe0e88b86fff77c37c25ddeb28382cd7c652c1ea72fac8c7a54b07'),
    'train mma3 nearest=0': (6226, 'ebeb7ccc1e3b9780bdba7a884c21f0d9f2a958ef9bef9c5bcd2f46d118207777'),
    'train mma0 nearest=1 force=43': (6226, '6ae48d0058a1e1236bbfef52f0987c67a52a7c0e260bd442253af70c1fc35a88'),
}


def test_plan_policy_is_what_the_engines_did_before_it_moved(monkeypatch):
    """conv_launch.py over every shape of the committed table and the same shapes at M = side^2 (shapes without a row), per build
    mode, matrix pipe, transfer mode, YM_NO_TUNED and YM_FORCE_STAGES: count and SHA-256 of [key, the eight plan fields, mma,
    source] (training: [key, stats, plan fields, mma]; weight gradient: [key, msplit, lds_buffers]).  POLICY was recorded by walking
    the same cases through _Conv.bind / apply_mma / _bind_pyramid (fake tensors) and _configure_conv / _configure_wgrad (bare
    descriptors built from the key) of the commit before this module existed, reading the plan back from the descriptor."""
    import hashlib
    from yolact_minimal_amd import conv_launch as CL, engine as E, plan_transfer as PT
    from yolact_minimal_amd.conv_plan import ConvPlan
    for v in ('YM_FORCE_STAGES', 'YM_FORCE_GRID'):
        monkeypatch.delenv(v, raising=False)
    table = json.load(open(E.TUNED_PATH))
    keys = [PT.parse_key(k) for k in table]

    def shifted(shapes):
        return sorted(set(shapes) | {(side * side,) + sh[1:] for sh in shapes for side in SIDES})

    def nkt(C, k):
        return -(-(k * k * C) // 32)

    def digest(rows):
        return len(rows), hashlib.sha256(json.dumps(rows, separators=(',', ':')).encode()).hexdigest()

    got = {}
    cases = shifted({f[1:9] for f in keys if f.prefix == ''})
    for mode, mma, near, no_tuned in [(m, p, n, False) for m in ('latency', 'throughput') for p in (0, 3, 6) for n in ('1', 'only', '0')] + \
            [('latency', 3, '1', True)]:
        monkeypatch.setenv('YM_TUNED_NEAREST', near)
        rows = []
        for M, N, C, k, s, nseg, r, lev in cases:
            key = PT.forward_key(M, N, C, k, s, nseg, r, lev)
            plan, pipe, source, _ = CL.infer_plan(table, key, (M, N, nkt(C, k), nseg), mode, mma, C % 32 == 0 and not lev,
                                                  no_tuned=no_tuned, pyramid=bool(lev))
            rows.append([key, *plan, pipe, source])
        got[f'infer {mode} mma{mma} nearest={near}' + (' no_tuned' if no_tuned else '')] = digest(rows)
    fwd = shifted({f[1:6] + (f.residual,) for f in keys if f.prefix == '' and f.nseg == 1 and not f.levels})
    dgrad, wgrad = (shifted({f[1:6] for f in keys if f.prefix == pre}) for pre in ('T_', 'W_'))
    for mma, near, force in [(p, n, '') for p in (0, 3) for n in ('1', 'only', '0')] + [(0, '1', '43')]:
        monkeypatch.setenv('YM_TUNED_NEAREST', near)
        monkeypatch.setenv('YM_FORCE_STAGES', force)
        rows = []
        for key, M, N, C, k, dg in [(PT.forward_key(M, N, C, k, s, 1, r), M, N, C, k, False) for M, N, C, k, s, r in fwd] + \
                [(PT.dgrad_key(*c), *c[:4], True) for c in dgrad]:
            for stats in ((False,) if dg else (False, True)):
                plan = CL.train_plan(table, key, (M, N, nkt(C, k), 1), stats)
                plan, pipe = CL.train_overrides(plan or ConvPlan(), table, key, mma, C % 32 == 0)
                rows.append([key, stats, *plan, pipe])
        rows += [[key, *(CL.wgrad_plan(table, key) or (0, 0))] for key in (PT.wgrad_key(*c) for c in wgrad)]
        got[f'train mma{mma} nearest={near}' + (f' force={force}' if force else '')] = digest(rows)
    assert got == POLICY, {k: v for k, v in got.items() if v != POLICY.get(k)}
    # the configurations tell the policy's branches apart
    assert all(n > 1000 for n, _ in POLICY.values())
    for a, b in (('infer latency mma0 nearest=1', 'infer throughput mma0 nearest=1'), ('infer latency mma0 nearest=1', 'infer latency mma3 nearest=1'),
                 ('infer latency mma0 nearest=1', 'infer latency mma0 nearest=only'), ('train mma0 nearest=1', 'train mma3 nearest=1')):
        assert POLICY[a][1] != POLICY[b][1], (a, b)
