"""CPU: the sweeps behind the tuned table (yolact_minimal_amd/conv_tuning.py): which plans are tried for a shape, in which order, and
how often a candidate is launched while it is timed.  No GPU, no kernel launch, no built library."""
import hashlib
import json
import types

import pytest

SWEEPS = {      # configuration -> (plans, sha256 of [[case, [plan, ...]], ...]), recorded at the commit before conv_tuning.py existed
    'infer mma0': (184996, '60694e2afdd49bf5972f27d0103b28f6b48a608f9aeac6cc24a7ffe3be8616dd'),
    'infer mma3': (82993, 'ee8335975227643d77b0bafeb6a9b75bc23a3932118d664e1c5b7f386e30be32'),
    'infer mma0 cus64': (212454, '345bdf70d465e2a28fbd6d615c95d1bd60a0b57c6cad5f5f126b38f802f5c2f8'),
    'infer mma0 no counters': (141741, '0aa4745d809fe1c54c06072ba959e69aab6a36d64df817b176c3fdf3e6db3d0f'),
    'infer explicit': (838, '0a9ad547797876840e47da5f503043b84894833ca3a6ac90d2928d6c39032031'),
    'train': (80267, '5a31e805efa13258930cd15439880ce564fbccd0e7c058b2c6dce38d366070fd'),
    'wgrad': (7400, '3962cad8c5b31c91ef75c8aa7892c7f94dddb4bb881bc7372d8b19dcc8b1b189'),
}
# (name, M, N, C, k, segments, pyramid levels, act): the stem, the 3-segment head, a pyramid input, a tanh and a ReLU epilogue
EXPLICIT = [('stem', 73984, 64, 4, 7, 1, 0, 1), ('head3', 4624, 351, 256, 3, 3, 0, 1), ('pyramid', 6125, 256, 256, 3, 1, 5, 1),
            ('tanh', 4624, 32, 256, 3, 1, 0, 2), ('relu', 4624, 32, 256, 3, 1, 0, 1)]


def _nkt(C, k):
    return -(-(k * k * C) // 32)


def _digest(rows):
    return sum(len(seq) for _, seq in rows), hashlib.sha256(json.dumps(rows, separators=(',', ':')).encode()).hexdigest()


def _table_keys():
    from yolact_minimal_amd import engine as E, plan_transfer as PT
    return [PT.parse_key(k) for k in json.load(open(E.TUNED_PATH))]


def _infer_seq(M, N, C, k, nseg, levels=0, act=1, counters=True, cus=256, mma=0):
    """What InferEngine.autotune applies for the shape: the baseline, then the module's list."""
    from yolact_minimal_amd import conv_tuning as CT
    from yolact_minimal_amd.conv_plan import ConvPlan
    return [ConvPlan()] + CT.infer_candidates(M, N, _nkt(C, k), nseg, C == 4, counters, act, cus, mma, C % 32 == 0 and not levels)


def _wgrad_cases(keys):
    """(key, M, N, C, k, Cout_real) of every `W_` shape: with Cout_real <= 64 and > 64 where the key allows it (N is Cout padded to 32, so
    that is Cout_real <= 64 exactly for N <= 64)."""
    from yolact_minimal_amd import plan_transfer as PT
    return [(PT.wgrad_key(M, N, C, k, s), M, N, C, k, cr) for M, N, C, k, s in sorted({(f.M, f.N, f.C, f.k, f.stride) for f in keys if f.prefix == 'W_'})
            for cr in sorted({min(N, 64), N}) if -(-cr // 32) * 32 == N]


def test_candidate_lists_are_what_the_engines_swept_before_they_moved():
    """conv_tuning.py's lists over every shape of the committed table: count and SHA-256 of [[case, [plan fields, ...]], ...] per
    configuration.  SWEEPS was recorded by driving the sweeps of the commit before this module existed on the CPU and logging the
    plans they applied / launched: InferEngine.autotune unbound on a namespace holding one fake conv (a bare ConvDesc of the key's
    shape) with torch.cuda.Event / synchronize replaced by stubs whose elapsed_time is constant (no candidate wins, all are tried),
    hip.conv2d_fwd / conv_workspace_bytes stubbed and ConvPlan.apply logged (baseline first); train_engine._configure_conv /
    _configure_wgrad with YM_TUNE_TRAIN=1, an empty table, a one-call timer and hip.conv2d_fwd / ym_conv2d_wgrad logging the
    descriptor's plan.  Inference: every non-pyramid forward shape under the f32 and the split-bf16 pipe, on 64 CUs and without
    arrival counters, plus EXPLICIT; training: every one-segment forward and `T_` shape; weight gradient: every `W_` shape."""
    from yolact_minimal_amd import conv_tuning as CT, plan_transfer as PT
    keys = _table_keys()
    got = {}
    cases = sorted({(f.M, f.N, f.C, f.k, f.stride, f.nseg, f.residual) for f in keys if f.prefix == '' and not f.levels})
    assert len(cases) > 1000
    for name, kw in (('infer mma0', {}), ('infer mma3', dict(mma=3)), ('infer mma0 cus64', dict(cus=64)),
                     ('infer mma0 no counters', dict(counters=False))):
        got[name] = _digest([[PT.forward_key(M, N, C, k, s, nseg, r), _infer_seq(M, N, C, k, nseg, **kw)] for M, N, C, k, s, nseg, r in cases
                             if not (kw.get('mma') and (C == 4 or C % 32))])         # (autotune skips what the split pipe cannot run)
    got['infer explicit'] = _digest([[name, _infer_seq(M, N, C, k, nseg, levels, act)] for name, M, N, C, k, nseg, levels, act in EXPLICIT])
    fwd = sorted({(f.M, f.N, f.C, f.k, f.stride, f.residual) for f in keys if f.prefix == '' and f.nseg == 1 and not f.levels})
    dgrad = sorted({(f.M, f.N, f.C, f.k, f.stride) for f in keys if f.prefix == 'T_'})
    got['train'] = _digest([[key, CT.train_conv_candidates(M, N, _nkt(C, k))] for key, M, N, C, k in
                            [(PT.forward_key(M, N, C, k, s, 1, r), M, N, C, k) for M, N, C, k, s, r in fwd] +
                            [(PT.dgrad_key(*c), *c[:4]) for c in dgrad]])
    got['wgrad'] = _digest([[f'{key} real{cr}', CT.wgrad_candidates(N, cr, k * k * C)] for key, M, N, C, k, cr in _wgrad_cases(keys)])
    assert got == SWEEPS, {k: v for k, v in got.items() if v != SWEEPS.get(k)}
    # the configurations tell the branches apart
    assert all(n > 1000 for name, (n, _) in SWEEPS.items() if name != 'infer explicit')
    assert len({SWEEPS[name][1] for name in ('infer mma0', 'infer mma3', 'infer mma0 cus64', 'infer mma0 no counters')}) == 4
    seqs = {name: _infer_seq(M, N, C, k, nseg, levels, act) for name, M, N, C, k, nseg, levels, act in EXPLICIT}
    assert {(p.tile_m, p.tile_n) for p in seqs['stem'][1:]} == {(128, 64)} and {p.stages for p in seqs['stem']} <= {0, 2, 3}
    assert any(p.persistent for p in seqs['relu']) and not any(p.persistent for p in seqs['tanh'] + seqs['head3'])
    assert any(p.tail_tiles for p in _infer_seq(4624, 351, 256, 3, 1)) and not any(p.tail_tiles for p in seqs['head3'])
    assert any(p.wave_dma for p in seqs['head3']) and any(p.persistent for p in seqs['pyramid']) and not any(p.wave_dma for p in seqs['pyramid'])
    reals = {cr <= 64 for *_, cr in _wgrad_cases(keys)}
    assert reals == {True, False}                                                     # both sides of the Cout_real <= 64 restriction


def test_the_tools_take_the_lists_they_had():
    """tools/tune_ws.py and train_layer_table.py: the weight-stationary tiles x rings; tools/tune_wave.py: the DMA-ring list with
    ring depths 22-24 (24 for 32x32 only), no waves-per-workgroup variants and no tail; tools/tune_forward.py: the engine's list,
    whose tail split ends at TILE_COUNTERS tiles (beyond it hip.conv2d_fwd launches without arrival counters, so without a tail)."""
    from yolact_minimal_amd import conv_tuning as CT, hip
    from yolact_minimal_amd.conv_plan import ConvPlan
    for cin in (32, 64, 96, 128, 256):
        want = [ConvPlan(tm, tn, 1, 0, st) for tm, tn in ((64, 256), (128, 128), (256, 64)) if not tn * cin * 4 > 64 * 1024 for st in (52, 53, 54)]
        assert CT.weight_stationary_candidates(cin) == want and len(want) == (9 if cin <= 64 else 6 if cin <= 128 else 3)
    for nkt in (1, 2, 3, 8, 72):
        want = [ConvPlan(tm, tn, 1, kwv, stg) for tm, tn in ((32, 32), (64, 32), (32, 64)) for kwv in (1, 2, 4) if kwv <= nkt
                for stg in (22, 23, 24) if not (stg == 24 and (tm, tn) != (32, 32))]
        assert CT.wave_dma_candidates(4624, 256, nkt, tail=False, rings=(22, 23, 24), waves_per_wg=()) == want
    for M, tails in ((256 * 32, 0), (18496, 3), (hip.TILE_COUNTERS * 32, 3), (hip.TILE_COUNTERS * 32 + 1, 0)):
        got = CT.wave_dma_candidates(M, 32, 72)
        assert sum(p.tail_tiles > 0 for p in got) == tails and got[:len(got) - tails] == CT.wave_dma_candidates(M, 32, 72, tail=False)
        assert all(p[:5] == (32, 32, 1, 4, 22) and p.tail_tiles == (-(-M // 32) % 256 or 256) for p in got if p.tail_tiles)


class _Event:
    def __init__(self, enable_timing=False):
        pass

    def record(self, *a):
        pass

    def elapsed_time(self, other):
        return 1.0                                   # ms, for every candidate: none beats the baseline by the margin, all are tried


@pytest.fixture
def stubs(monkeypatch):
    """The device out of the way: constant events, counted synchronisations, hip.conv2d_fwd logging the descriptor's plan."""
    import torch
    from yolact_minimal_amd import conv_tuning as CT, hip, train_engine as T
    from yolact_minimal_amd.conv_plan import ConvPlan
    log = types.SimpleNamespace(applied=[], launched=[], wgrad=[], syncs=0, remembered={})
    monkeypatch.setattr(torch.cuda, 'Event', _Event)
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a: setattr(log, 'syncs', log.syncs + 1))
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: 0)
    monkeypatch.setattr(hip, 'conv_workspace_bytes', lambda d: 0)
    monkeypatch.setattr(hip, 'conv2d_fwd', lambda d, ws=None: log.launched.append(ConvPlan.of(d)))
    apply = ConvPlan.apply
    monkeypatch.setattr(ConvPlan, 'apply', lambda self, d: (log.applied.append(self), apply(self, d))[1])

    class Lib:
        def ym_conv2d_wgrad_workspace_bytes(self, ref):
            return 1

        def ym_conv2d_wgrad(self, ref, ws, nbytes, stream):
            log.wgrad.append((ref._obj.msplit, ref._obj.lds_buffers))
            return 0

    monkeypatch.setattr(hip, 'lib', lambda: Lib())
    monkeypatch.setattr(hip, 'stream_ptr', lambda: None)
    monkeypatch.setattr(T, 'scratch', lambda dev, n: torch.empty(n, dtype=torch.uint8))
    monkeypatch.setattr(T, '_tile_counters', lambda dev: 0x3000)
    monkeypatch.setattr(T, '_table', lambda: {})
    monkeypatch.setattr(CT, 'remember', lambda key, row: log.remembered.__setitem__(key, row))
    monkeypatch.setenv('YM_AUTOTUNE', '1')
    for v in ('YM_FORCE_STAGES', 'YM_TRAIN_MMA'):
        monkeypatch.delenv(v, raising=False)
    return log


def _fake_conv(M, N, C, k, nseg, levels=0, act=1):
    from yolact_minimal_amd import hip
    d = hip.ConvDesc()
    d.B, d.Ho, d.Wo, d.Cout, d.Cin, d.k_pad, d.nseg, d.nlevels = 1, M, 1, N, C, _nkt(C, k) * 32, nseg, levels
    if levels:
        d.Ho = 0
        for l in range(levels):
            d.level_h[l], d.level_w[l] = (M - (levels - 1), 1) if l == 0 else (1, 1)
    d.tile_counters = 0x3000
    return types.SimpleNamespace(desc=d, stem=C == 4, act=act, sig=f'M{M}_N{N}_C{C}_k{k}', plan=None, mma=0)


def test_the_engines_time_the_lists_of_the_module_with_their_own_counts(stubs):
    """InferEngine.autotune applies and launches the baseline ConvPlan() and then conv_tuning.infer_candidates of the shape, each 2
    warm-up + 3 x `iters` times with a synchronisation before and after each repetition; train_engine._configure_conv launches
    conv_tuning.train_conv_candidates and _configure_wgrad conv_tuning.wgrad_candidates, each 2 warm-up + 2 x 5 times with a
    synchronisation after each repetition only (the counts of the timers these sweeps had before they shared one).  Five shapes of
    different families: the stem, a tail split on the workgroup and the wave kernel, a tiny layer, the head, a pyramid input."""
    from yolact_minimal_amd import conv_tuning as CT, engine as E, hip, train_engine as T
    from yolact_minimal_amd.conv_plan import ConvPlan, WgradPlan
    iters = 4
    for name, M, N, C, k, nseg, levels, act in EXPLICIT[:3] + [('tail', 18496, 256, 256, 1, 1, 0, 1), ('tiny', 25, 256, 256, 3, 1, 0, 1)]:
        for mma in (0, 3):
            if mma and (C == 4 or levels):
                continue
            c = _fake_conv(M, N, C, k, nseg, levels, act)
            del stubs.applied[:], stubs.launched[:]
            stubs.syncs = 0
            rows = E.InferEngine.autotune(types.SimpleNamespace(convs=[c], device='cpu', retune=lambda: None), iters=iters, mma=mma)
            want = _infer_seq(M, N, C, k, nseg, levels, act, mma=mma)
            assert want[0] == ConvPlan() and len(want) > 5 and stubs.applied == want, (name, mma)
            assert stubs.launched == [p for p in want for _ in range(2 + 3 * iters)], (name, mma)
            assert stubs.syncs == 6 * len(want), (name, mma)
            assert rows == {c.sig + ('_mma3' if mma else ''): ConvPlan().to_row()} and c.plan == ConvPlan()
        if name == 'tail':
            assert any(p.tail_tiles and not p.wave for p in want) and any(p.tail_tiles and p.wave_dma for p in _infer_seq(M, N, C, k, nseg))
        if C == 4 or levels:
            continue                                                                   # (training configures neither through a sweep)
        d = _fake_conv(M, N, C, k, 1).desc
        d.tile_counters = None
        del stubs.applied[:], stubs.launched[:]
        stubs.syncs = 0
        T._configure_conv(d, 'key')
        want = CT.train_conv_candidates(M, N, _nkt(C, k))
        assert want[0] == ConvPlan() and stubs.launched == [p for p in want for _ in range(2 + 2 * 5)], name
        assert stubs.applied == want + [ConvPlan()] and stubs.syncs == 2 * len(want) and d.tile_counters == 0x3000, name
        assert stubs.remembered.pop('key') == ConvPlan().to_row()
        for cout_real in (N, min(N, 64)):
            w = hip.WgradDesc()
            w.Cout, w.Cout_real, w.KH, w.KW, w.Cin = -(-cout_real // 32) * 32, cout_real, k, k, C
            del stubs.wgrad[:]
            stubs.syncs = 0
            T._configure_wgrad(w, 'wkey')
            want = CT.wgrad_candidates(w.Cout, cout_real, k * k * C)
            assert len(want) > 30 and stubs.wgrad == [tuple(p) for p in want for _ in range(12)] and stubs.syncs == 2 * len(want), name
            assert ({p.lds_buffers for p in want} == {1, 2, 22}) == (cout_real <= 64)
            assert stubs.remembered.pop('wkey') == list(WgradPlan(0, 2)) and (w.msplit, w.lds_buffers) == (0, 2)     # (all tie: the first stays)


def test_time_launch_returns_microseconds_per_call(stubs):
    from yolact_minimal_amd import conv_tuning as CT
    calls = []
    assert CT.time_launch(lambda: calls.append(1), iters=8, reps=3, warmup=2, sync_each_rep=True) == 1000 / 8
    assert len(calls) == 2 + 3 * 8 and stubs.syncs == 6
    joins = []
    assert CT.time_launch(lambda: calls.append(1), iters=5, reps=2, warmup=0, join=lambda: joins.append(len(calls))) == 200.0
    assert len(calls) == 26 + 10 and stubs.syncs == 6 + 2 and joins == [31, 36]          # (join: after the calls of each repetition)
    # fastest(): a candidate replaces the incumbent only where it beats it by the margin; one that cannot run is passed over
    times = {'a': 100.0, 'b': 99.0, 'c': None, 'd': 97.0, 'e': 96.0}
    assert CT.fastest('abcde', times.get, 100.0, 'base') == (97.0, 'd')
    assert CT.fastest('abc', times.get, 100.0, 'base') == (100.0, 'base') and CT.fastest('ab', times.get)[1] == 'a'
