"""GPU: the split-bf16 convolutions (ym_conv_desc.mma = 3 "bf16x3" / 6 "bf16x6": conv_igemm_f32<.., SPL = 2 | 3>) launched alone
through ym_conv2d_fwd, forward and data gradient, every tile and both register-staging variants, with K split, tail split, residual
add and fused BatchNorm sums -- against host references (tests/split_bf16_ref.py).  YM_TRAIN_MMA=3 sends a training step's forward
and data-gradient convs here; descriptors are built directly (conv_launch.conv_desc, d.mma set by hand), no environment variable,
no descriptor cache.

Every launch (`launch`): output prefilled with NaN and none left, guard bands intact, arrival counters zero afterwards, and one
repeat launch into the re-poisoned buffers bit-identical.

(a) random operands: the whole output against fp64 of the same fp32 operands at the project's per-launch bar 1e-4 * max|ref|, and
    against the fp64 sum of the kept plane products (`emulate`: only fp32 accumulation separates the kernel from it) at 4x the
    error the f32 pipe shows for the same plan and operands (floor 6e-6 * max|ref|, what the f32 families measured at full size).
(b) first-order census: integer operands with two (three) exact planes on one side and one plane on the other, thinned so that every
    partial sum is an fp32 integer: torch.equal with the int64 convolution.  A p1 q0 / p0 q1 / p2 q0 / p0 q2 product lost in one K
    half, one sub-tile, one register set or the last K tile of a slice fails outright.
(c) second-order census on the 1x1 shapes: two planes on both sides, one product per output: bf16x6 and the f32 pipe give x y,
    bf16x3 gives x y - p1x p1y exactly -- the one term it omits, nothing else missing or extra.
(d) fused sums of a launch whose products are split: forward statistics, BatchNorm-backward sums with the saved and with the
    re-derived ReLU mask, atomics and ordered partials + ym_bn_partials_finish, against fp64 sums over the launch's OWN output
    (rtol 1e-5, atol 1e-3 as in test_gpu_deterministic.py); on integer operands those sums are exact and must be equal.

Measured on one MI355X: docs/experiments.md ("Split-bf16 launches against host references").
"""
import ctypes
import functools

import pytest
import torch

from tests import split_bf16_ref as S

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 1024                    # floats before and after the output (a multiple of 4: the vector epilogue needs 16-byte alignment)
PART_GUARD = 3                  # rows behind the ordered partials
FILL = -12345.0
BAR = 1e-4                      # the project's per-launch bar: max|got - ref| <= BAR * max|ref|
EMU_FACTOR, EMU_FLOOR = 4.0, 6e-6

_worst = {}                     # (check, mma, 'fwd' | 'dgrad') -> worst figure


def _note(check, mma, geo, value):
    key = (check, mma, 'dgrad' if geo.transposed else 'fwd')
    _worst[key] = max(_worst.get(key, 0.0), value)


_counters = None


def _tile_counters():
    global _counters
    if _counters is None:
        from yolact_minimal_amd import hip
        _counters = torch.zeros(hip.TILE_COUNTERS, device=DEV, dtype=torch.int32)
    return _counters


def _pack(geo, w):
    """The launch's weight operand from the OIHW fp32 weight on the device."""
    from yolact_minimal_amd import hip
    if not geo.transposed:
        return hip.pack_conv_weight(w, geo.cin, geo.K)
    wd = torch.empty(geo.cin, geo.K, device=DEV)
    hip.check(hip.lib().ym_pack_conv_weight_dgrad(hip.ptr(w.contiguous()), hip.ptr(wd), geo.cout, geo.cin, geo.k, geo.k, geo.cout,
                                                  hip.stream_ptr()), 'ym_pack_conv_weight_dgrad')
    return wd


class Sums:
    """Which per-channel sums ride on the launch.  kind 'fwd': sum y, sum y^2; 'saved' / 'remask': the BatchNorm-backward sums
    sum dz, sum dz * xhat under the ReLU mask read from `out` / re-derived from gamma, beta.  `ordered`: partials + finish."""

    def __init__(self, kind, ordered, y=None, out=None, mean=None, invstd=None, gamma=None, beta=None):
        self.kind, self.ordered = kind, ordered
        self.y, self.out, self.mean, self.invstd, self.gamma, self.beta = y, out, mean, invstd, gamma, beta

    def expected(self, got):
        """fp64 [2][N] over the launch's own output `got` [M][N]."""
        v = got.double()
        if self.kind == 'fwd':
            return torch.stack([v.sum(0), (v * v).sum(0)])
        n = v.shape[1]
        xhat = ((self.y.reshape(-1, n) - self.mean) * self.invstd).double()           # fp32 like the kernel, then widened
        if self.kind == 'saved':
            mask = self.out.reshape(-1, n) > 0
        else:                                                                            # sign of fma(xhat, gamma, beta), exactly
            mask = (xhat * self.gamma.double() + self.beta.double()) > 0
        dd = torch.where(mask, v, torch.zeros_like(v))
        return torch.stack([dd.sum(0), (dd * xhat).sum(0)])


def launch(case, mma, a, wp, add=None, sums=None):
    """One launch of `case` under `mma` plus its repeat; returns (output [M][N] fp32, fused sums [2][N] fp64 or None)."""
    from yolact_minimal_amd import hip
    L = hip.lib()
    g = case.geo
    M, N = g.M, g.N
    assert tuple(a.shape) == g.in_shape and a.is_contiguous() and (add is None) == (not case.add)
    buf = torch.full((GUARD + M * N + GUARD,), FILL, device=DEV)
    region = buf[GUARD:GUARD + M * N]
    counters = _tile_counters()
    d = S.descriptor(case, mma, a.data_ptr(), wp.data_ptr(), region.data_ptr(), counters.data_ptr(), add.data_ptr() if case.add else None)
    eff = hip.conv_effective_plan(d)
    assert (eff.tile_m, eff.tile_n) == case.tile and (not mma or eff.stages == (3 if case.stages == 3 else 2)), (case.id, mma, eff)
    acc = part = None
    rows = 0
    if sums is not None:
        assert L.ym_conv2d_fuses_bn_stats(ctypes.byref(d)) == 1, case.id
        if sums.kind != 'fwd':
            d.bnb_y, d.bnb_mean, d.bnb_invstd, d.bnb_relu = sums.y.data_ptr(), sums.mean.data_ptr(), sums.invstd.data_ptr(), 1
            if sums.kind == 'saved':
                d.bnb_out = sums.out.data_ptr()
            else:
                d.bnb_out, d.bnb_gamma, d.bnb_beta = None, sums.gamma.data_ptr(), sums.beta.data_ptr()
        if sums.ordered:
            d.bn_ordered = 1
            rows = L.ym_conv2d_bn_partial_rows(ctypes.byref(d))
            assert rows > 0, case.id
            part = torch.empty(rows + PART_GUARD, 2, N, dtype=torch.float64, device=DEV)
            d.bn_sum, d.bn_sumsq = part.data_ptr(), None
        else:
            acc = torch.empty(2, N, dtype=torch.float64, device=DEV)
            d.bn_sum, d.bn_sumsq = acc[0].data_ptr(), acc[1].data_ptr()
    ws = torch.empty(max(hip.conv_workspace_bytes(d), 256), dtype=torch.uint8, device=DEV)

    def once():
        region.fill_(float('nan'))
        if part is not None:
            part.fill_(float('nan'))
        if acc is not None:
            acc.zero_()
        try:
            hip.conv2d_fwd(d, ws)
            torch.cuda.synchronize()
        except RuntimeError as e:
            if 'ym_conv2d_fwd failed' not in str(e):         # a device fault above all: nothing more is started on it
                pytest.exit(f'{case.id} mma {mma}: {e}', returncode=3)
            raise
        out = region.clone()
        assert not bool(torch.isnan(out).any()), f'{case.id} mma {mma}: {int(torch.isnan(out).sum())} output elements were not written'
        assert bool((buf[:GUARD] == FILL).all()) and bool((buf[-GUARD:] == FILL).all()), f'{case.id} mma {mma}: wrote outside its output'
        assert bool((counters == 0).all()), f'{case.id} mma {mma}: {int((counters != 0).sum())} arrival counters left non-zero'
        total = None
        if part is not None:
            assert bool(torch.isfinite(part[:rows]).all()), 'a (row, channel) pair of the partial buffer was not written'
            assert bool(torch.isnan(part[rows:]).all()), 'the launch wrote behind ym_conv2d_bn_partial_rows rows'
            total = torch.full((2, N), float('nan'), dtype=torch.float64, device=DEV)
            hip.check(L.ym_bn_partials_finish(ctypes.c_void_p(part.data_ptr()), rows, N, ctypes.c_void_p(total.data_ptr()), hip.stream_ptr()),
                      'ym_bn_partials_finish')
            torch.cuda.synchronize()
        elif acc is not None:
            total = acc.clone()
        return out, total, (part[:rows].clone() if part is not None else None)

    try:
        out, total, p1 = once()
        out2, total2, p2 = once()
    finally:
        counters.zero_()
    assert torch.equal(out, out2), f'{case.id} mma {mma}: a second launch into the same buffers differs'
    if p1 is not None:                                       # (the atomics of the default mode add in arrival order: not compared)
        assert torch.equal(p1, p2) and torch.equal(total, total2), f'{case.id} mma {mma}: a second launch wrote other partials'
    return out.view(M, N), total


# ---- (a) random operands ----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _random(geo):
    """Operands, packed weight, residual and the fp64 references of a shape, computed once: (a, wp, add, ref, {mma: emulation})."""
    gen = torch.Generator(device=DEV).manual_seed(1000 + sum(map(ord, geo.name)))
    a = torch.randn(geo.in_shape, device=DEV, generator=gen)
    w = torch.randn(geo.w_shape, device=DEV, generator=gen) * (1.0 / geo.K ** 0.5)
    add = torch.randn(geo.out_shape, device=DEV, generator=gen)
    ref = S.conv(a.double(), w.double(), geo).reshape(geo.M, geo.N)
    emu = {mma: S.emulate(a, w, geo, mma).reshape(geo.M, geo.N) for mma in (3, 6)}
    return a, _pack(geo, w), add, ref, emu


@functools.lru_cache(maxsize=None)
def _f32_error(case):
    """max|f32 pipe - fp64| / max|ref| of the same plan and operands (mma = 0)."""
    a, wp, add, ref, _ = _random(case.geo)
    got, _ = launch(case, 0, a, wp, add if case.add else None)
    if case.add:
        ref = ref + add.double().reshape(ref.shape)
    return float((got.double() - ref).abs().max() / ref.abs().max())


CASES = S.cases()


@pytest.mark.parametrize('mma', [3, 6])
@pytest.mark.parametrize('case', CASES, ids=[c.id for c in CASES])
def test_random_operands_against_fp64_and_against_the_kept_terms(case, mma):
    a, wp, add, ref, emu = _random(case.geo)
    got, _ = launch(case, mma, a, wp, add if case.add else None)
    emu = emu[mma]
    if case.add:
        ref, emu = ref + add.double().reshape(ref.shape), emu + add.double().reshape(ref.shape)
    top = float(ref.abs().max())
    err = float((got.double() - ref).abs().max()) / top
    e_emu = float((got.double() - emu).abs().max()) / top
    e_f32 = _f32_error(case)
    print(f'{case.id} mma {mma}: {err:.2e} of max|ref| against fp64; {e_emu:.2e} against the kept terms, the f32 pipe {e_f32:.2e} against fp64 '
          f'(ratio {e_emu / e_f32:.2f})')
    _note('fp64', mma, case.geo, err)
    _note('kept terms', mma, case.geo, e_emu)
    _note('kept terms / f32 pipe', mma, case.geo, e_emu / e_f32)
    _note('f32 pipe', 0, case.geo, e_f32)
    assert err <= BAR, (case.id, mma, err)
    assert e_emu <= max(EMU_FACTOR * e_f32, EMU_FLOOR), (case.id, mma, e_emu, e_f32)


# ---- (b) first-order census ----------------------------------------------------------------------------------------------------------

CENSUS_SHAPES = (S.D1, S.D4, S.F1)
ROLES = {3: ('ints16 activations', 'ints16 weights'), 6: ('ints20 activations', 'ints20 weights')}


@functools.lru_cache(maxsize=None)
def _census(geo, mma, role):
    """(a fp32 on the device, packed weight, int64 expected [M][N], a int64, w int64) of one exact operand set."""
    gen = torch.Generator().manual_seed(2000 + 10 * mma + sum(map(ord, geo.name + role)))
    wide = S.ints16 if mma == 3 else S.ints20
    top, products = (2, 64) if mma == 3 else (1, 8)           # the narrow side, and the non-zero products allowed per output
    if role.endswith('activations'):
        a, ai = wide(geo.in_shape, gen)
        if mma == 3:
            w, wi = S.small_ints(geo.w_shape, gen, top)
        else:
            wi = S._signs(geo.w_shape, gen)
            w = wi.float()
        keep = S.thin_weight(w, products, gen)[1 if geo.transposed else 0]
        w, wi = w * keep, wi * keep
    else:
        w, wi = wide(geo.w_shape, gen)
        if mma == 3:
            a, ai = S.small_ints(geo.in_shape, gen, top)
        else:
            ai = S._signs(geo.in_shape, gen)
            a = ai.float()
        # bf16x3: 7 channels at every pixel (at most 9 taps x 7 = 63 products per output); bf16x6: 8 channels at the pixels of a lattice
        # of the filter's period (every window holds one such pixel: 8 products)
        keep = S.thin_activation(geo.in_shape, 7, 1, gen) if mma == 3 else S.thin_activation(geo.in_shape, 8, geo.k, gen)
        a, ai = a * keep, ai * keep
    return a, w, ai, wi


@functools.lru_cache(maxsize=None)
def _census_on_device(geo, mma, role):
    a, w, ai, wi = _census(geo, mma, role)
    S.check_exact_range(ai, wi, geo)                         # first: the operands pin ONE exact result
    want = S.conv(ai, wi, geo).reshape(geo.M, geo.N)
    assert int((want != 0).sum()) > want.numel() // 2         # (a census of zeros would count nothing)
    return a.to(DEV), _pack(geo, w.to(DEV)), want


CENSUS_CASES = [c for c in S.cases(CENSUS_SHAPES) if not c.add]


@pytest.mark.parametrize('mma,role', [(m, r) for m in (3, 6) for r in ROLES[m]])
@pytest.mark.parametrize('case', CENSUS_CASES, ids=[c.id for c in CENSUS_CASES])
def test_first_order_terms_are_all_there_exactly(case, mma, role):
    a, wp, want = _census_on_device(case.geo, mma, role)
    got, _ = launch(case, mma, a, wp)
    bad = (got.cpu().long() != want) | (got.cpu() != got.cpu().round())
    assert not bool(bad.any()), (f'{case.id} mma {mma}, {role}: {int(bad.sum())} of {bad.numel()} outputs differ from the exact result, rows '
                                 f'{int(bad.nonzero()[:, 0].min())}..{int(bad.nonzero()[:, 0].max())}, channels '
                                 f'{int(bad.nonzero()[:, 1].min())}..{int(bad.nonzero()[:, 1].max())}')
    assert torch.equal(got.cpu().long(), want)


# ---- (c) second-order census ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _two_plane(geo):
    """1x1 stride 1: both sides two_plane, one non-zero weight per output channel: ({mma: int64 expected}, a, packed weight)."""
    assert geo.k == 1 and geo.stride == 1
    gen = torch.Generator().manual_seed(3000 + sum(map(ord, geo.name)))
    a, ai = S.two_plane(geo.in_shape, gen)
    w, wi = S.two_plane(geo.w_shape, gen)
    keep = S.thin_weight(w, 1, gen)[1 if geo.transposed else 0]
    w, wi = w * keep, wi * keep
    assert S.check_exact_range(ai, wi, geo) < S.EXACT_LIMIT
    low = lambda v: v.sign() * (v.abs() % 256)                # p1 of a two_plane value
    full = S.conv(ai, wi, geo).reshape(geo.M, geo.N)
    omitted = S.conv(low(ai), low(wi), geo).reshape(geo.M, geo.N)
    assert bool((omitted != 0).all())                         # every output tells bf16x3 from bf16x6
    return {0: full, 3: full - omitted, 6: full}, a.to(DEV), _pack(geo, w.to(DEV))


SECOND_CASES = [c for c in S.cases((S.D4, S.F2)) if not c.add]


@pytest.mark.parametrize('mma', [0, 3, 6])
@pytest.mark.parametrize('case', SECOND_CASES, ids=[c.id for c in SECOND_CASES])
def test_second_order_term_is_there_for_bf16x6_and_only_it_is_missing_for_bf16x3(case, mma):
    want, a, wp = _two_plane(case.geo)
    got, _ = launch(case, mma, a, wp)
    g = got.cpu()
    assert torch.equal(g, g.round())
    if not torch.equal(g.long(), want[mma]):
        names = {0: 'x y (every term)', 3: 'x y - p1x p1y (bf16x3)', 6: 'x y (every term)'}
        match = [names[m] for m in (3, 6) if torch.equal(g.long(), want[m])]
        bad = g.long() != want[mma]
        raise AssertionError(f'{case.id} mma {mma}: {int(bad.sum())} of {bad.numel()} outputs are not {names[mma]}'
                             + (f'; the output is {match[0]}' if match else ''))


# ---- (d) fused sums under split products ---------------------------------------------------------------------------------------------

def _check_sums(case, mma, got, total, sums, note):
    want = sums.expected(got)
    err = float(((total - want).abs() / (1e-3 + 1e-5 * want.abs())).max())
    _note(note, mma, case.geo, err)
    torch.testing.assert_close(total, want, rtol=1e-5, atol=1e-3)


SUM_PLANS = [((64, 64), 0, 1, (0, 0)), ((128, 128), 3, 1, (0, 0)), ((128, 64), 0, 1, (0, 0)), ((64, 64), 0, 3, (0, 0)), ((64, 64), 3, 1, (2, 3))]


def _sum_cases(shapes):
    return [S.Case(g, t, st, ksplit=ks, tail=tail) for g in shapes for t, st, ks, tail in SUM_PLANS if not tail[0] or g.name in ('D1', 'F1')]


FWD_SUM_CASES = _sum_cases((S.F1, S.F2))


@pytest.mark.parametrize('ordered', [False, True], ids=['atomics', 'ordered'])
@pytest.mark.parametrize('mma', [3, 6])
@pytest.mark.parametrize('case', FWD_SUM_CASES, ids=[c.id for c in FWD_SUM_CASES])
def test_forward_statistics_of_a_split_launch_sum_its_own_output(case, mma, ordered):
    a, wp, _, ref, _ = _random(case.geo)
    sums = Sums('fwd', ordered)
    got, total = launch(case, mma, a, wp, sums=sums)
    assert float((got.double() - ref).abs().max() / ref.abs().max()) <= BAR
    _check_sums(case, mma, got, total, sums, 'forward sums / bar')


@functools.lru_cache(maxsize=None)
def _bn_context(geo):
    gen = torch.Generator(device=DEV).manual_seed(4000 + sum(map(ord, geo.name)))
    n = geo.N
    y = torch.randn(geo.out_shape, device=DEV, generator=gen)
    out = torch.relu(torch.randn(geo.out_shape, device=DEV, generator=gen))
    mean, invstd = torch.randn(n, device=DEV, generator=gen) * 0.1, torch.rand(n, device=DEV, generator=gen) + 0.5
    gamma, beta = torch.rand(n, device=DEV, generator=gen) + 0.5, torch.randn(n, device=DEV, generator=gen) * 0.2
    return y, out, mean, invstd, gamma, beta


BWD_SUM_CASES = _sum_cases((S.D1, S.D2))


@pytest.mark.parametrize('ordered', [False, True], ids=['atomics', 'ordered'])
@pytest.mark.parametrize('kind', ['saved', 'remask'])
@pytest.mark.parametrize('mma', [3, 6])
@pytest.mark.parametrize('case', BWD_SUM_CASES, ids=[c.id for c in BWD_SUM_CASES])
def test_batchnorm_backward_sums_of_a_split_data_gradient(case, mma, kind, ordered):
    a, wp, _, ref, _ = _random(case.geo)
    y, out, mean, invstd, gamma, beta = _bn_context(case.geo)
    sums = Sums(kind, ordered, y=y, out=out, mean=mean, invstd=invstd, gamma=gamma, beta=beta)
    got, total = launch(case, mma, a, wp, sums=sums)
    assert float((got.double() - ref).abs().max() / ref.abs().max()) <= BAR
    _check_sums(case, mma, got, total, sums, 'backward sums / bar')


@pytest.mark.parametrize('ordered', [False, True], ids=['atomics', 'ordered'])
@pytest.mark.parametrize('case', [S.Case(S.D1, (64, 64), 0), S.Case(S.D1, (128, 128), 3), S.Case(S.D1, (64, 64), 0, ksplit=3)], ids=lambda c: c.id)
def test_integer_sums_are_exact(case, ordered):
    """The first census operands of D1 (ints16 activations), mean 0, invstd 1, integer y and a saved mask: dx is exact, every term of
    both sums an integer below 2^53 in any order, so the fused sums equal the fp64 sums over the exact output."""
    geo = case.geo
    a, wp, want = _census_on_device(geo, 3, ROLES[3][0])
    gen = torch.Generator().manual_seed(5)
    y = torch.randint(-8, 9, geo.out_shape, generator=gen).float().to(DEV)
    out = torch.randint(0, 2, geo.out_shape, generator=gen).float().to(DEV)
    sums = Sums('saved', ordered, y=y, out=out, mean=torch.zeros(geo.N, device=DEV), invstd=torch.ones(geo.N, device=DEV))
    got, total = launch(case, 3, a, wp, sums=sums)
    assert torch.equal(got.cpu().long(), want)
    v = torch.where(out.reshape(-1, geo.N) > 0, want.to(DEV), torch.zeros_like(want.to(DEV)))
    exact = torch.stack([v.sum(0), (v * y.reshape(-1, geo.N).long()).sum(0)])
    assert int(exact.abs().max()) < 1 << 53 and bool((exact != 0).any())
    assert torch.equal(total, exact.double())


def test_report_the_worst_figures():
    """Prints what the tests above measured in this process (docs/experiments.md quotes a full run); asserts nothing new."""
    for (check, mma, mode), v in sorted(_worst.items()):
        print(f'split-bf16 {mode:5s} mma {mma}: worst {check} {v:.2e}')
