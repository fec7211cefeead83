"""The training-side NHWC kernels (csrc/train_ops.hip, the max-pool / bilinear forward of csrc/elementwise.hip) through their raw
`ym_*` entry points, at the shapes where the lane maps, unrolled loops, grid caps, workspace paths and image borders change behaviour.
Every case compares with the plain float64 reference of tests/train_ops_ref.py (pinned to torch's fp64 autograd and ATen's max-pool
rules by tests/test_train_ops_cpu.py) and asserts through that module's geometry mirrors that it reaches the branch it is named for.
Every output and workspace buffer has a NaN guard zone behind it.

The bars are those of the project's older tests of the same kernels (fp64 sums rtol 1e-12 / atol 1e-9; mean, invstd rtol 1e-6; running
statistics rtol 1e-5 / atol 1e-6; out rtol 1e-4 / atol 2e-5; gradients max|got - ref| / max|ref| <= 1e-4; bilinear rtol 1e-5 / atol
1e-6; everything else exact).  They are loose for kernels that accumulate in fp64.  Worst figures measured on an MI355X over all cases
(WORST_MEASURED below; the module prints the same table under pytest -s): sums 2.7e-3 of their bar, save_mean / save_invstd 6.0e-2,
running statistics 9.4e-3, out 1.3e-2, bilinear 0.38 / 0.46; rel_err of dy 1.6e-7, dres 0, dgamma 9.0e-8, dbeta 5.1e-8, act_bias dz
5.4e-8, dbias 5.6e-8; SGD 0.97 of its one-ulp bound.

Two things the sums' 1e-12 bar needs said.  The operands of the backward sums are the kernel's documented float32 values (dz exactly,
xhat = (y - mean) * invstd rounded to float32, train_ops_ref.bn_bwd_sum_operands); and the bias-gradient sums are taken with ReLU, whose
operands are exact, while tanh (dz = dy * (1 - y^2) formed in float32) is held to the gradient bar in test_act_bias_bwd."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import train_ops_ref as R
from tests.test_gpu_deterministic import finish_np

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 64
NAN = float('nan')
EPS, MOM = 1e-5, 0.1
YM_EINVAL, YM_ENOSPC = -1, -2

# Worst figure per kernel family over all cases of this module, measured on an MI355X (docs/experiments.md "Training NHWC kernels at
# their edges"); the module prints the same table at its end (pytest -s).  "share" = worst |got - ref| / (atol + rtol |ref|).
WORST_MEASURED = {
    'fp64 sums, share of rtol 1e-12 / atol 1e-9': 2.7e-3,
    'save_mean, save_invstd, share of rtol 1e-6': 6.0e-2,          # float32 rounding of the fp64 value: at most 2^-24 / 1e-6
    'running statistics, share of rtol 1e-5 / atol 1e-6': 9.4e-3,
    'out, share of rtol 1e-4 / atol 2e-5': 1.3e-2,
    'bn backward rel_err: dy, dres, dgamma, dbeta': (1.6e-7, 0.0, 9.0e-8, 5.1e-8),
    'act_bias rel_err: dz, dbias': (5.4e-8, 5.6e-8),
    'bilinear forward, backward, share of rtol 1e-5 / atol 1e-6': (0.38, 0.46),
    'sgd, share of the one-ulp bound': 0.97,
}
_worst = {}


def _note(family, value):
    _worst[family] = max(_worst.get(family, 0.0), float(value))


@pytest.fixture(scope='module', autouse=True)
def _print_worst():
    yield
    for k in sorted(_worst):
        print(f'\nWORST {k}: {_worst[k]:.3e}', end='')
    print()


def L():
    from yolact_minimal_amd import hip
    return hip.lib()


def sp():
    from yolact_minimal_amd import hip
    return hip.stream_ptr()


def vp(t):
    if t is None:
        return None
    if isinstance(t, Buf):
        t = t.t
    assert t.is_cuda and t.is_contiguous()
    return ctypes.c_void_p(t.data_ptr())


class Buf:
    """An output or workspace buffer of `shape` with GUARD elements of NaN (0xEE for bytes) behind it."""

    def __init__(self, *shape, dtype=torch.float32, init=None):
        self.n = int(np.prod(shape))
        self.fill = 0xEE if dtype == torch.uint8 else NAN
        self.whole = torch.full((self.n + GUARD,), self.fill, dtype=dtype, device=DEV)
        self.t = self.whole[:self.n].view(*shape)
        if init is not None:
            self.t.copy_(init)

    def untouched(self):
        if self.whole.dtype == torch.uint8:
            return bool((self.whole == self.fill).all())
        return bool(torch.isnan(self.whole).all())

    def check(self, extent=None, finite=True):
        """Nothing behind the buffer was written; its first `extent` elements (all by default) were, with finite values."""
        torch.cuda.synchronize()
        tail = self.whole[self.n:]
        assert bool((tail == self.fill).all() if self.whole.dtype == torch.uint8 else torch.isnan(tail).all()), 'guard zone written'
        if finite and self.whole.dtype != torch.uint8:
            e = self.n if extent is None else extent
            assert bool(torch.isfinite(self.whole[:e]).all()), 'the documented extent holds a value the call did not write'
            assert bool(torch.isnan(self.whole[e:self.n]).all()), 'written past the documented extent'
        return self.t


def ok(rc, what):
    from yolact_minimal_amd import hip
    hip.check(rc, what)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same(a, b):
    """Exact equality that lets NaN equal NaN."""
    a, b = (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t) for t in (a, b))
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == 'f')


def close(got, ref, rtol, atol, family):
    ref = torch.as_tensor(ref)
    got = torch.as_tensor(got).to(ref.device).double()
    ref = ref.double()
    excess = ((got - ref).abs() / (atol + rtol * ref.abs()).clamp_min(1e-300)).max().item() if ref.numel() else 0.0
    print(f'  {family}: worst |got - ref| / (atol + rtol |ref|) = {excess:.3e}  (rtol {rtol:g}, atol {atol:g})')
    _note(family + ' [share of its bar]', excess)
    torch.testing.assert_close(got, ref, rtol=rtol, atol=atol)


def grad_bar(got, ref, family):
    e = R.rel_err(got, ref)
    print(f'  {family}: rel_err = {e:.3e}')
    _note(family + ' [rel_err]', e)
    assert e <= 1e-4, (family, e)


# ---- the three column-sum launches ------------------------------------------------------------------------------------------------
def bn_fwd_call(y, gamma, beta, nbytes, residual=None, relu=0, running=True, rm0=None, rv0=None):
    m, c = y.shape
    ws = Buf(nbytes // 8, dtype=torch.float64)
    out, mean, invstd = Buf(m, c), Buf(c), Buf(c)
    rm = Buf(c, init=rm0 if rm0 is not None else torch.linspace(-1, 1, c)) if running else None
    rv = Buf(c, init=rv0 if rv0 is not None else torch.linspace(0.5, 2, c)) if running else None
    before = L().ym_unordered_sum_launches()
    ok(L().ym_bn_train_fwd(vp(y), m, c, vp(gamma), vp(beta), EPS, MOM, vp(rm), vp(rv), vp(residual), relu, vp(out), vp(mean),
                           vp(invstd), vp(ws), nbytes, sp()), 'ym_bn_train_fwd')
    torch.cuda.synchronize()
    return dict(ws=ws, out=out, mean=mean, invstd=invstd, rm=rm, rv=rv, moved=L().ym_unordered_sum_launches() - before)


def bn_bwd_call(dout, out, y, gamma, beta, mean, invstd, relu, nbytes, want_dres=True, stats=None):
    """ym_bn_train_bwd, or (stats = the fp64 sums) ym_bn_train_bwd_apply."""
    m, c = y.shape
    dy, dres, dg, db = Buf(m, c), (Buf(m, c) if want_dres else None), Buf(c), Buf(c)
    before = L().ym_unordered_sum_launches()
    if stats is None:
        ws = Buf(nbytes // 8, dtype=torch.float64)
        ok(L().ym_bn_train_bwd(vp(dout), vp(out), vp(y), m, c, vp(gamma), vp(beta), vp(mean), vp(invstd), relu, vp(dy), vp(dres), vp(dg),
                               vp(db), vp(ws), nbytes, sp()), 'ym_bn_train_bwd')
    else:
        ws = None
        ok(L().ym_bn_train_bwd_apply(vp(dout), vp(out), vp(y), m, c, vp(gamma), vp(beta), vp(mean), vp(invstd), relu, vp(dy), vp(dres),
                                     vp(dg), vp(db), vp(stats), sp()), 'ym_bn_train_bwd_apply')
    torch.cuda.synchronize()
    for b in (dy, dres, dg, db):
        if b is not None:
            b.check()
    return dict(ws=ws, dy=dy.t, dres=dres.t if want_dres else None, dgamma=dg.t, dbeta=db.t, moved=L().ym_unordered_sum_launches() - before)


def act_bias_call(dy, y, act, nbytes, want_dz=False, want_dbias=True):
    m, c = dy.shape
    ws = Buf(max(nbytes // 8, 1), dtype=torch.float64) if want_dbias else None
    dz, dbias = (Buf(m, c) if want_dz else None), (Buf(c) if want_dbias else None)
    before = L().ym_unordered_sum_launches()
    ok(L().ym_act_bias_bwd(vp(dy), vp(y), m, c, act, vp(dz), vp(dbias), vp(ws), nbytes if want_dbias else 0, sp()), 'ym_act_bias_bwd')
    torch.cuda.synchronize()
    return dict(ws=ws, dz=dz, dbias=dbias, moved=L().ym_unordered_sum_launches() - before)


def check_sums(ws, k, c, ref, rows, family):
    """ws: the fp64 workspace Buf after a launch; k sums of c channels lead it, `rows` partial rows [2][c] follow (rows = 0: the atomic
    path).  Sums against the reference at the bar; on the partials path bit-equal to the documented ordered sum of the partials."""
    ws.check(extent=(2 * c + rows * 2 * c) if rows else k * c)
    w = ws.t.cpu().numpy()
    got = torch.from_numpy(w[:k * c].reshape(k, c).copy())
    close(got, ref[:k], 1e-12, 1e-9, family)
    if rows:
        part = w[2 * c:2 * c + rows * 2 * c].reshape(rows, 2, c)
        assert np.array_equal(bits(w[:2 * c].reshape(2, c)), bits(finish_np(part))), 'not the ordered sum of the partials the kernel wrote'


def column_case(m, c, y, gamma, beta, dout, out, on_device):
    """All three column-sum launches on both workspace sizes at one shape.  `on_device`: the reference is evaluated in fp64 on the GPU."""
    assert R.stats_workspace_bytes(m, c) == L().ym_bn_train_fwd_workspace_bytes(m, c) == L().ym_bn_train_bwd_workspace_bytes(m, c)
    to = (lambda t: t) if on_device else (lambda t: t.cpu())
    yr, gr, br, dr, outr = (to(t) for t in (y, gamma, beta, dout, out))
    rm0, rv0 = torch.linspace(-1, 1, c), torch.linspace(0.5, 2, c)
    fwd = R.bn_fwd(yr, gr, br, EPS, MOM, to(rm0.to(DEV)), to(rv0.to(DEV)))
    mean32, invstd32 = fwd['mean'].float(), fwd['invstd'].float()
    mask = outr > 0
    assert R.mask_takes_both_values(outr)
    bsum = R.bn_bwd_sum_operands(dr, yr, mean32, invstd32, mask)
    dy_r, dres_r, dg_r, db_r = R.bn_bwd(dr, yr, mean32, invstd32, gr, mask)
    _, dbias_r = R.act_bias_bwd(dr, outr, R.ACT_RELU)
    mean_d, invstd_d = mean32.to(DEV), invstd32.to(DEV)
    for partials in (False, True):
        tag = f'({m},{c}) ' + ('partials' if partials else 'atomic')
        print(tag)
        nbytes = R.stats_workspace_bytes(m, c) if partials else 16 * c
        rows = R.stats_grid(m, c, True) if partials else 0
        f = bn_fwd_call(y, gamma, beta, nbytes, rm0=rm0, rv0=rv0)
        assert f['moved'] == (0 if partials else 1)
        check_sums(f['ws'], 2, c, fwd['sums'], rows, 'sums')
        close(f['mean'].check(), fwd['mean'], 1e-6, 0.0, 'save_mean')
        close(f['invstd'].check(), fwd['invstd'], 1e-6, 0.0, 'save_invstd')
        close(f['rm'].check(), fwd['run_mean'], 1e-5, 1e-6, 'running')
        close(f['rv'].check(), fwd['run_var'], 1e-5, 1e-6, 'running')
        close(f['out'].check(), fwd['out'], 1e-4, 2e-5, 'out')
        b = bn_bwd_call(dout, out, y, gamma, beta, mean_d, invstd_d, 1, nbytes)
        assert b['moved'] == (0 if partials else 1)
        check_sums(b['ws'], 2, c, bsum, rows, 'sums')
        for name, ref in (('dy', dy_r), ('dres', dres_r), ('dgamma', dg_r), ('dbeta', db_r)):
            grad_bar(b[name], ref, 'bn_bwd ' + name)
        nb2 = R.bias_workspace_bytes(m, c) if partials else 8 * c
        a = act_bias_call(dout, out, R.ACT_RELU, nb2)
        assert a['moved'] == (0 if partials else 1)
        check_sums(a['ws'], 2 if partials else 1, c, torch.stack([dbias_r, torch.zeros_like(dbias_r)]),
                   R.bias_grid(m, c, True) if partials else 0, 'sums')
        grad_bar(a['dbias'].check(), dbias_r, 'act_bias dbias')


LANE_FACTS = {   # what each lane-map shape is in the table for, in the terms of train_ops_ref.lane_map / col_loops
    (1, 4): dict(CQ=1, RL=256, idle=0), (255, 4): dict(CQ=1, RL=256), (5000, 4): dict(CQ=1, RL=256),
    (37, 24): dict(CQ=6, RL=42, idle=4), (338, 96): dict(CQ=24, RL=10, idle=16), (77, 352): dict(CQ=88, RL=2, idle=80),
    (50, 1024): dict(CQ=256, RL=1, idle=0, passes=1), (19, 1536): dict(CQ=256, passes=2, last_pass_empty=128),
    (33, 2048): dict(CQ=256, passes=2, last_pass_empty=0),
}


@pytest.mark.parametrize('m,c', R.LANE_SHAPES, ids=lambda v: str(v))
def test_column_sums_lane_maps(m, c):
    lm = R.lane_map(c)
    for k, v in LANE_FACTS[(m, c)].items():
        assert lm[k] == v, (k, lm)
    if (m, c) == (1, 4):
        assert R.col_loops(m, c, R.stats_grid(m, c, True), 4)['idle_lanes'] == 255          # one row, 256 row lanes
    if (m, c) == (255, 4):
        assert R.col_loops(m, c, R.stats_grid(m, c, True), 4) == dict(main=0, remainder=1, strides=False, idle_lanes=1)
    if (m, c) == (5000, 4):
        lp = R.col_loops(m, c, R.stats_grid(m, c, True), 4)
        assert R.stats_grid(m, c, True) == 2 and lp['main'] >= 2 and lp['remainder'] >= 1 and lp['strides']
    column_case(m, c, *_small_inputs(m, c), on_device=False)


def _small_inputs(m, c):
    y, gamma, beta, _, dout, out = R.bn_inputs(m, c, 1000 * m + c, DEV)
    return y, gamma, beta, dout, out


@pytest.mark.parametrize('m,c', R.UNROLL_SHAPES, ids=lambda v: str(v))
def test_column_sums_unrolled_and_remainder_loops(m, c):
    assert R.lane_map(c)['RL'] == 1
    lp = {mode: R.col_loops(m, c, grid, unroll) for mode, grid, unroll in
          ((0, R.stats_grid(m, c, True), 4), (1, R.stats_grid(m, c, True), 2), (2, R.bias_grid(m, c, True), 4))}
    print(lp)
    assert all(v['main'] >= 1 for v in lp.values()), 'the unrolled loop does not run'
    if m == 16:
        assert all(v['remainder'] == 0 for v in lp.values())                 # unrolled loop alone
    else:
        assert lp[0]['remainder'] >= 1 and lp[2]['remainder'] >= 1           # unrolled loop, then the remainder loop
    if m in (17, 35):
        assert lp[1]['remainder'] == 1                                       # the 2-row loop of MODE 1 leaves one row
    column_case(m, c, *_small_inputs(m, c), on_device=False)


@pytest.mark.parametrize('m,c', R.CAP_SHAPES, ids=lambda v: str(v))
def test_column_sums_at_the_grid_caps(m, c):
    rl = R.lane_map(c)['RL']
    if m == 8292:
        assert R.stats_grid(m, c, False) == 512 < -(-m // (16 * rl)) and R.col_loops(m, c, 512, 4)['strides']
    if m == 16421:
        assert R.stats_grid(m, c, True) == 1024 < -(-m // (16 * rl)) and R.col_loops(m, c, 1024, 4)['strides']
    if m == 32773:
        assert R.bias_grid(m, c, True) == 1024 < -(-m // (32 * rl)) and R.col_loops(m, c, 1024, 4)['strides']
    if m == 65539:
        assert R.bias_grid(m, c, False) == 2048 < -(-m // (32 * rl)) and R.col_loops(m, c, 2048, 4)['strides']
    column_case(m, c, *R.big_bn_inputs(m, c, m, DEV), on_device=True)


def test_column_sums_conditioning():
    """Channel 0 constant (variance clamps to 0, invstd = 1/sqrt(eps), out = beta), channel 1 with mean 100 and std 0.1."""
    m, c = 501, 8
    y = R.conditioning_input(m, c, 7).to(DEV)
    _, gamma, beta, _, _, _ = R.bn_inputs(m, c, 8, DEV)
    ref = R.bn_fwd(y.cpu(), gamma.cpu(), beta.cpu(), EPS, MOM, torch.linspace(-1, 1, c), torch.linspace(0.5, 2, c))
    assert float(ref['var'][0]) == 0.0 and float(ref['mean'][1]) == 100.0 and abs(float(ref['var'][1]) ** 0.5 - 0.1) < 0.01
    for partials in (False, True):
        f = bn_fwd_call(y, gamma, beta, R.stats_workspace_bytes(m, c) if partials else 16 * c)
        check_sums(f['ws'], 2, c, ref['sums'], R.stats_grid(m, c, True) if partials else 0, 'sums')
        close(f['mean'].check(), ref['mean'], 1e-6, 0.0, 'save_mean')
        close(f['invstd'].check(), ref['invstd'], 1e-6, 0.0, 'save_invstd')
        close(f['rm'].check(), ref['run_mean'], 1e-5, 1e-6, 'running')
        close(f['rv'].check(), ref['run_var'], 1e-5, 1e-6, 'running')
        close(f['out'].check(), ref['out'], 1e-4, 2e-5, 'out')
        assert float(f['invstd'].t[0]) == float(np.float32(1.0 / math.sqrt(float(np.float32(EPS)))))
        assert torch.equal(f['out'].t[:, 0], beta[0].expand(m))


def test_bn_fwd_without_running_statistics_and_with_one_row():
    for m, c, running in ((37, 24, False), (1, 24, True), (1, 24, False)):
        y, gamma, beta, _, _, _ = R.bn_inputs(m, c, 11 + m, DEV)
        rm0, rv0 = torch.linspace(-1, 1, c), torch.linspace(0.5, 2, c)
        ref = R.bn_fwd(y.cpu(), gamma.cpu(), beta.cpu(), EPS, MOM, rm0 if running else None, rv0 if running else None)
        f = bn_fwd_call(y, gamma, beta, 16 * c, running=running, rm0=rm0, rv0=rv0)
        check_sums(f['ws'], 2, c, ref['sums'], 0, 'sums')
        close(f['mean'].check(), ref['mean'], 1e-6, 0.0, 'save_mean')
        close(f['invstd'].check(), ref['invstd'], 1e-6, 0.0, 'save_invstd')
        close(f['out'].check(), ref['out'], 1e-4, 2e-5, 'out')
        if running:
            close(f['rm'].check(), ref['run_mean'], 1e-5, 1e-6, 'running')
            close(f['rv'].check(), ref['run_var'], 1e-5, 1e-6, 'running')             # M = 1: the biased variance (0)
            assert torch.equal(f['rv'].t.cpu(), ((1.0 - float(np.float32(MOM))) * rv0.double()).float())


@pytest.mark.parametrize('c', R.FINISH_C)
@pytest.mark.parametrize('rows', R.FINISH_ROWS)
def test_partials_finish_is_the_ordered_sum(rows, c):
    lp = R.col_finish_loops(rows)
    assert (lp['main'] >= 1) == (rows > 48) and lp['empty_slice'] == (rows < 16)
    g = torch.Generator().manual_seed(rows * 100 + c)
    part = torch.randn(rows, 2, c, generator=g, dtype=torch.float64) * 2.0 ** torch.randint(-20, 40, (rows, 2, c), generator=g).double()
    dev = Buf(rows, 2, c, dtype=torch.float64, init=part)
    sums = Buf(2, c, dtype=torch.float64)
    ok(L().ym_bn_partials_finish(vp(dev), rows, c, vp(sums), sp()), 'ym_bn_partials_finish')
    got = sums.check().cpu().numpy()
    assert same(dev.t, part), 'the partials were modified'
    assert np.array_equal(bits(got), bits(finish_np(part.numpy())))


# ---- forward apply ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('residual,relu', [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize('m,c', R.LANE_SHAPES, ids=lambda v: str(v))
def test_bn_train_fwd_apply(m, c, residual, relu):
    y, gamma, beta, res, _, _ = R.bn_inputs(m, c, 31 * m + c, DEV)
    rm0, rv0 = torch.linspace(-1, 1, c), torch.linspace(0.5, 2, c)
    ref = R.bn_fwd(y.cpu(), gamma.cpu(), beta.cpu(), EPS, MOM, rm0, rv0, res.cpu() if residual else None, relu)
    f = bn_fwd_call(y, gamma, beta, 16 * c, res if residual else None, int(relu), rm0=rm0, rv0=rv0)
    close(f['mean'].check(), ref['mean'], 1e-6, 0.0, 'save_mean')
    close(f['invstd'].check(), ref['invstd'], 1e-6, 0.0, 'save_invstd')
    close(f['rm'].check(), ref['run_mean'], 1e-5, 1e-6, 'running')
    close(f['rv'].check(), ref['run_var'], 1e-5, 1e-6, 'running')
    close(f['out'].check(), ref['out'], 1e-4, 2e-5, 'out')
    if relu:
        assert bool((f['out'].t >= 0).all())


FWD_STATS_FACTS = {(37, 64): 1, (338, 96): 3, (40, 28): 7, (77, 352): 11, (9, 268): None, (1, 2048): 2, (250, 64): 1}


@pytest.mark.parametrize('residual,relu', [(False, False), (True, True)])
@pytest.mark.parametrize('m,c', R.FWD_STATS_SHAPES, ids=lambda v: str(v))
def test_bn_train_fwd_stats_gives_the_same_floats(m, c, residual, relu):
    """ym_bn_train_fwd_stats on the sums ym_bn_train_fwd left behind: bit-identical statistics and output."""
    geo = R.fwd_stats_geometry(m, c)
    print(geo)
    assert geo['step'] == FWD_STATS_FACTS[(m, c)] and geo['fused'] == (FWD_STATS_FACTS[(m, c)] is not None)
    if (m, c) == (1, 2048):
        # the one-block grid is raised to the step: 256 * grid == C/4 exactly, the fewest threads that can publish every channel.
        # (256 * step is a multiple of C/4, so the rounded grid always covers C/4: the `grid * 256 < C4` loop behind it cannot run.)
        assert geo['grid0'] == 1 and geo['grid'] == 2 and geo['grid'] * 256 == c // 4
    if (m, c) == (250, 64):
        assert any(a >= 1 for a, _ in geo['loops']) and any(b >= 1 for _, b in geo['loops']), geo
    y, gamma, beta, res, _, _ = R.bn_inputs(m, c, 17 * m + c, DEV)
    res = res if residual else None
    rm0, rv0 = torch.linspace(-1, 1, c), torch.linspace(0.5, 2, c)
    ref = R.bn_fwd(y.cpu(), gamma.cpu(), beta.cpu(), EPS, MOM, rm0, rv0, res.cpu() if residual else None, relu)
    f = bn_fwd_call(y, gamma, beta, R.stats_workspace_bytes(m, c), res, int(relu), rm0=rm0, rv0=rv0)
    out, mean, invstd, rm, rv = Buf(m, c), Buf(c), Buf(c), Buf(c, init=rm0), Buf(c, init=rv0)
    ok(L().ym_bn_train_fwd_stats(vp(y), m, c, vp(gamma), vp(beta), EPS, MOM, vp(rm), vp(rv), vp(res), int(relu), vp(out), vp(mean),
                                 vp(invstd), vp(f['ws']), sp()), 'ym_bn_train_fwd_stats')
    close(out.check(), ref['out'], 1e-4, 2e-5, 'out')
    close(mean.check(), ref['mean'], 1e-6, 0.0, 'save_mean')
    close(invstd.check(), ref['invstd'], 1e-6, 0.0, 'save_invstd')
    close(rm.check(), ref['run_mean'], 1e-5, 1e-6, 'running')
    close(rv.check(), ref['run_var'], 1e-5, 1e-6, 'running')
    for name, a, b in (('out', out, f['out']), ('save_mean', mean, f['mean']), ('save_invstd', invstd, f['invstd']),
                       ('running_mean', rm, f['rm']), ('running_var', rv, f['rv'])):
        assert torch.equal(a.t, b.t), f'{name}: ym_bn_train_fwd_stats and ym_bn_train_fwd differ'
    # without running statistics
    out2, mean2, invstd2 = Buf(m, c), Buf(c), Buf(c)
    ok(L().ym_bn_train_fwd_stats(vp(y), m, c, vp(gamma), vp(beta), EPS, MOM, None, None, vp(res), int(relu), vp(out2), vp(mean2),
                                 vp(invstd2), vp(f['ws']), sp()), 'ym_bn_train_fwd_stats')
    assert torch.equal(out2.check(), out.t) and torch.equal(mean2.check(), mean.t) and torch.equal(invstd2.check(), invstd.t)


# ---- backward apply ---------------------------------------------------------------------------------------------------------------
def bwd_apply_case(m, c, y, gamma, beta, dout, want_dres, on_device):
    nbytes = R.stats_workspace_bytes(m, c)
    f = bn_fwd_call(y, gamma, beta, nbytes, None, 1)
    out, mean, invstd = f['out'].check(), f['mean'].check(), f['invstd'].check()
    to = (lambda t: t) if on_device else (lambda t: t.cpu())
    mask = to(out) > 0
    assert R.mask_takes_both_values(to(out))
    res = {}
    for mode in ('none', 'saved', 'rederived'):
        print(f'({m},{c}) dres={want_dres} mask={mode}')
        relu = int(mode != 'none')
        b = bn_bwd_call(dout, out if mode == 'saved' else None, y, gamma, beta, mean, invstd, relu, nbytes, want_dres)
        ref = R.bn_bwd(to(dout), to(y), to(mean), to(invstd), to(gamma), mask if relu else None)
        names = ('dy', 'dres', 'dgamma', 'dbeta') if want_dres else ('dy', 'dgamma', 'dbeta')
        for name in names:
            grad_bar(b[name], ref[('dy', 'dres', 'dgamma', 'dbeta').index(name)], 'bn_bwd ' + name)
        a = bn_bwd_call(dout, out if mode == 'saved' else None, y, gamma, beta, mean, invstd, relu, 0, want_dres, stats=b['ws'])
        for name in names:
            assert torch.equal(a[name], b[name]), f'{name}: ym_bn_train_bwd_apply on the sums of ym_bn_train_bwd differs from it'
        res[mode] = (b, names)
    for name in res['saved'][1]:
        assert torch.equal(res['saved'][0][name], res['rederived'][0][name]), f'{name}: the re-derived ReLU mask differs from the saved one'


@pytest.mark.parametrize('want_dres', [False, True])
@pytest.mark.parametrize('m,c', R.BWD_APPLY_SHAPES, ids=lambda v: str(v))
def test_bn_bwd_apply(m, c, want_dres):
    geo = R.bwd_apply_geometry(m, c)
    print(geo)
    if (m, c) == (250, 64):
        assert geo['fixed_c'] and not geo['capped']
        assert any(a >= 1 for a, _ in geo['loops']) and any(a == 0 and b >= 1 for a, b in geo['loops']), geo
    else:
        assert not geo['fixed_c'] and (geo['grid'] * 256) % (c // 4) != 0
    y, gamma, beta, _, dout, _ = R.bn_inputs(m, c, 13 * m + c, DEV)
    bwd_apply_case(m, c, y, gamma, beta, dout, want_dres, on_device=False)


def test_bn_bwd_apply_past_the_grid_cap():
    c = 256
    m = R.bwd_apply_large_m(c)
    geo = R.bwd_apply_geometry(m, c)
    print(m, geo)
    assert geo['capped'] and geo['grid'] == 8192 and geo['fixed_c']
    assert any(a >= 2 for a, _ in geo['loops']) and any(b >= 1 for _, b in geo['loops'])
    y, gamma, beta, dout, _ = R.big_bn_inputs(m, c, 5, DEV)
    bwd_apply_case(m, c, y, gamma, beta, dout, True, on_device=True)


# ---- activation + bias backward ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('outputs', ['dz', 'dbias', 'both'])
@pytest.mark.parametrize('act', [R.ACT_NONE, R.ACT_RELU, R.ACT_TANH], ids=['none', 'relu', 'tanh'])
def test_act_bias_bwd(act, outputs):
    m, c = 77, 352
    g = torch.Generator().manual_seed(act * 10 + len(outputs))
    dy = torch.randn(m, c, generator=g)
    if act == R.ACT_RELU:
        y = torch.relu(torch.randn(m, c, generator=g))
        assert bool((y == 0).any(0).all()) and bool((y > 0).any(0).all())                # exact zeros, in every channel
    else:
        y = torch.tanh(torch.randn(m, c, generator=g) * 3)
        y[0], y[1] = 1.0, -1.0                                                            # |y| up to 1: tanh' is exactly 0 there
        assert float(y.abs().max()) == 1.0
    dz_r, dbias_r = R.act_bias_bwd(dy, y, act)
    dy_d, y_d = dy.to(DEV), y.to(DEV)
    for partials in (False, True):
        nbytes = R.bias_workspace_bytes(m, c) if partials else 8 * c
        r = act_bias_call(dy_d, y_d if act != R.ACT_NONE else None, act, nbytes, outputs != 'dbias', outputs != 'dz')
        assert same(dy_d, dy) and same(y_d, y)
        if r['dz'] is not None:
            if act == R.ACT_NONE:
                assert r['dz'].untouched()                                               # dz = dy: nothing to compute
            else:
                grad_bar(r['dz'].check(), dz_r, 'act_bias dz')
                if act == R.ACT_RELU:
                    assert torch.equal(r['dz'].t.cpu(), dz_r.float())
                else:
                    assert bool((r['dz'].t[:2] == 0).all())
        if r['dbias'] is not None:
            assert r['moved'] == (0 if partials else 1)
            grad_bar(r['dbias'].check(), dbias_r, 'act_bias dbias')
            r['ws'].check(extent=(2 * c + R.bias_grid(m, c, True) * 2 * c) if partials else c)
        else:
            assert r['moved'] == 0
    if act == R.ACT_NONE:                                                                 # dz == dy is allowed
        db, ws = Buf(c), Buf(c, dtype=torch.float64)
        ok(L().ym_act_bias_bwd(vp(dy_d), None, m, c, act, vp(dy_d), vp(db), vp(ws), 8 * c, sp()), 'ym_act_bias_bwd')
        grad_bar(db.check(), dbias_r, 'act_bias dbias')
        assert same(dy_d, dy)


# ---- max-pool -----------------------------------------------------------------------------------------------------------------------
def pool_case(x, seed):
    b, h, w, c = x.shape
    ho, wo = R.pool_out(h), R.pool_out(w)
    dy = R.pool_grad(x, seed)
    out_r, arg_r = R.maxpool_fwd(x)
    dx_r = torch.from_numpy(R.maxpool_bwd(arg_r, dy.numpy(), h, w)).float()
    xd, dyd = x.to(DEV), dy.to(DEV)
    out, idx, out0 = Buf(b, ho, wo, c), Buf(b, ho, wo, c, dtype=torch.uint8), Buf(b, ho, wo, c)
    ok(L().ym_maxpool3x3s2_fwd_idx(vp(xd), vp(out), vp(idx), b, h, w, c, sp()), 'ym_maxpool3x3s2_fwd_idx')
    ok(L().ym_maxpool3x3s2_fwd(vp(xd), vp(out0), b, h, w, c, sp()), 'ym_maxpool3x3s2_fwd')
    out.check(finite=False), idx.check(), out0.check(finite=False)
    assert same(out.t, torch.from_numpy(out_r).float()) and same(out0.t, out.t), 'forward values'
    dx_i, dx_s = Buf(b, h, w, c), Buf(b, h, w, c)
    ok(L().ym_maxpool3x3s2_bwd_idx(vp(idx), vp(dyd), vp(dx_i), b, h, w, c, sp()), 'ym_maxpool3x3s2_bwd_idx')
    ok(L().ym_maxpool3x3s2_bwd(vp(xd), vp(dyd), vp(dx_s), b, h, w, c, sp()), 'ym_maxpool3x3s2_bwd')
    dx_i.check(), dx_s.check()
    bad_arg = int((idx.t.cpu() != torch.from_numpy(arg_r)).sum())
    bad_i, bad_s = int((dx_i.t.cpu() != dx_r).sum()), int((dx_s.t.cpu() != dx_r).sum())
    print(f'  pool {tuple(x.shape)}: argmax bytes off {bad_arg}, dx off: saved argmax {bad_i}, re-scan {bad_s}; '
          f'sum dx saved {float(dx_i.t.sum()):.4f} re-scan {float(dx_s.t.sum()):.4f} reference {float(dx_r.sum()):.4f}')
    assert bad_arg == 0, 'argmax bytes'
    assert bad_i == 0, 'ym_maxpool3x3s2_bwd_idx against the reference'
    assert bad_s == 0, 'ym_maxpool3x3s2_bwd against the reference'
    assert torch.equal(dx_i.t, dx_s.t)


@pytest.mark.parametrize('shape', R.POOL_SHAPES, ids=lambda v: 'x'.join(map(str, v)))
def test_maxpool_with_ties(shape):
    x = R.pool_input(shape, sum(shape))
    assert R.windows_with_ties(x) > 0 or shape == (1, 1, 1, 4)          # (a 1 x 1 image has one-element windows)
    pool_case(x, 1)


def test_maxpool_window_of_minus_infinity():
    """The gradient of a window whose valid elements are all -inf goes to its first valid element (ATen), on both backward kernels."""
    x = R.pool_inf_input()
    assert bool(torch.isinf(R.window(x, 0, 0)).all()) and R.window(x, 0, 0).shape[1] == 4 and bool(torch.isinf(R.window(x, 2, 2)).all())
    pool_case(x, 2)


def test_maxpool_windows_with_nan():
    """The last NaN of a window wins (ATen), on the forward and on both backward kernels."""
    x = R.pool_nan_input()
    assert [int(torch.isnan(R.window(x, *w)[0, :, 0]).sum()) for w in ((0, 0), (2, 2), (0, 2))] == [1, 2, 3]
    pool_case(x, 3)


# ---- bilinear x2 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('align', [0, 1])
@pytest.mark.parametrize('shape', R.BILINEAR_SHAPES, ids=lambda v: 'x'.join(map(str, v)))
def test_bilinear2x(shape, align):
    b, h, w, c = shape
    g = torch.Generator().manual_seed(sum(shape) + align)
    x, dy = torch.randn(shape, generator=g), torch.randn(b, 2 * h, 2 * w, c, generator=g)
    out, dx = Buf(b, 2 * h, 2 * w, c), Buf(b, h, w, c)
    xd, dyd = x.to(DEV), dy.to(DEV)
    ok(L().ym_bilinear2x_fwd(vp(xd), vp(out), b, h, w, c, align, sp()), 'ym_bilinear2x_fwd')
    ok(L().ym_bilinear2x_bwd(vp(dyd), vp(dx), b, h, w, c, align, sp()), 'ym_bilinear2x_bwd')
    close(out.check(), torch.from_numpy(R.bilinear2x_fwd(x.numpy(), align)), 1e-5, 1e-6, 'bilinear fwd')
    close(dx.check(), torch.from_numpy(R.bilinear2x_bwd(dy.numpy(), align)), 1e-5, 1e-6, 'bilinear bwd')


# ---- head gradient gather ---------------------------------------------------------------------------------------------------------
LEVELS = {1: [6], 3: [12, 6, 2], 5: [20, 12, 6, 2, 1]}


def _i32(vals):
    arr = (ctypes.c_int32 * len(vals))(*vals)
    return arr, ctypes.cast(arr, ctypes.c_void_p)


@pytest.mark.parametrize('scaled', [False, True])
@pytest.mark.parametrize('pitch', [39, 48])
@pytest.mark.parametrize('batch', [1, 3])
@pytest.mark.parametrize('nlev', [1, 3, 5])
def test_head_grad_gather(nlev, batch, pitch, scaled):
    na, nc, cd = 3, 5, 4
    assert na * (nc + 4 + cd) == 39
    pix = LEVELS[nlev]
    n = na * sum(pix)
    g = torch.Generator().manual_seed(nlev * 100 + batch * 10 + pitch)
    dclass, dbox = torch.randn(batch, n, nc, generator=g), torch.randn(batch, n, 4, generator=g)
    dcoef, coef = torch.randn(batch, n, cd, generator=g), torch.tanh(torch.randn(batch, n, cd, generator=g))
    scale = torch.tensor([0.37, 1.5, 6.125]) * torch.rand(3, generator=g) if scaled else None
    ref = R.head_grad_gather(dclass, dbox, dcoef, coef, batch, pix, nc, cd, na, pitch, scale)
    assert ref.dtype == torch.float32
    row, anchor = R.head_levels(batch, pix, na)
    (_r, rowp), (_a, anchorp) = _i32(row), _i32(anchor)
    dz = Buf(row[-1], pitch)
    dev = [t.to(DEV) if t is not None else None for t in (dclass, dbox, dcoef, coef, scale)]      # (kept alive across the launch)
    ok(L().ym_head_grad_gather(vp(dev[0]), vp(dev[1]), vp(dev[2]), vp(dev[3]), batch, n, nc, cd, na, nlev, rowp, anchorp, pitch, vp(dev[4]),
                               vp(dz), sp()), 'ym_head_grad_gather')
    got = dz.check().cpu()
    assert torch.equal(got, ref)
    if pitch > 39:
        assert bool((got[:, 39:] == 0).all()) and bool((got[:, :39] != 0).any())


def test_head_grad_gather_refuses_inconsistent_levels():
    na, nc, cd, batch, pix = 3, 5, 4, 2, [6, 2]
    n = na * sum(pix)
    row, anchor = R.head_levels(batch, pix, na)
    z = torch.zeros(batch, n, nc + 4 + cd, device=DEV)
    for bad_row, bad_anchor in ((list(row), [0, anchor[1] + 1, anchor[2]]), ([0, row[1] + 1, row[2]], list(anchor))):
        (_r, rowp), (_a, anchorp) = _i32(bad_row), _i32(bad_anchor)
        dz = Buf(row[-1], 48)
        rc = L().ym_head_grad_gather(vp(z), vp(z), vp(z), vp(z), batch, n, nc, cd, na, 2, rowp, anchorp, 48, None, vp(dz), sp())
        torch.cuda.synchronize()
        assert rc == YM_EINVAL and b'inconsistent' in L().ym_last_error()
        assert dz.untouched()


# ---- scatter3, SGD, dgrad weight image ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('sizes', [(a, b, c) for a in (0, 5) for b in (0, 300) for c in (0, 7)], ids=str)
def test_scatter3(sizes, accumulate):
    g = torch.Generator().manual_seed(sum(sizes) + accumulate)
    src = torch.randn(max(sum(sizes), 1), generator=g)
    start = [torch.randn(n, generator=g) for n in sizes]
    dst = [Buf(n, init=s) if n else None for n, s in zip(sizes, start)]
    srcd = src.to(DEV)
    ok(L().ym_scatter3(vp(srcd), vp(dst[0]), sizes[0], vp(dst[1]), sizes[1], vp(dst[2]), sizes[2], accumulate, sp()), 'ym_scatter3')
    want = R.scatter3(src[:sum(sizes)], start, accumulate)
    for d, wnt in zip(dst, want):
        if d is not None:
            assert torch.equal(d.check().cpu(), wnt)
    assert same(srcd, src)


@pytest.mark.parametrize('wd,mom', [(5e-4, 0.9), (0.0, 0.9), (5e-4, 0.0)], ids=['wd_momentum', 'wd0', 'momentum0'])
@pytest.mark.parametrize('n', R.SGD_SIZES)
def test_sgd_step(n, wd, mom):
    """Against the fp64 formula, for first_step 1 and 0: the kernel rounds three times per element (g' = fma(wd, p, g); momentum * buf;
    their sum) and once more for p = fma(-lr, buf, p), each by at most half an ulp of its own result, so with u = 2^-23 and
    S = |momentum * buf| + |g| + |wd * p| the new buf is within u * S and the new p within u * (|p| + 2 * lr * S) of the exact
    values: "one float32 ulp" at the magnitude of the terms (to first order in u; 2^-20 covers the second-order terms).  The bound
    is tight: 0.97 of it is reached among 2M elements.  Then three steps bit-equal to torch.optim.SGD on the device."""
    if n > 8192 * 256:
        assert -(-n // 256) > 8192                                                       # past the grid cap: lanes stride
    lr = 0.01
    u = 2.0 ** -23
    g = torch.Generator(device=DEV).manual_seed(n)
    p0, buf0 = torch.randn(n, generator=g, device=DEV), torch.randn(n, generator=g, device=DEV)
    for first in (1, 0):
        gr = torch.randn(n, generator=g, device=DEV)
        p, buf = Buf(n, init=p0), Buf(n, init=buf0)
        ok(L().ym_sgd_step(vp(p), vp(gr), vp(buf), n, lr, mom, wd, first, sp()), 'ym_sgd_step')
        p.check(), buf.check()
        p_r, buf_r = R.sgd_step(p0, gr, buf0, lr, mom, wd, first)
        lr32, mom32, wd32 = (float(np.float32(v)) for v in (lr, mom, wd))
        s = (0.0 if first else (mom32 * buf0.double()).abs()) + gr.double().abs() + (wd32 * p0.double()).abs()
        e_buf = ((buf.t.double() - buf_r).abs() / (u * s)).max().item()
        e_p = ((p.t.double() - p_r).abs() / (u * (p0.double().abs() + 2 * lr32 * s))).max().item()
        print(f'  sgd n={n} first={first}: buf error {e_buf:.3f}, p error {e_p:.3f} (in units of the bound)')
        _note('sgd [share of the one-ulp bound]', max(e_buf, e_p))
        assert e_buf <= 1.0 + 2.0 ** -20 and e_p <= 1.0 + 2.0 ** -20
    q = torch.nn.Parameter(p0.clone())
    opt = torch.optim.SGD([q], lr=lr, momentum=mom, weight_decay=wd)
    p, buf = Buf(n, init=p0), Buf(n, init=torch.zeros(n))
    for step in range(3):
        gr = torch.randn(n, generator=g, device=DEV)
        q.grad = gr.clone()
        opt.step()
        ok(L().ym_sgd_step(vp(p), vp(gr), vp(buf), n, lr, mom, wd, int(step == 0), sp()), 'ym_sgd_step')
        p.check(), buf.check()
        diff = int((p.t != q.data).sum())
        print(f'  sgd n={n} step {step}: {diff} parameters differ from torch.optim.SGD')
        assert diff == 0


@pytest.mark.parametrize('cout,cin,k,cout_pad', R.DGRAD_SHAPES, ids=lambda v: str(v))
def test_dgrad_weight_image(cout, cin, k, cout_pad):
    from yolact_minimal_amd import train_engine as T
    from yolact_minimal_amd.trainer import FlatSGD
    g = torch.Generator().manual_seed(cout)
    w = torch.randn(cout, cin, k, k, generator=g)
    img, wd = Buf(cin, k, k, cout_pad), w.to(DEV)
    ok(L().ym_pack_conv_weight_dgrad(vp(wd), vp(img), cout, cin, k, k, cout_pad, sp()), 'ym_pack_conv_weight_dgrad')
    assert same(img.check(), R.dgrad_weight_image(w.numpy(), cout_pad))
    # the batched launch: a trainer-owned weight's image is cached, and re-packed by ym_pack_conv_weights_batch after an optimizer step
    conv = torch.nn.Conv2d(cin, cout, k, bias=False).to(DEV)
    opt = FlatSGD(list(conv.parameters()), lr=0.1)
    first = T._pack_dgrad(conv.weight, cout_pad)
    assert same(first.view(cin, k, k, cout_pad), R.dgrad_weight_image(conv.weight.detach().cpu().numpy(), cout_pad))
    before = conv.weight.detach().clone()
    for p in opt.params:
        p.grad = None
        p._ym_grad_slot.normal_()
        p._ym_in_slot = True
    opt.step()
    again = T._pack_dgrad(conv.weight, cout_pad)
    torch.cuda.synchronize()
    assert again.data_ptr() == first.data_ptr() and not torch.equal(conv.weight.detach(), before)
    assert same(again.view(cin, k, k, cout_pad), R.dgrad_weight_image(conv.weight.detach().cpu().numpy(), cout_pad))


# ---- refusals before any launch ---------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone():
    c = 8
    z = torch.zeros(16, c, device=DEV)
    v = torch.ones(c, device=DEV)
    for m, cc, nbytes, want in ((16, 6, 16 * c, YM_EINVAL), (0, c, 16 * c, YM_EINVAL), (16, c, 16 * c - 1, YM_ENOSPC)):
        out, mean, invstd, ws = Buf(16, c), Buf(c), Buf(c), Buf(2 * c, dtype=torch.float64)
        before = L().ym_unordered_sum_launches()
        rc = L().ym_bn_train_fwd(vp(z), m, cc, vp(v), vp(v), EPS, MOM, None, None, None, 0, vp(out), vp(mean), vp(invstd), vp(ws), nbytes, sp())
        torch.cuda.synchronize()
        assert rc == want and all(b.untouched() for b in (out, mean, invstd, ws)) and L().ym_unordered_sum_launches() == before
        dy, dres, dg, db, ws = Buf(16, c), Buf(16, c), Buf(c), Buf(c), Buf(2 * c, dtype=torch.float64)
        rc = L().ym_bn_train_bwd(vp(z), vp(z), vp(z), m, cc, vp(v), vp(v), vp(v), vp(v), 1, vp(dy), vp(dres), vp(dg), vp(db), vp(ws), nbytes,
                                 sp())
        torch.cuda.synchronize()
        assert rc == want and all(b.untouched() for b in (dy, dres, dg, db, ws)) and L().ym_unordered_sum_launches() == before
        if want == YM_EINVAL:
            rc = L().ym_bn_train_fwd_stats(vp(z), m, cc, vp(v), vp(v), EPS, MOM, None, None, None, 0, vp(out), vp(mean), vp(invstd), vp(ws),
                                           sp())
            assert rc == want and out.untouched() and mean.untouched()
            rc = L().ym_bn_train_bwd_apply(vp(z), vp(z), vp(z), m, cc, vp(v), vp(v), vp(v), vp(v), 1, vp(dy), vp(dres), vp(dg), vp(db), vp(ws),
                                           sp())
            assert rc == want and dy.untouched() and dg.untouched()
            dz, dbias = Buf(16, c), Buf(c)
            rc = L().ym_act_bias_bwd(vp(z), vp(z), m, cc, R.ACT_RELU, vp(dz), vp(dbias), vp(ws), 16 * c, sp())
            assert rc == want and dz.untouched() and dbias.untouched()
    dbias, ws = Buf(c), Buf(c, dtype=torch.float64)
    rc = L().ym_act_bias_bwd(vp(z), None, 16, c, R.ACT_NONE, None, vp(dbias), vp(ws), 8 * c - 1, sp())
    torch.cuda.synchronize()
    assert rc == YM_ENOSPC and dbias.untouched() and ws.untouched()
    img, w = Buf(3, 3, 3, 48), torch.zeros(35, 3, 3, 3, device=DEV)
    rc = L().ym_pack_conv_weight_dgrad(vp(w), vp(img), 35, 3, 3, 3, 48, sp())
    torch.cuda.synchronize()
    assert rc == YM_EINVAL and img.untouched()
