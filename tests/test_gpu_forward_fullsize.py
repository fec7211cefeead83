"""GPU: every FORWARD row of the tuned table (tuned_gfx950.json: plain, `_mma3`, `_L5`, `_st`, `_tp` keys), launched alone through
ym_conv2d_fwd under exactly the plan its row names, at a real layer geometry (tests/conv_geometry.py), against fp64 -- the forward
twin of test_gpu_train_fullsize.py.  A row decides which kernel computes a layer (register staging, register ring, direct-to-LDS
ring, wave kernel with DMA rings, persistent walker, weight-stationary 1x1), with which tile, K split, tail split and grid; the
end-to-end digests run the 544 px rows only and cannot be tight per layer.

Per row:
1. the launch is accepted and leaves ym_last_error alone; rows with a K split or a tail split report the row's own tile count through
   ym_conv2d_tile_counters.  The library is asked which plan it runs for the launch's descriptor (ym_conv2d_effective_plan) and
   that plan is the row's own -- tile, kwaves, kernel family and ring depth, tail -- or, for a row of
   conv_geometry.KNOWN_FALLBACKS, exactly the plan listed there; the family a row is tallied under is the one that ran;
2. the output was prefilled with NaN: none is left;
3. the guard bands around every output segment keep their fill pattern;
4. EVERY output element is compared with an fp64 evaluation of the same fp32 operands (plain torch ops on the device, one fp64
   GEMM per filter tap; pyramid levels one by one, so zero padding cannot leak across a level boundary);
5. max|got - ref| <= 1e-4 * max|ref| per output segment, operands scaled as in the sibling file (weights / sqrt(Cin k^2)), for the
   f32 rows and for the split-bf16 (`_mma3`) rows alike;
6. the arrival counters are all zero again, and a second launch into the same (re-poisoned) buffers is bit-identical.
`_st` rows also have their two fused per-channel BatchNorm sums checked over the whole output.

No row is skipped: a shard fails unless it launched every key it was given, and the shards partition the forward keys of the
table.  The table is read through engine.tuned_table() (YM_TUNED_PATH: tools/table_gate.py runs this file against a candidate
table); YM_FORWARD_ROW_KEYS=key,key,... narrows the run to those keys (unset = all).

Wall time on one MI355X, same machine and call: 4.2 s for this file (1351 rows, 7.3 Tflop of fp64 reference), 3.7 s for
test_gpu_train_fullsize.py (195 rows, sampled references) -- so every row gets the full fp64 comparison, none the hybrid one.
Measured then: worst error 2.1e-5 of max|ref| on the split-bf16 rows, <= 5.8e-6 on every f32 family.
"""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

from tests import conv_geometry as G

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NSHARDS = 8
KEYS_ENV = 'YM_FORWARD_ROW_KEYS'
GUARD = 1024                    # floats before and after a plain output (a multiple of 4: the vector epilogue needs 16-byte alignment)
ANCHORS_BEFORE, ANCHORS_AFTER = 37, 29      # anchors of other levels around a segmented head output, per image
FILL = -12345.0
BAR = 1e-4                      # the project's per-launch bar: max|got - ref| <= BAR * max|ref|
HEAD_CUTS = (0, 243, 255, 351)  # conf | bbox | coef of the fused prediction head (3 anchors x 81 / 4 / 32), tanh on the third
ACT_NONE, ACT_RELU, ACT_TANH = 0, 1, 2

_tally = {}                     # shard -> (launched, worst, {family: [rows, worst]})


def selected_keys():
    from yolact_minimal_amd.engine import tuned_table
    keys = G.forward_keys(tuned_table())
    only = os.environ.get(KEYS_ENV)
    if only is not None:
        want = {k for k in only.split(',') if k}
        keys = [k for k in keys if k in want]
    return keys


def _shards(items, n=NSHARDS):
    return [items[i::n] for i in range(n)]


class Launch:
    """Operands, output buffers with guard bands, descriptor and fp64 reference of one row's launch."""

    def __init__(self, g, plan, mma, gen, counters):
        from yolact_minimal_amd import conv_launch, hip
        self.g, self.plan = g, plan
        b, N, C, k = g.batch, g.N, g.C, g.k
        cin = 3 if C == 4 else C
        self.sides = [(s, s) for s in g.levels] if g.levels else [(g.h, g.ho)]          # (input side, output side) per level
        self.x = [torch.randn(b, hi, hi, C, device=DEV, generator=gen) for hi, _ in self.sides]
        if C == 4:                                                                      # the image: channel 3 is padding
            for x in self.x:
                x[..., 3] = 0
        self.x_all = torch.cat([x.reshape(-1, C) for x in self.x]) if g.levels else self.x[0]
        self.w = torch.randn(N, cin, k, k, device=DEV, generator=gen) * (1.0 / (cin * k * k) ** 0.5)
        k_pad = (k * k * C + 31) // 32 * 32
        self.wp = hip.pack_conv_weight(self.w, C, k_pad)
        self.pix = sum(ho * ho for _, ho in self.sides)                                 # output pixels per image
        assert b * self.pix == g.M, g.describe()
        self.scale = self.shift = self.residual = self.sums = None
        if g.nseg == 3:
            assert (N, C, k, g.stride) == (351, 256, 3, 1) and not g.residual, g.describe()
            self.cuts, self.acts = HEAD_CUTS, (ACT_NONE, ACT_NONE, ACT_TANH)
            self.shift = torch.randn(N, device=DEV, generator=gen) * 0.1
        else:
            assert g.nseg == 1, g.describe()
            self.cuts = (0, N)
            if g.suffix == '_st':                    # the training forward: raw conv output + its BatchNorm sums
                self.acts = (ACT_NONE,)
                self.sums = torch.zeros(2, N, device=DEV, dtype=torch.float64)
            else:                                    # folded BatchNorm + ReLU
                self.acts = (ACT_RELU,)
                self.scale = torch.rand(N, device=DEV, generator=gen) + 0.5
                self.shift = torch.randn(N, device=DEV, generator=gen) * 0.1
        if g.residual:
            assert not g.levels, g.describe()
            self.residual = torch.randn(g.M, N, device=DEV, generator=gen)
        # ---- outputs ----
        self.bufs, self.regions, segs = [], [], []
        if g.nseg == 1:
            buf = torch.full((GUARD + g.M * N + GUARD,), FILL, device=DEV)
            self.bufs.append(buf)
            self.regions.append(buf[GUARD:GUARD + g.M * N])
            segs.append((0, N, self.regions[0].data_ptr(), 0 if g.levels else g.ho * g.ho * N, N, self.acts[0]))
        else:
            na = 3                                   # anchors per pixel
            n, n_total = self.pix * na, ANCHORS_BEFORE + self.pix * na + ANCHORS_AFTER
            for i in range(3):
                c = (self.cuts[i + 1] - self.cuts[i]) // na
                t = torch.full((b, n_total, c), FILL, device=DEV)
                self.bufs.append(t)
                self.regions.append(t[:, ANCHORS_BEFORE:ANCHORS_BEFORE + n])
                segs.append((self.cuts[i], self.cuts[i + 1], t.data_ptr() + ANCHORS_BEFORE * c * 4, n_total * c, na * c, self.acts[i]))
        # ---- descriptor: the engines' own builder ----
        hi, ho = self.sides[0]
        d = self.desc = conv_launch.conv_desc(b, hi, hi, C, N, k, k, g.stride, g.pad, ho, ho, k_pad, segs,
                                              levels=self.sides if g.levels else None)
        d.inp, d.weight = self.x_all.data_ptr(), self.wp.data_ptr()
        d.scale = self.scale.data_ptr() if self.scale is not None else None
        d.shift = self.shift.data_ptr() if self.shift is not None else None
        d.residual = self.residual.data_ptr() if self.residual is not None else None
        plan.apply(d)
        d.mma = mma
        d.tile_counters = counters.data_ptr()
        lib = hip.lib()
        lib.ym_conv2d_workspace_bytes(None)                       # plants a known message in ym_last_error()
        self.sentinel = lib.ym_last_error()
        nbytes = lib.ym_conv2d_workspace_bytes(ctypes.byref(d))
        assert lib.ym_last_error() == self.sentinel, (g.describe(), lib.ym_last_error())
        self.tiles = lib.ym_conv2d_tile_counters(ctypes.byref(d))
        if self.sums is not None:
            assert lib.ym_conv2d_fuses_bn_stats(ctypes.byref(d)) == 1, g.describe()
            d.bn_sum, d.bn_sumsq = self.sums[0].data_ptr(), self.sums[1].data_ptr()
        self.ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=DEV)

    def poison(self):
        for r in self.regions:
            r.fill_(float('nan'))
        if self.sums is not None:
            self.sums.zero_()

    def run(self):
        from yolact_minimal_amd import hip
        hip.conv2d_fwd(self.desc, self.ws)
        torch.cuda.synchronize()
        assert hip.lib().ym_last_error() == self.sentinel, (self.g.describe(), hip.lib().ym_last_error())

    def got(self):
        """[M, Cout] in the reference's row order."""
        if self.g.nseg == 1:
            return self.regions[0].view(self.g.M, self.g.N)
        b = self.g.batch
        return torch.cat([r.reshape(b, self.pix, -1) for r in self.regions], 2).reshape(self.g.M, self.g.N)

    def guards_intact(self):
        if self.g.nseg == 1:
            buf = self.bufs[0]
            return bool((buf[:GUARD] == FILL).all()) and bool((buf[-GUARD:] == FILL).all())
        n = self.regions[0].shape[1]
        return all(bool((t[:, :ANCHORS_BEFORE] == FILL).all()) and bool((t[:, ANCHORS_BEFORE + n:] == FILL).all()) for t in self.bufs)

    def reference(self):
        """fp64 [M, Cout] of the same fp32 operands: one fp64 GEMM per filter tap and level, then the epilogue in fp64."""
        g = self.g
        b, N, C, k, s, pad = g.batch, g.N, g.C, g.k, g.stride, g.pad
        wd = self.w.double()
        if C == 4:
            wd = F.pad(wd, (0, 0, 0, 0, 0, 1))                    # a zero filter for the padding channel
        levels = []
        for x, (hi, ho) in zip(self.x, self.sides):
            xp = F.pad(x.double(), (0, 0, pad, pad, pad, pad))
            acc = torch.zeros(b * ho * ho, N, device=DEV, dtype=torch.float64)
            for kh in range(k):
                for kw in range(k):
                    xs = xp[:, kh:kh + s * (ho - 1) + 1:s, kw:kw + s * (ho - 1) + 1:s].reshape(-1, C)
                    acc.addmm_(xs, wd[:, :, kh, kw].t())
            del xp
            levels.append(acc.view(b, ho * ho, N))
        if g.nseg == 1:                               # plain output: the input's row order ([level][image][pixel])
            y = torch.cat([v.reshape(-1, N) for v in levels]) if len(levels) > 1 else levels[0].reshape(-1, N)
        else:                                         # segmented output: [image][level][pixel], the reference's cat over levels
            y = torch.cat(levels, 1).reshape(-1, N)
        del levels
        if self.scale is not None:
            y *= self.scale.double()
        if self.shift is not None:
            y += self.shift.double()
        if self.residual is not None:
            y += self.residual.double()
        for i, act in enumerate(self.acts):
            seg = y[:, self.cuts[i]:self.cuts[i + 1]]
            if act == ACT_RELU:
                seg.clamp_(min=0)
            elif act == ACT_TANH:
                seg.tanh_()
        return y


def check_row(key, row, gen, counters):
    """Launch one row and check points 1-6 of the module docstring; returns (kernel family, error as a fraction of max|ref|)."""
    g = G.resolve(key)
    assert g is not None, f'{key}: no layer of any model / image size / batch has this shape'
    plan, mma = G.launch_plan(g, row)
    L = Launch(g, plan, mma, gen, counters)
    effective = G.check_effective(g, row, plan, mma, L.desc)
    where = f'{g.describe()} row {row}'
    if plan.tile_m and plan.ksplit >= 1:                       # the row's own tile count, when slices of K meet in memory
        split = plan.tail_tiles > 0 or (plan.ksplit > 1 and not plan.wave)
        full = -(-g.M // plan.tile_m) * -(-g.N // plan.tile_n)
        assert L.tiles == (full if split else 0), (where, L.tiles, full)
    L.poison()
    L.run()
    got = L.got()
    assert not bool(torch.isnan(got).any()), f'{where}: {int(torch.isnan(got).sum())} output elements were not written'
    assert L.guards_intact(), f'{where}: wrote outside its output'
    ref = L.reference()
    assert ref.shape == got.shape and ref.numel() == g.M * g.N
    diff = (got.double() - ref).abs_()
    err = 0.0
    for i in range(len(L.acts)):
        n0, n1 = L.cuts[i], L.cuts[i + 1]
        e = float(diff[:, n0:n1].max() / ref[:, n0:n1].abs().max())
        err = max(err, e)
        if e > BAR:
            at = divmod(int(diff[:, n0:n1].argmax()), n1 - n0)
            bad = (diff[:, n0:n1] > BAR * ref[:, n0:n1].abs().max()).nonzero()
            raise AssertionError(f'{where}: segment {i} error {e:.3e} of max|ref| (worst at row {at[0]}, channel {n0 + at[1]}; {len(bad)} '
                                 f'elements over the bar, rows {int(bad[:, 0].min())}..{int(bad[:, 0].max())}, '
                                 f'channels {n0 + int(bad[:, 1].min())}..{n0 + int(bad[:, 1].max())})')
    if L.sums is not None:
        # sums of the launch's OWN fp32 output (tight: fp64 accumulation, at most a 32-row partial sum in fp32 = 32 * 2^-24 relative
        # to sum|y|) -- and with the output within BAR * max|ref| of fp64 everywhere, within M * BAR * max|ref| of the fp64 sums
        y = got.double()
        s0, s1, a0 = y.sum(0), (y * y).sum(0), y.abs().sum(0)
        assert bool(((L.sums[0] - s0).abs() <= 1e-5 * a0).all()) and bool(((L.sums[1] - s1).abs() <= 1e-5 * s1).all()), \
            (where, float(((L.sums[0] - s0).abs() / a0).max()), float(((L.sums[1] - s1).abs() / s1).max()))
        r0, r1, top = ref.sum(0), (ref * ref).sum(0), float(ref.abs().max())
        assert bool(((L.sums[0] - r0).abs() <= g.M * BAR * top).all()) and bool(((L.sums[1] - r1).abs() <= 3 * g.M * BAR * top * top).all()), where
    del ref, diff
    assert bool((counters == 0).all()), f'{where}: {int((counters != 0).sum())} arrival counters left non-zero'
    first = [t.clone() for t in L.bufs]
    L.poison()
    L.run()
    assert all(torch.equal(a, t) for a, t in zip(first, L.bufs)), f'{where}: a second launch into the same buffers differs'
    assert bool((counters == 0).all()), where
    return G.family(g, effective, mma), err


@pytest.mark.parametrize('shard', range(NSHARDS))
def test_every_tuned_forward_launch_at_full_size(shard):
    from yolact_minimal_amd.engine import tuned_table
    from yolact_minimal_amd import hip
    table = tuned_table()
    keys = _shards(selected_keys())[shard]
    if os.environ.get(KEYS_ENV) is None:
        assert keys
    gen = torch.Generator(device=DEV).manual_seed(300 + shard)
    counters = torch.zeros(hip.TILE_COUNTERS, device=DEV, dtype=torch.int32)
    launched, failed, fams = [], [], {}
    for key in keys:
        try:
            fam, err = check_row(key, table[key], gen, counters)
        except AssertionError as e:
            failed.append(f'{key}: {e}')
            counters.zero_()
        except RuntimeError as e:
            if 'ym_conv2d_fwd failed' not in str(e):         # anything else, a device fault above all: nothing more is started on it
                pytest.exit(f'{key} row {table[key]}: {e}', returncode=3)
            failed.append(f'{key} row {table[key]}: rejected: {e}')
        else:
            f = fams.setdefault(fam, [0, 0.0])
            f[0], f[1] = f[0] + 1, max(f[1], err)
            launched.append(key)
    worst = max([v[1] for v in fams.values()], default=0.0)
    _tally[shard] = (len(launched), worst, fams)
    print(f'forward rows, shard {shard}: {len(launched)} of {len(keys)} launched and checked, worst error {worst:.2e} of max|ref|; '
          + ', '.join(f'{k} {n} ({e:.1e})' for k, (n, e) in sorted(fams.items())))
    assert failed == [], '\n'.join(failed)
    assert launched == keys                                   # nothing skipped: there is no exclusion list


def test_the_shards_cover_every_forward_key():
    """The shards partition the selected keys (all forward keys of the table unless narrowed), and whatever shards ran in this
    process launched all of theirs; with every shard run, the total is the number of forward keys in the table."""
    from yolact_minimal_amd.engine import tuned_table
    keys = selected_keys()
    shards = _shards(keys)
    assert sorted(k for s in shards for k in s) == keys and len(set(keys)) == len(keys)
    if os.environ.get(KEYS_ENV) is None:
        assert keys == G.forward_keys(tuned_table()) and len(keys) > 1000
    for shard, (n, _, _) in _tally.items():
        assert n == len(shards[shard]), (shard, n, len(shards[shard]))
    if len(_tally) == NSHARDS:
        total, fams = 0, {}
        for n, _, f in _tally.values():
            total += n
            for k, (rows, e) in f.items():
                t = fams.setdefault(k, [0, 0.0])
                t[0], t[1] = t[0] + rows, max(t[1], e)
        print(f'forward rows: {total} launched of {len(keys)} keys; ' + ', '.join(f'{k} {n} ({e:.1e})' for k, (n, e) in sorted(fams.items())))
        assert total == len(keys)
