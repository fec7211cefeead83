"""Host checks of tests/split_bf16_ref.py (the model tests/test_gpu_split_bf16.py holds the split-bf16 kernels to) and of that
file's launch matrix: the plane identities of the exact operands, the derived per-product error bounds, and that the planner
resolves every descriptor of the matrix to the tile, register sets and split-bf16 variant that was asked for.  No GPU."""
import ctypes
import os
import re

import pytest
import torch

from tests import split_bf16_ref as S


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def test_planes_are_bf16_and_their_residuals_exact():
    x = torch.randn(1 << 16, generator=_gen(1)) * torch.exp2(torch.randint(-20, 20, (1 << 16,), generator=_gen(2)).float())
    p = S.planes(x, 3)
    r = x.clone()
    for q in p:
        assert torch.equal(q, q.to(torch.bfloat16).float())                          # 8 significant bits
        assert torch.equal(q, r.to(torch.bfloat16).float())
        assert torch.equal((r.double() - q.double()).float().double(), r.double() - q.double())   # the fp32 residual is exact
        r = r - q
    assert bool((r.abs() <= x.abs() * 2.0 ** -24).all())
    assert S.kept_terms(3) == ((0, 0), (0, 1), (1, 0))
    assert set(S.kept_terms(6)) == set(S.kept_terms(3)) | {(0, 2), (2, 0), (1, 1)} and len(S.kept_terms(6)) == 6


def test_ints16_has_two_exact_planes():
    x, xi = S.ints16((1 << 16,), _gen(3))
    assert torch.equal(x.long(), xi) and int(xi.abs().min()) >= 1 << 8 and int(xi.abs().max()) < 1 << 16
    assert bool((xi > 0).any()) and bool((xi < 0).any())
    p0, p1, p2 = S.planes(x, 3)
    assert torch.equal(p0.long() + p1.long(), xi) and not bool(p2.any())
    nz = float((p1 != 0).float().mean())
    assert nz >= 0.95, nz                                   # ~98 %: nearly every element tests the first-order terms


def test_ints20_has_three_exact_planes():
    x, xi = S.ints20((1 << 16,), _gen(4))
    assert torch.equal(x.long(), xi) and int(xi.min()) >= 1 << 16 and int(xi.max()) < 1 << 20
    p0, p1, p2, p3 = S.planes(x, 4)
    assert torch.equal(p0.long() + p1.long() + p2.long(), xi) and not bool(p3.any())
    nz = float((p2 != 0).float().mean())
    assert nz >= 1 / 3, nz                                  # ~53 %


def test_two_plane_values_split_into_their_digits():
    x, xi = S.two_plane((1 << 16,), _gen(5))
    p0, p1, p2 = S.planes(x, 3)
    b = xi.abs() % 256
    assert int(b.min()) >= 1 and int(b.max()) <= 7 and int((xi.abs() // 256).min()) >= 8 and int((xi.abs() // 256).max()) <= 15
    assert torch.equal(p0.long(), xi.sign() * (xi.abs() - b)) and torch.equal(p1.long(), xi.sign() * b) and not bool(p2.any())
    assert int(xi.abs().max()) ** 2 < S.EXACT_LIMIT


@pytest.mark.parametrize('mma,bound', [(3, 3 * 2.0 ** -16), (6, 5 * 2.0 ** -24)])
def test_kept_terms_stay_within_the_derived_bound(mma, bound):
    """10^6 normal pairs: |sum of kept plane products - x y| <= bound |x y| (derivation: module docstring of split_bf16_ref.py;
    measured 2.7e-5 = 1.8 * 2^-16 for bf16x3 and 5.4e-8 = 0.9 * 2^-24 for bf16x6)."""
    n = 1_000_000
    x, y = torch.randn(n, generator=_gen(6)), torch.randn(n, generator=_gen(7))
    px, py = [p.double() for p in S.planes(x, 3)], [p.double() for p in S.planes(y, 3)]
    kept = sum(px[i] * py[j] for i, j in S.kept_terms(mma))
    exact = x.double() * y.double()
    rel = ((kept - exact).abs() / exact.abs()).max()
    print(f'mma {mma}: worst kept-term error {float(rel):.2e} of |x y| (bound {bound:.2e})')
    assert float(rel) <= bound


def test_emulation_and_exact_reference_agree_on_exact_operands():
    """`conv` against torch's own convolutions, and `emulate` = the exact product where the operands have no dropped term."""
    import torch.nn.functional as F
    for geo in (S.Geo('t', True, 2, 7, 32, 32, 3, 2), S.Geo('f', False, 2, 7, 32, 32, 3, 2), S.Geo('t1', True, 1, 5, 32, 64, 1, 2)):
        a, w = torch.randn(geo.in_shape, generator=_gen(8)).double(), torch.randn(geo.w_shape, generator=_gen(9)).double()
        if geo.transposed:
            opad = geo.side - ((geo.out - 1) * geo.stride - 2 * geo.pad + geo.k)
            want = F.conv_transpose2d(a.permute(0, 3, 1, 2), w, None, geo.stride, geo.pad, output_padding=opad)
        else:
            want = F.conv2d(a.permute(0, 3, 1, 2), w, None, geo.stride, geo.pad)
        torch.testing.assert_close(S.conv(a, w, geo), want.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    geo = S.Geo('e', False, 1, 6, 32, 32, 3, 1)
    a, ai = S.ints16(geo.in_shape, _gen(10))
    w, wi = S.small_ints(geo.w_shape, _gen(11), 2)
    keep = S.thin_weight(w, 64, _gen(12))[0]
    w, wi = w * keep, wi * keep
    assert S.check_exact_range(ai, wi, geo) < S.EXACT_LIMIT
    assert torch.equal(S.emulate(a, w, geo, 3).long(), S.conv(ai, wi, geo))
    with pytest.raises(AssertionError):
        S.check_exact_range(ai, S.ints16(geo.w_shape, _gen(13))[1], geo)


def _built_variants():
    """(BM, BN, MODE, NS, DL, PF, RG, SPL) of every conv_igemm_f32 instantiation in launch_igemm's list (conv_mfma.hip)."""
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'yolact_minimal_amd', 'csrc', 'conv_mfma.hip')
    rows = re.findall(r'^\s*YM_V\(\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+)\)\s*$', open(src).read(), re.M)
    return {tuple(int(v) for v in r) for r in rows}


def test_every_descriptor_of_the_gpu_matrix_resolves_on_the_host():
    """ym_conv2d_effective_plan for every (case, mma) of tests/test_gpu_split_bf16.py: YM_OK, the asked tile, stages 3 where 3 was
    asked and else 2, the asked K split (the class-ordered plan of a stride-2 data gradient without arrival counters falls back to
    the gather over all taps, where K has all its tiles again), the tail; and the variant is in launch_igemm's list, which holds
    all 32 split-bf16 instantiations (forward / data gradient x bf16x3 / bf16x6 x four tiles x one / two register sets)."""
    from yolact_minimal_amd import hip
    built = _built_variants()
    split = {v for v in built if v[7]}
    assert split == {(bm, bn, mode, ns, 0, 0, 0, spl) for bm, bn in S.TILES for mode in (0, 2) for ns in (2, 3) for spl in (2, 3)}
    seen = set()
    cases = S.cases()
    assert len(cases) >= 6 * 10
    for case in cases:
        for mma in (0, 3, 6):
            d = S.descriptor(case, mma, 0x1000, 0x2000, 0x10000, 0x3000, add=0x6000 if case.add else None)
            eff = hip.conv_effective_plan(d)                   # raises unless YM_OK
            g = case.geo
            assert (eff.tile_m, eff.tile_n) == case.tile, (case.id, mma, eff)
            if mma:
                assert eff.stages == (3 if case.stages == 3 else 2), (case.id, mma, eff)
                assert eff.kwaves == 0 and eff.grid_wgs == 0
                variant = (eff.tile_m, eff.tile_n, 2 if g.transposed else 0, eff.stages, 0, 0, 0, S.nplanes(mma))
                assert variant in built, (case.id, mma, variant)
                seen.add(variant)
            nkt = g.K // 32
            if g.transposed and g.stride == 2 and (case.counters or case.ksplit == 1):
                nkt = (-(-g.k // 2)) ** 2 * (g.cout // 32)                 # the largest parity class's taps
            want_ks = -(-nkt // -(-nkt // case.ksplit))
            assert eff.ksplit == want_ks, (case.id, mma, eff, want_ks)
            assert (eff.tail_tiles, eff.tail_ksplit) == case.tail, (case.id, mma, eff)
            lib = hip.lib()
            tiles = lib.ym_conv2d_tile_counters(ctypes.byref(d))
            slots = case.ksplit > 1 or case.tail[0] > 0
            if slots and not (g.transposed and g.stride == 2):
                assert tiles == -(-g.M // case.tile[0]) * -(-g.N // case.tile[1]), (case.id, tiles)
            assert lib.ym_conv2d_fuses_bn_stats(ctypes.byref(d)) == int(case.counters or not slots), case.id
    assert seen == split, sorted(split - seen)
