"""CPU: what train_engine launches for a convolution.  `_conv_forward`, `_conv_dgrad` and `_conv_wgrad_now` run on CPU tensors with the
launches replaced by recorders, and everything that reaches a launch (cache key, descriptor, workspace request, fused BatchNorm sums,
ordered partials and their finish) is compared with tests/golden/train_conv_launches.json, recorded at the commit its `recorded_at`
names (`python tests/test_train_launch_cpu.py --record <commit>`) and not re-recorded since: a change to the launch path keeps every
launch what it was.  The planner's queries (ym_conv2d_fuses_bn_stats, ym_conv2d_bn_partial_rows, ym_conv2d_workspace_bytes,
ym_conv2d_wgrad_workspace_bytes) are host-only and answer for real, from the committed tuned table.  No GPU, no kernel launch."""
import ctypes
import json
import os
import sys

import pytest
import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'train_conv_launches.json')
CONFIGS = [(det, mma) for det in (False, True) for mma in (0, 3)]
HOST_ONLY = ('ym_conv2d_fuses_bn_stats', 'ym_conv2d_bn_partial_rows', 'ym_conv2d_workspace_bytes', 'ym_conv2d_wgrad_workspace_bytes')
COUNTERS = 0x3000
# the plain tuples the recording commit used as cache keys, by position (a key with `_asdict` names its own fields)
TUPLE_KEYS = {'f': 'kind device b h w cin cout kh kw stride pad act residual stats segs mma ordered',
              'd': 'kind device b h w cin cout kh kw stride pad ho wo residual mma stats ordered',
              'w': 'kind device b h w cin_pad cin ho wo cout_pad cout kh kw stride pad segs'}


def _ru(x, m):
    return (x + m - 1) // m * m


def _key_fields(key):
    f = key._asdict() if hasattr(key, '_asdict') else dict(zip(TUPLE_KEYS[key[0]].split(), key))
    return {k: v for k, v in f.items() if v is not None}          # (a field a kind does not use is None, or was not there)


def _desc_fields(s, role):
    """The non-zero fields of a ctypes descriptor; every pointer (c_void_p) as the role of the tensor it points to."""
    out = {}
    for name, ct in s._fields_:
        v = getattr(s, name)
        if issubclass(ct, ctypes.Array):
            if issubclass(ct._type_, ctypes.Structure):
                v = [_desc_fields(e, role) for e in v]
                while v and not v[-1]:
                    v.pop()
            elif ct._type_ is ctypes.c_void_p:
                v = [role(e) for e in v] if any(v) else []
            else:
                v = list(v) if any(v) else []
        elif ct is ctypes.c_void_p:
            v = role(v) if v else None
        if v:
            out[name] = v
    return out


class Rig:
    """The device out of the way: recorders for the launches, fixed fakes for the buffers, the real library for the queries."""

    def __init__(self, monkeypatch, det, mma):
        from yolact_minimal_amd import engine as E, hip, train_engine as T
        self.T, self.hip = T, hip
        self.roles, self.launches, self.queries = {}, [], 0
        self.scratch_req = self.part_req = None
        real = hip.lib()
        rig = self

        class Lib:
            def __getattr__(self, name):
                if name in HOST_ONLY:
                    def query(*a):
                        rig.queries += 1
                        return getattr(real, name)(*a)
                    return query
                if name == 'ym_last_error':
                    return real.ym_last_error
                if name in ('ym_conv2d_wgrad', 'ym_conv2d_wgrad_slabs'):
                    return lambda ref, ws, nbytes, *rest: rig._launched(ref._obj, name, nbytes) or 0
                if name in ('ym_pack_conv_weight', 'ym_pack_conv_weight_dgrad'):         # (the image itself is not looked at)
                    return lambda src, dst, *rest: rig.roles.__setitem__(dst.value, 'w') or 0
                raise AssertionError(f'{name}: not a host-only call, and no launch this test replaces')

        with open(os.path.join(os.path.dirname(E.__file__), 'tuned_gfx950.json')) as f:
            self.table = json.load(f)
        for v in ('YM_TUNE_TRAIN', 'YM_AUTOTUNE', 'YM_FORCE_STAGES', 'YM_FORCE_GRID', 'YM_TUNED_NEAREST', 'YM_DGRAD_CLASSES'):
            monkeypatch.delenv(v, raising=False)
        monkeypatch.setenv('YM_TRAIN_MMA', str(mma))
        monkeypatch.setattr(T, '_DETERMINISTIC', det)
        monkeypatch.setattr(T, '_table', lambda: self.table)
        monkeypatch.setattr(T, '_desc_cache', {})
        monkeypatch.setattr(T, 'launch_counts', {})
        monkeypatch.setattr(T, '_stats_pool', T._StatsPool())
        monkeypatch.setattr(T, '_pending_reduce', {})
        monkeypatch.setattr(T, '_slab_arena', {})
        monkeypatch.setattr(T, 'scratch', self._scratch)
        monkeypatch.setattr(T, '_partials', self._partials)
        monkeypatch.setattr(T, '_finish_partials', self._finish)
        monkeypatch.setattr(T, '_tile_counters', lambda dev: COUNTERS)
        monkeypatch.setattr(hip, 'lib', lambda: Lib())
        monkeypatch.setattr(hip, 'conv2d_fwd', lambda d, ws=None: self._launched(d, 'ym_conv2d_fwd', None))
        monkeypatch.setattr(hip, 'stream_ptr', lambda: None)
        monkeypatch.setattr(hip, 'ptr', lambda t, dtype=torch.float32: None if t is None else ctypes.c_void_p(t.data_ptr()))
        monkeypatch.setattr(torch.cuda, 'current_device', lambda: 0)

    # ---- the replaced pieces ----
    def _scratch(self, dev, nbytes):
        self.scratch_req = nbytes
        return torch.empty(max(nbytes, 16), dtype=torch.uint8)

    def _partials(self, dev, rows, c):
        self.part_req = (rows, c)
        self.part = torch.empty(rows * 2 * c, dtype=torch.float64)
        self.roles[self.part.data_ptr()] = 'partials'
        return self.part

    def _finish(self, part, rows, c, stats):
        assert part is self.part and self.launches and 'finish' not in self.launches[-1]
        self.launches[-1]['finish'] = dict(rows=rows, c=c, sums=stats.data_ptr())

    def _launched(self, d, entry, ws_numel):
        self.launches.append(dict(entry=entry, desc=type(d).from_buffer_copy(d), ws_numel=ws_numel, scratch=self.scratch_req, part=self.part_req))
        self.scratch_req = self.part_req = None

    # ---- one call ----
    def tensor(self, role, *shape, dtype=torch.float32):
        t = torch.empty(*shape, dtype=dtype)
        self.name(t, role)
        return t

    def name(self, t, role):
        self.roles[t.data_ptr()] = role

    def role(self, p):
        assert p in self.roles, f'a pointer to nothing this call was given: {p:#x}'
        return self.roles[p]

    def call(self, fn, named=None):
        """Run one engine call (exactly one launch); the record of what it launched.  `named(result)`: roles known only afterwards."""
        T = self.T
        before, n_cache, self.queries = dict(T.launch_counts), len(T._desc_cache), 0
        del self.launches[:]
        self.roles[COUNTERS] = 'counters'
        result = fn()
        if named is not None:
            named(result)
        (key,) = [k for k, n in T.launch_counts.items() if n != before.get(k, 0)]
        (ln,) = self.launches
        d = ln['desc']
        rec = dict(key=_key_fields(key), entry=ln['entry'], desc=_desc_fields(d, self.role), ws_bytes=ln['scratch'],
                   fuses=bool(getattr(d, 'bn_sum', None)), part_rows=ln['part'][0] if ln['part'] else 0, finish=None)
        if 'finish' in ln:
            rec['finish'] = dict(ln['finish'], sums=self.role(ln['finish']['sums']))
            assert ln['part'] == (ln['finish']['rows'], ln['finish']['c'])
        if ln['entry'] == 'ym_conv2d_wgrad_slabs':              # (private slab scratch instead of the stream's)
            rec['ws_bytes'] = ln['ws_numel']
        ent = T._desc_cache[key]
        if hasattr(ent, '_fields'):                              # (the recording commit kept plain tuples of another order per kind)
            assert (ent.fuses, ent.ws_bytes, ent.part_rows) == (rec['fuses'], rec['ws_bytes'], rec['part_rows'])
            assert bytes(ent.desc) == bytes(d)
        self.first_use = len(T._desc_cache) > n_cache
        assert self.first_use or self.queries == 0, 'a cached shape asked the library again'
        self.roles.clear()
        return json.loads(json.dumps(rec)), result

    # ---- the engine's three entry points on fresh CPU tensors ----
    def forward(self, b, hw, cin, cout, k, stride, stats=False, shift=False, act=0, residual=False, out=False, head=False):
        T = self.T
        pad = k // 2
        ho = (hw + 2 * pad - k) // stride + 1
        k_pad = cin if (k == 1 and cin % 32 == 0) else _ru(k * k * cin, 32)
        x, wp = self.tensor('x', b, hw, hw, cin), self.tensor('w', _ru(cout, 32) if head else cout, k_pad)
        kw = {}
        if stats:
            st = kw['bn_stats'] = self.tensor('stats', 2 * cout, dtype=torch.float64)
            self.roles[st.data_ptr() + 8 * cout] = 'stats+8C'
        if residual:
            kw['residual'] = self.tensor('residual', b, ho, ho, cout)
        if out:
            kw['out'] = self.tensor('out', b, ho, ho, cout)
        if head:                                                  # conf | box | coef of the 544 px anchors, this level first
            n_total, nc, cd, na = 18525, 81, 32, 3
            ends = (0, na * nc, na * nc + na * 4, cout)
            assert ends[-1] == na * (nc + 4 + cd)
            outs = [(self.tensor(name, b, n_total, c), a) for name, c, a in (('conf', nc, T.ACT_NONE), ('box', 4, T.ACT_NONE), ('coef', cd, T.ACT_TANH))]
            kw['segs'] = [(ends[i], ends[i + 1], t.data_ptr(), n_total * t.shape[2], ends[i + 1] - ends[i], a) for i, (t, a) in enumerate(outs)]
        sh = self.tensor('shift', _ru(cout, 32) if head else cout) if shift else None

        def named(res):
            y = res[0] if stats else res
            if y is not None:
                self.name(y, 'out')
        rec, res = self.call(lambda: T._conv_forward(x, wp, k_pad, cout, k, k, stride, pad, sh, act, **kw), named)
        if stats:
            assert res[1] == rec['fuses']
        return rec

    def dgrad(self, b, hw, cin, cout_pad, k, stride, add=False, link=False, out=False):
        T = self.T
        pad = k // 2
        ho = (hw + 2 * pad - k) // stride + 1
        dz, w = self.tensor('dz', b, ho, ho, cout_pad), torch.empty(cout_pad, cin, k, k)
        kw, keep = {}, []
        if add:
            kw['add'] = self.tensor('add', b, hw, hw, cin)
        if out:
            kw['out'] = self.tensor('out', b, hw, hw, cin)
        if link:
            ln = kw['bn_bwd'] = T.BnGradLink()
            keep = [self.tensor('bnb.' + n, *s) for n, s in (('y', (b, hw, hw, cin)), ('mean', (cin,)), ('invstd', (cin,)), ('gamma', (cin,)), ('beta', (cin,)))]
            ln.y, ln.mean, ln.invstd, ln.gamma, ln.beta = [t.data_ptr() for t in keep]
            ln.out, ln.relu, ln.c, ln.m = None, 1, cin, b * hw * hw
        T._stats_pool.begin(torch.device('cpu'))

        def named(dx):
            self.name(dx, 'out')
            if link and ln.stats is not None:
                self.name(ln.stats, 'stats')
                self.roles[ln.stats.data_ptr() + 8 * cin] = 'stats+8C'
        rec, dx = self.call(lambda: T._conv_dgrad(dz, w, cout_pad, (b, hw, hw, cin), stride, pad, **kw), named)
        if link:
            assert (ln.stats is not None) == rec['fuses'] and (ln.dout_ptr == dx.data_ptr()) == rec['fuses']
        return rec

    def wgrad(self, b, hw, cin, cout, k, stride, segments=False, accumulate=False, defer=False):
        T = self.T
        pad = k // 2
        ho = (hw + 2 * pad - k) // stride + 1
        x, dz = self.tensor('x', b, hw, hw, cin), self.tensor('dy', b, ho, ho, _ru(cout, 32))
        kw = dict(accumulate=accumulate, defer=defer)
        if segments:                                              # the head's three parameters behind one 351-channel filter
            kw['dw'] = self.tensor('dw', 243, cin, k, k)
            kw['segments'] = (243, 255, self.tensor('dw1', 12, cin, k, k), self.tensor('dw2', 96, cin, k, k))
        elif accumulate or defer:
            kw['dw'] = self.tensor('dw', cout, cin, k, k)
        rec, dw = self.call(lambda: T._conv_wgrad_now(x, dz, (cout, cin, k, k), stride, pad, **kw), lambda dw: self.name(dw, 'dw'))
        assert rec['fuses'] is False and rec['part_rows'] == 0 and (kw.get('dw') is None or dw is kw['dw'])
        return rec


def run_cases(rig):
    """[(case, record)]: res101 at 544 px, batch 8 (shapes the tuned table has rows for) unless the name says otherwise."""
    T, t = rig.T, rig.table
    out = []

    def case(name, rec, first_use=True):
        assert rig.first_use == first_use, name
        out.append([name, rec])
    case('stem 7x7 s2, stats', rig.forward(8, 544, 4, 64, 7, 2, stats=True))
    case('1x1 1024>256, stats', rig.forward(8, 34, 1024, 256, 1, 1, stats=True))
    case('3x3 s1 64>64, stats', rig.forward(8, 136, 64, 64, 3, 1, stats=True))
    case('3x3 s2 128>128, stats', rig.forward(8, 136, 128, 128, 3, 2, stats=True))
    assert 52 <= t['M36992_N512_C128_k1_s1_seg1_r0_st'][4] <= 54 and t['M147968_N64_C256_k1_s1_seg1_r0_st'][4] == 22
    case('1x1 128>512, stats, _st row (weight-stationary)', rig.forward(8, 68, 128, 512, 1, 1, stats=True))
    case('1x1 256>64, stats, _st row', rig.forward(8, 136, 256, 64, 1, 1, stats=True))
    case('3x3 256>256, shift + ReLU, out=', rig.forward(8, 68, 256, 256, 3, 1, shift=True, act=T.ACT_RELU, out=True))
    case('1x1 1024>256, shift, residual', rig.forward(8, 34, 1024, 256, 1, 1, shift=True, residual=True))
    case('head 3x3 256>351, three segments', rig.forward(8, 68, 256, 351, 3, 1, shift=True, head=True))
    for stride, (hw, cin, cout) in ((1, (34, 256, 256)), (2, (136, 128, 128))):
        case(f'dgrad 3x3 s{stride}', rig.dgrad(8, hw, cin, cout, 3, stride))
        case(f'dgrad 3x3 s{stride}, add', rig.dgrad(8, hw, cin, cout, 3, stride, add=True))
        case(f'dgrad 3x3 s{stride}, BnGradLink', rig.dgrad(8, hw, cin, cout, 3, stride, link=True))
        case(f'dgrad 3x3 s{stride}, BnGradLink, again', rig.dgrad(8, hw, cin, cout, 3, stride, link=True), first_use=False)
    case('dgrad 1x1 256>1024, add, BnGradLink, out=', rig.dgrad(8, 34, 256, 1024, 1, 1, add=True, link=True, out=True))
    case('dgrad head 3x3 256<352', rig.dgrad(8, 68, 256, 352, 3, 1, out=True))
    case('wgrad 3x3 256>256', rig.wgrad(8, 34, 256, 256, 3, 1))
    case('wgrad 3x3 256>256, accumulate', rig.wgrad(8, 34, 256, 256, 3, 1, accumulate=True), first_use=False)
    case('wgrad 3x3 256>256, slabs only', rig.wgrad(8, 34, 256, 256, 3, 1, defer=True), first_use=False)
    case('wgrad head 3x3 256>351, segments', rig.wgrad(8, 68, 256, 351, 3, 1, segments=True))
    case('wgrad 3x3 s2 128>128', rig.wgrad(8, 136, 128, 128, 3, 2))
    # 256 px, batch 4: no row of their own -> the nearest tuned shape's (plan_transfer); the last one has a row, for the wave kernel
    assert not any(k in t for k in ('M4096_N512_C128_k1_s1_seg1_r0', 'M4096_N512_C128_k1_s1_seg1_r0_st', 'T_M4096_N256_C256_k3_s1'))
    case('256 px: 1x1 128>512, stats', rig.forward(4, 32, 128, 512, 1, 1, stats=True))
    case('256 px: dgrad 3x3 s1, BnGradLink', rig.dgrad(4, 32, 256, 256, 3, 1, link=True))
    assert t['M4096_N64_C64_k3_s1_seg1_r0'][3] > 0
    case('256 px: 3x3 64>64, stats, wave kernel', rig.forward(4, 32, 64, 64, 3, 1, stats=True))
    return out


def _name(det, mma):
    return f'deterministic {int(det)}, YM_TRAIN_MMA={mma}'


@pytest.mark.parametrize('det,mma', CONFIGS)
def test_every_launch_is_what_the_recording_commit_launched(monkeypatch, det, mma):
    """Cache key, descriptor (pointers by role), workspace request, fused sums, partial rows and finish of every case, equal to the
    fixture's; a second call of a shape hits the cache, asks the library nothing and rebinds every pointer (a stale one has no role)."""
    with open(FIXTURE) as f:
        want = json.load(f)
    got = run_cases(Rig(monkeypatch, det, mma))
    assert [n for n, _ in got] == [n for n, _ in want['launches'][_name(det, mma)]]
    for (name, g), (_, w) in zip(got, want['launches'][_name(det, mma)]):
        assert g == w, (name, {k: (g[k], w[k]) for k in g if g[k] != w.get(k)})
    # the cases do reach the paths they are named for
    recs = dict(got)
    assert all(r['fuses'] == (not r['desc'].get('kwaves')) for n, r in got if 'stats' in n or 'BnGradLink' in n)     # (wave kernels do not fuse)
    assert not recs['256 px: 3x3 64>64, stats, wave kernel']['fuses'] and recs['256 px: dgrad 3x3 s1, BnGradLink']['fuses']
    assert all((r['part_rows'] > 0) == (det and r['fuses']) and (r['finish'] is not None) == (r['part_rows'] > 0) for _, r in got)
    assert (recs['1x1 128>512, stats, _st row (weight-stationary)']['desc'].get('stages') in (52, 53, 54)) == (mma == 0)     # (an f32 kernel)
    assert {r['desc'].get('mma', 0) for n, r in got if r['entry'] == 'ym_conv2d_fwd' and 'stem' not in n and not r['desc'].get('kwaves')} == {mma}
    assert recs['stem 7x7 s2, stats']['desc'].get('mma', 0) == 0 and recs['wgrad 3x3 256>256, slabs only']['entry'] == 'ym_conv2d_wgrad_slabs'


def test_cache_keys_are_named_and_keep_what_tells_launches_apart():
    """Every `_desc_cache` key is a ConvKey or a WgradKey, every entry a CacheEntry; launches that differ only in the deterministic
    switch, only in YM_TRAIN_MMA or only in whether a gradient is added get keys of their own."""
    keys = set()
    for det, mma in CONFIGS:
        with pytest.MonkeyPatch.context() as mp:
            rig = Rig(mp, det, mma)
            T = rig.T
            rig.forward(8, 34, 1024, 256, 1, 1, stats=True)
            rig.dgrad(8, 34, 256, 256, 3, 1, link=True)
            rig.dgrad(8, 34, 256, 256, 3, 1, link=True, add=True)
            rig.wgrad(8, 34, 256, 256, 3, 1)
            assert len(T._desc_cache) == 4
            assert all(isinstance(k, (T.ConvKey, T.WgradKey)) and isinstance(e, T.CacheEntry) for k, e in T._desc_cache.items())
            assert sorted(k.kind for k in T._desc_cache) == ['d', 'd', 'f', 'w']
            assert all(k.mma == mma and k.ordered == det and k.stats for k in T._desc_cache if k.kind != 'w')
            assert sorted(k.residual for k in T._desc_cache if k.kind == 'd') == [False, True]
            keys |= {k for k in T._desc_cache if k.kind != 'w'}
    assert len(keys) == 3 * len(CONFIGS)


if __name__ == '__main__':                         # python tests/test_train_launch_cpu.py --record <commit the tree is at>
    assert sys.argv[1] == '--record' and len(sys.argv) == 3
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    launches = {}
    for det_, mma_ in CONFIGS:
        with pytest.MonkeyPatch.context() as mp_:
            launches[_name(det_, mma_)] = run_cases(Rig(mp_, det_, mma_))
    with open(FIXTURE, 'w') as f_:
        json.dump(dict(recorded_at=sys.argv[2], pointers='by the role of the tensor they point to; fields that are zero / null are left out',
                       launches=launches), f_, indent=0, sort_keys=True)
    print(sum(len(v) for v in launches.values()), 'launches ->', FIXTURE)
