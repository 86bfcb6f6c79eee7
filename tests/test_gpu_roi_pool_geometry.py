"""RoIPoolF off the 7x7, 1/8 geometry: every kernel form against the CPU oracle, bit for bit.

The reference of every check is oracle.roi_pool_f followed by oracle.roi_feature_boost (tied to the
operator's definition at each of these geometries by test_roi_geometry_cases.py): the maximum is
exact and the boost is one fp32 multiply, so no tolerance appears in this file - the operand
writers are decoded on the CPU (their scale is a power of two) and compared bit for bit as well.
The one bound, of the backward's atomic sums, is the one of test_gpu_body_backward.py.

Case lists and the census that keeps them from being vacuous: roi_geometry_cases.py."""
import functools

import numpy as np
import pytest
import torch

import body_grad_ref as bgr
import guard
import roi_geometry_cases as g

pytestmark = pytest.mark.gpu

FAST = [e for e in g.GEOMETRIES if e[0] * e[1] <= g.FAST_LIMIT]
PAST = [e for e in g.GEOMETRIES if e[0] * e[1] > g.FAST_LIMIT]
LARGE = [e for e in g.GEOMETRIES if e[0] * e[1] >= 196]
SWEEPS = [(1, 1, 1 / 8), (1, 1, 1 / 16), (2, 2, 1 / 8), (2, 2, 1 / 16)]
# (geometry, roi list, map): the random and the rounding list at every geometry, the sweeps at
# pooled 1x1 and 2x2 (both scales), the large grids on the 5x7 map too (every bin <= 1 pixel)
CASES = ([(e, name, 'map') for e in g.GEOMETRIES for name in ('random', 'rounding')]
         + [(e, name, 'map') for e in SWEEPS for name in ('interior', 'clipped')]
         + [(e, 'random', 'small') for e in LARGE])
FAST_CASES = [c for c in CASES if c[0] in FAST or c[0] in SWEEPS]


def _id(case):
    (ph, pw, scale), name, where = case
    return '%dx%d-s%d-%s-%s' % (ph, pw, round(1 / scale), name, where)


def _t(a, dev):
    return torch.from_numpy(np.array(a, order='C')).to(dev)     # (a copy: the cached arrays are read-only)


def _dims(where):
    return (g.MAP_H, g.MAP_W) if where == 'map' else (g.SMALL_H, g.SMALL_W)


@functools.lru_cache(maxsize=None)
def _rois(name, scale, where):
    h, w = _dims(where)
    r = {'random': lambda: g.random_rois(h, w, scale), 'rounding': lambda: g.rounding_rois(scale),
         'interior': lambda: g.window_sweep(h, w, scale),
         'clipped': lambda: g.clipped_sweep(h, w, scale)}[name]()
    assert r.shape[0] % 2 == 1                                     # an odd count, every list
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def _x(where, operand):
    """[2, 128, H, W]; operand: the input of the fp16 / bf16 writers - the NaN pixel zeroed, image
    1 at a hundredth of image 0's range."""
    h, w = _dims(where)
    x = g.features(128, h, w)
    if operand:
        x = np.nan_to_num(x, nan=0.0)
        x[1] *= np.float32(0.01)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _ref(case, operand=False):
    """(y boosted, argmax, boost) of the 128-channel tensor, computed once per case and shared
    (read-only); fewer channels are its leading slice."""
    from oracle import oracle
    (ph, pw, scale), name, where = case
    rois = _rois(name, scale, where)
    y, am = oracle.roi_pool_f(_x(where, operand), rois, ph, pw, scale)
    boost = g.boost_for(rois.shape[0])
    y = oracle.roi_feature_boost(y, boost)
    for a in (y, am, boost):
        a.setflags(write=False)
    return y, am, boost


@pytest.fixture(scope='module')
def dev_x(dev):
    """dev_x(where, operand, c, layout): the first c channels of _x on the device, uploaded once per
    module and released with it."""
    cache = {}

    def get(where, operand, c, layout):
        key = (where, operand, c, layout)
        if key not in cache:
            x = _t(_x(where, operand)[:, :c], dev)
            cache[key] = x.permute(0, 2, 3, 1).contiguous() if layout == 'NHWC' else x
        return cache[key]
    yield get
    cache.clear()


def _same(t, ref):
    """Bit for bit (NaN-safe, signed zeros apart)."""
    got = t.detach().cpu().numpy()
    bits = {4: np.int32, 2: np.int16}[got.dtype.itemsize]
    return got.shape == ref.shape and np.array_equal(got.view(bits), np.ascontiguousarray(ref).view(bits))


# ------------------------------------------------------------------------------- fp32 forms ----
@pytest.mark.parametrize('case', CASES, ids=_id)
def test_fp32_forms_bitexact(dev, case, dev_x):
    """ops.roi_pool_f, NCHW and NHWC, with and without argmax, C = 30 (scalar kernel), 68 (float4
    kernel, ragged 256-channel tile) and 128 (XCD-sliced kernel; hier=True too): values and argmax.
    Past 256 bins (16x17) the plain entry stays exact through whichever kernel it falls to."""
    from naws_hip import ops
    (ph, pw, scale), name, where = case
    y_ref, am_ref, boost = _ref(case)
    assert np.isnan(_x(where, False)).any()
    rois = _t(_rois(name, scale, where), dev)
    bd = _t(boost, dev)
    for c in (30, 68, 128):
        for layout in ('NCHW', 'NHWC'):
            xd = dev_x(where, False, c, layout)
            y, am = ops.roi_pool_f(xd, rois, ph, pw, scale, boost=bd, layout=layout, with_argmax=True)
            assert _same(am, am_ref[:, :c]), (c, layout, 'argmax')
            assert _same(y, y_ref[:, :c]), (c, layout, 'with argmax')
            y2 = ops.roi_pool_f(xd, rois, ph, pw, scale, boost=bd, layout=layout)
            assert _same(y2, y_ref[:, :c]), (c, layout)
    if ph * pw <= g.FAST_LIMIT:
        yh = ops.roi_pool_f(dev_x(where, False, 128, 'NHWC'), rois, ph, pw, scale, boost=bd,
                            layout='NHWC', hier=True)
        assert _same(yh, y_ref), 'hier'
    # without the boost (a null pointer in every kernel): the plain maxima
    if name == 'rounding':
        from oracle import oracle
        plain, _ = oracle.roi_pool_f(_x(where, False)[:, :68], _rois(name, scale, where), ph, pw, scale)
        for layout in ('NCHW', 'NHWC'):
            y3 = ops.roi_pool_f(dev_x(where, False, 68, layout), rois, ph, pw, scale, layout=layout)
            assert _same(y3, plain), layout


# -------------------------------------------------------------------------- operand writers ----
def _amax_bits(x):
    return np.array([np.abs(x[i]).max() for i in range(x.shape[0])], np.float32)


def _f16x2_expected(y, batch, boost, amax):
    """The CPU decode of the fp16x2 operand of y [R, K] (boosted): s_r = 2^(141 - e), e the
    exponent field of fp32(amax[batch] * |boost|) clamped to [40, 250] (141 for a zero or
    non-finite bound) - the rule of naws_f16x2_scales; t = y * s_r is exact, hi = fp16(t), lo =
    fp16(t - hi) (0 where |t| > 65504).  -> (planes uint16 [2, K/16, R, 16], inv_scale fp32 [R])."""
    bound = (amax[np.minimum(batch, len(amax) - 1)] * np.abs(boost)).astype(np.float32)
    bits = bound.view(np.uint32)
    e = ((bits >> 23) & 0xff).astype(np.int64)
    e[(bits == 0) | (e == 0xff)] = 127 + 14
    e = np.clip(e, 40, 250)
    s = np.ldexp(np.float32(1), 141 - e).astype(np.float32)
    inv = np.ldexp(np.float32(1), e - 141).astype(np.float32)
    assert np.array_equal(1 / s, inv)
    t = (y * s[:, None]).astype(np.float32)
    assert np.array_equal(t.astype(np.float64), y.astype(np.float64) * s[:, None])    # exact
    hi = t.astype(np.float16)
    rr = t - hi.astype(np.float32)
    rr[~(np.abs(t) <= 65504)] = 0
    lo = rr.astype(np.float16)
    r, k = y.shape
    lay = lambda a: a.view(np.uint16).reshape(r, k // 16, 16).transpose(1, 0, 2)
    return np.ascontiguousarray(np.stack([lay(hi), lay(lo)])), inv


def _operand_case(case, c, dev, dev_x):
    (ph, pw, scale), name, where = case
    y_ref, _, boost = _ref(case, True)
    x = _x(where, True)
    rois = _rois(name, scale, where)
    amax = _amax_bits(x[:, :c])
    assert 50 < amax[0] / amax[1] < 200                             # the two images' own maxima
    y = np.array(y_ref[:, :c], order='C').reshape(rois.shape[0], -1)     # (a copy: the cache is read-only)
    xd = dev_x(where, True, c, 'NHWC')
    words = _t(amax.view(np.int32), dev)
    return y, rois, boost, amax, xd, words


@pytest.mark.parametrize('case', FAST_CASES, ids=_id)
def test_f16_planes_bitexact_against_a_cpu_decode(dev, case, dev_x):
    """roi_pool_f_f16x2 direct, hierarchical and over caller-built maps, and the per-image _range
    form split at an odd r0 with odd counts: planes == fp16(t), fp16(t - fp16(t)) of the oracle's
    boosted maxima in the [2, K/16, R, 16] layout, inv_scale == 1 / s_r, all bit for bit."""
    from naws_hip import ops
    (ph, pw, scale), name, where = case
    for c in (64, 128):
        y, rois, boost, amax, xd, words = _operand_case(case, c, dev, dev_x)
        r, k = y.shape
        planes, inv = _f16x2_expected(y, rois[:, 0].astype(np.int64), boost, amax)
        rd, bd = _t(rois, dev), _t(boost, dev)
        m2, m4 = torch.empty_like(xd), torch.empty_like(xd)
        ops.roi_maxmaps(xd, m2, m4)
        forms = {
            'direct': ops.roi_pool_f_f16x2(xd, rd, words, ph, pw, scale, boost=bd, hier=False),
            'hier': ops.roi_pool_f_f16x2(xd, rd, words, ph, pw, scale, boost=bd, hier=True),
            'maps': ops.roi_pool_f_f16x2(xd, rd, words, ph, pw, scale, boost=bd, maps=(m2, m4)),
        }
        out = ops.roi_pool_operand(r, k, dev)
        out.planes.view(torch.int16).fill_(0x7FC1)
        out.scales.fill_(float('nan'))
        cut = 37 if r > 40 else 5                                   # an odd r0, odd counts
        for r0, r1 in ((cut, r - 1), (0, cut), (r - 1, r)):
            assert (r1 - r0) % 2 == 1
            ops.roi_pool_f_f16x2_range(xd, rd, words, out, r0, r1, (m2, m4), ph, pw, scale, boost=bd)
        forms['range'] = out
        for form, op in forms.items():
            assert op.planes.shape == (2, k // 16, r, 16), form
            assert _same(op.planes.view(torch.int16), planes.view(np.int16)), (c, form)
            assert _same(op.inv_scale, inv), (c, form)


@pytest.mark.parametrize('case', FAST_CASES, ids=_id)
def test_bf16_slab_bitexact_against_the_rounded_oracle(dev, case, dev_x):
    from naws_hip import ops
    (ph, pw, scale), name, where = case
    for c in (64, 128):
        y, rois, boost, amax, xd, words = _operand_case(case, c, dev, dev_x)
        r, k = y.shape
        want = torch.from_numpy(y).bfloat16().view(r, k // 16, 16).permute(1, 0, 2).contiguous()
        m2, m4 = torch.empty_like(xd), torch.empty_like(xd)
        ops.roi_maxmaps(xd, m2, m4)
        slab = ops.roi_pool_f_bf16_slab(xd, _t(rois, dev), (m2, m4), ph, pw, scale, boost=_t(boost, dev))
        assert slab.shape == (k // 16, r, 16)
        assert _same(slab.view(torch.int16), want.view(torch.int16).numpy()), c


# --------------------------------------------------------------------------------- transposes ----
def test_transposes_at_a_k_that_is_no_multiple_of_256(dev, dev_x):
    """f16_planes_transpose / bf16_slab_transpose on pooled 3x5 operands of 64 channels (K = 960,
    three 256-feature blocks and a ragged fourth), R = 81: the exact transposition, pad rows zero,
    nothing outside the result touched."""
    from naws_hip import ops
    case = ((3, 5, 1 / 8), 'random', 'map')
    y, rois, boost, amax, xd, words = _operand_case(case, 64, dev, dev_x)
    r, k = y.shape
    assert (r, k) == (81, 960) and k % 256 != 0
    rd, bd = _t(rois, dev), _t(boost, dev)
    planes, _ = _f16x2_expected(y, rois[:, 0].astype(np.int64), boost, amax)
    op = ops.roi_pool_f_f16x2(xd, rd, words, 3, 5, 1 / 8, boost=bd)
    rpad = 96
    dense = planes.transpose(0, 2, 1, 3).reshape(2, r, k)                      # [2, R, K]
    want = np.zeros((2, rpad, k), np.uint16)
    want[:, :r] = dense
    want = np.ascontiguousarray(want.reshape(2, rpad // 16, 16, k).transpose(0, 1, 3, 2))
    gq = guard.carve((2 * (rpad // 16), k, 16), torch.float16, dev)
    tp = ops.f16_planes_transpose(op, out=gq.t.view(2, rpad // 16, k, 16))
    assert _same(tp.planes.view(torch.int16), want.view(np.int16))
    assert bool((tp.inv_scale == 1).all())
    gq.check('transposed planes')
    # the bf16 slab: Rpad = 128
    m2, m4 = torch.empty_like(xd), torch.empty_like(xd)
    ops.roi_maxmaps(xd, m2, m4)
    slab = ops.roi_pool_f_bf16_slab(xd, rd, (m2, m4), 3, 5, 1 / 8, boost=bd)
    yb = torch.from_numpy(y).bfloat16().view(torch.int16).numpy()              # [R, K]
    rp = 128
    wb = np.zeros((rp, k), np.int16)
    wb[:r] = yb
    wb = np.ascontiguousarray(wb.reshape(rp // 16, 16, k).transpose(0, 2, 1))
    gb = guard.carve((rp // 16, k, 16), torch.bfloat16, dev)
    q = ops.bf16_slab_transpose(slab, out=gb.t)
    assert _same(q.view(torch.int16), wb)
    gb.check('transposed slab')


# ----------------------------------------------------------------------------------- backward ----
@pytest.mark.parametrize('geom', [(3, 5, 1 / 8), (6, 6, 1 / 8)], ids=['3x5', '6x6'])
def test_backward_against_a_float64_scatter(dev, geom, dev_x):
    """roi_pool_f_grad through the forward's own argmax, NCHW and NHWC: per element within
    n_e 2^-24 sum|terms| of the float64 scatter-add (the bound of test_roi_pool_f_gradient: the
    worst case of any summation order, so it holds under atomics); elements without a term are 0.
    dX is carved: nothing outside it is written."""
    from naws_hip import ops, lib as L
    ph, pw, scale = geom
    case = (geom, 'random', 'map')
    rois = _rois('random', scale, 'map')
    c = 68
    n, h, w = 2, g.MAP_H, g.MAP_W
    rd = _t(rois, dev)
    xd = dev_x('map', True, c, 'NCHW')
    _, am = ops.roi_pool_f(xd, rd, ph, pw, scale, with_argmax=True)
    amn = am.cpu().numpy()
    assert np.array_equal(amn, _ref(case, True)[1][:, :c])
    dy = np.random.default_rng(31).standard_normal(amn.shape).astype(np.float32)
    ref, cnt, asum = bgr.roi_pool_grad64(dy, amn, rois, (n, c, h, w))
    assert cnt.max() >= 4 and (cnt == 0).any()
    bound = cnt * 2.0 ** -24 * asum
    dyd = _t(dy, dev)
    g1 = ops.roi_pool_f_grad(dyd, am, rd, (n, c, h, w)).cpu().numpy()
    g2 = ops.roi_pool_f_grad(dyd, am, rd, (n, h, w, c), layout='NHWC').cpu().numpy().transpose(0, 3, 1, 2)
    for name, got in (('NCHW', g1), ('NHWC', g2)):
        err = np.abs(got - ref)
        print('RoIPoolF grad %dx%d %s: max err %.3g, max err / bound %.3g, up to %d terms'
              % (ph, pw, name, err.max(), (err[cnt > 0] / np.maximum(bound[cnt > 0], 1e-300)).max(),
                 cnt.max()))
        assert (err <= bound).all(), name
        assert not got[cnt == 0].any(), name
    gx = guard.carve((n * h * w * c,), torch.float32, dev)
    L.call('naws_roi_pool_f_bwd', dyd.data_ptr(), am.data_ptr(), rd.data_ptr(), rois.shape[0],
           L.LAYOUT_NHWC, n, c, h, w, ph, pw, gx.t.data_ptr(), torch.cuda.current_stream().cuda_stream)
    got = gx.t.view(n, h, w, c).cpu().numpy().transpose(0, 3, 1, 2)
    assert (np.abs(got - ref) <= bound).all()
    gx.check('dX')


# ------------------------------------------------------------------------------ past the limit ----
@pytest.mark.parametrize('geom', PAST, ids=lambda e: '%dx%d' % e[:2])
def test_fast_entries_refuse_more_than_256_bins_before_they_launch(dev, geom, dev_x):
    """16x17: the plane, slab and hierarchical entries raise NawsError(UNSUPPORTED); outputs and
    workspace prefilled with the sentinel still hold it (nothing was enqueued)."""
    from naws_hip import ops, lib as L
    ph, pw, scale = geom
    c, r = 64, 5
    k = c * ph * pw
    xd = dev_x('map', True, c, 'NHWC')
    n, h, w, _ = xd.shape
    rd = _t(_rois('rounding', scale, 'map')[:r], dev)
    words = _t(_amax_bits(_x('map', True)[:, :c]).view(np.int32), dev)
    m2, m4 = torch.empty_like(xd), torch.empty_like(xd)
    ops.roi_maxmaps(xd, m2, m4)
    s = torch.cuda.current_stream().cuda_stream
    gp = guard.carve((2 * (k // 16), r, 16), torch.float16, dev)
    gs = guard.carve((2, r), torch.float32, dev)
    gy = guard.carve((r, k), torch.float32, dev)
    gw = guard.carve((2 * n * h * w * c,), torch.float32, dev)
    op = ops.F16x2(gp.t.view(2, k // 16, r, 16), gs.t)
    geo = (ph, pw, float(scale))
    head = (xd.data_ptr(), n, c, h, w, rd.data_ptr(), r, 0)
    calls = {
        'direct': lambda: L.call('naws_roi_pool_f_f16x2_fwd', *head, *geo, words.data_ptr(), n,
                                 gp.t.data_ptr(), gs.t.data_ptr(), s),
        'hier': lambda: L.call('naws_roi_pool_f_f16x2_hier_fwd', *head, *geo, words.data_ptr(), n,
                               gw.t.data_ptr(), gp.t.data_ptr(), gs.t.data_ptr(), s),
        'maps': lambda: L.call('naws_roi_pool_f_f16x2_mapped_fwd', *head, *geo, words.data_ptr(), n,
                               m2.data_ptr(), m4.data_ptr(), gp.t.data_ptr(), gs.t.data_ptr(), s),
        'range': lambda: ops.roi_pool_f_f16x2_range(xd, rd, words, op, 1, 4, (m2, m4), ph, pw, scale),
        'slab': lambda: L.call('naws_roi_pool_f_bf16_slab_mapped_fwd', *head, *geo, m2.data_ptr(),
                               m4.data_ptr(), gp.t.data_ptr(), s),
        'fp32 hier': lambda: ops.roi_pool_f(xd, rd, ph, pw, scale, layout='NHWC', hier=True,
                                            out=gy.t.view(r, c, ph, pw), workspace=gw.t),
    }
    for form, fn in calls.items():
        with pytest.raises(L.NawsError) as ei:
            fn()
        assert ei.value.code == L.ERR_UNSUPPORTED, form
    torch.cuda.synchronize()
    for what, gd in (('planes', gp), ('scales', gs), ('y', gy), ('workspace', gw)):
        assert guard.holds_sentinel(gd.t), what
        gd.check(what)


# --------------------------------------------------------------------------------- guard bands ----
GUARDED = [((3, 5, 1 / 8), 30, 'NHWC'), ((3, 5, 1 / 8), 30, 'NCHW'), ((5, 3, 1 / 16), 68, 'NHWC'),
           ((4, 9, 1 / 8), 128, 'NHWC'), ((12, 12, 1 / 16), 30, 'NHWC'), ((10, 16, 1 / 16), 30, 'NHWC'),
           ((14, 14, 1 / 8), 30, 'NHWC'), ((16, 16, 1 / 8), 128, 'NHWC'),
           ((16, 17, 1 / 8), 30, 'NHWC'), ((16, 17, 1 / 8), 68, 'NHWC'), ((16, 17, 1 / 8), 128, 'NHWC')]


@pytest.mark.parametrize('geom,c,layout', GUARDED,
                         ids=['%dx%d-c%d-%s' % (e[0], e[1], c, l) for e, c, l in GUARDED])
def test_fp32_forms_write_inside_their_output_only(dev, geom, c, layout, dev_x):
    """Every fp32 kernel (scalar staged / unstaged, float4, XCD-sliced, hierarchical, NCHW) into a
    carved Y: every element written, nothing around it; the hierarchical form's workspace too."""
    from naws_hip import ops, lib as L
    ph, pw, scale = geom
    case = (geom, 'random', 'map')
    y_ref, am_ref, boost = _ref(case)
    rois = _rois('random', scale, 'map')
    r = rois.shape[0]
    rd, bd = _t(rois, dev), _t(boost, dev)
    xd = dev_x('map', False, c, layout)
    for unaligned in (False, True):
        gy = guard.carve((r, c * ph * pw), torch.float32, dev, aligned=not unaligned)
        y = ops.roi_pool_f(xd, rd, ph, pw, scale, boost=bd, layout=layout, out=gy.t.view(r, c, ph, pw))
        assert _same(y, y_ref[:, :c])
        gy.check('Y')
    if c % 64 == 0 and ph * pw <= g.FAST_LIMIT:
        n, h, w, _ = xd.shape
        need = L.load().naws_roi_pool_workspace_floats(n, c, h, w)
        gw = guard.carve((need,), torch.float32, dev)
        gy = guard.carve((r, c * ph * pw), torch.float32, dev)
        y = ops.roi_pool_f(xd, rd, ph, pw, scale, boost=bd, layout='NHWC', hier=True,
                           out=gy.t.view(r, c, ph, pw), workspace=gw.t)
        assert _same(y, y_ref[:, :c])
        gy.check('Y (hier)')
        gw.check('workspace')


@pytest.mark.parametrize('geom', [(5, 3, 1 / 16), (12, 12, 1 / 16), (14, 14, 1 / 8), (16, 16, 1 / 8)],
                         ids=['5x3', '12x12', '14x14', '16x16'])
def test_operand_writers_write_inside_their_planes_only(dev, geom, dev_x):
    """The K-slab write-out of every operand form into carved planes / scales (C entries): each
    element written, bit-exact, nothing around them; the hierarchical form's workspace too.
    12x12 and above ask for more than 64 KB of LDS for two rois, 16x16 for one as well."""
    from naws_hip import ops, lib as L
    ph, pw, scale = geom
    case = (geom, 'random', 'map')
    c = 64
    y, rois, boost, amax, xd, words = _operand_case(case, c, dev, dev_x)
    r, k = y.shape
    n, h, w, _ = xd.shape
    planes, inv = _f16x2_expected(y, rois[:, 0].astype(np.int64), boost, amax)
    rd, bd = _t(rois, dev), _t(boost, dev)
    m2, m4 = torch.empty_like(xd), torch.empty_like(xd)
    ops.roi_maxmaps(xd, m2, m4)
    s = torch.cuda.current_stream().cuda_stream
    geo = (ph, pw, float(scale))
    head = (xd.data_ptr(), n, c, h, w, rd.data_ptr(), r, bd.data_ptr())
    need = L.load().naws_roi_pool_workspace_floats(n, c, h, w)
    for form in ('direct', 'hier', 'maps', 'range'):
        gp = guard.carve((2 * (k // 16), r, 16), torch.float16, dev)
        gs = guard.carve((2, r), torch.float32, dev)
        gw = guard.carve((need,), torch.float32, dev)
        tail = (gp.t.data_ptr(), gs.t.data_ptr(), s)
        if form == 'direct':
            L.call('naws_roi_pool_f_f16x2_fwd', *head, *geo, words.data_ptr(), n, *tail)
        elif form == 'hier':
            L.call('naws_roi_pool_f_f16x2_hier_fwd', *head, *geo, words.data_ptr(), n,
                   gw.t.data_ptr(), *tail)
        elif form == 'maps':
            L.call('naws_roi_pool_f_f16x2_mapped_fwd', *head, *geo, words.data_ptr(), n,
                   m2.data_ptr(), m4.data_ptr(), *tail)
        else:
            op = ops.F16x2(gp.t.view(2, k // 16, r, 16), gs.t)
            for r0, r1 in ((37, r), (0, 37)):
                ops.roi_pool_f_f16x2_range(xd, rd, words, op, r0, r1, (m2, m4), ph, pw, scale, boost=bd)
        assert _same(gp.t.view(torch.int16).view(2, k // 16, r, 16), planes.view(np.int16)), form
        assert _same(gs.t[1], inv), form
        assert guard.holds_sentinel(gs.t[0]), form                 # (row 0 of the scales: unused)
        for what, gd in (('planes', gp), ('scales', gs), ('workspace', gw)):
            gd.check('%s (%s)' % (what, form))
    gb = guard.carve((k // 16, r, 16), torch.bfloat16, dev)
    L.call('naws_roi_pool_f_bf16_slab_mapped_fwd', *head, *geo, m2.data_ptr(), m4.data_ptr(),
           gb.t.data_ptr(), s)
    want = torch.from_numpy(y).bfloat16().view(r, k // 16, 16).permute(1, 0, 2).contiguous()
    assert _same(gb.t.view(torch.int16), want.view(torch.int16).numpy())
    gb.check('slab')
