"""Guard bands around the conv body's outputs (tests/guard.py): every convolution and pooling entry
writes into an `out=` carved from a sentinel-filled buffer, reads an input that sits inside poison,
and must leave every word around the output untouched.

N = 2; H x W = 9 x 33 (one past the 8 x 32 pixel tile both ways; odd for F(2x2); 1 mod 4 for
F(4x4)), 19 x 23 and 10 x 34; the smallest channel counts each entry accepts, plus Cout = 96 on the
f16x2 direct form (its 128-wide channel tile a quarter empty).

Inputs, weights and biases are small integers, so the direct forms (fp32, f32x3, f16x2, bf16: an
integer <= 2^8 is exact in every plane) and Winograd F(2x2, 3x3) (G has halves: U is in quarters)
are EXACT and must equal the float64 convolution.  F(4x4, 3x3) has sixths in G: it keeps the bound
of its own test, tests/test_gpu_h2.py test_conv3x3_winograd4_f16x2 (2e-5 of max|y|)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guard

pytestmark = pytest.mark.gpu

N = 2
SIZES = [(9, 33), (19, 23), (10, 34)]


@functools.lru_cache(maxsize=None)
def _case(cin, cout, h, w, dil, relu=True):
    """(x NCHW, weight OIHW, bias, float64 reference NHWC) - CPU tensors, made once, never modified."""
    rng = np.random.default_rng(1000 * cin + 10 * cout + h + w + dil)
    x = torch.from_numpy(rng.integers(-4, 5, (N, cin, h, w)).astype(np.float32))
    wt = torch.from_numpy(rng.integers(-4, 5, (cout, cin, 3, 3)).astype(np.float32))
    b = torch.from_numpy(rng.integers(-64, 65, (cout,)).astype(np.float32))
    ref = F.conv2d(x.double(), wt.double(), b.double(), padding=dil, dilation=dil)
    if relu:
        ref = ref.relu()
    assert float(ref.abs().max()) < 2 ** 24 and bool((ref > 0).any())
    return x, wt, b, ref.permute(0, 2, 3, 1).contiguous()


def _pool2(ref):
    """MaxPool 2x2 / stride 2 (floor) of an NHWC float64 tensor."""
    return F.max_pool2d(ref.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).contiguous()


def _run(dev, cin, cout, h, w, dil, call, pool2=False, x_nchw=False, exact=True, bound=None):
    """call(ops, x (in poison), weight OIHW, bias, out (carved)) runs the entry; the carved output
    must equal the reference, the guards around it and around x must be intact."""
    from naws_hip import ops
    x, wt, b, ref = _case(cin, cout, h, w, dil)
    if pool2:
        ref = _pool2(ref)
    xin = x if x_nchw else x.permute(0, 2, 3, 1).contiguous()
    gx = guard.place(xin.to(dev))
    gy = guard.carve(tuple(ref.shape), torch.float32, dev)
    ret = call(ops, gx.t, wt.to(dev), b.to(dev), gy.t)
    assert ret.data_ptr() == gy.t.data_ptr()
    got = gy.t.double().cpu()
    if exact:
        assert torch.equal(got, ref)
    else:
        assert bool(torch.isfinite(got).all())
        assert float((got - ref).abs().max()) < bound * float(ref.abs().max())
    gy.check('out')
    gx.check('x')
    return gy


def _packed(ops, wt):
    cout, cin = wt.shape[:2]
    return ops.conv3x3_pack_weight(wt).view(cout, 9 * cin)


@pytest.mark.parametrize('h,w', SIZES)
def test_c3_first_layer(dev, h, w):
    _run(dev, 3, 16, h, w, 1, lambda ops, x, wt, b, y: ops.conv3x3_c3_nchw_to_nhwc(x, wt, b, True, out=y),
         x_nchw=True)


@pytest.mark.parametrize('dil', [1, 2])
@pytest.mark.parametrize('h,w', SIZES)
def test_fp32_direct(dev, h, w, dil):
    _run(dev, 32, 4, h, w, dil,
         lambda ops, x, wt, b, y: ops.conv3x3_nhwc(x, ops.conv3x3_pack_weight(wt), b, dil, True, out=y))


def _ws_guard(dev, sizer, *dims):
    from naws_hip import lib as L
    need = getattr(L.load(), sizer)(*dims)
    assert need > 0
    return guard.carve((need,), torch.float32, dev)


@pytest.mark.parametrize('h,w', SIZES)
def test_fp32_winograd(dev, h, w):
    gws = _ws_guard(dev, 'naws_winograd_workspace_floats', N, h, w, 4, 4, 1)
    _run(dev, 4, 4, h, w, 1, lambda ops, x, wt, b, y: ops.conv3x3_winograd_nhwc(
        x, ops.winograd_weight_transform(wt), b, 1, True, out=y, workspace=gws.t))
    gws.check('workspace')


@pytest.mark.parametrize('dil', [1, 2])
@pytest.mark.parametrize('h,w', SIZES)
def test_f32x3_direct(dev, h, w, dil):
    _run(dev, 16, 4, h, w, dil, lambda ops, x, wt, b, y: ops.conv3x3_nhwc_f32x3(
        x, ops.split_bf16x3(_packed(ops, wt)), b, dil, True, out=y))


@pytest.mark.parametrize('h,w', SIZES)
def test_f32x3_direct_pool2(dev, h, w):
    _run(dev, 16, 64, h, w, 1, lambda ops, x, wt, b, y: ops.conv3x3_nhwc_f32x3(
        x, ops.split_bf16x3(_packed(ops, wt)), b, 1, True, out=y, pool2=True), pool2=True)


@pytest.mark.parametrize('h,w', SIZES)
def test_f32x3_winograd(dev, h, w):
    gws = _ws_guard(dev, 'naws_winograd_f32x3_workspace_floats', N, h, w, 16, 4, 1)
    _run(dev, 16, 4, h, w, 1, lambda ops, x, wt, b, y: ops.conv3x3_winograd_nhwc_f32x3(
        x, ops.split_bf16x3(ops.winograd_weight_transform(wt)), b, 1, True, out=y, workspace=gws.t))
    gws.check('workspace')


@pytest.mark.parametrize('with_amax', [False, True])
@pytest.mark.parametrize('mode', ['dil1', 'dil2', 'pool2'])
@pytest.mark.parametrize('cout', [32, 96])
@pytest.mark.parametrize('h,w', SIZES)
def test_f16x2_direct(dev, h, w, cout, mode, with_amax):
    """cout 32: the 64-wide channel tile half empty; cout 96: the 128-wide one a quarter empty.
    amax_out (a guarded word of its own) receives the bit pattern of max|y| of what the kernel
    stored (the pooled output under pool2): checked against the carved result."""
    dil, pool2 = (2 if mode == 'dil2' else 1), mode == 'pool2'
    gam = guard.carve((1,), torch.int32, dev) if with_amax else None

    def call(ops, x, wt, b, y):
        return ops.conv3x3_nhwc_f16x2(x, ops.split_f16x2(_packed(ops, wt)), b, True, out=y,
                                      amax_out=gam.t if gam else None, pool2=pool2, dilation=dil)
    gy = _run(dev, 32, cout, h, w, dil, call, pool2=pool2)
    if gam:
        gam.check('amax_out')
        assert gam.t.view(torch.float32).item() == float(gy.t.max())


@pytest.mark.parametrize('cin,cout', [(256, 256), (128, 256)])
@pytest.mark.parametrize('h,w', SIZES)
def test_f16x2_winograd(dev, h, w, cin, cout):
    """256 -> 256: the fused GEMM + output-transform kernel; 128 -> 256 (Cin % 256 != 0): input
    transform, batch-16 GEMM and output transform as three kernels (csrc/winograd.hip)."""
    gws = _ws_guard(dev, 'naws_winograd_f16x2_workspace_floats', N, h, w, cin, cout, 1)
    gam = guard.carve((1,), torch.int32, dev)
    gy = _run(dev, cin, cout, h, w, 1, lambda ops, x, wt, b, y: ops.conv3x3_winograd_nhwc_f16x2(
        x, ops.split_f16x2(ops.winograd_weight_transform(wt)), b, 1, True, out=y, amax_out=gam.t,
        workspace=gws.t))
    gws.check('workspace')
    gam.check('amax_out')
    assert gam.t.view(torch.float32).item() == float(gy.t.max())


@pytest.mark.parametrize('h,w', SIZES)
def test_f16x2_winograd4(dev, h, w):
    """F(4x4, 3x3): G holds sixths, U is not exact in any binary format - the bound of
    tests/test_gpu_h2.py test_conv3x3_winograd4_f16x2, unchanged: 2e-5 of max|y|."""
    gws = _ws_guard(dev, 'naws_winograd4_f16x2_workspace_floats', N, h, w, 32, 4, 1)
    _run(dev, 32, 4, h, w, 1, lambda ops, x, wt, b, y: ops.conv3x3_winograd_nhwc_f16x2(
        x, ops.split_f16x2(ops.winograd4_weight_transform(wt)), b, 1, True, out=y, workspace=gws.t),
        exact=False, bound=2e-5)
    gws.check('workspace')


@pytest.mark.parametrize('dil', [1, 2])
@pytest.mark.parametrize('h,w', SIZES)
def test_bf16_direct(dev, h, w, dil):
    _run(dev, 32, 4, h, w, dil,
         lambda ops, x, wt, b, y: ops.conv3x3_nhwc_bf16(x, ops.conv3x3_pack_weight(wt), b, dil, True, out=y))


@pytest.mark.parametrize('mode', ['dil1', 'dil2', 'pool2'])
@pytest.mark.parametrize('h,w', SIZES)
def test_bf16_wave_private(dev, h, w, mode):
    dil, pool2 = (2 if mode == 'dil2' else 1), mode == 'pool2'
    _run(dev, 64, 64, h, w, dil, lambda ops, x, wt, b, y: ops.conv3x3_nhwc_bf16_wp(
        x, ops.to_bf16_slab(_packed(ops, wt)), b, dil, True, out=y, pool2=pool2), pool2=pool2)


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('h,w', SIZES)
def test_maxpool(dev, h, w, stride):
    from naws_hip import ops
    rng = np.random.default_rng(h * w + stride)
    x = torch.from_numpy(rng.integers(-100, 101, (N, h, w, 4)).astype(np.float32))
    ref = F.max_pool2d(x.permute(0, 3, 1, 2).double(), 2, stride).permute(0, 2, 3, 1).contiguous()
    gx = guard.place(x.to(dev))
    gy = guard.carve(tuple(ref.shape), torch.float32, dev)
    ops.maxpool2x2_nhwc(gx.t, stride, out=gy.t)
    assert torch.equal(gy.t.double().cpu(), ref)
    gy.check('out')
    gx.check('x')
