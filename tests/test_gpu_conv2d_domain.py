"""naws_conv2d_nhwc_fwd over everything include/naws.h (a-1c) says it accepts: kernel 1 / 3 / 7 x
stride 1 / 2 x dilation 1 / 2 x every pad in 0 .. dilation * (kernel - 1) - 60 forms, written down
here from the header's rule, not asked of the code under test - on (Cin, Cout) = (3, 32) (the gather
path, K = 3 / 27 / 147 in one to five chunks that are mostly padding), (32, 96) (a K chunk is one
tap; the second 64-channel tile half empty) and (64, 32) (two K chunks inside one tap; kernel 7
walks 49 taps).

Exact inputs, as tests/test_gpu_guard_conv.py: x and weight are integers in [-4, 4], the bias an
integer in [-64, 64]; the kernel runs on the fp32-input MFMA, the largest K is 49 * 64 = 3136, so
every partial sum is an integer below 16 * 3136 + 64 < 2^24, exact in fp32 in any order: the result
must EQUAL F.conv2d in float64, element for element (torch.equal; no tolerance anywhere here).

Sizes, N = 2 throughout (e = H + 2 pad - span is what the floor rule divides, span =
dilation * (kernel - 1) + 1):
  (a) H = W = max(1, span - 2 pad): the smallest legal input - 1 x 1 outputs (M = 2) while
      2 pad < span; beyond that a single pixel, whose output is (2 pad - span + 1) / stride + 1
      wide and holds windows that lie in padding altogether (they give the bias alone);
  (b) H != W, both >= span - 2 pad + 3: e = 9 x 12 at stride 1 (10 x 13 outputs), 17 x 22 at stride 2
      (9 x 12 outputs; one e odd, one even: the floor rule), more where the pad is so large that H
      or W would fall below 2 x 3; Ho * Wo is never a multiple of 64, so a 64-pixel tile holds
      pixels of both images.
Image 1 is zero but for its top-left pixel (4 in every channel): a window of image 0 that ran on
into the next image picks it up as a wrong integer.

At size (b) every form is run with bias / without x ReLU / without; at the extreme pads (0 and the
maximum) X sits inside poison and Y is carved from a sentinel-filled buffer (tests/guard.py).

The test of the test: at size (b) the float64 reference differs, in image 0, from the reference with
the weight's kh and kw swapped, from the one with dilation 1 in place of 2 (dilation 1, and kernel 1
whose single tap no dilation moves: pad + 1 instead, cropped), and at stride 2 from the windows one
pixel further on.  A 1 x 1 weight has nothing to swap: that wrong reference does not exist for
kernel 1 and is not made."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guard

pytestmark = pytest.mark.gpu

N = 2
KERNELS, STRIDES, DILATIONS = (1, 3, 7), (1, 2), (1, 2)             # include/naws.h (a-1c)
GROUPS = [(k, s, d) for k in KERNELS for s in STRIDES for d in DILATIONS]
CHANNELS = [(3, 32), (32, 96), (64, 32)]
ERR_SHAPE, ERR_ARG, ERR_NULL, ERR_UNSUPPORTED = -1, -2, -3, -5       # include/naws.h


def _span(k, d):
    return d * (k - 1) + 1


def _pads(k, d):
    """The header's rule: any 0 <= pad <= dilation * (kernel - 1)."""
    return list(range(0, d * (k - 1) + 1))


def _out(h, w, k, s, p, d):
    """The header's floor rule."""
    return (h + 2 * p - _span(k, d)) // s + 1, (w + 2 * p - _span(k, d)) // s + 1


def _size_a(k, s, p, d):
    h = max(1, _span(k, d) - 2 * p)
    e = h + 2 * p - _span(k, d)
    assert e >= 0 and (e == 0 or h == 1) and _out(h, h, k, s, p, d) == (e // s + 1, e // s + 1)
    return h, h


def _size_b(k, s, p, d):
    low = _span(k, d) - 2 * p
    eh, ew = (9, 12) if s == 1 else (17, 22)
    h, w = max(2, low + eh), max(3, low + ew)

    def good(h, w):
        ho, wo = _out(h, w, k, s, p, d)
        parity = s == 1 or (h - low) % 2 != (w - low) % 2
        return h != w and parity and (ho * wo) % 64 != 0
    while not good(h, w):
        w += 1
    ho, wo = _out(h, w, k, s, p, d)
    assert h != w and h >= low + 3 and w >= low + 3 and 64 < ho * wo < 400 and (ho * wo) % 64 != 0
    assert s == 1 or sorted(((h - low) % 2, (w - low) % 2)) == [0, 1]
    return h, w


def _inputs(cin, cout, k, h, w, seed):
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.integers(-4, 5, (N, cin, h, w)).astype(np.float32))
    x[1] = 0
    x[1, :, 0, 0] = 4.0
    wt = torch.from_numpy(rng.integers(-4, 5, (cout, cin, k, k)).astype(np.float32))
    b = torch.from_numpy(rng.integers(-64, 65, (cout,)).astype(np.float32))
    return x, wt, b


def _refs(x, wt, b, s, p, d, mixed=True):
    """{(bias, relu): float64 NHWC reference}; the inputs keep every one of them below 2^24, and the
    ReLU ones hold zeros and non-zeros (mixed False: the few outputs of size (a), where every
    window may lie in padding and the output is the bias alone, are not asked for that)."""
    pre = F.conv2d(x.double(), wt.double(), None, s, p, d)
    out = {}
    for bias in (False, True):
        y = pre + b.double().view(1, -1, 1, 1) if bias else pre
        for relu in (False, True):
            r = (y.relu() if relu else y).permute(0, 2, 3, 1).contiguous()
            assert float(r.abs().max()) < 2 ** 24
            if relu and mixed:
                assert bool((r == 0).any()) and bool((r > 0).any())
            out[(bias, relu)] = r
    return out


def _wrong_refs(x, wt, s, p, d, ref):
    """The wrong references of the module docstring, each cropped to ref's shape (NHWC, no bias)."""
    k = wt.shape[2]
    n, ho, wo, _c = ref.shape
    x64, w64 = x.double(), wt.double()

    def crop(y):
        assert y.shape[2] >= ho and y.shape[3] >= wo
        return y[:, :, :ho, :wo].permute(0, 2, 3, 1).contiguous()
    # stride 1 with one more pixel of padding: full[i] is the window that starts at i - 1 - pad
    full = F.conv2d(x64, w64, None, 1, p + 1, d)
    assert torch.equal(crop(full[:, :, 1:-1:s, 1:-1:s]), ref)           # the reference, restated
    wrong = {}
    if k > 1:
        wrong['kh and kw swapped'] = crop(F.conv2d(x64, w64.transpose(2, 3).contiguous(), None, s, p, d))
    if d == 2 and k > 1:
        wrong['dilation 1'] = crop(F.conv2d(x64, w64, None, s, p, 1))
    else:
        wrong['pad + 1'] = crop(full[:, :, ::s, ::s])
    if s == 2:
        wrong['windows one pixel on'] = crop(full[:, :, 2::2, 2::2])
    return wrong


def _run(dev, ops, x, wp, b, k, s, p, d, refs, combos, guarded):
    xin = x.permute(0, 2, 3, 1).contiguous().to(dev)
    gx = guard.place(xin) if guarded else None
    bd = b.to(dev)
    for bias, relu in combos:
        ref = refs[(bias, relu)]
        gy = guard.carve(tuple(ref.shape), torch.float32, dev) if guarded else None
        got = ops.conv2d_nhwc(gx.t if guarded else xin, wp, bd if bias else None, k, s, p, d, relu,
                              out=gy.t if guarded else None)
        assert tuple(got.shape) == tuple(ref.shape)
        tag = (k, s, p, d, tuple(x.shape), wp.shape[0], bias, relu)
        assert torch.equal(got.double().cpu(), ref), tag
        if guarded:
            assert got.data_ptr() == gy.t.data_ptr()
            gy.check('out %r' % (tag,))
            gx.check('x %r' % (tag,))


@functools.lru_cache(maxsize=None)
def _sweep(dev, k, s, d):
    """Every pad of (kernel, stride, dilation) on every channel pair -> the forms it ran."""
    from naws_hip import ops
    ran = []
    for p in _pads(k, d):
        ha, wa = _size_a(k, s, p, d)
        hb, wb = _size_b(k, s, p, d)
        for cin, cout in CHANNELS:
            seed = ((k * 10 + s) * 10 + d) * 10000 + p * 100 + cin
            x, wt, b = _inputs(cin, cout, k, hb, wb, seed)
            wp = ops.conv2d_pack_weight(wt.to(dev))                  # once per (form, channel pair)
            refs = _refs(x, wt, b, s, p, d)
            for name, bad in _wrong_refs(x, wt, s, p, d, refs[(False, False)]).items():
                assert not torch.equal(bad[0], refs[(False, False)][0]), (name, k, s, p, d, cin)
            _run(dev, ops, x, wp, b, k, s, p, d, refs, sorted(refs),
                 guarded=p in (0, d * (k - 1)))
            xa = _inputs(cin, cout, k, ha, wa, seed + 1)[0]
            ra = _refs(xa, wt, b, s, p, d, mixed=False)
            assert tuple(ra[(True, True)].shape) == (N,) + _out(ha, wa, k, s, p, d) + (cout,)
            assert 2 * p >= _span(k, d) or tuple(ra[(True, True)].shape[1:3]) == (1, 1)
            _run(dev, ops, xa, wp, b, k, s, p, d, ra, [(False, False), (True, True)], guarded=False)
        ran.append((k, s, d, p))
    return tuple(ran)


@pytest.mark.parametrize('k,s,d', GROUPS, ids=['k%d-s%d-d%d' % g for g in GROUPS])
def test_every_pad_exact_against_float64(dev, k, s, d):
    ran = _sweep(dev, k, s, d)
    assert len(ran) == d * (k - 1) + 1 == len(set(ran))


def test_sweep_visits_all_60_forms(dev):
    """The twelve tests above (their results are kept: nothing runs twice) visit every form the
    header accepts: 4 x 1 pads with kernel 1, 2 x (3 + 5) with kernel 3, 2 x (7 + 13) with kernel 7."""
    assert len(GROUPS) == 12
    ran = [f for g in GROUPS for f in _sweep(dev, *g)]
    assert len(ran) == len(set(ran)) == 60
    for k, s, d, p in ran:
        assert k in KERNELS and s in STRIDES and d in DILATIONS and 0 <= p <= d * (k - 1)


@pytest.mark.parametrize('cin,k', [(3, 1), (3, 3), (32, 7), (64, 3)])
def test_packed_weight(dev, cin, k):
    """[Cout, Kp]: the first K columns are W as (kh, kw, ci), the rest exactly 0."""
    from naws_hip import lib, ops
    cout, kk = 32, k * k * cin
    kp = int(lib.load().naws_conv2d_packed_k(cin, k))
    assert kp == (kk + 31) // 32 * 32
    wt = _inputs(cin, cout, k, 1, 1, 7 * cin + k)[1]
    wp = ops.conv2d_pack_weight(wt.to(dev)).cpu()
    assert tuple(wp.shape) == (cout, kp)
    assert torch.equal(wp[:, :kk], wt.permute(0, 2, 3, 1).reshape(cout, kk))
    assert bool((wp[:, kk:] == 0).all()) and not bool(torch.signbit(wp[:, kk:]).any())


# --------------------------------------------------------------------------------- refusals ----
# A good call, and what each refusal changes in it.  Every one of these was read against the host
# code of csrc/conv2d.hip: each returns before the launch.
GOOD = dict(N=2, H=5, W=6, Cin=32, Cout=32, kernel=3, stride=1, pad=1, dilation=1, relu=1)
DIM = [dict(N=0), dict(H=0), dict(W=-1), dict(Cin=0), dict(Cout=-32)]
ARG = [dict(kernel=5), dict(kernel=2), dict(stride=3), dict(stride=0), dict(dilation=3),
       dict(dilation=0), dict(pad=3), dict(pad=-1), dict(kernel=7, dilation=2, pad=13)]
CHAN = [dict(Cin=16), dict(Cout=48), dict(Cin=6), dict(Cout=16)]
SMALL = [dict(kernel=7, dilation=2, pad=0), dict(pad=0, H=2), dict(pad=0, W=1, dilation=2)]
NULLS = [dict(X=None), dict(Wp=None), dict(Y=None)]
OFF16 = [dict(X='off'), dict(Wp='off'), dict(Y='off')]
STAGES = [(DIM, ERR_SHAPE), (ARG, ERR_ARG), (CHAN, ERR_UNSUPPORTED), (SMALL, ERR_SHAPE),
          (NULLS, ERR_NULL), (OFF16, ERR_ARG)]                        # the header's order


BUF = 65536        # floats in each of X, Wp and Y: more than GOOD (or GOOD with kernel 7) needs


def _refusal(dev, **change):
    """naws_conv2d_nhwc_fwd's return code for GOOD with `change`; after a refusal neither Y nor
    anything around it has been written."""
    from naws_hip import lib
    a = dict(GOOD, X='ok', Wp='ok', Y='ok')
    a.update(change)
    bufs = {}
    for name in ('X', 'Wp'):
        t = torch.zeros((BUF + 1,), device=dev)
        bufs[name] = t
        assert t.data_ptr() % 16 == 0
    gy = guard.carve((BUF,), torch.float32, dev, aligned=a['Y'] != 'off')
    ptr = {}
    for name in ('X', 'Wp'):
        ptr[name] = None if a[name] is None else bufs[name].data_ptr() + (4 if a[name] == 'off' else 0)
    ptr['Y'] = None if a['Y'] is None else gy.t.data_ptr()
    assert a['Y'] != 'off' or ptr['Y'] % 16 == 4
    bias = torch.zeros((64,), device=dev)
    rc = lib.load().naws_conv2d_nhwc_fwd(ptr['X'], ptr['Wp'], bias.data_ptr(), a['N'], a['H'], a['W'],
                                         a['Cin'], a['Cout'], a['kernel'], a['stride'], a['pad'],
                                         a['dilation'], a['relu'], ptr['Y'], None)
    torch.cuda.synchronize()
    assert guard.holds_sentinel(gy.t) == (rc != 0), change
    gy.check('Y of the call %r' % (change,))
    return rc


def test_refusals_one_fault(dev):
    """GOOD itself runs (and writes Y); each single change to it is refused with its stage's code."""
    assert _refusal(dev) == 0
    for faults, code in STAGES:
        for f in faults:
            assert _refusal(dev, **f) == code, f


def _two_faults():
    """(changes, code): a fault of one stage with a fault of a later one - the earlier one's code.
    Two faults that change the same argument are not two faults: left out."""
    for i, (first, code) in enumerate(STAGES):
        for later, _c in STAGES[i + 1:]:
            for f in first:
                for g in later:
                    if not set(f) & set(g):
                        yield dict(f, **g), code


def test_refusals_earlier_fault_wins(dev):
    """Two faults in one call: the code of the one the header lists first."""
    pairs = list(_two_faults())
    assert len(pairs) > 200
    for both, code in pairs:
        assert _refusal(dev, **both) == code, both


def test_pack_refusals(dev):
    """naws_conv2d_pack_weight: 'errors as naws_conv2d_nhwc_fwd' - SHAPE, ARG (kernel),
    UNSUPPORTED, NULL, in that order, Wp untouched."""
    from naws_hip import lib
    w = torch.zeros((4096,), device=dev)
    cases = [((0, 32, 3), ERR_SHAPE), ((32, -1, 3), ERR_SHAPE), ((32, 32, 5), ERR_ARG),
             ((32, 16, 3), ERR_UNSUPPORTED), ((48, 32, 3), ERR_UNSUPPORTED),
             ((0, 32, 5), ERR_SHAPE), ((32, 16, 5), ERR_ARG)]
    for (cout, cin, k), code in cases:
        gw = guard.carve((4096,), torch.float32, dev)
        assert lib.load().naws_conv2d_pack_weight(w.data_ptr(), cout, cin, k, gw.t.data_ptr(), None) == code
        torch.cuda.synchronize()
        assert guard.holds_sentinel(gw.t)
        gw.check('Wp')
    gw = guard.carve((4096,), torch.float32, dev)
    assert lib.load().naws_conv2d_pack_weight(None, 32, 32, 1, gw.t.data_ptr(), None) == ERR_NULL
    assert lib.load().naws_conv2d_pack_weight(w.data_ptr(), 32, 32, 1, None, None) == ERR_NULL
    assert lib.load().naws_conv2d_pack_weight(None, 32, 16, 1, gw.t.data_ptr(), None) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert guard.holds_sentinel(gw.t)
    gw.check('Wp')
