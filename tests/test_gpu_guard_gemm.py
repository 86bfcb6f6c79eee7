"""Guard bands and strided views around the GEMMs (tests/guard.py).

Every operand here is integer-valued (|a|, |b| <= 4; bias, aux, C0 integers; dropout ratio 0.5,
i.e. a scale of 2; alpha 2), so every partial sum is an integer below 2^24 and the fp32 / f16x2 /
bf16 results must EQUAL the float64 product: a comparison with no tolerance, in which one stray
row or column shows.  A, B, aux and out are row-strided views (ld = cols + 4 unless noted) carved
out of sentinel-filled buffers: what a kernel writes outside `out` is found by the guard check,
what it reads outside an operand is a NaN and reaches the result.

Shapes of ops.gemm: the smallest that reaches each tile form of csrc/gemm_f32.hip dispatch(), one
past a tile edge where the contiguous dimension may be odd, four past where it is read with
16-byte loads (M of a transposed A: `m + 3` below)."""
import numpy as np
import pytest
import torch

import guard
from test_gpu_gemm_pipelined import SHAPES as PIPE_SHAPES

pytestmark = pytest.mark.gpu

EPIS = ['none', 'bias_relu_drop', 'gate_pos']
SEED = 77


def _ints(g, shape, dev, lim=4):
    return torch.randint(-lim, lim + 1, shape, device=dev, generator=g).float()


def _gen(dev, *key):
    s = 0
    for v in key:
        s = s * 1000003 + (sum(map(ord, v)) if isinstance(v, str) else int(v))
    return torch.Generator(device=dev).manual_seed(s % (2 ** 31))


def _epi_code(epi):
    from naws_hip import lib as L
    return {'none': L.EPI_NONE, 'bias_relu_drop': L.EPI_BIAS_RELU_DROP, 'gate_pos': L.EPI_GATE_POS}[epi]


def _expected(prod, epi, bias, aux, c0, dev):
    """float64 epilogue of the float64 product (all exact in fp32 for the operands used here)."""
    from naws_hip import ops
    v = prod
    if epi == 'bias_relu_drop':
        keep = ops.dropout_mask(SEED, 0.5, prod.numel(), dev).view(prod.shape).double()
        v = (v + bias.double().unsqueeze(-2)).clamp_min(0.0) * keep * 2.0
    elif epi == 'gate_pos':
        v = torch.where(aux.double() > 0, v * 2.0, torch.zeros_like(v))
    if c0 is not None:
        v = v + c0.double()
    return v


def _bs(rows, ld, batch):
    """Batch stride with a gap of 8 elements behind each item (None when unbatched)."""
    return rows * ld + 8 if batch else None


# ---------------------------------------------------------------------------------------------
# ops.gemm: the tile forms
# ---------------------------------------------------------------------------------------------
# (form, M, N, K, M of the batch-3 variant: the dispatch counts tiles over the batch)
TILE_FORMS = [('64x64', 65, 68, 36, 65),
              ('64x128', 1473, 4100, 20, 449),
              ('128x128', 3969, 4100, 20, 3969),
              ('128x64', 65409, 40, 16, 65409)]
VARIANTS = ['strided', 'odd_ldc', 'batch3', 'accumulate']


def _gemm_case(dev, m, n, k, ta, tb, epi, variant, ld_pad=4, out_aligned=True):
    from naws_hip import ops
    batch = 3 if variant == 'batch3' else 0
    lead = (batch,) if batch else ()
    g = _gen(dev, m, n, k, ta, tb, epi, variant)
    a = _ints(g, lead + ((k, m) if ta else (m, k)), dev)
    b = _ints(g, lead + ((n, k) if tb else (k, n)), dev)
    bias = _ints(g, lead + (n,), dev)
    aux = _ints(g, lead + (m, n), dev)
    c0 = _ints(g, lead + (m, n), dev) if variant == 'accumulate' else None
    ga = guard.place(a, ld=a.shape[-1] + 4, batch_stride=_bs(a.shape[-2], a.shape[-1] + 4, batch))
    gb = guard.place(b, ld=b.shape[-1] + 4, batch_stride=_bs(b.shape[-2], b.shape[-1] + 4, batch))
    ldc = n + ld_pad
    gaux = guard.place(aux, ld=ldc, batch_stride=_bs(m, ldc, batch), aligned=out_aligned)
    gout = guard.carve(lead + (m, n), torch.float32, dev, ld=ldc, batch_stride=_bs(m, ldc, batch),
                       aligned=out_aligned)
    if c0 is not None:
        gout.t.copy_(c0)
    ops.gemm(ga.t, gb.t, ta, tb, out=gout.t, epilogue=_epi_code(epi), bias=bias,
             aux=gaux.t if epi == 'gate_pos' else None, alpha=2.0, drop_ratio=0.5, seed=SEED,
             accumulate=c0 is not None)
    a64 = a.double().transpose(-1, -2) if ta else a.double()
    b64 = b.double().transpose(-1, -2) if tb else b.double()
    want = _expected(a64 @ b64, epi, bias, aux, c0, dev)
    assert torch.equal(gout.t.double(), want)
    for gd, nm in ((gout, 'out'), (ga, 'A'), (gb, 'B'), (gaux, 'aux')):
        gd.check(nm)


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('epi', EPIS)
@pytest.mark.parametrize('ta,tb', [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize('form,m,n,k,mb', TILE_FORMS)
def test_gemm_tile_forms_equal_float64_inside_guards(dev, form, m, n, k, mb, ta, tb, epi, variant):
    """odd_ldc: ldc = ldaux = N + 1 and C / aux one word off a 16-byte boundary - the tile forms
    store and read them one float at a time (include/naws.h: only the operands need 16 bytes)."""
    mm = mb if variant == 'batch3' else m
    if ta:
        mm += 3                       # four past the tile edge: M is A's contiguous dimension
    if variant == 'odd_ldc':
        _gemm_case(dev, mm, n, k, ta, tb, epi, variant, ld_pad=1, out_aligned=False)
    else:
        _gemm_case(dev, mm, n, k, ta, tb, epi, variant)


def test_gemm_rejects_what_its_16_byte_operand_loads_cannot_read(dev):
    """An odd contiguous extent, an odd lda / ldb and an operand off 16 bytes are refused
    (NAWS_ERR_ARG), not read."""
    from naws_hip import ops, lib as L
    g = _gen(dev, 1)
    a, b = _ints(g, (36, 65), dev), _ints(g, (36, 68), dev)
    with pytest.raises(L.NawsError) as e:
        ops.gemm(a, b, True, False)                                  # M = 65 contiguous
    assert e.value.code == L.ERR_ARG
    a = _ints(g, (65, 36), dev)
    for bad in (guard.place(a, ld=37), guard.place(a, ld=40, aligned=False)):
        with pytest.raises(L.NawsError) as e:
            ops.gemm(bad.t, b, False, False)
        assert e.value.code == L.ERR_ARG
    a3 = _ints(g, (3, 65, 36), dev)
    odd = guard.place(a3, ld=40, batch_stride=65 * 40 + 2)           # strideA % 4 != 0
    with pytest.raises(L.NawsError) as e:
        ops.gemm(odd.t, b.unsqueeze(0).expand(3, 36, 68).contiguous(), False, False)
    assert e.value.code == L.ERR_ARG


# ---------------------------------------------------------------------------------------------
# ops.gemm: the short-K MFMA kernel (NN, K <= 64, M N >= 2^20), both template depths
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', ['strided', 'batch3', 'accumulate'])
@pytest.mark.parametrize('epi', EPIS)
@pytest.mark.parametrize('align', ['aligned', 'out_off_16', 'ld_odd'])
@pytest.mark.parametrize('k', [40, 64])
def test_gemm_short_k_form_and_its_fallback(dev, k, align, epi, variant):
    """aligned: ldc, ldaux and the pointers are multiples of 16 bytes - the short-K kernel (NONE /
    GATE_POS; BIAS_RELU_DROP is not one of its epilogues and takes the tile form).  out_off_16 /
    ld_odd: C and aux start one word off, or ldc = ldaux = N + 1 - the entry falls back to the tile
    form.  Every route must equal the float64 product."""
    m, n = 1025, 1028
    if align == 'aligned':
        _gemm_case(dev, m, n, k, False, False, epi, variant)
    elif align == 'out_off_16':
        _gemm_case(dev, m, n, k, False, False, epi, variant, out_aligned=False)
    else:
        _gemm_case(dev, m, n, k, False, False, epi, variant, ld_pad=1)


# ---------------------------------------------------------------------------------------------
# ops.gemm: 256 x 256 tiles on 16 waves (NT, K >= 2048, >= 512 tiles)
# ---------------------------------------------------------------------------------------------
BIG = (3841, 7937, 2048)


@pytest.fixture(scope='module')
def big(dev):
    """Operands and the float64 product of the 256 x 256 case: computed once for the module, never
    modified, released with it.  The device's float64 product is itself checked on the CPU, for the
    first and last row and column of every tile row and tile column."""
    m, n, k = BIG
    g = _gen(dev, *BIG)
    a, b = _ints(g, (m, k), dev), _ints(g, (n, k), dev)
    prod = a.double() @ b.double().t()
    an, bn = a.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64)
    rows = sorted(set(r for t in range(0, m, 256) for r in (t, min(t + 255, m - 1))))
    cols = sorted(set(c for t in range(0, n, 256) for c in (t, min(t + 255, n - 1))))
    assert np.array_equal(prod[rows].cpu().numpy(), an[rows] @ bn.T)
    assert np.array_equal(prod[:, cols].cpu().numpy(), an @ bn[cols].T)
    return dict(a=guard.place(a, ld=k + 4), b=guard.place(b, ld=k + 4), prod=prod,
                bias=_ints(g, (n,), dev), aux=guard.place(_ints(g, (m, n), dev), ld=n + 4),
                c0=_ints(g, (m, n), dev))


@pytest.mark.parametrize('epi', EPIS + ['accumulate'])
def test_gemm_256x256_form_equals_float64_inside_guards(dev, big, epi):
    from naws_hip import ops
    m, n, k = BIG
    o = big
    acc = epi == 'accumulate'
    e = 'none' if acc else epi
    gout = guard.carve((m, n), torch.float32, dev, ld=n + 4)
    if acc:
        gout.t.copy_(o['c0'])
    ops.gemm(o['a'].t, o['b'].t, False, True, out=gout.t, epilogue=_epi_code(e), bias=o['bias'],
             aux=o['aux'].t if e == 'gate_pos' else None, alpha=2.0, drop_ratio=0.5, seed=SEED,
             accumulate=acc)
    want = _expected(o['prod'], e, o['bias'], o['aux'].t, o['c0'] if acc else None, dev)
    assert torch.equal(gout.t.double(), want)
    del want
    for gd, nm in ((gout, 'out'), (o['a'], 'A'), (o['b'], 'B'), (o['aux'], 'aux')):
        gd.check(nm)


# ---------------------------------------------------------------------------------------------
# ops.gemm_splitk: guarded workspace of exactly the declared size
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('batch', [0, 3])
@pytest.mark.parametrize('with_bias', [False, True])
@pytest.mark.parametrize('ksplit', [1, 4, 6])
@pytest.mark.parametrize('ta,tb', [(False, False), (False, True), (True, False), (True, True)])
def test_gemm_splitk_stays_inside_its_declared_workspace(dev, ta, tb, ksplit, with_bias, batch):
    from naws_hip import ops, lib as L
    m, n, k = 40, 4100, 2052
    lead = (batch,) if batch else ()
    g = _gen(dev, m, n, k, ta, tb, ksplit, with_bias, batch)
    a = _ints(g, lead + ((k, m) if ta else (m, k)), dev)
    b = _ints(g, lead + ((n, k) if tb else (k, n)), dev)
    bias = _ints(g, lead + (n,), dev)
    ga = guard.place(a, ld=a.shape[-1] + 4, batch_stride=_bs(a.shape[-2], a.shape[-1] + 4, batch))
    gb = guard.place(b, ld=b.shape[-1] + 4, batch_stride=_bs(b.shape[-2], b.shape[-1] + 4, batch))
    gout = guard.carve(lead + (m, n), torch.float32, dev, ld=n + 4, batch_stride=_bs(m, n + 4, batch))
    need = L.load().naws_gemm_f32_splitk_workspace_floats(m, n, max(batch, 1), ksplit)
    assert need == m * n * max(batch, 1) * ksplit
    gws = guard.carve((need,), torch.float32, dev)
    ops.gemm_splitk(ga.t, gb.t, ta, tb, out=gout.t, epilogue=L.EPI_BIAS if with_bias else L.EPI_NONE,
                    bias=bias if with_bias else None, ksplit=ksplit, workspace=gws.t)
    a64 = a.double().transpose(-1, -2) if ta else a.double()
    b64 = b.double().transpose(-1, -2) if tb else b.double()
    want = a64 @ b64
    if with_bias:
        want = want + bias.double().unsqueeze(-2)
    assert torch.equal(gout.t.double(), want)
    for gd, nm in ((gws, 'workspace'), (gout, 'out'), (ga, 'A'), (gb, 'B')):
        gd.check(nm)
    with pytest.raises(TypeError):
        ops.gemm_splitk(ga.t, gb.t, ta, tb, ksplit=ksplit, workspace=gws.t[:need - 1])


# ---------------------------------------------------------------------------------------------
# The plane GEMMs: f16x2, f32x3, bf16 (fp32 operands rounded in the kernel), bf16 slab
# ---------------------------------------------------------------------------------------------
def _embed(x, lo=2, hi=1):
    """x's rows between `lo` rows and `hi` rows of NaN: the source of a row-sliced plane operand."""
    big = torch.full(x.shape[:-2] + (x.shape[-2] + lo + hi, x.shape[-1]), float('nan'),
                     device=x.device)
    big[..., lo:lo + x.shape[-2], :] = x
    return big, lo, lo + x.shape[-2]


def _op_f16x2(ops, x, strided):
    if not strided:
        return ops.split_f16x2(x), []
    big, r0, r1 = _embed(x)
    return ops.split_f16x2(big).rows(r0, r1), []


def _op_f32x3(ops, x, strided):
    if not strided:
        return ops.split_bf16x3(x), []
    big, r0, r1 = _embed(x)
    return ops.split_bf16x3(big)[..., r0:r1, :], []


def _op_slab(ops, x, strided):
    if not strided:
        return ops.to_bf16_slab(x), []
    big, r0, r1 = _embed(x)
    return ops.to_bf16_slab(big)[..., r0:r1, :], []


def _op_bf16(ops, x, strided):
    if not strided:
        return x, []
    ld = x.shape[-1] + 8                      # naws_gemm_bf16_nt: lda, ldb multiples of 8
    gx = guard.place(x, ld=ld, batch_stride=_bs(x.shape[-2], ld, x.dim() == 3))
    return gx.t, [gx]


PLANE_ENTRIES = {'f16x2': ('gemm_f32_f16x2_nt', _op_f16x2), 'f32x3': ('gemm_f32x3_nt', _op_f32x3),
                 'bf16': ('gemm_bf16_nt', _op_bf16), 'bf16_slab': ('gemm_bf16_slab_nt', _op_slab)}


def _plane_case(dev, entry, m, n, k, epi, batch=0):
    """The contiguous call, then the strided call (row-sliced operands, carved aux and out): both
    equal the float64 product, bit for bit the same, guards intact."""
    from naws_hip import ops
    fn, make = PLANE_ENTRIES[entry]
    fn = getattr(ops, fn)
    acc = epi == 'accumulate'
    e = 'none' if acc else epi
    lead = (batch,) if batch else ()
    g = _gen(dev, entry, m, n, k, epi, batch)
    a, b = _ints(g, lead + (m, k), dev), _ints(g, lead + (n, k), dev)
    bias = _ints(g, lead + (n,), dev)
    aux = _ints(g, lead + (m, n), dev)
    c0 = _ints(g, lead + (m, n), dev) if acc else None
    kw = dict(epilogue=_epi_code(e), bias=bias, alpha=2.0, drop_ratio=0.5, seed=SEED, accumulate=acc)
    want = _expected(a.double() @ b.double().transpose(-1, -2), e, bias, aux, c0, dev)

    ac, _ = make(ops, a, False)
    bc, _ = make(ops, b, False)
    plain = fn(ac, bc, out=c0.clone() if acc else None, aux=aux if e == 'gate_pos' else None, **kw)
    assert torch.equal(plain.double(), want)

    av, guards_a = make(ops, a, True)
    bv, guards_b = make(ops, b, True)
    gaux = guard.place(aux, ld=n + 4, batch_stride=_bs(m, n + 4, batch))
    gout = guard.carve(lead + (m, n), torch.float32, dev, ld=n + 4, batch_stride=_bs(m, n + 4, batch))
    if acc:
        gout.t.copy_(c0)
    fn(av, bv, out=gout.t, aux=gaux.t if e == 'gate_pos' else None, **kw)
    assert torch.equal(gout.t.double(), want)
    assert guard.same_bits(gout.t, plain)
    for gd in [gout, gaux] + guards_a + guards_b:
        gd.check(entry)


@pytest.mark.parametrize('epi', EPIS + ['accumulate'])
@pytest.mark.parametrize('h2', [0, 5, 19])
@pytest.mark.parametrize('m,n,k', PIPE_SHAPES)
@pytest.mark.parametrize('entry', sorted(PLANE_ENTRIES))
def test_plane_gemms_strided_equal_float64_and_the_contiguous_call(dev, entry, m, n, k, h2, epi):
    from naws_hip import lib as L
    try:
        L.set_variant('h2', h2)
        _plane_case(dev, entry, m, n, k, epi)
        torch.cuda.synchronize()
    finally:
        L.set_variant('h2', 0)


@pytest.mark.parametrize('epi', ['none', 'gate_pos', 'accumulate'])
@pytest.mark.parametrize('entry', sorted(PLANE_ENTRIES))
def test_plane_gemms_batch_of_16_on_the_short_k_ring(dev, entry, epi):
    """batch 16 at K <= 1024: the 3-stage 16-deep form of the f16x2 and f32x3 GEMMs (the Winograd
    batch products); aux and out carved with EQUAL batch strides and a gap behind each item."""
    _plane_case(dev, entry, 129, 80, 96, epi, batch=16)


# ---------------------------------------------------------------------------------------------
# batched aux: the kernels step it by out's batch stride
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('entry', ['f32'] + sorted(PLANE_ENTRIES))
def test_batched_aux_with_another_batch_stride_than_out_is_refused(dev, entry):
    from naws_hip import ops, lib as L
    m, n, k, batch = 65, 68, 64, 3
    g = _gen(dev, entry, 5)
    a, b = _ints(g, (batch, m, k), dev), _ints(g, (batch, n, k), dev)
    aux = _ints(g, (batch, m, n), dev)                                   # batch stride m * n
    gout = guard.carve((batch, m, n), torch.float32, dev, ld=n, batch_stride=m * n + 8)
    if entry == 'f32':
        def run(out, x):
            return ops.gemm(a, b, False, True, out=out, epilogue=L.EPI_GATE_POS, aux=x, alpha=2.0)
    else:
        fn, make = PLANE_ENTRIES[entry]
        ao, bo = make(ops, a, False)[0], make(ops, b, False)[0]

        def run(out, x):
            return getattr(ops, fn)(ao, bo, out=out, epilogue=L.EPI_GATE_POS, aux=x, alpha=2.0)
    for bad in (aux, aux[0]):                      # another stride; one 2-D aux for three items
        with pytest.raises(L.NawsError) as e:
            run(gout.t, bad)
        assert e.value.code == L.ERR_ARG
    assert guard.holds_sentinel(gout.t)            # refused before anything ran
    gaux = guard.place(aux, ld=n, batch_stride=m * n + 8)                # the working case
    run(gout.t, gaux.t)
    want = _expected(a.double() @ b.double().transpose(-1, -2), 'gate_pos', None, aux, None, dev)
    assert torch.equal(gout.t.double(), want)
    gout.check('out')
    gaux.check('aux')
