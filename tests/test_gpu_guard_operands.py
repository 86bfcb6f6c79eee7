"""Guard bands around the operand builders (tests/guard.py): the splits and transposes that turn
fp32 matrices into the plane / slab operands of the GEMMs, and the per-image RoI pooling that
writes row ranges of one shared operand.

Splits and transposes: x is a row-strided view (ld = cols + 4) inside poison, plain and
transposed, single and as a batch of 3 with a gap behind each item, and the outputs are carved from
sentinel-filled buffers.  The result must be bit-identical to the contiguous call's, the documented
padding (K up to 32 / 16 / 64, Rpad) must be zero, and every guard intact.  An entry that cannot
take a strided or gapped input must refuse it."""
import numpy as np
import pytest
import torch

import guard
from helpers import make_rois

pytestmark = pytest.mark.gpu

SHAPES = [(33, 40), (65, 100), (1, 36)]
BATCHES = [0, 3]


def _x(dev, rows, cols, batch, seed=0):
    """(contiguous x, the same values as a strided / gapped view inside poison)."""
    g = torch.Generator(device=dev).manual_seed(100 * rows + cols + batch + seed)
    x = torch.randn(((batch,) if batch else ()) + (rows, cols), device=dev, generator=g)
    if batch:
        x[1] *= 37.0
    ld = cols + 4
    gx = guard.place(x, ld=ld, batch_stride=(rows * ld + 8) if batch else None)
    return x, gx


def _dense_k(planes):
    """[..., K/16, outer, 16] -> [..., outer, K]."""
    p = planes.transpose(-3, -2)
    return p.reshape(p.shape[:-2] + (-1,))


def _lead(batch):
    return (batch,) if batch else ()


@pytest.mark.parametrize('batch', BATCHES)
@pytest.mark.parametrize('transpose', [False, True])
@pytest.mark.parametrize('rows,cols', SHAPES)
def test_split_f16x2(dev, rows, cols, transpose, batch):
    from naws_hip import ops
    x, gx = _x(dev, rows, cols, batch)
    want = ops.split_f16x2(x, transpose=transpose)
    gp = guard.carve(tuple(want.planes.shape), torch.float16, dev)
    gs = guard.carve(tuple(want.scales.shape), torch.float32, dev)
    ops.split_f16x2(gx.t, transpose=transpose, out=ops.F16x2(gp.t, gs.t))
    assert guard.same_bits(gp.t, want.planes)
    assert guard.same_bits(gs.t[1], want.scales[1])                 # ([0] is scratch)
    k = rows if transpose else cols
    assert gp.t.shape[-3] * 16 == (k + 31) // 32 * 32
    assert not bool(_dense_k(gp.t)[..., k:].any())                  # K padded to 32 with zeros
    for gd, nm in ((gp, 'planes'), (gs, 'scales'), (gx, 'x')):
        gd.check(nm)


@pytest.mark.parametrize('batch', BATCHES)
@pytest.mark.parametrize('rows,cols', SHAPES)
def test_split_f16x2_dual(dev, rows, cols, batch):
    from naws_hip import ops
    x, gx = _x(dev, rows, cols, batch, seed=1)

    def blocks(guarded):
        out = []
        for outer, dim in ((rows, -1), (cols, -2)):
            shape = (2,) + _lead(batch) + (outer,)
            gd = guard.carve(shape, torch.float32, dev) if guarded else None
            sc = gd.t if guarded else torch.empty(shape, device=dev)
            sc.zero_()
            sc[0].view(torch.int32).copy_(x.abs().amax(dim=dim).view(torch.int32))   # the maxima
            out.append((sc, gd))
        return out

    (sn, _), (st, _) = blocks(False)
    wn, wt = ops.split_f16x2_dual(x, sn, st)
    (gsn_t, gsn), (gst_t, gst) = blocks(True)
    gpn = guard.carve(tuple(wn.planes.shape), torch.float16, dev)
    gpt = guard.carve(tuple(wt.planes.shape), torch.float16, dev)
    ops.split_f16x2_dual(gx.t, gsn_t, gst_t, out_n=ops.F16x2(gpn.t, gsn_t), out_t=ops.F16x2(gpt.t, gst_t))
    assert guard.same_bits(gpn.t, wn.planes) and guard.same_bits(gpt.t, wt.planes)
    assert guard.same_bits(gsn_t, sn) and guard.same_bits(gst_t, st)
    assert not bool(_dense_k(gpn.t)[..., cols:].any()) and not bool(_dense_k(gpt.t)[..., rows:].any())
    for gd, nm in ((gpn, 'planes_n'), (gpt, 'planes_t'), (gsn, 'scales_n'), (gst, 'scales_t'), (gx, 'x')):
        gd.check(nm)


@pytest.mark.parametrize('batch', BATCHES)
@pytest.mark.parametrize('transpose', [False, True])
@pytest.mark.parametrize('rows,cols', SHAPES)
@pytest.mark.parametrize('entry,kmul', [('split_bf16x3', 16), ('to_bf16_slab', 64)])
def test_bf16_planes_and_slab(dev, entry, kmul, rows, cols, transpose, batch):
    from naws_hip import ops
    x, gx = _x(dev, rows, cols, batch, seed=2)
    fn = getattr(ops, entry)
    want = fn(x, transpose=transpose)
    gp = guard.carve(tuple(want.shape), torch.bfloat16, dev)
    fn(gx.t, transpose=transpose, out=gp.t)
    assert guard.same_bits(gp.t, want)
    k = rows if transpose else cols
    assert gp.t.shape[-3] * 16 == (k + kmul - 1) // kmul * kmul
    assert not bool(_dense_k(gp.t)[..., k:].any())                  # K padded with zeros
    gp.check('planes')
    gx.check('x')


@pytest.mark.parametrize('batch', BATCHES)
@pytest.mark.parametrize('rows,cols', SHAPES)
def test_transpose_to_bf16(dev, rows, cols, batch):
    """Batch items must follow each other at rows * ld: a strided batch is taken, a batch with
    gaps between the items is refused."""
    from naws_hip import ops
    x, gx = _x(dev, rows, cols, batch, seed=3)
    want = ops.transpose_to_bf16(x)
    rp = (rows + 7) // 8 * 8
    assert want.shape == _lead(batch) + (cols, rp)
    if batch:
        with pytest.raises(TypeError):
            ops.transpose_to_bf16(gx.t)
        gx = guard.place(x, ld=cols + 4, batch_stride=rows * (cols + 4))
    gy = guard.carve(tuple(want.shape), torch.bfloat16, dev)
    ops.transpose_to_bf16(gx.t, out=gy.t)
    assert guard.same_bits(gy.t, want)
    assert torch.equal(gy.t[..., :rows].float(), x.transpose(-1, -2).bfloat16().float())
    assert not bool(gy.t[..., rows:].any())                         # rows_pad: zeros
    gy.check('out')
    gx.check('x')


@pytest.mark.parametrize('rows,cols', SHAPES)
def test_f16_planes_transpose(dev, rows, cols):
    from naws_hip import ops
    x, _ = _x(dev, rows, cols, 0, seed=4)
    op = ops.split_f16x2(x)
    want = ops.f16_planes_transpose(op)
    rpad = (rows + 31) // 32 * 32
    assert want.planes.shape == (2, rpad // 16, op.planes.shape[1] * 16, 16)
    # its input is one operand's planes, whole: a row-sliced view is refused, not read
    big = ops.split_f16x2(torch.cat([x, x], 0))
    with pytest.raises(TypeError):
        ops.f16_planes_transpose(big.rows(0, rows))
    gin = guard.place(op.planes)
    gq = guard.carve(tuple(want.planes.shape), torch.float16, dev)
    got = ops.f16_planes_transpose(ops.F16x2(gin.t, op.scales), out=gq.t)
    assert got.planes.data_ptr() == gq.t.data_ptr()
    assert guard.same_bits(gq.t, want.planes)
    assert not bool(_dense_k(gq.t)[..., rows:].any())               # rows up to Rpad: zeros
    gq.check('out')
    gin.check('planes')


@pytest.mark.parametrize('rows,cols', SHAPES)
def test_bf16_slab_transpose(dev, rows, cols):
    from naws_hip import ops
    x, _ = _x(dev, rows, cols, 0, seed=5)
    slab = ops.to_bf16_slab(x)
    want = ops.bf16_slab_transpose(slab)
    rp = (rows + 63) // 64 * 64
    assert want.shape == (rp // 16, slab.shape[0] * 16, 16)
    big = ops.to_bf16_slab(torch.cat([x, x], 0))
    with pytest.raises(TypeError):
        ops.bf16_slab_transpose(big[:, :rows])
    gin = guard.place(slab)
    gq = guard.carve(tuple(want.shape), torch.bfloat16, dev)
    ops.bf16_slab_transpose(gin.t, out=gq.t)
    assert guard.same_bits(gq.t, want)
    # (the slab carries x's columns zero-padded to 64: the transposed operand has that many rows)
    assert guard.same_bits(gq.t[:, :cols], ops.to_bf16_slab(x, transpose=True))
    assert not bool(gq.t[:, cols:].any())
    assert not bool(_dense_k(gq.t)[..., rows:].any())               # rows up to Rpad: zeros
    gq.check('out')
    gin.check('slab')


# ---------------------------------------------------------------------------------------------
# per-image RoI pooling: row ranges of one shared fc6 operand
# ---------------------------------------------------------------------------------------------
def _roi_case(dev):
    from naws_hip import ops
    rng = np.random.default_rng(600)
    n, c, h, w, r = 2, 128, 20, 30, 150
    x = torch.from_numpy(rng.standard_normal((n, h, w, c)).astype(np.float32)).to(dev)
    rois = torch.from_numpy(make_rois(rng, n, r // n, h * 8, w * 8)).to(dev)
    boost = torch.from_numpy((rng.uniform(0, 1, r) + 1).astype(np.float32)).to(dev)
    amax = torch.tensor([np.float32(8.0).view(np.int32)] * n, device=dev, dtype=torch.int32)
    m2, m4 = torch.empty_like(x), torch.empty_like(x)
    ops.roi_maxmaps(x, m2, m4)
    whole = ops.roi_pool_f_f16x2(x, rois, amax, 7, 7, 0.125, boost=boost, maps=(m2, m4))
    return ops, x, rois, boost, amax, (m2, m4), whole, r, c * 49


def _carved_operand(ops, dev, r, k):
    gp = guard.carve((2, k // 16, r, 16), torch.float16, dev)
    gs = guard.carve((2, r), torch.float32, dev)
    return gp, gs, ops.F16x2(gp.t, gs.t)


def test_roi_range_pooling_leaves_the_other_rows_untouched(dev):
    """Planes and scales prefilled with the sentinel: after the range [37, 101) the rows outside it
    still hold it bit for bit (another image's stream may be writing them at that moment), the
    rows inside equal the one-launch operand."""
    ops, x, rois, boost, amax, maps, whole, r, k = _roi_case(dev)
    gp, gs, op = _carved_operand(ops, dev, r, k)
    ops.roi_pool_f_f16x2_range(x, rois, amax, op, 37, 101, maps, 7, 7, 0.125, boost=boost)
    assert guard.same_bits(gp.t[:, :, 37:101], whole.planes[:, :, 37:101])
    assert guard.same_bits(gs.t[1, 37:101], whole.scales[1, 37:101])
    assert guard.holds_sentinel(gp.t[:, :, :37]) and guard.holds_sentinel(gp.t[:, :, 101:])
    assert guard.holds_sentinel(gs.t[:, :37]) and guard.holds_sentinel(gs.t[:, 101:])
    gp.check('planes')
    gs.check('scales')


def test_roi_range_pooling_three_ranges_equal_the_one_launch(dev):
    ops, x, rois, boost, amax, maps, whole, r, k = _roi_case(dev)
    gp, gs, op = _carved_operand(ops, dev, r, k)
    for r0, r1 in ((101, 150), (0, 37), (37, 101)):
        ops.roi_pool_f_f16x2_range(x, rois, amax, op, r0, r1, maps, 7, 7, 0.125, boost=boost)
    assert guard.same_bits(gp.t, whole.planes)
    assert guard.same_bits(gs.t[1], whole.scales[1])
    gp.check('planes')
    gs.check('scales')
