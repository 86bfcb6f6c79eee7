"""The software-pipelined K loop of the 256 x 256 fp16x2 GEMM (csrc/gemm_x3_m16_body.inc,
gemm_x3_m16p_kernel): LDS fragment reads issued one sub-phase ahead of their MFMAs, the step's
barrier in front of its last sub-phase.  Every accumulator receives the products of the two-phase
loop in the same order, so the outputs must be BIT-IDENTICAL to that loop's, which the `h2` knob keeps
reachable: 5 = the 256 x 256 form with the default (pipelined) loop, 19 = the same form with the
two-phase loop, at shapes that would otherwise run a 128-wide form.

Shapes: T = K / 32 steps; T = 1 (no step to prefetch), T = 2 (no DMA inside the loop), odd T (the
loop is unrolled by two), rows / columns one past a tile edge, several tiles, a batch.

The fc6 weight-gradient kernel (csrc/gemm_btr_body.inc, gemm_h2_btrp_kernel, plain and with the SGD
update in its epilogue) carries the same loop; its 256 x 256 form runs from 256 tiles on, and h2 = 18
selects its two-phase loop."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PIPELINED, TWO_PHASE = 5, 19

SHAPES = [(129, 80, 32),       # T = 1
          (300, 272, 64),      # T = 2
          (257, 513, 96),      # odd T, one row / column past a tile edge
          (512, 512, 160)]


def _operands(dev, m, n, k, batch=0, seed=0):
    from naws_hip import ops
    g = torch.Generator(device=dev).manual_seed(1000 * m + n + k + seed)
    lead = (batch,) if batch else ()
    a = torch.randn(lead + (m, k), device=dev, generator=g)
    b = torch.randn(lead + (n, k), device=dev, generator=g) * 0.05
    if batch:
        b[1] *= 37.0                                  # batch items with different scales
    return ops.split_f16x2(a), ops.split_f16x2(b), g


def _both(run):
    """run() under the pipelined and under the two-phase loop, 256 x 256 tiles forced."""
    from naws_hip import lib as L
    out = []
    try:
        for knob in (PIPELINED, TWO_PHASE):
            L.set_variant('h2', knob)
            out.append(run())
        torch.cuda.synchronize()
    finally:
        L.set_variant('h2', 0)
    return out


def _same(x, y):
    # bit patterns: NaN-safe, and -0.0 != +0.0
    return torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


@pytest.mark.parametrize('epi', ['none', 'bias_relu_drop', 'gate_pos', 'accumulate', 'maxima'])
@pytest.mark.parametrize('m,n,k', SHAPES)
def test_pipelined_loop_is_bit_identical_to_the_two_phase_loop(dev, m, n, k, epi):
    from naws_hip import ops, lib as L
    a2, b2, g = _operands(dev, m, n, k)
    bias = torch.randn((n,), device=dev, generator=g)
    aux = torch.randn((m, n), device=dev, generator=g)
    c0 = torch.randn((m, n), device=dev, generator=g)
    rowmul = torch.exp2(torch.randint(-6, 7, (m,), device=dev, generator=g).float())

    def run():
        if epi == 'none':
            return (ops.gemm_f32_f16x2_nt(a2, b2),)
        if epi == 'bias_relu_drop':
            return (ops.gemm_f32_f16x2_nt(a2, b2, epilogue=L.EPI_BIAS_RELU_DROP, bias=bias,
                                          drop_ratio=0.5, seed=77),)
        if epi == 'gate_pos':
            return (ops.gemm_f32_f16x2_nt(a2, b2, epilogue=L.EPI_GATE_POS, aux=aux, alpha=2.0),)
        if epi == 'accumulate':
            c = c0.clone()
            ops.gemm_f32_f16x2_nt(a2, b2, out=c, accumulate=True)
            return (c,)
        sc_n, sc_t = ops.amax_scales(0, m, dev), ops.amax_scales(0, n, dev)
        c = ops.gemm_f32_f16x2_nt(a2, b2, epilogue=L.EPI_GATE_POS, aux=aux, alpha=2.0,
                                  rowmax=ops.amax_words(sc_n), colmax=ops.amax_words(sc_t),
                                  colmax_rowmul=rowmul)
        return c, sc_n[0], sc_t[0]

    new, old = _both(run)
    assert len(new) == len(old)
    for x, y in zip(new, old):
        assert _same(x, y)
    assert bool(new[0].abs().max() > 0)
    if epi == 'maxima':
        assert bool(new[1].view(torch.int32).max() > 0) and bool(new[2].view(torch.int32).max() > 0)


def test_pipelined_loop_batched(dev):
    from naws_hip import ops
    a2, b2, _ = _operands(dev, 260, 264, 64, batch=3)
    new, old = _both(lambda: ops.gemm_f32_f16x2_nt(a2, b2))
    assert new.shape == (3, 260, 264) and _same(new, old)


def test_pipelined_loop_against_float64_product_of_the_split_operands(dev):
    """The bound of test_gemm_h2_fp32_accurate (test_gpu_h2.py), against the float64 product of the
    operands the kernel actually reads: (hi + lo) / scale."""
    from naws_hip import ops, lib as L
    m, n, k = 257, 513, 96
    rng = np.random.default_rng(42)
    a = torch.from_numpy(rng.uniform(-1, 1, (m, k)).astype(np.float32)).to(dev)
    b = torch.from_numpy(rng.uniform(-1, 1, (n, k)).astype(np.float32)).to(dev)
    a2, b2 = ops.split_f16x2(a), ops.split_f16x2(b)

    def dense(op):
        p = op.planes.double()                               # [2, K/16, outer, 16]
        s = (p[0] + p[1]).movedim(-3, -2)
        return s.reshape(s.shape[0], -1) * op.inv_scale.double().unsqueeze(-1)

    ref = (dense(a2) @ dense(b2).t()).cpu().numpy()
    try:
        L.set_variant('h2', PIPELINED)
        c = ops.gemm_f32_f16x2_nt(a2, b2).cpu().numpy()
    finally:
        L.set_variant('h2', 0)
    err = np.abs(c - ref).max() / np.abs(ref).max()
    assert err < 5e-6 * max(1.0, np.sqrt(k / 4096.0)), err


def test_pipelined_loop_deterministic(dev):
    from naws_hip import ops, lib as L
    a2, b2, _ = _operands(dev, 700, 900, 1024, seed=3)       # several tiles, T = 32
    try:
        L.set_variant('h2', PIPELINED)
        c1 = ops.gemm_f32_f16x2_nt(a2, b2)
        c2 = ops.gemm_f32_f16x2_nt(a2, b2)
        torch.cuda.synchronize()
    finally:
        L.set_variant('h2', 0)
    assert _same(c1, c2)


# ---- gemm_h2_btr: dW = dY^T X from X's forward planes -------------------------------------------
BTR_MN = [(4096, 4096), (4000, 4112)]        # 256 and 17 x 16 = 272 tiles of 256 x 256; ragged edges
BTR_R = [32, 64, 70, 160]                    # T = 1, 2, 3 (70 proposals padded to 96), 5
BTR_TWO_PHASE = 18


def _btr_both(run):
    from naws_hip import lib as L
    out = []
    try:
        for knob in (0, BTR_TWO_PHASE):
            L.set_variant('h2', knob)
            out.append(run())
        torch.cuda.synchronize()
    finally:
        L.set_variant('h2', 0)
    return out


def _btr_case(dev, m, n, r):
    from naws_hip import ops
    g = torch.Generator(device=dev).manual_seed(31 * m + n + r)
    dy = torch.randn((r, m), device=dev, generator=g) * 1e-3
    dy[torch.rand((r, m), device=dev, generator=g) < 0.5] = 0.0
    x = torch.randn((r, n), device=dev, generator=g).relu_()
    x[: r // 2] *= 0.01                                          # rows with different scales
    xp = ops.split_f16x2(x)
    a2 = ops.split_f16x2(dy, transpose=True, rowmul=xp.inv_scale)
    n_all = xp.planes.shape[-3] * 16              # the planes carry n zero-padded to a multiple of 32
    w = torch.randn((m, n_all), device=dev, generator=g) * 0.02
    w[3] *= 40.0
    mom = torch.randn((m, n_all), device=dev, generator=g) * 1e-3
    return ops, xp, a2, w, mom


@pytest.mark.parametrize('r', BTR_R)
@pytest.mark.parametrize('m,n', BTR_MN)
def test_pipelined_wgrad_is_bit_identical_and_deterministic(dev, m, n, r):
    ops, xp, a2, _, _ = _btr_case(dev, m, n, r)
    assert a2.planes.shape[-3] * 16 == (r + 31) // 32 * 32
    # (ncols: x's planes carry its columns zero-padded to a multiple of 32; the product is n wide)
    new, old = _btr_both(lambda: ops.gemm_f32_f16x2_nt_xk(a2, xp, ncols=(0, n)))
    assert new.shape == (m, n) and _same(new, old)
    assert bool(new.abs().max() > 0)
    assert _same(ops.gemm_f32_f16x2_nt_xk(a2, xp, ncols=(0, n)), new)   # launched again: the same bits


@pytest.mark.parametrize('first', [0, 1])
@pytest.mark.parametrize('r', BTR_R)
@pytest.mark.parametrize('m,n', BTR_MN)
def test_pipelined_wgrad_sgd_is_bit_identical(dev, m, n, r, first):
    ops, xp, a2, w, mom = _btr_case(dev, m, n, r)
    lr = torch.tensor([3e-3], device=dev)
    bound = ops.split_f16x2(w).scales[0].view(torch.int32).clone()

    def run():
        w1, m1 = w.clone(), mom.clone()
        planes = ops.split_f16x2(w1)
        rowmax = torch.zeros((m,), device=dev, dtype=torch.int32)
        inv = torch.zeros((m,), device=dev)
        ovf = torch.zeros((1,), device=dev, dtype=torch.int32)
        ops.gemm_f32_f16x2_nt_xk_sgd(a2, xp, w1, m1, lr, 1.0, 5e-4, 0.9, 0, 4, 0 if first else 3,
                                     planes.planes, bound, rowmax, inv, ovf, 7, ncols=(0, n))
        return w1, m1, planes.planes[0], planes.planes[1], rowmax, inv, ovf

    def same(xs, ys):
        for x, y in zip(xs, ys):
            bits = torch.int16 if x.dtype == torch.float16 else torch.int32
            if not torch.equal(x.contiguous().view(bits), y.contiguous().view(bits)):
                return False
        return len(xs) == len(ys)

    new, old = _btr_both(run)
    assert not torch.equal(new[0], w)
    assert same(new, old)
    assert same(run(), new)                  # launched again from the same inputs: the same bits
