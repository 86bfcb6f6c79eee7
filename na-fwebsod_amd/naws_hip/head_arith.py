"""The arithmetic plans of the fc head, one object each (plan(name)): how an fp32 matrix becomes a
GEMM operand, how a row range or the first batches are cut out of an operand (views, no copy),
which kernel multiplies two operands, and the few facts planes.FcPlanes and the engine branch on.
Operands keep the types the kernel wrappers take: ops.F16x2 (fp16x2), raw bf16 plane tensors
(fp32x3 [3, (b,) K/16, outer, 16], bf16 [(b,) K/16, outer, 16]) and, fp32, a lazy (tensor,
transposed) pair: nothing is copied, the flag becomes trans_a / trans_b.  DESIGN.md §3a has what
each plan computes and costs."""

import collections

import torch

from . import lib as L
from . import ops

Fp32Operand = collections.namedtuple('Fp32Operand', 'x t')


class Fp32(object):
    """Every product on the fp32 MFMA; its facts are the other plans' defaults."""
    planes16 = False            # operands are 16-bit planes (FcPlanes keeps the weights')
    reports_maxima = False      # ... row-scaled: the GEMM epilogues report max|.| for the scales
    wgrad_update = False        # fc6_w can be updated in the epilogue of its wgrad GEMM
    update_after = 0            # conv chain entries run before the deferred update is queued (0: none)
    roi_maps_on_chains = False  # RoIPoolF reads block-maxima maps of conv5_3, built beside the chains
    roi_pool_slab = False       # ... and writes fc6's one-plane operand over them itself
    fmt = kpad = dtype = None   # FcPlanes: format constant, K padding, element type, leading planes
    lead = ()

    def __init__(self, name, conv_prefix, **facts):
        self.name, self.conv_prefix = name, conv_prefix     # the conv forms `conv_prefix`_* use `split`
        self.__dict__.update(facts)

    @staticmethod
    def split(x, transpose=False, out=None):
        return Fp32Operand(x, transpose)

    def is_operand(self, x):
        return isinstance(x, Fp32Operand)

    def operand(self, x, transpose=False, out=None, **kw):
        """The plan's GEMM operand of the fp32 matrix x (or of x^T); an operand passes through."""
        if not self.is_operand(x):
            return self.split(x, transpose=transpose, out=out, **kw)
        if transpose:
            raise TypeError('%s: x is an operand already and cannot be transposed here' % self.name)
        return x

    def rows(self, op, r0, r1):
        """Outer indices r0..r1 of an operand."""
        return Fp32Operand(op.x[..., r0:r1] if op.t else op.x[..., r0:r1, :], op.t)

    def batches(self, op, nb):
        return Fp32Operand(op.x[:nb], op.t)

    def gemm_nt(self, a, b, out=None, **kw):
        """C = A B^T (kw: the kernel wrapper's epilogue / maxima keywords)."""
        return ops.gemm(a.x, b.x, trans_a=a.t, trans_b=not b.t, out=out, **kw)


class Planes(Fp32):
    """16-bit planes [lead, (b,) K/16, outer, 16]: raw bf16 tensors, or (row-scaled: reports_maxima)
    ops.F16x2; split / gemm_nt: the plan's wrappers."""
    planes16 = True

    def is_operand(self, x):
        return isinstance(x, ops.F16x2) if self.reports_maxima else x.dtype == self.dtype

    def rows(self, op, r0, r1):
        return op.rows(r0, r1) if self.reports_maxima else op[..., r0:r1, :]

    def batches(self, op, nb):
        lead = (slice(None),) * len(self.lead)
        return op.batches(nb) if self.reports_maxima else op[lead + (slice(nb),)]


PLANS = collections.OrderedDict((a.name, a) for a in (
    Fp32('fp32', 'f32'),
    Planes('fp32x3', 'x3', split=ops.split_bf16x3, gemm_nt=ops.gemm_f32x3_nt, fmt=L.PLANES_BF16X3,
           kpad=16, lead=(3,), dtype=torch.bfloat16),
    Planes('fp16x2', 'h2', split=ops.split_f16x2, gemm_nt=ops.gemm_f32_f16x2_nt, fmt=L.PLANES_F16X2,
           kpad=32, lead=(2,), dtype=torch.float16, reports_maxima=True, wgrad_update=True,
           update_after=1, roi_maps_on_chains=True),
    Planes('bf16', 'bf16', split=ops.to_bf16_slab, gemm_nt=ops.gemm_bf16_slab_nt, fmt=L.PLANES_BF16,
           kpad=64, lead=(), dtype=torch.bfloat16, wgrad_update=True, update_after=2,
           roi_maps_on_chains=True, roi_pool_slab=True)))


def plan(name):
    """The arithmetic object of mfma_dtype `name` (an object passes through)."""
    if not isinstance(name, Fp32) and name not in PLANS:
        raise ValueError('mfma_dtype must be one of %s, not %r' % (', '.join(map(repr, PLANS)), name))
    return PLANS.get(name, name)
