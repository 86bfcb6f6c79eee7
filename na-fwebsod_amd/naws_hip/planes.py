"""The 16-bit operand planes of fc6_w [rows6, k6] / fc7_w [rows6 / hidden, hidden, hidden] / fc7_w^T
(fp16x2, fp32x3 and bf16 plans) and the region tables that tell the plane-writing SGD kernel
(ops.acm_sgd_update_planes) which rows of them an update owns.  The fp16x2 scale words of both
matrices live in ONE arena, [fc6: maxima | 1/scale][fc7: maxima | 1/scale] with rows6 words each, so
that the SGD kernels can report the updated rows' maxima straight into them; `maxima`, `inv_scale`
and `bound` name its parts, and nothing outside this module indexes it."""

import torch

from . import head_arith
from . import ops

SKIP_ROWS = 32      # reducer.owner_blocks cuts fc6_w in multiples of this: a skipped block's batch
ALL = 'all'         # every row of fc6_w, for begin() / resplit6()


class FcPlanes(object):
    def __init__(self, plan, rows6, k6, hidden, o6, ob, o7, total, device, one_run6=True,
                 one_run7=True):
        """plan: the engine's mfma_dtype (or its head_arith object); o6 / ob / o7 / total: first arena
        element of fc6_w / fc6_b / fc7_w and the arena's length; one_run6 / one_run7: the matrix has
        ONE (lr_mult, weight decay).  Allocates and launches nothing: split_all() fills the planes."""
        ar = self.arith = head_arith.plan(plan)
        if not ar.planes16:
            raise ValueError('the %r plan has no operand planes' % (ar.name,))
        self.rows6, self.k6, self.hidden = rows6, k6, hidden
        self.o6, self.ob, self.o7, self.total, self.all6 = o6, ob, o7, total, (0, rows6)
        nb = rows6 // hidden
        self.convert, self.fmt = ar.operand, ar.fmt
        s6 = (-(-k6 // ar.kpad) * ar.kpad // 16, rows6, 16)
        s7 = (nb, -(-hidden // ar.kpad) * ar.kpad // 16, hidden, 16)

        def alloc(shape):
            return torch.empty(ar.lead + shape, device=device, dtype=ar.dtype)
        self.scales = self.ovf = self.rm_table = self._bound = None
        # the SGD kernel can write the planes: a wave's 256 floats stay in one row, one pair of
        # hyper-parameters per matrix (otherwise: the element-wise kernel + re-split, no tables)
        writable = k6 % 256 == 0 and one_run6 and one_run7
        if ar.reports_maxima:
            self.scales = torch.zeros((4 * rows6,), device=device, dtype=torch.float32)
            self._arena = self.scales.view(2, 2, rows6)       # [operand][maxima | 1/scale][rows]
            self.operands = dict(
                w6=ops.F16x2(alloc(s6), self.scales[:2 * rows6].view(2, rows6)),
                w7=ops.F16x2(alloc(s7), self.scales[2 * rows6:].view(2, nb, hidden)),
                # fc7_w's COLUMN maxima = the row maxima of fc7_w^T (the dgrad's operand): the SGD
                # kernel reports them too, so the transposed planes need no maxima pass either
                w7t=ops.F16x2(alloc(s7), torch.empty((2, nb, hidden), device=device,
                                                     dtype=torch.float32)))
            self.rm_table = ops.RowmaxTable([(o6, o6 + rows6 * k6, k6, 0),
                                              (o7, o7 + rows6 * hidden, hidden, 2 * rows6)], device)
            if writable:
                # [w6 rows | w7 rows] maxima before an update = the planes' scale bounds; the overflow word
                self._bound = torch.zeros((2 * rows6,), device=device, dtype=torch.int32)
                self.ovf = torch.zeros((1,), device=device, dtype=torch.int32)
        else:
            self.operands = dict(w6=alloc(s6), w7=alloc(s7), w7t=alloc(s7))
        # the one-launch tables: every row owned, and fc6_w "updated elsewhere" (train_step)
        self.whole = self.table(self.all6) if writable else None
        self.rest = self.table(None, [self.all6]) if writable else None

    # ---- the fp16x2 scale words by name (fc6's take an optional row range) ----------------------
    def maxima(self, op, rows=(None,)):
        """int32 words: max|w| per row of fc`op`_w as the last update (or split) reported them."""
        return self._arena[op - 6, 0].view(torch.int32)[slice(*rows)]

    def inv_scale(self, op, rows=(None,)):
        return self._arena[op - 6, 1][slice(*rows)]

    def bound(self, op, rows=(None,)):
        """int32 words: the maxima before the update, from which it derives the rows' scales."""
        return self._bound.view(2, self.rows6)[op - 6][slice(*rows)]

    @property
    def colmax7(self):
        return self.operands['w7t'].scales[0].view(torch.int32)

    # ---- region tables --------------------------------------------------------------------------
    def table(self, own6, skip6=(), origin=0, with7=True):
        """ops.SgdPlaneRegions for an update launched on the arena from element `origin`: the
        fc6_w rows own6 = (r0, r1) (or None) are updated with their planes, the row ranges in
        `skip6` are left alone, fc7_w (with7) is updated whole."""
        h2 = self.arith.reports_maxima
        p6, p7 = ((self.operands[k].planes if h2 else self.operands[k]) for k in ('w6', 'w7'))
        regs = [(self.o6 + r0 * self.k6 - origin, r1 - r0, self.k6,
                 self.rows6 if (r0, r1) == self.all6 else SKIP_ROWS, None, None, None, None)
                for r0, r1 in skip6]
        if own6 is not None:
            words = [f(6, own6) if h2 else None for f in (self.bound, self.maxima, self.inv_scale)]
            regs.append((self.o6 + own6[0] * self.k6 - origin, own6[1] - own6[0], self.k6, self.rows6,
                         p6 if own6 == self.all6 else (p6, own6[0]), *words))
        regs.sort(key=lambda r: r[0])
        if with7:
            words = ([self.bound(7), self.maxima(7), self.inv_scale(7), self.colmax7] if h2
                     else [None, None, None])
            regs.append((self.o7 - origin, self.rows6, self.hidden, self.hidden, p7, *words))
        return ops.SgdPlaneRegions(regs, self.fmt)

    # the pipelined update's launches over fc6_w's rows r0..r1 alone and over the arena from fc7_w
    # on (fc6's biases, ob..o7, go between them), each (first arena element, count, table)
    def piece(self, r0, r1):
        start = self.o6 + r0 * self.k6
        return start, (r1 - r0) * self.k6, self.table((r0, r1), origin=start, with7=False)

    def tail(self):
        return self.o7, self.total - self.o7, self.table(None, origin=self.o7)

    def shard_table(self, b0, b1):
        """The owner-only update: this rank's rows b0..b1 of fc6_w, the other owners' skipped."""
        return self.table((b0, b1), [r for r in ((0, b0), (b1, self.rows6)) if r[0] < r[1]])

    # ---- the steps every fp16x2 update route shares ---------------------------------------------
    def begin(self, rows6, with7):
        """Before the plane-writing kernel: the maxima of fc6_w's rows `rows6` (None, ALL or
        (r0, r1)) and (with7) of fc7_w become the bounds of this update and are zeroed for the
        kernel to report the new ones into; so are fc7_w's column maxima."""
        if rows6 is ALL and with7:              # both operands whole: one copy, one fill
            self._bound.view(2, self.rows6).copy_(self._arena[:, 0].view(torch.int32))
            self._arena[:, 0].zero_()
        else:
            if rows6 is not None:
                rows6 = self.all6 if rows6 is ALL else rows6
                self.bound(6, rows6).copy_(self.maxima(6, rows6))
                self.maxima(6, rows6).zero_()
            if with7:                           # (cleared as fp32 words, as the joint fill does)
                self.bound(7).copy_(self.maxima(7))
                self._arena[1, 0].zero_()
        if with7:
            self.operands['w7t'].scales[0].zero_()

    def zeroed_rowmax(self):
        """Both operands' maxima zeroed -> the arena's words (element-wise kernel + rm_table)."""
        self._arena[:, 0].zero_()
        return self.scales.view(torch.int32)

    def resplit6(self, w6, rows, ovf=None, tag=0, rowmax=None):
        """Redo the planes of fc6_w's rows `rows` (ALL or (r0, r1)) from `rowmax` (default: the
        exact maxima the update reported) if ovf[0] == tag when the kernel runs (ovf None: always);
        otherwise - no row outgrew its bound - the workgroups leave at once."""
        rowmax = self.maxima(6) if rowmax is None else rowmax
        if rows is ALL:
            ops.split_f16x2_rows_if(w6, rowmax, self.operands['w6'], ovf, tag)
        else:
            ops.split_f16x2_row_range_if(w6, rowmax, self.operands['w6'], rows[0], rows[1],
                                         cond=ovf, cond_value=tag)

    def finish7(self, w7, ovf, tag):
        """After the kernel: fc7_w's conditional exact re-split, and fc7_w^T from the column
        maxima the kernel has just reported (one pass: no maxima pass, no transposing split)."""
        ops.split_f16x2_rows_if(w7, self.maxima(7), self.operands['w7'], ovf, tag)
        ops.split_f16x2_dual(w7, None, self.operands['w7t'].scales, out_t=self.operands['w7t'])

    def split_from_maxima(self, w6, w7):
        """fp16x2 after the element-wise kernel: planes from the row maxima it reported."""
        for w, op in ((w6, self.operands['w6']), (w7, self.operands['w7'])):
            ops.split_f16x2_dual(w, op.scales, None, out_n=op)
        ops.split_f16x2(w7, transpose=True, out=self.operands['w7t'])

    def split_all(self, w6, w7):
        """Every plane from scratch (exact maxima)."""
        self.convert(w6, out=self.operands['w6'])
        self.convert(w7, out=self.operands['w7'])
        self.convert(w7, transpose=True, out=self.operands['w7t'])
