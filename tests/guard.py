"""Guard bands around device tensors (a helper module of the GPU tests, not a conftest).

`carve()` returns a Guarded whose `.t` is a view into ONE flat device buffer that was filled with
a sentinel word in advance; the caller chooses the shape, the dtype, the row stride (`ld`), the
batch stride and whether the view starts on a 16-byte boundary.  Everything in the buffer that is
not an element of the view - the margins in front of and behind it, the gap after every row, the
gap after every batch item - must still hold the sentinel, bit for bit, after a kernel ran:
`check()` compares bit patterns and reports the first damaged element as (batch, row, col) relative
to the view.

The sentinel 0x7FC17FC1 is a NaN as one fp32 word and as two fp16 or two bf16 halves, so poison
around an INPUT (`place()`) reaches the result when a kernel reads outside its operand and uses
what it read."""
import torch

SENTINEL = 0x7FC17FC1                       # fp32 NaN; halves 0x7FC1: fp16 NaN and bf16 NaN
MARGIN_BYTES = 1024                         # in front of and behind the view (a multiple of 16)

_ELEM_BITS = {4: (torch.int32, SENTINEL), 2: (torch.int16, SENTINEL & 0xFFFF)}


class Guarded(object):
    """.t: the carved view; .buf: the flat buffer in the view's dtype; .check(): guards intact."""

    def __init__(self, shape, dtype, device, ld=None, batch_stride=None, aligned=True):
        shape = tuple(int(s) for s in shape)
        es = torch.empty((), dtype=dtype).element_size()
        if es not in _ELEM_BITS:
            raise TypeError('guard: 2- and 4-byte element types only')
        # the view as [batch, rows, cols]; a shape of any other rank is carved as one contiguous row
        if len(shape) == 3:
            batch, rows, cols = shape
        elif len(shape) == 2:
            (rows, cols), batch = shape, 1
        else:
            if ld is not None or batch_stride is not None:
                raise ValueError('guard: strides are for 2-D and 3-D views')
            batch, rows, cols = 1, 1, 1
            for s in shape:
                cols *= s
        ld = cols if ld is None else int(ld)
        bs = rows * ld if batch_stride is None else int(batch_stride)
        if ld < cols or (batch > 1 and bs < (rows - 1) * ld + cols):
            raise ValueError('guard: overlapping rows or batch items')
        per_word = 4 // es
        margin = MARGIN_BYTES // es
        self.offset = margin + (0 if aligned else per_word)          # one fp32 word off 16 bytes
        span = (batch - 1) * bs + (rows - 1) * ld + cols
        nelem = self.offset + span + margin
        nwords = (nelem + per_word - 1) // per_word
        nwords = (nwords + 3) // 4 * 4
        self._words = torch.full((nwords,), SENTINEL, dtype=torch.int32, device=device)
        assert self._words.data_ptr() % 16 == 0
        self.buf = self._words.view(dtype)
        self.batch, self.rows, self.cols, self.ld, self.bs = batch, rows, cols, ld, bs
        v3 = torch.as_strided(self.buf, (batch, rows, cols), (bs, ld, 1), self.offset)
        if len(shape) == 3:
            self.t = v3
        elif len(shape) == 2:
            self.t = v3[0]
        else:
            self.t = v3.view(shape)
        assert (self.t.data_ptr() % 16 == 0) == bool(aligned)
        bits, self._sent = _ELEM_BITS[es]
        self._bits = self._words.view(bits)
        inside = torch.zeros((self._bits.numel(),), dtype=torch.bool, device=device)
        torch.as_strided(inside, (batch, rows, cols), (bs, ld, 1), self.offset).fill_(True)
        self._outside = ~inside

    def poison(self):
        """Refill the view itself with the sentinel (an output that must be written completely)."""
        self.t.view(self._bits.dtype).fill_(self._sent)
        return self

    def damage(self):
        """None, or (batch, row, col, element offset from the view's start) of the first word
        outside the view that no longer holds the sentinel."""
        bad = (self._bits != self._sent) & self._outside
        if not bool(bad.any()):
            return None
        rel = int(bad.nonzero()[0, 0]) - self.offset
        if rel < 0:                                   # the margin in front: (-1, -1, offset)
            return (-1, -1, rel, rel)
        b = min(rel // self.bs, self.batch - 1)
        row = (rel - b * self.bs) // self.ld          # (>= rows: the margin behind the last row)
        return (b, row, rel - b * self.bs - row * self.ld, rel)

    def check(self, what='tensor'):
        d = self.damage()
        assert d is None, ('%s: write outside the view at (batch %d, row %d, col %d), element %d '
                           'from its start (view %d x %d x %d, ld %d, batch stride %d)'
                           % ((what,) + d + (self.batch, self.rows, self.cols, self.ld, self.bs)))


def carve(shape, dtype=torch.float32, device='cuda', ld=None, batch_stride=None, aligned=True):
    """A sentinel-filled buffer with a view of `shape` carved out of it (the view holds the
    sentinel too: an element the kernel skips stays NaN)."""
    return Guarded(shape, dtype, device, ld=ld, batch_stride=batch_stride, aligned=aligned)


def place(x, ld=None, batch_stride=None, aligned=True):
    """A carved copy of the tensor x: the same values, poison all around them."""
    g = Guarded(x.shape, x.dtype, x.device, ld=ld, batch_stride=batch_stride, aligned=aligned)
    g.t.copy_(x)
    return g


def same_bits(x, y):
    """Bit-pattern equality (NaN-safe, -0.0 != +0.0) of two tensors of one shape and dtype."""
    if x.shape != y.shape or x.dtype != y.dtype:
        return False
    bits = {4: torch.int32, 2: torch.int16}[x.element_size()]
    return torch.equal(x.contiguous().view(bits), y.contiguous().view(bits))


def holds_sentinel(x):
    """Every element of x still is the sentinel, bit for bit."""
    bits, sent = _ELEM_BITS[x.element_size()]
    return bool((x.contiguous().view(bits) == sent).all())
