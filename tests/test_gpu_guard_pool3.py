"""Guard bands (tests/guard.py) around the output of naws_maxpool3x3_nhwc_fwd: the kernel writes
into an `out=` carved from a sentinel-filled buffer, reads an input that sits inside poison (a read
outside it would bring a NaN into the result), and must leave every word around both untouched.
(2, 9, 7, 64): odd sizes, the last window half in padding, a strip of four output pixels cut short;
(1, 2, 2, 4): one window clipped on all sides."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guard

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('shape', [(2, 9, 7, 64), (1, 2, 2, 4)])
def test_maxpool3x3(dev, shape, stride):
    from naws_hip import ops
    rng = np.random.default_rng(sum(shape) + stride)
    x = torch.from_numpy(rng.integers(-100, 0, shape).astype(np.float32))       # all negative
    ref = F.max_pool2d(x.permute(0, 3, 1, 2), 3, stride, 1).permute(0, 2, 3, 1).contiguous()
    gx = guard.place(x.to(dev))
    gy = guard.carve(tuple(ref.shape), torch.float32, dev)
    ret = ops.maxpool3x3_nhwc(gx.t, stride, out=gy.t)
    torch.cuda.synchronize()
    assert ret.data_ptr() == gy.t.data_ptr()
    assert guard.same_bits(gy.t.cpu(), ref)
    gy.check('out')
    gx.check('x')
