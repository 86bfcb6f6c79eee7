"""tests/guard.py on the CPU: the sentinel is a NaN in every type, the carved view has the strides
and alignment that were asked for, and check() finds a stray word in each kind of gap."""
import pytest
import torch

import guard


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16, torch.bfloat16])
def test_sentinel_is_nan_and_view_is_carved_as_asked(dtype):
    g = guard.carve((3, 5, 6), dtype, 'cpu', ld=10, batch_stride=64)
    assert g.t.shape == (3, 5, 6) and g.t.stride() == (64, 10, 1)
    assert g.t.data_ptr() % 16 == 0
    assert bool(torch.isnan(g.buf).all()) and guard.holds_sentinel(g.t)
    g.t.zero_()
    g.check()
    u = guard.carve((5, 6), dtype, 'cpu', ld=8, aligned=False)
    assert u.t.data_ptr() % 16 == 4 and u.t.stride() == (8, 1)
    n = guard.carve((2, 3, 4, 8), dtype, 'cpu')
    assert n.t.is_contiguous() and n.t.shape == (2, 3, 4, 8)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16, torch.int32])
@pytest.mark.parametrize('where,expect', [
    (-1, (-1, -1, -1)),                # the word in front of the view
    (6, (0, 0, 6)),                    # the gap after row 0
    (4 * 10 + 6, (0, 4, 6)),           # after the last row of item 0: the gap between items
    (64 + 2 * 10 + 9, (1, 2, 9)),      # the last gap word of a row of item 1
    (2 * 64 + 4 * 10 + 6, (2, 4, 6)),  # the first word behind the view
])
def test_check_reports_the_first_damaged_word(dtype, where, expect):
    g = guard.carve((3, 5, 6), dtype, 'cpu', ld=10, batch_stride=64)
    g.t.zero_()
    g.buf[g.offset + where] = 1
    assert g.damage()[:3] == expect
    with pytest.raises(AssertionError, match='write outside the view'):
        g.check()


def test_a_rewritten_sentinel_value_is_not_damage_and_a_nan_of_other_bits_is():
    g = guard.carve((4, 4), torch.float32, 'cpu', ld=8)
    g.buf[g.offset + 5] = float('nan')              # the default NaN 0x7FC00000: other bits
    assert g.damage()[:3] == (0, 0, 5)
    p = guard.place(torch.arange(12.).view(3, 4), ld=8)
    assert torch.equal(p.t, torch.arange(12.).view(3, 4)) and p.damage() is None
    assert guard.same_bits(p.t, torch.arange(12.).view(3, 4))
    assert not guard.same_bits(torch.zeros(2), -torch.zeros(2))
