#!/usr/bin/env python3
"""What the GEMM / split / conv3x3 wrappers of naws_hip/ops.py pass to the C ABI, per operand form.

`naws_hip.lib.call` is replaced by a recorder that launches nothing: each case calls wrappers on
named device tensors and yields the tuples they would have passed, every pointer rewritten as
(name of the tensor whose storage holds it, byte offset from the storage base) - or '?' for a
buffer the wrapper allocated itself - plus a description of what the wrapper returned, or the
exception it raised.  A device is needed only because the wrappers refuse CPU tensors.

    python tests/golden/make_ops_call_args.py --record [--ops PATH/TO/ops.py]

writes ops_call_args_before.json; --ops records another version of the module (the fixture was
recorded with the ops.py of the commit BEFORE the wrappers were rewritten over shared helpers).
"""
import importlib.util
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, 'ops_call_args_before.json')

F32, BF16, F16, I32 = torch.float32, torch.bfloat16, torch.float16, torch.int32
M, N, K, B = 48, 32, 64, 2


class Tensors(object):
    """Named device tensors; pointers are reported relative to their storages."""

    def __init__(self, dev):
        self.dev, self.named = dev, {}

    def __call__(self, name, shape, dtype=F32):
        t = torch.empty(shape, device=self.dev, dtype=dtype)
        self.named[name] = t
        return t

    def locate(self, v):
        for name, t in self.named.items():
            base = t.untyped_storage().data_ptr()
            if base <= v < base + max(t.untyped_storage().nbytes(), 1):
                return ['ptr', name, v - base]
        return ['ptr', '?'] if 1 << 32 <= v < 1 << 63 else v      # (a masked negative seed is >= 2^63)


def _describe(r):
    if r is None:
        return None
    if isinstance(r, (tuple, list)):
        return [_describe(x) for x in r]
    if isinstance(r, torch.Tensor):
        return [str(r.dtype), list(r.shape), list(r.stride())]
    return {'planes': _describe(r.planes), 'scales': _describe(r.scales)}      # ops.F16x2


def f16x2(ops, t, name, outer, k, batch=None):
    b = () if batch is None else (batch,)
    return ops.F16x2(t(name + '.planes', (2, *b, k // 16, outer, 16), F16),
                     t(name + '.scales', (2, *b, outer)))


# ---- cases: name -> fn(ops, t) -----------------------------------------------------------------------
CASES = []


def case(f):
    CASES.append((f.__name__, f))
    return f


def _dense(ops, t, fn, batched=False, strided=False, dtype_b=F32, **kw):
    b = (B,) if batched else ()
    a = t('a', (*b, M, K))
    bt = t('b', (*b, N, K), dtype_b)
    if strided:
        kw['out'] = t('out', (*b, M, 48))[..., :32]
        if fn != 'gemm_splitk':
            kw['aux'] = t('aux', (*b, M, 48))[..., :32]
            kw['epilogue'] = ops.L.EPI_GATE_POS
    return getattr(ops, fn)(a, bt, **({'trans_b': True} if fn != 'gemm_bf16_nt' else {}), **kw)


for _fn in ('gemm', 'gemm_splitk', 'gemm_bf16_nt'):
    def _mk(fn):
        def plain(ops, t): return _dense(ops, t, fn)
        def batched(ops, t): return _dense(ops, t, fn, batched=True)
        def strided(ops, t): return _dense(ops, t, fn, strided=True)
        def batched_strided(ops, t): return _dense(ops, t, fn, batched=True, strided=True)

        def row_sliced(ops, t):
            a, b = t('a', (B, 64, K))[:, 16:48], t('b', (B, N, K))
            return getattr(ops, fn)(a, b, **({'trans_b': True} if fn != 'gemm_bf16_nt' else {}))

        def bias2d(ops, t):
            return _dense(ops, t, fn, batched=True, epilogue=ops.L.EPI_BIAS,
                          bias=t('bias', (B, 40))[:, :N])

        def wrong_dtype(ops, t): return _dense(ops, t, fn, dtype_b=torch.float64)

        def noncontiguous(ops, t):
            a, b = t('a', (M, 2 * K))[:, ::2], t('b', (N, K))
            return getattr(ops, fn)(a, b, **({'trans_b': True} if fn != 'gemm_bf16_nt' else {}))

        def k_mismatch(ops, t):
            a, b = t('a', (M, K)), t('b', (N, K + 16))
            return getattr(ops, fn)(a, b, **({'trans_b': True} if fn != 'gemm_bf16_nt' else {}))
        for f in (plain, batched, strided, batched_strided, row_sliced, bias2d, wrong_dtype,
                  noncontiguous, k_mismatch):
            CASES.append(('%s.%s' % (fn, f.__name__), f))
        if fn != 'gemm_splitk':
            def foreign_aux(ops, t):
                return _dense(ops, t, fn, batched=True, aux=t('aux', (B, M + 1, N))[:, :M],
                              epilogue=ops.L.EPI_GATE_POS)
            CASES.append(('%s.foreign_aux' % fn, foreign_aux))
    _mk(_fn)


@case
def gemm_trans_and_amax(ops, t):
    return ops.gemm(t('a', (K, M)), t('b', (K, N)), trans_a=True, alpha=0.5, seed=-3, accumulate=True,
                    rowmax=t('rowmax', (M,), I32), colmax=t('colmax', (N,), I32),
                    colmax_rowmul=t('mul', (M,)))


@case
def gemm_splitk_workspace(ops, t):
    return ops.gemm_splitk(t('a', (M, K)), t('b', (N, K)), trans_b=True, ksplit=3,
                           workspace=t('ws', (M * N * 3,)), epilogue=ops.L.EPI_BIAS, bias=t('bias', (N,)))


def _slab(t, name, rows, k=K, batch=None, lead=()):
    b = () if batch is None else (batch,)
    return t(name, (*lead, *b, k // 16, rows, 16), BF16)


def _planes_cases(fn, mk, sliced, nplanes_err):
    """mk(ops, t, rows_a, batch) -> (a, b) operands of the wrapper `fn`."""
    def plain(ops, t): return getattr(ops, fn)(*mk(ops, t, M, None))
    def batched(ops, t): return getattr(ops, fn)(*mk(ops, t, M, B))

    def row_sliced(ops, t):
        a, b = mk(ops, t, 64, B)
        return getattr(ops, fn)(sliced(a), b)

    def strided(ops, t):
        a, b = mk(ops, t, M, B)
        return getattr(ops, fn)(a, b, out=t('out', (B, M, 48))[..., :32], aux=t('aux', (B, M, 48))[..., :32],
                                epilogue=ops.L.EPI_GATE_POS, alpha=2.0, seed=(1 << 64) + 5, accumulate=1)

    def bias2d(ops, t):
        a, b = mk(ops, t, M, B)
        return getattr(ops, fn)(a, b, epilogue=ops.L.EPI_BIAS_RELU_DROP, drop_ratio=0.5,
                                bias=t('bias', (B, 40))[:, :N])

    def foreign_aux(ops, t):
        a, b = mk(ops, t, M, B)
        return getattr(ops, fn)(a, b, aux=t('aux', (B, M + 1, N))[:, :M], epilogue=ops.L.EPI_GATE_POS)

    def k_mismatch(ops, t):
        a, _ = mk(ops, t, M, None)
        t2 = Tensors(t.dev)
        _, b = mk(ops, t2, M, None, k=K + 32)
        t.named.update({'k2.' + n: v for n, v in t2.named.items()})
        return getattr(ops, fn)(a, b)
    for f in (plain, batched, row_sliced, strided, bias2d, foreign_aux, k_mismatch, nplanes_err):
        CASES.append(('%s.%s' % (fn, f.__name__), f))


def _mk_slab(ops, t, rows_a, batch, k=K):
    return _slab(t, 'a', rows_a, k, batch), _slab(t, 'b', N, k, batch)


def _mk_x3(ops, t, rows_a, batch, k=K):
    return _slab(t, 'a', rows_a, k, batch, (3,)), _slab(t, 'b', N, k, batch, (3,))


def _mk_h2(ops, t, rows_a, batch, k=K):
    return f16x2(ops, t, 'a', rows_a, k, batch), f16x2(ops, t, 'b', N, k, batch)


def _bad_slab(ops, t): return ops.gemm_bf16_slab_nt(t('a', (K // 16, M, 16), F16), _slab(t, 'b', N))
def _bad_x3(ops, t): return ops.gemm_f32x3_nt(_slab(t, 'a', M, lead=(2,)), _slab(t, 'b', N, lead=(3,)))


def _bad_h2(ops, t):
    a, b = _mk_h2(ops, t, M, None)
    return ops.gemm_f32_f16x2_nt(ops.F16x2(a.planes.transpose(-1, -2), a.scales), b)


_planes_cases('gemm_bf16_slab_nt', _mk_slab, lambda a: a[..., 16:48, :], _bad_slab)
_planes_cases('gemm_f32x3_nt', _mk_x3, lambda a: a[..., 16:48, :], _bad_x3)
_planes_cases('gemm_f32_f16x2_nt', _mk_h2, lambda a: a.rows(16, 48), _bad_h2)


@case
def gemm_f32_f16x2_nt_amax(ops, t):
    a, b = _mk_h2(ops, t, M, None)
    return ops.gemm_f32_f16x2_nt(a, b, rowmax=t('rowmax', (M,), I32), rowmax_seg=256,
                                 colmax=t('colmax', (N,), I32), colmax_rowmul=t('mul', (M,)))


@case
def gemm_f32_f16x2_nt_strided_scales(ops, t):
    a, b = _mk_h2(ops, t, M, None)
    return ops.gemm_f32_f16x2_nt(ops.F16x2(a.planes, t('s2', (2, M, 2))[..., 0]), b)


def _cols(ops, t, **kw):
    a = f16x2(ops, t, 'a', M, K)
    b = f16x2(ops, t, 'b', 64, K).rows(16, 48)
    return ops.gemm_f32_f16x2_nt_cols(a, b, t('out', (M, 64))[:, 16:48], 16, 48, **kw)


@case
def gemm_f32_f16x2_nt_cols(ops, t):
    return _cols(ops, t, epilogue=ops.L.EPI_BIAS_RELU_DROP, bias=t('bias', (64,))[16:48],
                 drop_ratio=0.5, seed=7, rowmax=t('rowmax', (M,), I32), colmax=t('colmax', (64,), I32)[16:48])


@case
def gemm_f32_f16x2_nt_cols_batched_operand(ops, t):
    return ops.gemm_f32_f16x2_nt_cols(f16x2(ops, t, 'a', M, K, B), f16x2(ops, t, 'b', N, K, B),
                                      t('out', (M, N)), 0, N)


@case
def gemm_f32_f16x2_nt_cols_bad_out(ops, t):
    return ops.gemm_f32_f16x2_nt_cols(f16x2(ops, t, 'a', M, K), f16x2(ops, t, 'b', N, K),
                                      t('out', (M, N + 1)), 0, N)


def _xk_ops(ops, t):
    # a: K = 64 proposals (padded), M = 48; x: forward planes of a [R = 48, N_all = 64] matrix
    return f16x2(ops, t, 'a', M, K), f16x2(ops, t, 'x', 48, 64)


@case
def gemm_f32_f16x2_nt_xk(ops, t):
    return ops.gemm_f32_f16x2_nt_xk(*_xk_ops(ops, t))


@case
def gemm_f32_f16x2_nt_xk_ncols(ops, t):
    a, x = _xk_ops(ops, t)
    return ops.gemm_f32_f16x2_nt_xk(a, x, out=t('out', (M, 64))[:, 16:32], ncols=(16, 32),
                                    scale_x=t('sx', (64,))[16:32])


@case
def gemm_f32_f16x2_nt_xk_bad_ncols(ops, t):
    return ops.gemm_f32_f16x2_nt_xk(*_xk_ops(ops, t), ncols=(8, 32))


@case
def gemm_f32_f16x2_nt_xk_batched_operand(ops, t):
    return ops.gemm_f32_f16x2_nt_xk(f16x2(ops, t, 'a', M, K, B), f16x2(ops, t, 'x', 48, 64))


def _xk_sgd(ops, t, rows=None, ncols=None, m_all=M, wdtype=F16):
    a, x = _xk_ops(ops, t)
    if rows is not None:
        a = f16x2(ops, t, 'a', rows[1] - rows[0], K)
    return ops.gemm_f32_f16x2_nt_xk_sgd(
        a, x, t('param', (m_all, 64)), t('mom', (m_all, 64)), t('lr', (1,)), 1.0, 5e-4, 0.9, False, 2, 3,
        t('wplanes', (2, 4, m_all, 16), wdtype), t('bound', (m_all,), I32), t('rowmax', (m_all,), I32),
        t('inv', (m_all,)), t('overflow', (1,), I32), 9, ncols=ncols, rows=rows)


@case
def gemm_f32_f16x2_nt_xk_sgd(ops, t): return _xk_sgd(ops, t)
@case
def gemm_f32_f16x2_nt_xk_sgd_rows_ncols(ops, t): return _xk_sgd(ops, t, rows=(16, 48), ncols=(16, 32), m_all=64)
@case
def gemm_f32_f16x2_nt_xk_sgd_bad_rows(ops, t): return _xk_sgd(ops, t, rows=(16, 40), m_all=64)
@case
def gemm_f32_f16x2_nt_xk_sgd_bad_planes(ops, t): return _xk_sgd(ops, t, wdtype=BF16)


def _slab_sgd(ops, t, rows=None, m_all=M, wdtype=BF16):
    m = M if rows is None else rows[1] - rows[0]
    return ops.gemm_bf16_slab_nt_sgd(
        _slab(t, 'a', m), _slab(t, 'b', N), t('param', (m_all, N)), t('mom', (m_all, N)), t('lr', (1,)),
        1.0, 5e-4, 0.9, True, 1, 0, t('wplane', (N // 16, m_all, 16), wdtype), rows=rows)


@case
def gemm_bf16_slab_nt_sgd(ops, t): return _slab_sgd(ops, t)
@case
def gemm_bf16_slab_nt_sgd_rows(ops, t): return _slab_sgd(ops, t, rows=(16, 48), m_all=64)
@case
def gemm_bf16_slab_nt_sgd_bad_rows(ops, t): return _slab_sgd(ops, t, rows=(16, 80), m_all=64)
@case
def gemm_bf16_slab_nt_sgd_bad_plane(ops, t): return _slab_sgd(ops, t, wdtype=F16)


# splits: 2-D, batched, row-strided source, transposed, caller's out
for _fn in ('split_bf16x3', 'to_bf16_slab', 'split_f16x2'):
    def _mk(fn):
        def plain(ops, t): return getattr(ops, fn)(t('x', (M, 40)))
        def batched_t(ops, t): return getattr(ops, fn)(t('x', (B, M, 40)), transpose=True)
        def strided(ops, t): return getattr(ops, fn)(t('x', (B, 64, 48))[:, 16:48, :40])
        def wrong_dtype(ops, t): return getattr(ops, fn)(t('x', (M, 40), torch.float64))
        def noncontiguous(ops, t): return getattr(ops, fn)(t('x', (M, 80))[:, ::2])
        for f in (plain, batched_t, strided, wrong_dtype, noncontiguous):
            CASES.append(('%s.%s' % (fn, f.__name__), f))
    _mk(_fn)


@case
def split_bf16x3_out(ops, t): return ops.split_bf16x3(t('x', (M, 40)), out=t('p', (3, 3, M, 16), BF16))
@case
def to_bf16_slab_out(ops, t): return ops.to_bf16_slab(t('x', (M, 40)), out=t('p', (4, M, 16), BF16))


@case
def split_f16x2_out_rowmul(ops, t):
    return ops.split_f16x2(t('x', (M, 40)), out=f16x2(ops, t, 'o', M, 64), rowmul=t('mul', (M,)))


@case
def split_f16x2_bad_rowmul(ops, t): return ops.split_f16x2(t('x', (M, 40)), rowmul=t('mul', (M + 1,)))


def _dual(ops, t, x, batch=None, **kw):
    b = () if batch is None else (batch,)
    rows, cols = x.shape[-2:]
    return ops.split_f16x2_dual(x, scales_n=t('sn', (2, *b, rows)), scales_t=t('st', (2, *b, cols)), **kw)


@case
def split_f16x2_dual(ops, t): return _dual(ops, t, t('x', (M, 40)), rowmul=t('mul', (M,)))
@case
def split_f16x2_dual_batched_strided(ops, t): return _dual(ops, t, t('x', (B, 64, 48))[:, 16:48, :40], B)
@case
def split_f16x2_dual_t_only(ops, t): return ops.split_f16x2_dual(t('x', (M, 40)), scales_t=t('st', (2, 40)))
@case
def split_f16x2_dual_wrong_dtype(ops, t): return _dual(ops, t, t('x', (M, 40), F16))
@case
def split_f16x2_dual_noncontiguous(ops, t): return _dual(ops, t, t('x', (M, 80))[:, ::2])
@case
def split_f16x2_dual_bad_scales(ops, t): return ops.split_f16x2_dual(t('x', (M, 40)), scales_n=t('sn', (2, M + 1)))


@case
def transpose_to_bf16(ops, t): return ops.transpose_to_bf16(t('x', (M, 40)))
@case
def transpose_to_bf16_batched_pad_out(ops, t):
    return ops.transpose_to_bf16(t('x', (B, M, 40)), rows_pad=64, out=t('y', (B, 40, 64), BF16))
@case
def transpose_to_bf16_row_strided(ops, t): return ops.transpose_to_bf16(t('x', (M, 48))[:, :40])
@case
def transpose_to_bf16_bad_batch_stride(ops, t): return ops.transpose_to_bf16(t('x', (B, 64, 40))[:, :M])


@case
def split_f16x2_rows_if(ops, t):
    return ops.split_f16x2_rows_if(t('x', (M, 40)), t('rowmax', (M,), I32), f16x2(ops, t, 'o', M, 64),
                                   t('cond', (1,), I32), 1)


@case
def split_f16x2_rows_if_batched_strided(ops, t):
    return ops.split_f16x2_rows_if(t('x', (B, 64, 48))[:, 16:48, :40], t('rowmax', (B * 32,), I32),
                                   f16x2(ops, t, 'o', 32, 64, B), None, 0)


# conv3x3 wrappers at 1 x 8 x 32 x 16 -> 64 channels: out allocated / supplied, pool2 on / off
CN, CH, CW, CI, CO = 1, 8, 32, 16, 64


def _conv_cases(fn, weight, pool, **kw):
    def alloc(ops, t): return getattr(ops, fn)(t('x', (CN, CH, CW, CI)), weight(ops, t), t('bias', (CO,)), **kw)

    def out(ops, t):
        return getattr(ops, fn)(t('x', (CN, CH, CW, CI)), weight(ops, t), None, relu=False,
                                out=t('y', (CN, CH, CW, CO)), **kw)

    def bad_out(ops, t):        # wrong shape: refused only by the wrappers that validate `out`
        return getattr(ops, fn)(t('x', (CN, CH, CW, CI)), weight(ops, t), t('bias', (CO,)),
                                out=t('y', (CN, CH, CW, CO + 1)), **kw)
    fs = [alloc, out, bad_out]
    if pool:
        def pool2(ops, t):
            return getattr(ops, fn)(t('x', (CN, CH, CW, CI)), weight(ops, t), t('bias', (CO,)), pool2=True, **kw)

        def pool2_out(ops, t):
            return getattr(ops, fn)(t('x', (CN, CH, CW, CI)), weight(ops, t), t('bias', (CO,)), pool2=True,
                                    out=t('y', (CN, CH // 2, CW // 2, CO)), **kw)

        def pool2_bad_out(ops, t):
            return getattr(ops, fn)(t('x', (CN, CH, CW, CI)), weight(ops, t), t('bias', (CO,)), pool2=True,
                                    out=t('y', (CN, CH, CW, CO)), **kw)
        fs += [pool2, pool2_out, pool2_bad_out]
    for f in fs:
        CASES.append(('%s.%s' % (fn, f.__name__), f))


_conv_cases('conv3x3_nhwc', lambda ops, t: t('w', (CO, 3, 3, CI)), False, dilation=2)
_conv_cases('conv3x3_nhwc_bf16', lambda ops, t: t('w', (CO, 3, 3, CI)), False)
_conv_cases('conv3x3_nhwc_bf16_wp', lambda ops, t: t('w', (9 * CI // 16, CO, 16), BF16), True)
_conv_cases('conv3x3_nhwc_f32x3', lambda ops, t: t('w', (3, 9 * CI // 16, CO, 16), BF16), True)
_conv_cases('conv3x3_nhwc_f16x2', lambda ops, t: f16x2(ops, t, 'w', CO, 9 * CI), True,
            amax_in=None, amax_out=None)


@case
def conv3x3_nhwc_f16x2_amax(ops, t):
    return ops.conv3x3_nhwc_f16x2(t('x', (CN, CH, CW, CI)), f16x2(ops, t, 'w', CO, 9 * CI), t('bias', (CO,)),
                                  amax_in=t('ain', (1,), I32), in_mul=2.0, in_add=0.5,
                                  amax_out=t('aout', (1,), I32), amax_out_zeroed=True, dilation=2)


@case
def conv3x3_nhwc_bf16_wp_bad_weight(ops, t):
    return ops.conv3x3_nhwc_bf16_wp(t('x', (CN, CH, CW, CI)), t('w', (9 * CI // 16, CO, 16), F16), None)


@case
def conv3x3_nhwc_f32x3_bad_weight(ops, t):
    return ops.conv3x3_nhwc_f32x3(t('x', (CN, CH, CW, CI)), t('w', (2, 9 * CI // 16, CO, 16), BF16), None)


def record(ops, dev):
    """-> {case name: {'calls': [...], 'ret': ...} or {'raises': ...}} with `ops`' wrappers."""
    L = ops.L
    real, out = L.call, {}
    try:
        for name, fn in CASES:
            assert name not in out, name
            t, calls = Tensors(dev), []

            def rec(fname, *args):
                calls.append([fname] + [t.locate(a) if isinstance(a, int) and not isinstance(a, bool)
                                        else a for a in args])
                return 0
            L.call = rec
            try:
                e = {'ret': _describe(fn(ops, t))}
            except (TypeError, ValueError, L.NawsError) as ex:
                e = {'raises': type(ex).__name__, 'text': str(ex)}
            e['calls'] = calls
            out[name] = e
    finally:
        L.call = real
    return json.loads(json.dumps(out))          # tuples -> lists, as the fixture holds them


def main():
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'na-fwebsod_amd')]
    from naws_hip import ops
    if '--ops' in sys.argv:      # another version of the module, inside the same package
        spec = importlib.util.spec_from_file_location('naws_hip.ops_recorded',
                                                      sys.argv[sys.argv.index('--ops') + 1])
        ops = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(ops)
    res = record(ops, torch.device('cuda:0'))
    print('%d cases, %d raise' % (len(res), sum('raises' in e for e in res.values())))
    if '--record' in sys.argv:
        out = OUT if '--out' not in sys.argv else sys.argv[sys.argv.index('--out') + 1]
        with open(out, 'w') as f:
            f.write('{\n' + ',\n'.join(' %s: %s' % (json.dumps(k), json.dumps(v, separators=(',', ':')))
                                       for k, v in sorted(res.items())) + '\n}\n')
        print('wrote', out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()
