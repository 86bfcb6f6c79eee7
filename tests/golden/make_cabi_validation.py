#!/usr/bin/env python3
"""The argument-validation cases of the GEMM / conv3x3 entry points that share one front end
(csrc/entry_args.h), and the codes the library returns for them.

Per entry point: one base tuple that satisfies every condition, and a table of violations (each
replaces a few arguments so that exactly one condition fails).  The cases are every single
violation and every pair of violations that do not touch the same argument - pairs are what pin
the ORDER of the checks.  The base tuple itself is never called: it would reach the launch.
Every case returns before any launch or device call (the f16x2 conv's base passes
amax_out_zeroed = 1, so its memset is never reached), which is why this runs without a GPU.

Pointers are symbolic: 'buf' / 'buf2' two 64-float host buffers, 'mis' = buf + 4 bytes, 'null'.

    python tests/golden/make_cabi_validation.py          # prints the table sizes
    NAWS_LIB=<libnaws_hip.so of the commit to record> \\
        python tests/golden/make_cabi_validation.py --record   # writes cabi_validation_before.json

The fixture's "codes" were recorded from the library of the commit BEFORE the shared front end.
"""
import ctypes
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, 'cabi_validation_before.json')

NONE, BIAS, BIAS_RELU, DROP, GATE = range(5)
BIG = 65536

# ---- GEMM family --------------------------------------------------------------------------------
_EPI_TAIL = [('epilogue', NONE), ('bias', 'null'), ('strideBias', 0), ('aux', 'null'), ('ldaux', 0),
             ('alpha', 1.0), ('drop_ratio', 0.0), ('seed', 0), ('accumulate', 0)]
_EPI_BAD = [('epi_hi', {'epilogue': 99}), ('epi_lo', {'epilogue': -1}),
            ('gate_no_aux', {'epilogue': GATE}),
            ('drop_one', {'epilogue': DROP, 'drop_ratio': 1.0}),
            ('drop_neg', {'epilogue': DROP, 'drop_ratio': -0.5})]
_DIMS_BAD = [('M0', {'M': 0}), ('N0', {'N': -1}), ('K0', {'K': 0}), ('batch0', {'batch': 0})]
_AMAX_TAIL = [('rowmax', 'null'), ('seg', 0), ('colmax', 'null'), ('colmul', 'null')]
_SEG_BAD = [('seg_256', {'rowmax': 'buf', 'seg': 16})]
_C_EXTENT = [('batch_big', {'batch': BIG}),
             ('c_extent', {'M': BIG, 'ldc': BIG, 'slabA': BIG * 16}),
             ('aux_extent', {'aux': 'buf', 'ldaux': 1 << 27})]


def _plane_nt(kbad, planes):
    """Violations of the [K/16, rows, 16] operand geometry of the _nt forms."""
    v = [('slabA_small', {'slabA': 256}), ('slabB_small', {'slabB': 256}), ('ldc_small', {'ldc': 16}),
         ('K_mult', {'K': kbad}), ('slabA_mis', {'slabA': 516}), ('slabB_mis', {'slabB': 516})]
    if planes:
        v += [('planeA_mis', {'planeA': 4}), ('planeB_mis', {'planeB': 4})]
    return v + [('strideA_mis', {'strideA': 4}), ('strideB_mis', {'strideB': 4}),
                ('A_mis', {'A': 'mis'}), ('B_mis', {'B': 'mis'})]


_SGD_TAIL = [('lr', 'buf'), ('lr_mult', 1.0), ('wd', 0.0), ('momentum', 0.9), ('nesterov', 0),
             ('gpu_num', 1), ('iter_count', 0)]
_XK_HEAD = [('M', 32), ('N', 32), ('K', 32), ('A', 'buf'), ('slabA', 512), ('planeA', 1024),
            ('scaleA', 'buf'), ('X', 'buf'), ('slabX', 512), ('planeX', 1024), ('xrows', 32),
            ('scaleX', 'null')]
_XK_BAD = [('M0', {'M': 0}), ('N0', {'N': 0}), ('K0', {'K': -32}), ('xrows0', {'xrows': 0}),
           ('xrows_big', {'xrows': 64, 'slabX': 1024}), ('K_mult', {'K': 48}), ('N_mult', {'N': 24}),
           ('A_null', {'A': 'null'}), ('X_null', {'X': 'null'}), ('scaleA_null', {'scaleA': 'null'}),
           ('A_mis', {'A': 'mis'}), ('X_mis', {'X': 'mis'}), ('scaleX_mis', {'scaleX': 'mis'}),
           ('slabA_small', {'slabA': 256}), ('slabX_small', {'slabX': 256})]

GEMM = {
    'naws_gemm_f32x3_nt': (
        [('M', 32), ('N', 32), ('K', 32), ('A', 'buf'), ('slabA', 512), ('planeA', 1024),
         ('B', 'buf'), ('slabB', 512), ('planeB', 1024), ('C', 'buf'), ('ldc', 32), ('batch', 1),
         ('strideA', 0), ('strideB', 0), ('strideC', 0)] + _EPI_TAIL + [('stream', 'null')],
        _DIMS_BAD + [('A_null', {'A': 'null'}), ('B_null', {'B': 'null'}), ('C_null', {'C': 'null'})]
        + _EPI_BAD + _plane_nt(24, True) + _C_EXTENT),
    'naws_gemm_f32_f16x2_nt_amax': (
        [('M', 32), ('N', 32), ('K', 32), ('A', 'buf'), ('slabA', 512), ('planeA', 1024),
         ('scaleA', 'buf'), ('B', 'buf'), ('slabB', 512), ('planeB', 1024), ('scaleB', 'buf'),
         ('C', 'buf'), ('ldc', 32), ('batch', 1), ('strideA', 0), ('strideB', 0), ('strideC', 0),
         ('strideScaleA', 0), ('strideScaleB', 0)] + _EPI_TAIL + _AMAX_TAIL + [('stream', 'null')],
        _DIMS_BAD + [('A_null', {'A': 'null'}), ('B_null', {'B': 'null'}), ('C_null', {'C': 'null'}),
                     ('scaleA_null', {'scaleA': 'null'}), ('scaleB_null', {'scaleB': 'null'})]
        + _EPI_BAD + _plane_nt(16, True) + _C_EXTENT + _SEG_BAD),
    'naws_gemm_f32_f16x2_nt_cols': (
        [('M', 32), ('N', 32), ('K', 32), ('A', 'buf'), ('slabA', 512), ('planeA', 1024),
         ('scaleA', 'buf'), ('B', 'buf'), ('slabB', 512), ('planeB', 1024), ('scaleB', 'buf'),
         ('C', 'buf'), ('ldc', 64), ('epilogue', NONE), ('bias', 'null'), ('drop_ratio', 0.0),
         ('seed', 0), ('rowmax', 'null'), ('seg', 0), ('colmax', 'null'), ('drop_ld', 64),
         ('drop_col0', 0), ('stream', 'null')],
        [('M0', {'M': 0}), ('drop_ld0', {'drop_ld': 0}), ('drop_ld_neg', {'drop_ld': -64}),
         ('col0_neg', {'drop_col0': -16}), ('col0_past', {'drop_col0': 48}),
         ('A_null', {'A': 'null'}), ('scaleB_null', {'scaleB': 'null'}), ('epi_hi', {'epilogue': 99}),
         ('drop_one', {'epilogue': DROP, 'drop_ratio': 1.0}), ('slabB_small', {'slabB': 256}),
         ('ldc_small', {'ldc': 16}), ('K_mult', {'K': 16}), ('planeA_mis', {'planeA': 4}),
         ('B_mis', {'B': 'mis'}), ('c_extent', {'M': BIG, 'ldc': BIG, 'slabA': BIG * 16})]
        + _SEG_BAD),
    'naws_gemm_bf16_slab_nt': (
        [('M', 32), ('N', 32), ('K', 64), ('A', 'buf'), ('slabA', 512), ('B', 'buf'), ('slabB', 512),
         ('C', 'buf'), ('ldc', 32), ('batch', 1), ('strideA', 0), ('strideB', 0), ('strideC', 0)]
        + _EPI_TAIL + [('stream', 'null')],
        _DIMS_BAD + [('A_null', {'A': 'null'}), ('B_null', {'B': 'null'}), ('C_null', {'C': 'null'})]
        + _EPI_BAD + _plane_nt(32, False) + _C_EXTENT),
    'naws_gemm_bf16_slab_nt_sgd': (
        [('M', 32), ('N', 32), ('K', 64), ('A', 'buf'), ('slabA', 512), ('B', 'buf'), ('slabB', 512),
         ('mom', 'buf'), ('param', 'buf'), ('ldp', 32)] + _SGD_TAIL
        + [('P', 'buf'), ('prows', 32), ('stream', 'null')],
        [('M0', {'M': 0}), ('N0', {'N': 0}), ('K0', {'K': 0}), ('gpu0', {'gpu_num': 0}),
         ('prows_small', {'prows': 16}), ('ldp_small', {'ldp': 16}),
         ('A_null', {'A': 'null'}), ('B_null', {'B': 'null'}), ('mom_null', {'mom': 'null'}),
         ('param_null', {'param': 'null'}), ('lr_null', {'lr': 'null'}), ('P_null', {'P': 'null'}),
         ('slabA_small', {'slabA': 256}), ('slabB_small', {'slabB': 256}), ('K_mult', {'K': 32}),
         ('N_mult', {'N': 24}), ('ldp_mis', {'ldp': 34}), ('slabA_mis', {'slabA': 516}),
         ('slabB_mis', {'slabB': 516}), ('A_mis', {'A': 'mis'}), ('B_mis', {'B': 'mis'}),
         ('mom_mis', {'mom': 'mis'}), ('param_mis', {'param': 'mis'}), ('P_mis', {'P': 'mis'}),
         ('iter_neg', {'iter_count': -1})]),
    'naws_gemm_f32_amax': (
        [('transA', 0), ('transB', 1), ('M', 32), ('N', 32), ('K', 32), ('A', 'buf'), ('lda', 32),
         ('B', 'buf'), ('ldb', 32), ('C', 'buf'), ('ldc', 32), ('batch', 1), ('strideA', 0),
         ('strideB', 0), ('strideC', 0)] + _EPI_TAIL + _AMAX_TAIL + [('stream', 'null')],
        _DIMS_BAD + [('A_null', {'A': 'null'}), ('B_null', {'B': 'null'}), ('C_null', {'C': 'null'})]
        + _EPI_BAD
        + [('lda_small', {'lda': 16}), ('ldb_small', {'ldb': 16}), ('ldc_small', {'ldc': 16}),
           ('transA_lda', {'transA': 1, 'M': 64}), ('lda_mis', {'lda': 34}), ('ldb_mis', {'ldb': 34}),
           ('strideA_mis', {'strideA': 2}), ('strideB_mis', {'strideB': 2}), ('A_mis', {'A': 'mis'}),
           ('B_mis', {'B': 'mis'}), ('K_mis', {'K': 30}), ('N_mis_nn', {'transB': 0, 'N': 30}),
           ('batch_big', {'batch': BIG}),
           ('a_extent', {'M': 1 << 20, 'K': 1024, 'lda': 1024, 'ldb': 1024})] + _SEG_BAD),
    'naws_gemm_f32_splitk': (
        [('transA', 0), ('transB', 1), ('M', 32), ('N', 32), ('K', 32), ('A', 'buf'), ('lda', 32),
         ('B', 'buf'), ('ldb', 32), ('C', 'buf'), ('ldc', 32), ('batch', 1), ('strideA', 0),
         ('strideB', 0), ('strideC', 0), ('epilogue', NONE), ('bias', 'null'), ('strideBias', 0),
         ('ksplit', 2), ('workspace', 'buf'), ('stream', 'null')],
        _DIMS_BAD + [('ksplit0', {'ksplit': 0}), ('A_null', {'A': 'null'}), ('B_null', {'B': 'null'}),
                     ('C_null', {'C': 'null'}), ('ws_null', {'workspace': 'null'}),
                     ('epi_relu', {'epilogue': BIAS_RELU, 'bias': 'buf'}),
                     ('bias_null', {'epilogue': BIAS}), ('lda_mis', {'lda': 34}),
                     ('ldb_mis', {'ldb': 34}), ('strideA_mis', {'strideA': 2}),
                     ('strideB_mis', {'strideB': 2}), ('A_mis', {'A': 'mis'}), ('B_mis', {'B': 'mis'}),
                     ('lda_small', {'lda': 16}), ('ldb_small', {'ldb': 16}), ('ldc_small', {'ldc': 16}),
                     ('a_extent', {'M': 1 << 20, 'K': 1024, 'lda': 1024, 'ldb': 1024}),
                     ('slices_big', {'batch': BIG})]),
    'naws_gemm_bf16_nt': (
        [('M', 32), ('N', 32), ('K', 32), ('A', 'buf'), ('a_is_bf16', 0), ('lda', 32), ('B', 'buf'),
         ('b_is_bf16', 1), ('ldb', 32), ('C', 'buf'), ('ldc', 32), ('batch', 1), ('strideA', 0),
         ('strideB', 0), ('strideC', 0)] + _EPI_TAIL + [('stream', 'null')],
        _DIMS_BAD + [('A_null', {'A': 'null'}), ('B_null', {'B': 'null'}), ('C_null', {'C': 'null'})]
        + _EPI_BAD
        + [('lda_small', {'lda': 16}), ('ldb_small', {'ldb': 16}), ('ldc_small', {'ldc': 16}),
           ('K_mis', {'K': 28}), ('lda_mis', {'lda': 36}), ('ldb_mis', {'ldb': 36}),
           ('strideA_mis', {'strideA': 4}), ('strideB_mis', {'strideB': 4}), ('A_mis', {'A': 'mis'}),
           ('B_mis', {'B': 'mis'}), ('batch_big', {'batch': BIG}),
           ('a_extent', {'M': 1 << 21, 'K': 1024, 'lda': 1024, 'ldb': 1024})]),
    'naws_gemm_f32_f16x2_nt_xk': (
        _XK_HEAD + [('C', 'buf'), ('ldc', 32), ('stream', 'null')],
        _XK_BAD + [('ldc_small', {'ldc': 16}), ('ldc_mis', {'ldc': 34}), ('C_null', {'C': 'null'}),
                   ('C_mis', {'C': 'mis'})]),
    'naws_gemm_f32_f16x2_nt_xk_sgd': (
        _XK_HEAD + [('param', 'buf'), ('mom', 'buf'), ('ldp', 32)] + _SGD_TAIL
        + [('planes', 'buf'), ('plane_stride', 1024), ('plane_rows', 32), ('bound', 'buf'),
           ('rowmax', 'buf2'), ('inv_scale', 'buf'), ('overflow', 'buf'), ('overflow_tag', 1),
           ('stream', 'null')],
        _XK_BAD + [('gpu0', {'gpu_num': 0}), ('iter_neg', {'iter_count': -1}),
                   ('plane_rows0', {'plane_rows': 0}), ('ldp_small', {'ldp': 16}),
                   ('ldp_mis', {'ldp': 34}), ('param_null', {'param': 'null'}),
                   ('mom_null', {'mom': 'null'}), ('lr_null', {'lr': 'null'}),
                   ('planes_null', {'planes': 'null'}), ('bound_null', {'bound': 'null'}),
                   ('rowmax_null', {'rowmax': 'null'}), ('inv_null', {'inv_scale': 'null'}),
                   ('overflow_null', {'overflow': 'null'}), ('param_mis', {'param': 'mis'}),
                   ('mom_mis', {'mom': 'mis'}), ('planes_mis', {'planes': 'mis'}),
                   ('bound_is_rowmax', {'rowmax': 'buf'}), ('plane_rows_small', {'plane_rows': 16})]),
}

# ---- conv3x3 family -----------------------------------------------------------------------------
_CONV_BAD = [('N0', {'N': 0}), ('H0', {'H': 0}), ('W0', {'W': -8}), ('Cin0', {'Cin': 0}),
             ('Cout0', {'Cout': 0}), ('Cin_mult', {'Cin': 24}), ('X_null', {'X': 'null'}),
             ('W_null', {'Wt': 'null'}), ('Y_null', {'Y': 'null'}), ('relu_no_bias', {'bias': 'null'}),
             ('X_mis', {'X': 'mis'}), ('W_mis', {'Wt': 'mis'}), ('pix_big', {'N': BIG, 'H': BIG}),
             ('bytes_big', {'H': 32768, 'W': 2048})]

CONV = {
    'naws_conv3x3_nhwc_f32x3_fwd': (
        [('X', 'buf'), ('Wt', 'buf'), ('bias', 'buf'), ('N', 1), ('H', 8), ('W', 8), ('Cin', 16),
         ('Cout', 64), ('dilation', 1), ('relu', 1), ('Y', 'buf'), ('stream', 'null')],
        _CONV_BAD + [('dil0', {'dilation': 0}), ('Cout_mult', {'Cout': 66})]),
    'naws_conv3x3_nhwc_f32x3_pool_fwd': (
        [('X', 'buf'), ('Wt', 'buf'), ('bias', 'buf'), ('N', 1), ('H', 8), ('W', 8), ('Cin', 16),
         ('Cout', 64), ('relu', 1), ('Y', 'buf'), ('stream', 'null')],
        _CONV_BAD + [('H1', {'H': 1}), ('W1', {'W': 1}), ('Cout_mult', {'Cout': 96}),
                     ('Cout_big', {'Cout': 320}), ('plane_big', {'Cin': 160000, 'Cout': 256})]),
    'naws_conv3x3_nhwc_bf16_wp_fwd': (
        [('X', 'buf'), ('Wt', 'buf'), ('bias', 'buf'), ('N', 1), ('H', 8), ('W', 8), ('Cin', 64),
         ('Cout', 64), ('dilation', 1), ('relu', 1), ('pool2', 0), ('Y', 'buf'), ('stream', 'null')],
        _CONV_BAD + [('dil3', {'dilation': 3}), ('dil2_pool', {'dilation': 2, 'pool2': 1}),
                     ('pool_H1', {'pool2': 1, 'H': 1}), ('Cin_k64', {'Cin': 16}),
                     ('Cout_mult', {'Cout': 96}), ('plane_big', {'Cin': BIG, 'Cout': 4096})]),
    'naws_conv3x3_nhwc_f16x2_fwd': (
        [('X', 'buf'), ('Wt', 'buf'), ('scaleW', 'buf'), ('bias', 'buf'), ('N', 1), ('H', 8), ('W', 8),
         ('Cin', 32), ('Cout', 64), ('dilation', 1), ('relu', 1), ('Y', 'buf'), ('amax_in', 'buf'),
         ('in_mul', 1.0), ('in_add', 0.0), ('amax_out', 'buf2'), ('amax_out_zeroed', 1), ('pool2', 0),
         ('stream', 'null')],
        _CONV_BAD + [('dil3', {'dilation': 3}), ('dil2_pool', {'dilation': 2, 'pool2': 1}),
                     ('pool_W1', {'pool2': 1, 'W': 1}), ('Cin_k32', {'Cin': 16}),
                     ('Cout_mult', {'Cout': 48}), ('Cout_wide', {'Cout': 192}),
                     ('scaleW_null', {'scaleW': 'null'}), ('amax_in_null', {'amax_in': 'null'}),
                     ('in_mul0', {'in_mul': 0.0}), ('in_add_neg', {'in_add': -1.0}),
                     ('amax_in_is_out', {'amax_out': 'buf'}),
                     ('plane_big', {'Cin': BIG, 'Cout': 1024})]),
}

FAMILIES = {'gemm': GEMM, 'conv': CONV}


def cases(base, violations):
    """-> [(label, argument list)]: singles, then the pairs that touch disjoint arguments."""
    names = [n for n, _ in base]
    out = []

    def build(mods):
        vals = dict(base)
        for m in mods:
            assert set(m) <= set(names), m
            vals.update(m)
        return [vals[n] for n in names]

    for i, (la, ma) in enumerate(violations):
        out.append((la, build([ma])))
    for i, (la, ma) in enumerate(violations):
        for lb, mb in violations[i + 1:]:
            if not set(ma) & set(mb):
                out.append((la + '+' + lb, build([ma, mb])))
    return out


def table():
    return {fam: {fn: cases(base, viol) for fn, (base, viol) in fns.items()}
            for fam, fns in FAMILIES.items()}


def digest(case_list):
    """Ties a fixture entry to the exact case list it was recorded for."""
    return hashlib.sha1(json.dumps(case_list, sort_keys=True).encode()).hexdigest()


class Pointers(object):
    """The symbolic pointers of a case as addresses (kept alive by this object)."""

    def __init__(self):
        self.a = (ctypes.c_float * 68)()          # 'mis' + 64 floats stays inside
        self.b = (ctypes.c_float * 64)()
        base = ctypes.addressof(self.a)
        base += (-base) % 16
        self.map = {'buf': base, 'buf2': ctypes.addressof(self.b), 'mis': base + 4, 'null': None}

    def resolve(self, args):
        return [self.map[v] if isinstance(v, str) else v for v in args]


def main():
    tab = table()
    n = sum(len(c) for fns in tab.values() for c in fns.values())
    print('%d entry points, %d cases' % (sum(len(f) for f in tab.values()), n))
    if '--record' not in sys.argv:
        return
    sys.path.insert(0, os.path.join(ROOT, 'na-fwebsod_amd'))
    from naws_hip import lib
    L = lib.load()
    ptrs = Pointers()
    out = {}
    for fam, fns in tab.items():
        out[fam] = {}
        for fn, case_list in fns.items():
            codes = [getattr(L, fn)(*ptrs.resolve(args)) for _, args in case_list]
            bad = [l for (l, _), c in zip(case_list, codes) if not -5 <= c <= -1 or c == lib.ERR_LAUNCH]
            assert not bad, (fn, bad)
            # one digit per case, in case order: the negated code (1 SHAPE, 2 ARG, 3 NULL, 5 UNSUPPORTED)
            out[fam][fn] = {'n': len(codes), 'cases_sha1': digest(case_list),
                            'codes': ''.join(str(-c) for c in codes)}
    with open(OUT, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
