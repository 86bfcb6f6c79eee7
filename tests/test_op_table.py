"""The operator table of the op-by-op plan (detectron/core/op_table.py) without a GPU: the gradient
generator that reads it records exactly the ops the two lists in detector.py recorded (digests of
the parent commit, tests/golden/op_signatures_before.json), the table agrees with itself and with
every shipped build, the executor gathers inputs strictly, and the three NotImplementedError
messages keep their texts."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
try:
    import make_golden_op_signatures as sig
finally:
    sys.path.pop(0)
BEFORE = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'op_signatures_before.json')))
REFUSED = ['deeplab/train/trainable', 'wsddn_context/train/trainable',
           'wsddn_context_oicr/train/trainable']


def test_every_build_records_the_ops_it_recorded_before(cfgmod):
    """11 builds x train / test x frozen / trainable body: forward and backward op lists digest to
    the parent commit's values, and the three builds it refused are refused with the same type."""
    now = sig.record()
    assert sorted(now) == sorted(BEFORE) and len(BEFORE) == 44
    assert sorted(k for k, v in BEFORE.items() if 'refused' in v) == REFUSED
    assert all(BEFORE[k] == {'refused': 'NotImplementedError'} for k in REFUSED)
    diff = [k for k in BEFORE if now[k] != BEFORE[k]]
    assert not diff, diff


def test_every_emitted_op_has_its_entry(cfgmod):
    """Every forward op type the builds emit has an entry with a forward rule and no more inputs
    than the entry allows; every gradient op type has a gradient rule; grad_fwd_idx names, for each
    gradient op, the forward op it came from."""
    from detectron.core.op_table import TABLE
    seen_f, seen_g = set(), set()
    for key in sorted(BEFORE):
        if key in REFUSED:
            continue
        name, mode, body = key.split('/')
        m = sig.create(name, mode == 'train', body == 'frozen')
        for o in m.net.ops:
            e = TABLE.get(o.type)
            assert e is not None and e.forward is not None, (key, o.type)
            assert e.n_in is None or len(o.inputs) <= e.n_in, (key, o.type, o.inputs)
            seen_f.add(o.type)
        assert len(m.grad_fwd_idx) == len(m.grad_ops) and (mode == 'train') == bool(m.grad_ops)
        for g, idx in zip(m.grad_ops, m.grad_fwd_idx):
            f = m.net.ops[idx]
            assert g.type == f.type + 'Gradient' and g.inputs == f.inputs + f.outputs
            assert TABLE[f.type].gradient is not None, (key, g.type)
            assert sorted(g.args) == sorted(list(f.args) + ['_gout', '_gin', '_accumulate'])
            seen_g.add(f.type)
    assert {'CenterLoss', 'RoIAlign', 'RoIContext', 'RoILabel', 'MinEntropyLoss', 'Conv'} <= seen_f
    assert {'CenterLoss', 'RoIAlign', 'RoIPoolF', 'Conv', 'MaxPool', 'SoftmaxWithLossN'} <= seen_g


def test_the_table_agrees_with_itself():
    """Over the whole table: gradient input indices if and only if a gradient rule; a flow-cutting
    entry has neither; every index is a possible input position; state only where there is a
    forward rule.  The sets are the ones detector.py listed."""
    from detectron.core import op_table as T
    for t, e in T.TABLE.items():
        assert (e.grad_inputs is None) == (e.gradient is None), t
        if e.cuts:
            assert e.grad_inputs is None and e.gradient is None, t
        if e.grad_inputs is not None:
            assert e.grad_inputs and all(0 <= i and (e.n_in is None or i < e.n_in)
                                         for i in e.grad_inputs), t
        assert e.state is None or e.forward is not None, t
        assert T.cuts_flow(t) == e.cuts and T.grad_inputs(t) == e.grad_inputs
    assert not T.cuts_flow('NoSuchOp') and T.grad_inputs('NoSuchOp') is None
    assert {t for t, e in T.TABLE.items() if e.cuts} == {
        'StopGradient', 'RoIIoU', 'Stat', 'Accuracy', 'ConstantFill', 'Shape', 'Cast',
        'DequeueBlobs', 'RoILabel', 'RoIEntropy', 'BoxWithNMSLimit', 'RoIContext'}
    assert {t: e.grad_inputs for t, e in T.TABLE.items() if e.grad_inputs is not None} == {
        'FC': (0, 1, 2), 'Relu': (0,), 'Dropout': (0,), 'Softmax': (0,), 'Transpose': (0,),
        'Mul': (0, 1), 'Add': (0, 1), 'Sub': (0, 1), 'ReduceSum': (0,), 'AveragedLoss': (0,),
        'WeightedCrossEntropyWithLogits': (0,), 'CrossEntropyWithLogits': (0,),
        'RoIFeatureBoost': (0,), 'MinEntropyLoss': (0,), 'SoftmaxWithLossN': (0,),
        'CenterLoss': (2,), 'Conv': (0, 1, 2), 'MaxPool': (0,), 'RoIPoolF': (0,), 'RoIAlign': (0,)}
    assert {t for t, e in T.TABLE.items() if e.state is not None} == {
        'Stat', 'RoILabel', 'RoIEntropy', 'CenterLoss'}
    assert T.TABLE['DequeueBlobs'].forward is None


def _helper(train=False):
    from detectron.modeling.detector import DetectionModelHelper
    return DetectionModelHelper(name='hand', train=train, num_classes=21)


def _executor(model):
    from detectron.core.executor import NetExecutor
    ex = NetExecutor(model, torch.device('cpu'), force_interpreted=True)     # launches nothing
    assert ex.plan == 'interpreted'
    return ex


def test_a_missing_input_blob_is_an_error_not_a_shift(cfgmod, monkeypatch):
    """Relu on a fed blob, then Mul of its output with a blob nobody feeds: run() reaches the Relu
    entry (stubbed through the table, so no kernel is needed) and then raises KeyError naming the
    operator, its output and the missing blob, before any call into detectron.ops.  On the parent
    commit the same net dropped the missing name and reached O.Mul with too few arguments (an
    IndexError on x[1]; with a third input it would have multiplied the wrong pair)."""
    from detectron.core.op_table import TABLE
    reached = []

    def relu(ex, idx, op, x):
        reached.append((idx, op.type, [tuple(v.shape) for v in x]))
        return (x[0].clamp(min=0),)

    def mul(ex, idx, op, x):
        raise AssertionError('the Mul rule ran')
    monkeypatch.setitem(TABLE, 'Relu', TABLE['Relu']._replace(forward=relu))
    monkeypatch.setitem(TABLE, 'Mul', TABLE['Mul']._replace(forward=mul))
    m = _helper()
    m.net.Relu(['fed'], ['act'])
    m.net.Mul(['act', 'never_fed'], ['prod'])
    ex = _executor(m)
    ex.feed({'fed': torch.tensor([[-1.0, 2.0]])})
    with pytest.raises(KeyError) as e:
        ex.run()
    assert reached == [(0, 'Relu', [(1, 2)])]
    assert ex.fetch('act').tolist() == [[0.0, 2.0]] and 'prod' not in ex.ws
    for word in ('Mul', 'prod', 'never_fed'):
        assert word in str(e.value), str(e.value)


def test_not_implemented_messages_keep_their_texts(cfgmod):
    """An unknown forward type, a type without a gradient rule whose output needs a gradient, and
    a gradient op type without a rule."""
    from detectron.modeling.detector import Op
    m = _helper()
    m.net.NoSuchOp(['fed'], ['out'])
    ex = _executor(m)
    ex.feed({'fed': torch.zeros((1,))})
    with pytest.raises(NotImplementedError) as e:
        ex.run()
    assert str(e.value) == 'operator NoSuchOp is not on the MI355X hot path'
    with pytest.raises(NotImplementedError) as e:        # known to the generator only
        ex._forward(0, Op('DequeueBlobs', [], ['data'], {}), ex.ws)
    assert str(e.value) == 'operator DequeueBlobs is not on the MI355X hot path'

    t = _helper(train=True)
    t.net.Log(['fed'], ['lg'])
    with pytest.raises(NotImplementedError) as e:
        t.AddGradientOperators({'lg': 'lg_grad'})
    assert str(e.value) == 'no gradient for op Log (blob lg needs one)'
    t.net.ops[0] = Op('NoSuchOp', ['fed'], ['lg'], {})    # a type the table does not know at all
    with pytest.raises(NotImplementedError) as e:
        t.AddGradientOperators({'lg': 'lg_grad'})
    assert str(e.value) == 'no gradient for op NoSuchOp (blob lg needs one)'

    g = Op('LogGradient', ['fed', 'lg'], ['fed_grad'],
           dict(_gout=['lg_grad'], _gin=['fed_grad'], _accumulate=[False]))
    with pytest.raises(NotImplementedError) as e:
        ex._backward(g, {})
    assert str(e.value) == 'gradient of Log'
