"""The operators of the op-by-op plan, each declared once: TABLE maps an operator type to

  forward      (executor, idx, op, x) -> the values of op.outputs, in order; x holds the values of
               op.inputs.  None: the type is known to the gradient generator only (DequeueBlobs).
  n_in         the most inputs the operator takes (None: any number)
  cuts         the gradient flow stops here: nothing upstream of the op gets a gradient through it
  grad_inputs  indices of the inputs that receive a gradient (the others are constants); None: the
               operator has no gradient rule and the generator raises when one is needed
  gradient     (executor, idx, op, x, y, gout) -> one gradient per input, in order (None, or a
               shorter list, where an input gets none); x / y hold the values of the forward op's
               inputs / outputs, gout the gradients of its outputs, idx is the forward op's index
  state        op -> the object the executor keeps per op instance, in NetExecutor._state[idx]

DetectionModelHelper.AddGradientOperators reads cuts / grad_inputs, NetExecutor runs forward /
gradient / state.  Adding an operator is adding one entry here.  An argument the op does not carry
falls to the keyword default of detectron.ops (_kw), except where the plan's default is its own.
"""
import collections

import torch

import detectron.ops as O

Entry = collections.namedtuple('Entry', 'forward n_in cuts grad_inputs gradient state')


def _op(forward, n_in, grad_inputs=None, gradient=None, cuts=False, state=None):
    return Entry(forward, n_in, cuts, grad_inputs, gradient, state)


def _kw(op, *names):
    return {k: op.args[k] for k in names if k in op.args}


def _dx_first(dW, db, dX):
    return [dX, dW, db]


def _need_dx(op):       # the generator drops dX behind StopGradient: a GEMM nobody reads
    return op.args['_gin'][0] is not None


def _pool(op):
    return dict(kernel=op.args['kernel'], pad=op.args['pad'], stride=op.args['stride'])


def _roi(op):
    return op.args['pooled_h'], op.args['pooled_w'], op.args['spatial_scale']


def _binary(name, grad_inputs=None, gradient=None):
    return _op(lambda ex, i, op, x: (getattr(O, name)(x[0], x[1]),), 2, grad_inputs, gradient)


_CONV = ('kernel', 'pad', 'stride', 'dilation')


def _conv(op):
    """A Conv op without a pad argument has none (the operator's default, which the 1x1 shortcuts
    of the ResNet builders rely on), not O.Conv's keyword default of 1."""
    return dict({'pad': 0}, **_kw(op, *_CONV))

TABLE = {
    # ------------------------------------------------------------------ conv body
    # inputs X, W[, b]: a Conv the builders make with no_bias carries two
    'Conv': _op(lambda ex, i, op, x: (O.Conv(x[0], x[1], x[2] if len(x) > 2 else None,
                                             **_conv(op)),), 3, (0, 1, 2),
                lambda ex, i, op, x, y, g: _dx_first(*O.ConvGradient(
                    x[0], x[1], g[0], need_dx=_need_dx(op), **_conv(op)))),
    'Relu': _op(lambda ex, i, op, x: (O.Relu(x[0]),), 1, (0,),
                lambda ex, i, op, x, y, g: [O.ReluGradient(y[0], g[0])]),
    'MaxPool': _op(lambda ex, i, op, x: (O.MaxPool(x[0], **_pool(op)),), 1, (0,),
                   lambda ex, i, op, x, y, g: [O.MaxPoolGradient(x[0], y[0], g[0], **_pool(op))]),
    # the ResNet bodies (forward only: they run frozen).  inputs X, s, b; in place when the builder
    # names the input as the output
    'AffineChannel': _op(lambda ex, i, op, x: (O.AffineChannel(
        x[0], x[1], x[2], out=x[0] if op.outputs[0] == op.inputs[0] else None),), 3),
    'Sum': _op(lambda ex, i, op, x: (O.Sum(x[0], x[1]),), 2),
    'StopGradient': _op(lambda ex, i, op, x: (x[0],), 1, cuts=True),
    'DequeueBlobs': _op(None, 0, cuts=True),     # the loader's op: named by a builder, never run
    # -------------------------------------------------------------------- RoI ops
    # the two poolings: features only; RoIPoolF's gradient takes the forward's own argmax,
    # RoIAlign's rebuilds the geometry from the rois
    'RoIPoolF': _op(lambda ex, i, op, x: O.RoIPoolF(x[0], x[1], *_roi(op)), 2, (0,),
                    lambda ex, i, op, x, y, g: [O.RoIPoolFGradient(x[0], x[1], y[1], g[0])]),
    'RoIAlign': _op(lambda ex, i, op, x: (O.RoIAlign(x[0], x[1], *_roi(op),
                                                     op.args.get('sampling_ratio', 0)),), 2, (0,),
                    lambda ex, i, op, x, y, g: [O.RoIAlignGradient(
                        x[0], x[1], g[0], *_roi(op), op.args.get('sampling_ratio', 0))]),
    # inputs (rois, data): the clamp bounds are the dims of the image blob, whatever is wired in
    'RoIContext': _op(lambda ex, i, op, x: O.RoIContext(x[0], ex.ws['data'],
                                                        **_kw(op, 'context_ratio')), 2, cuts=True),
    'RoILoopPool': _op(lambda ex, i, op, x: O.RoILoopPool(x[0], x[1], *_roi(op)), 2),
    'RoIFeatureBoost': _op(lambda ex, i, op, x: (O.RoIFeatureBoost(x[0], x[1]),), 2, (0,),
                           lambda ex, i, op, x, y, g: [O.RoIFeatureBoostGradient(g[0], x[1])]),
    'RoIIoU': _op(lambda ex, i, op, x: (O.RoIIoU(x[0]),), 1, cuts=True),
    # ----------------------------------------------------------------------- head
    'FC': _op(lambda ex, i, op, x: (O.FC(x[0], x[1], x[2]),), 3, (0, 1, 2),
              lambda ex, i, op, x, y, g: _dx_first(*O.FCGradient(
                  x[0], x[1], g[0].contiguous(), need_dx=_need_dx(op)))),
    'Dropout': _op(lambda ex, i, op, x: O.Dropout(
                       x[0], is_test=op.args.get('is_test', False) or ex.disable_dropout,
                       seed=ex.dropout_seed(i), **_kw(op, 'ratio')), 1, (0,),
                   lambda ex, i, op, x, y, g: [g[0] if y[1] is None else
                                               O.DropoutGradient(g[0], y[1], **_kw(op, 'ratio'))]),
    'Softmax': _op(lambda ex, i, op, x: (O.Softmax(x[0], **_kw(op, 'axis')),), 1, (0,),
                   lambda ex, i, op, x, y, g: [O.SoftmaxGradient(y[0], g[0])]),
    'Transpose': _op(lambda ex, i, op, x: (O.Transpose(x[0], **_kw(op, 'axes')),), 1, (0,),
                     lambda ex, i, op, x, y, g: [O.Transpose(g[0])]),
    # ---------------------------------------------------------------- arithmetic
    'Add': _binary('Add', (0, 1), lambda ex, i, op, x, y, g: [g[0], g[0]]),
    'Sub': _binary('Sub', (0, 1), lambda ex, i, op, x, y, g: [g[0], O.Scale(g[0], scale=-1.0)]),
    'Mul': _binary('Mul', (0, 1),
                   lambda ex, i, op, x, y, g: [O.Mul(g[0], x[1]), O.Mul(g[0], x[0])]),
    'Div': _binary('Div'),
    'Max': _binary('Max'),
    'MatMul': _binary('MatMul'),
    'ReduceSum': _op(lambda ex, i, op, x: (O.ReduceSum(x[0], **_kw(op, 'axes', 'keepdims')),), 1,
                     (0,),      # broadcast the [1,C] gradient down the rows
                     lambda ex, i, op, x, y, g: [O.Mul(O.ConstantFill(like=x[0], value=1.0),
                                                       g[0])]),
    'Log': _op(lambda ex, i, op, x: (O.Log(x[0]),), 1),
    'Scale': _op(lambda ex, i, op, x: (O.Scale(x[0], **_kw(op, 'scale')),), 1),
    'ReplaceNaN': _op(lambda ex, i, op, x: (O.ReplaceNaN(x[0], **_kw(op, 'value')),), 1),
    'LeakyRelu': _op(lambda ex, i, op, x: (O.LeakyRelu(x[0], **_kw(op, 'alpha')),), 1),
    # the plan's own bounds, not O.Clip's (the float32 extremes)
    'Clip': _op(lambda ex, i, op, x: (O.Clip(x[0], min=op.args.get('min', -3.4e38),
                                             max=op.args.get('max', 3.4e38)),), 1),
    'Mean': _op(lambda ex, i, op, x: (O.Mean(*x),), None),
    'Tile': _op(lambda ex, i, op, x: (O.Tile(x[0], **_kw(op, 'tiles', 'axis')),), 1),
    'Split': _op(lambda ex, i, op, x: torch.split(x[0], op.args['split'],
                                                  dim=op.args.get('axis', 1)), 1),
    'Concat': _op(lambda ex, i, op, x: (torch.cat(x, dim=op.args.get('axis', 1)).contiguous(),),
                  None),
    'ConstantFill': _op(lambda ex, i, op, x: (O.ConstantFill(
        like=x[0] if x else None, shape=op.args.get('shape'), device=ex.device,
        **_kw(op, 'value')),), 1, cuts=True),
    # on the host: a list of ints, then a tensor of them
    'Shape': _op(lambda ex, i, op, x: ([x[0].shape[d] for d in
                                        op.args.get('axes', range(x[0].dim()))],), 1, cuts=True),
    'Cast': _op(lambda ex, i, op, x: (torch.tensor([float(v) for v in x[0]], device=ex.device),),
                1, cuts=True),
    # --------------------------------------------------------- losses and metrics
    'WeightedCrossEntropyWithLogits': _op(
        lambda ex, i, op, x: (O.WeightedCrossEntropyWithLogits(x[0], x[1], x[2],
                                                               **_kw(op, 'is_mean')),), 3, (0,),
        lambda ex, i, op, x, y, g: [O.WeightedCrossEntropyWithLogitsGradient(
            x[0], x[1], x[2], g[0], **_kw(op, 'is_mean'))]),
    'CrossEntropyWithLogits': _op(
        lambda ex, i, op, x: (O.CrossEntropyWithLogits(x[0], x[1], **_kw(op, 'is_mean')),), 2, (0,),
        lambda ex, i, op, x, y, g: [O.CrossEntropyWithLogitsGradient(x[0], x[1], g[0],
                                                                     **_kw(op, 'is_mean'))]),
    'AveragedLoss': _op(lambda ex, i, op, x: (O.AveragedLoss(x[0]),), 1, (0,),
                        lambda ex, i, op, x, y, g: [O.Scale(g[0].reshape(1),
                                                            1.0 / max(x[0].numel(), 1))]),
    'MinEntropyLoss': _op(lambda ex, i, op, x: (O.MinEntropyLoss(x[0], x[1]),), 2, (0,),
                          lambda ex, i, op, x, y, g: [O.MinEntropyLossGradient(x[0], x[1], g[0])]),
    # inputs X, T[, W]; outputs P, loss; the seed is d(loss)
    'SoftmaxWithLossN': _op(
        lambda ex, i, op, x: O.SoftmaxWithLossN(x[0], x[1], x[2] if len(x) > 2 else None,
                                                **_kw(op, 'scale')), 3, (0,),
        lambda ex, i, op, x, y, g: [O.SoftmaxWithLossNGradient(
            x[0], x[1], x[2] if len(x) > 2 else None, y[0], g[1], **_kw(op, 'scale'))]),
    # inputs X, P, F, CF, dCF, ndCF; outputs L, D, S, picks.  The features only
    # (center_loss_op.cc:55-58): the centres update themselves.  The selection reaches the
    # gradient half through the object's workspace, which both halves share: the `_center_picks`
    # blob is a view of it, kept in the net for fetching, not read here.
    'CenterLoss': _op(
        lambda ex, i, op, x: ex._state[i].forward(*x[:6]), 6, (2,),
        lambda ex, i, op, x, y, g: [None, None, ex._state[i].gradient(
            y[1], y[2], g[0], x[2].shape[0], x[3], x[4], x[5])],
        state=lambda op: O.CenterLoss(**_kw(op, 'top_k', 'update', 'lr', 'display', 'max_iter',
                                            'ignore_label'))),
    'Accuracy': _op(lambda ex, i, op, x: (O.Accuracy(x[0], x[1]),), 2, cuts=True),
    'Stat': _op(lambda ex, i, op, x: ex._state[i](x[0].reshape(-1), x[1].reshape(-1),
                                                  gpu_id=ex.rank), 2, cuts=True,
                state=lambda op: O.Stat(**_kw(op, 'display', 'prefix'))),
    'RoILabel': _op(lambda ex, i, op, x: ex._state[i](*x), 4, cuts=True,
                    state=lambda op: O.RoILabel(**_kw(op, 'display', 'uuid', 'fg_thresh',
                                                      'bg_thresh_hi', 'bg_thresh_lo', 'num_pos',
                                                      'num_neg', 'top_k'))),
    'RoIEntropy': _op(lambda ex, i, op, x: (ex._state[i](x[0], x[1]),), 2, cuts=True,
                      state=lambda op: O.RoIEntropy(**_kw(op, 'display', 'num_classes', 'rm_bg'))),
    'BoxWithNMSLimit': _op(lambda ex, i, op, x: O.BoxWithNMSLimit(
        x[0], x[1], **_kw(op, 'score_thresh', 'nms', 'detections_per_im')), 2, cuts=True),
}


def cuts_flow(op_type):
    return op_type in TABLE and TABLE[op_type].cuts


def grad_inputs(op_type):
    """Indices of the inputs that receive a gradient; None for a type without a gradient rule."""
    return TABLE[op_type].grad_inputs if op_type in TABLE else None
