"""Recorder of an engine's launch-and-sync schedule, shared by
tests/golden/make_golden_update_trace.py and tests/test_gpu_update_trace.py.  Inside
`with Recorder() as rec:` every

  * `naws_hip.lib.call` becomes a row [entry, arg ...]: ints and the u64 seed exactly, floats by
    repr, a pointer as null / not null (as tests/golden/make_golden_opbyop_call_trace.py records
    them) - except the LAST argument, the HIP stream of the launch (the C ABI's convention), which
    becomes 's<k>', k = the stream's ordinal by first appearance in the recording;
  * `torch.cuda.Stream.record_event` becomes ['record_event', 's<k>', 'e<j>'] with a fresh j;
  * `torch.cuda.Stream.wait_event` becomes ['wait_event', 's<k>', 'e<j>'] (the WAITING stream; e-1:
    an event the recording has not seen recorded);
  * call of one of the five exchange methods on a reducer passed to `rec.watch()` becomes
    ['reducer.<method>', elements] (`wait`: no number; `wait_first`: its n).
Streams are told apart by their HIP handle, events by identity (kept alive by the recorder)."""
import torch

REDUCER_METHODS = ('reduce_async', 'reduce_to_owner_async', 'gather_blocks_async', 'wait',
                   'wait_first')


def pack(scenarios):
    """{scenario: dict(trace=rows, digests=...)} -> the form kept on disk, lossless: every distinct
    row once in a table and per scenario the indices into it; an event ordinal is implied by the
    order of the record_event rows, so those drop it and a wait_event keeps how many records back
    its event lies (iterations and scenarios then repeat the same few rows)."""
    table, out = {}, {}
    for name, sc in scenarios.items():
        idx, n = [], 0
        for row in sc['trace']:
            if row[0] == 'record_event':
                assert row[2] == 'e%d' % n
                row, n = row[:2], n + 1
            elif row[0] == 'wait_event':
                row = row[:2] + [n - int(row[2][1:])]
            idx.append(table.setdefault(tuple(row), len(table)))
        out[name] = dict(trace=idx, digests=sc['digests'])
    return dict(rows=[list(r) for r in table], scenarios=out)


def unpack(packed):
    """The inverse of pack()."""
    out = {}
    for name, sc in packed['scenarios'].items():
        rows, n = [], 0
        for row in (list(packed['rows'][i]) for i in sc['trace']):
            if row[0] == 'record_event':
                row, n = row + ['e%d' % n], n + 1
            elif row[0] == 'wait_event':
                row[2] = 'e%d' % (n - row[2])
            rows.append(row)
        out[name] = dict(trace=rows, digests=sc['digests'])
    return out


class Recorder(object):
    def __init__(self):
        self.rows, self._streams, self._events, self._undo = [], {}, {}, []

    def _s(self, handle):
        return 's%d' % self._streams.setdefault(int(handle or 0), len(self._streams))

    def _patch(self, owner, name, make):
        real = getattr(owner, name)
        self._undo.append((owner, name, real, name in vars(owner)))
        setattr(owner, name, make(real))

    def __enter__(self):
        from naws_hip import lib as L

        def call(real):
            def recording(entry, *args):
                kinds, row = L.PROTOTYPES[entry], [entry]
                for k, (kind, v) in enumerate(zip(kinds, args)):
                    v = getattr(v, 'value', v)
                    if kind is L.p:
                        row.append(self._s(v) if k == len(kinds) - 1 else bool(v))
                    else:
                        row.append(repr(float(v)) if kind is L.f32 else int(v))
                self.rows.append(row)
                return real(entry, *args)
            return recording

        def record_event(real):
            def recording(stream, event=None):
                ev = real(stream, event)
                self._events[id(ev)] = (len(self._events), ev)
                self.rows.append(['record_event', self._s(stream.cuda_stream),
                                  'e%d' % self._events[id(ev)][0]])
                return ev
            return recording

        def wait_event(real):
            def recording(stream, event):
                self.rows.append(['wait_event', self._s(stream.cuda_stream),
                                  'e%d' % self._events.get(id(event), (-1,))[0]])
                return real(stream, event)
            return recording
        self._patch(L, 'call', call)
        self._patch(torch.cuda.Stream, 'record_event', record_event)
        self._patch(torch.cuda.Stream, 'wait_event', wait_event)
        return self

    def watch(self, reducer):
        """Record the exchange methods of this reducer object (instance attributes: whoever calls
        them through the object is seen)."""
        def method(name):
            def make(real):
                def recording(*args):
                    row = ['reducer.' + name]
                    if name == 'wait_first':
                        row.append(int(args[0]))
                    elif name != 'wait':
                        row.append(int(args[0].numel()))
                    self.rows.append(row)
                    return real(*args)
                return recording
            return make
        for name in REDUCER_METHODS:
            self._patch(reducer, name, method(name))
        return reducer

    def __exit__(self, *exc):
        for owner, name, real, own in reversed(self._undo):
            if own:
                setattr(owner, name, real)
            else:
                delattr(owner, name)          # (a reducer's bound method: back to the class's)
        self._undo = []
        return False
