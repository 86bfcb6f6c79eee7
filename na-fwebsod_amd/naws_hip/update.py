"""The update schedule of a WsddnEngine: when and where the SGD update of a step runs, on which
stream, behind which events, and by which kernel route.  One object (UpdateSchedule) owns all of
its state; the engine keeps the arithmetic of a step and calls

    queue()                 sgd_step(): run the update now, or leave it WAITING for a launch site
    waits_for_heads(have)   conv_body: is an update waiting for the per-image chain heads?
    launch(events)          ... then behind them (or at once): WAITING -> QUEUED on the side stream
    join_for_head()         before the head reads the parameters: None, or the pieces' events
    finish_pieces(pieces)   the main stream joins what a piece-by-piece update still has in flight
    flush()                 join everything (checkpoints, lr changes, blob(), end of run)
    begin_backward(fuse)    -> BackwardStep: the gradient messages of this step and, train_step()
                            with an exchange, its update queued part by part behind them
    w6_done(rest)           fc6_w was updated in its wgrad epilogue: the deferred kernel skips it

The toggles (reducer, allreduce_chunks, pipeline_update, sharded_update, defer_update, fused_planes,
fuse_wgrad_update) and bench.py's event lists stay plain attributes of the engine and are read
from it at the time of use.  Which kernels a whole-arena update runs is decided once, by
choose_route() from plain values (Facts): tests/test_update_route.py enumerates it on the CPU."""
import collections

import torch

from . import ops
from .planes import ALL
from .reducer import message_plan, owner_blocks

HIDDEN = 4096
# NAWS.PIPELINE_UPDATE: the row pieces of fc6_w whose forward starts behind its own update - one
# branch each: 16 x 16 tiles of 256 x 256 at R = 4000 = one round of the 256 CUs
FWD_PIECES = ((0, HIDDEN), (HIDDEN, 2 * HIDDEN))
# ... one launch's slice of the arena (seg: the seg_tables of it; regions None: the element-wise
# kernel), and an engine's tables (pieces: per FWD_PIECES; ovf: [piece ... | tail])
UpdatePart = collections.namedtuple('UpdatePart', 'start count seg regions')
PipeTables = collections.namedtuple('PipeTables', 'pieces bias tail ovf')

IDLE, WAITING, QUEUED = 'idle', 'waiting', 'queued'     # UpdateSchedule.state

# ---- the route of a whole-arena update ----------------------------------------------------------
# What it depends on: the fused_planes toggle; a region table exists (FcPlanes is there, k6 % 256
# == 0, one hyper-parameter run per weight matrix); ITER_SIZE 1; the planes are dirty (a caller
# wrote through blob(): they carry stale maxima); the plan's GEMMs report maxima (fp16x2); its
# operands are 16-bit planes and FcPlanes is built; k6 % 256 == 0 (a wave's 256 floats stay in one
# row); fc6_w can be updated in the epilogue of its wgrad GEMM
Facts = collections.namedtuple('Facts', 'fused_planes regions iter1 dirty maxima planes16 k6_256 '
                                        'wgrad_update')
ROUTES = ('planes_f16x2',        # the plane-writing fp16x2 kernel over the whole arena
          'planes_f16x2_rest',   # the same with fc6_w skipped: its wgrad epilogue updated it
          'planes16',            # the plane-writing kernel in the bf16 / fp32x3 plane formats
          'planes16_rest',       # the same after the (bf16) wgrad epilogue, then `convert` of w7t
          'rowmax',              # fp16x2: the update reports row maxima, the planes split from them
          'split_all',           # plain update, every plane from scratch
          'plain')               # plain update, no planes (fp32)


def rows_whole(f):
    """The kernels that keep per-row words of fc6_w (maxima, scales, owners) can run."""
    return f.iter1 and f.k6_256


def planes_valid(f):
    """The plane-writing kernel can run on the planes as they are."""
    return f.regions and not f.dirty


def choose_route(f, w6_done):
    """The name (ROUTES) of the whole-arena update under Facts `f`; w6_done: fc6_w (weights,
    momentum, planes) was updated by its wgrad GEMM in this step's backward - the rest MUST take
    the plane-writing kernel with fc6_w's region skipped, even if an A/B tool has flipped
    fused_planes since."""
    if w6_done:
        if not (f.planes16 and f.regions and f.wgrad_update):
            raise RuntimeError('fc6_w was updated in its wgrad epilogue but the plane state '
                               'it belongs to is gone (engine toggles changed mid-step?)')
        return 'planes_f16x2_rest' if f.maxima else 'planes16_rest'
    if f.fused_planes and f.iter1 and planes_valid(f):
        return 'planes_f16x2' if f.maxima else 'planes16'
    if f.maxima and f.planes16 and rows_whole(f):
        return 'rowmax'
    return 'split_all' if f.planes16 else 'plain'


class BackwardStep(object):
    """One step's gradient hand-over, opened by UpdateSchedule.begin_backward().  plan: the
    messages (reducer.message_plan) the engine walks; sent: they go out in the pipelined order
    [fc6 biases][fc6_w row chunks ...][the rest]; eager: train_step() - each part of the
    piece-by-piece update is queued on the update stream RIGHT BEHIND the message it waits for,
    from inside backward (bias_sent / chunk_sent / tail_sent; no-ops otherwise), instead of after
    it: fc6_w, its planes and fc6's biases are not read again once the forward has run.  In queue
    order the update's parts then sit between the messages, so the pipeline also holds where HIP
    puts the update stream and the collective's stream on one hardware queue (two streams on one
    queue run in order; measured with ROCm's default queue count: queued after backward, every part
    waited behind the whole exchange)."""

    def __init__(self, sched, plan, sent, eager):
        self.sched, self.plan, self.sent, self.eager = sched, plan, sent, eager
        # per forward piece: how many fc6_w messages start below its last row (= must have arrived
        # before its rows are complete)
        self.need = [sum(1 for kind, rows in plan if kind == 'fc6_w' and rows[0] < r1)
                     for _r0, r1 in FWD_PIECES]
        self.queued = 0          # forward pieces whose update is queued (eager)

    def begin(self):
        """Start of the piece-by-piece update (current stream = the update stream)."""
        self.sched.pipe_tables()
        self.arrived, self.events, self.grads_ready = 0, [], None
        self.tag = self.sched.eng.sgd_iter_count + 1

    def bias_sent(self):
        if self.eager:
            with torch.cuda.stream(self.sched.stream):
                self.bias()

    def chunk_sent(self, r1):
        """fc6_w's gradient rows below r1 are on their way."""
        while self.eager and self.queued < len(FWD_PIECES) and FWD_PIECES[self.queued][1] <= r1:
            with torch.cuda.stream(self.sched.stream):          # every chunk of this piece is out
                self.piece(self.queued)
            self.queued += 1

    def tail_sent(self):
        if self.eager:
            s = self.sched
            self.grads_ready = torch.cuda.current_stream(s.eng.device).record_event()
            with torch.cuda.stream(self.sched.stream):
                self.tail()
                s.event = s.stream.record_event()
            s.state = QUEUED

    # ---- the three parts (current stream = the update stream) ------------------------------------
    def bias(self):
        eng, b = self.sched.eng, self.sched.pipe.bias
        sl = slice(b.start, b.start + b.count)
        eng.reducer.wait_first(1)
        ops.acm_sgd_update(eng.grads[sl], eng.momentum_buf[sl], eng.lr, eng.params[sl], None,
                           *b.seg, eng.momentum, 0, 1, eng.gpu_num, eng.sgd_iter_count)

    def piece(self, i):
        s, eng, rows = self.sched, self.sched.eng, FWD_PIECES[i]
        eng.reducer.wait_first(self.need[i] - self.arrived)
        self.arrived = self.need[i]
        fc, ovf = eng._fc, s.pipe.ovf[i:i + 1]
        fc.begin(rows, with7=False)
        s.sgd_f16x2(s.pipe.pieces[i].regions, ovf, self.tag, s.pipe.pieces[i])
        fc.resplit6(eng._weight_views()[0], rows, ovf, self.tag)
        self.events.append((rows[0], rows[1], s.stream.record_event()))

    def tail(self):
        s, eng, t = self.sched, self.sched.eng, self.sched.pipe.tail
        # bench.py (comm_events): how long this stream, with this rank's gradients complete, still
        # waits for the exchange (`grads_ready`: the main stream behind the last gradient kernel)
        if getattr(eng, 'comm_events', None) is not None and self.grads_ready is not None:
            s.stream.wait_event(self.grads_ready)
        with eng._timed('comm_events'):
            eng.reducer.wait()
        fc, ovf = eng._fc, s.pipe.ovf[-1:]
        with eng._timed('update_events'):
            fc.begin(None, with7=True)
            s.sgd_f16x2(t.regions, ovf, self.tag, t)
        eng.sgd_iter_count += 1
        fc.finish7(eng._weight_views()[1], ovf, self.tag)
        eng._planes_dirty = False
        s.piece_events = dict(fc6=self.events, done=s.stream.record_event())


class UpdateSchedule(object):
    def __init__(self, eng, new_stream):
        """new_stream(): the side stream the deferred update runs on, made on first use (an
        ordinary stream: a low-priority one, or one confined to a subset of the compute units,
        measured worse in every form - docs/history: 13.7-23 vs 13.5 ms per step)."""
        self.eng, self._new_stream = eng, new_stream
        self.state = IDLE            # IDLE | WAITING for a launch site | QUEUED behind self.event
        self.stream = self.event = self.grads_ready = None
        self.piece_events = None     # pipelined update: dict(fc6=[(r0, r1, event)], done=event)
        self.pipe = None             # its PipeTables (built on first use)
        self.step = BackwardStep(self, [], False, False)     # the step in flight
        self.w6_rest = None          # the region table for the deferred kernel once fc6_w is done
        self.shard, self.mom_synced = None, True             # NAWS.SHARDED_UPDATE
        self.warned = False

    def facts(self):
        eng, fc = self.eng, self.eng._fc
        return Facts(bool(eng.fused_planes), fc is not None and fc.whole is not None,
                     eng.iter_size == 1, bool(eng._planes_dirty), eng.arith.reports_maxima,
                     fc is not None, eng.k6 % 256 == 0, eng.arith.wgrad_update)

    # ---- which routes are in force ---------------------------------------------------------------
    def pipelined(self):
        """True when this process's updates run piece by piece (NAWS.PIPELINE_UPDATE)."""
        eng, red, f = self.eng, self.eng.reducer, self.facts()
        want = True if eng.pipeline_update is None else eng.pipeline_update
        on = bool(want and red.active and hasattr(red, 'wait_first') and f.maxima
                  and not eng.sharded_update and rows_whole(f) and f.fused_planes
                  and (eng.defer_update is None or eng.defer_update))
        if on and not self.warned:
            self.warned = True
            if eng.pg is not None and eng.world_size > 1:
                import torch.distributed as dist
                if dist.get_backend(eng.pg) != 'gloo':
                    # per-message Work.wait() on the update stream from inside backward,
                    # SGD pieces between collectives still in flight, fc6 forward pieces gated on
                    # per-piece events - validated over gloo (2 and 8 ranks on one GPU) and with
                    # one-rank RCCL only; no multi-GPU node was ever available
                    import warnings
                    warnings.warn('NAWS.PIPELINE_UPDATE on backend %r with %d ranks has never run '
                                  'on hardware (validated over gloo and one-rank RCCL only); '
                                  'NAWS.PIPELINE_UPDATE False is the fallback: the one-launch update '
                                  'behind the whole exchange.  bench.py checks the ranks\' state '
                                  'digests after warm-up and falls back by itself on a stall'
                                  % (dist.get_backend(eng.pg), eng.world_size))
        return on

    def can_fuse_wgrad_update(self):
        eng, f = self.eng, self.facts()
        return bool(eng.fuse_wgrad_update and not eng.reducer.active and f.wgrad_update
                    and f.fused_planes and rows_whole(f) and planes_valid(f))

    def shard_blocks(self):
        """The owners' row blocks of fc6_w when the sharded update is in force, else None."""
        eng, red = self.eng, self.eng.reducer
        if not (eng.sharded_update and red.active):
            return None
        if self.shard is None:
            f = self.facts()
            if not (f.maxima and rows_whole(f)):
                raise NotImplementedError('NAWS.SHARDED_UPDATE needs the fp16x2 plan, ITER_SIZE 1 '
                                          'and a 256-multiple fc6 input')
            blocks = owner_blocks(2 * HIDDEN, red.world_size)
            if blocks is None:
                raise NotImplementedError('NAWS.SHARDED_UPDATE: 8192 rows do not divide into '
                                          '32-row multiples over %d ranks' % red.world_size)
            self.shard = dict(blocks=blocks)
            if eng.pg is not None:
                import warnings
                import torch.distributed as dist
                if dist.get_backend(eng.pg) != 'gloo':
                    # the RCCL legs of this route (per-owner dist.reduce, in-place
                    # all_gather_into_tensor on fp32 and int32 buffers, issued from the update
                    # stream) have never executed - no multi-GPU node was available; only the gloo
                    # emulation (all_reduce / broadcast) has
                    warnings.warn('NAWS.SHARDED_UPDATE on backend %r has never run on hardware '
                                  '(validated over gloo only); check the first steps against the '
                                  'all-reduce route' % dist.get_backend(eng.pg))
        return self.shard['blocks']

    def set_route(self, pipeline_update, sharded_update):
        self.flush()
        if self.shard_blocks() is not None:
            self.gather_sharded_state()
        self.eng.pipeline_update, self.eng.sharded_update = pipeline_update, bool(sharded_update)
        self.shard, self.mom_synced, self.step.sent = None, True, False

    # ---- when and where --------------------------------------------------------------------------
    def queue(self):
        """sgd_step(): by default the update goes to a side stream, where it waits for the gradient
        all-reduce and runs the (HBM-bound) fused SGD kernel while the main stream already runs the
        next iteration's (MFMA-bound, parameter-free) conv body + RoIPool.  It is launched by that
        conv body behind conv1_1 of every image (or by flush): started at once, the SGD kernel's
        workgroups fill the CUs and the two conv1_1 launches at the head of the dependent chains
        took 0.7 ms each."""
        if self.step.eager:
            self.step.eager = False       # train_step: backward has queued the update already
        elif self.eng.defer_update is not None and not self.eng.defer_update:
            self.apply()                  # inline on the main stream
        else:
            self.stream = self.stream or self._new_stream()
            self.grads_ready = torch.cuda.current_stream(self.eng.device).record_event()
            self.state = WAITING

    def waits_for_heads(self, have_heads):
        """conv_body: True when an update is waiting and there are per-image chain heads to put it
        behind (-> launch(their events)); a waiting update without them is launched at once."""
        if self.state == WAITING and not have_heads:
            self.launch(())
        return self.state == WAITING

    def launch(self, after):
        """Queue the update on its side stream, behind the gradients and the events in `after`."""
        self.state = QUEUED
        self.stream.wait_event(self.grads_ready)
        for e in after:
            self.stream.wait_event(e)
        self.piece_events = None
        with torch.cuda.stream(self.stream):
            self.apply()
            self.event = self.stream.record_event()

    def flush(self):
        if self.state != IDLE:
            if self.state == WAITING:
                self.launch(())
            self.state, self.piece_events = IDLE, None
            torch.cuda.current_stream(self.eng.device).wait_event(self.event)

    def join_for_head(self):
        """Before the head reads the parameters: join the deferred update - entirely (-> None), or,
        when it ran piece by piece, hand the pieces' events to head_forward, which waits for each
        one right before the launch that needs it."""
        if self.state == IDLE:
            return None
        if self.state == WAITING:
            self.launch(())
        if self.piece_events is None:
            return self.flush()
        pieces, self.piece_events = self.piece_events, None
        return pieces

    def finish_pieces(self, pieces):
        """The main stream joins what is left of a pipelined update (everything after fc6_w)."""
        self.state = IDLE
        torch.cuda.current_stream(self.eng.device).wait_event(pieces['done'])

    def begin_backward(self, fuse_update):
        eng = self.eng
        pipelined = self.pipelined()
        plan = message_plan(eng.arena, 2 * HIDDEN, eng.allreduce_chunks, eng.reducer.active,
                            pipelined)
        eager = bool(pipelined and fuse_update and planes_valid(self.facts()))
        st = self.step = BackwardStep(self, plan, pipelined, eager)
        if eager:
            self.stream = self.stream or self._new_stream()
            self.flush()                 # (nothing can be pending here: the head joined it)
            with torch.cuda.stream(self.stream):
                st.begin()
        return st

    def w6_done(self, rest):
        """The route is decided HERE: the deferred kernel of this step must skip fc6_w whatever
        the toggles say by the time it runs (the table to use, FcPlanes.rest, travels with it)."""
        self.w6_rest = rest

    # ---- by which kernels ------------------------------------------------------------------------
    def apply(self):
        """This step's update on the current stream."""
        eng = self.eng
        # the messages of this step went out in the pipelined order AND the plane-writing kernel can
        # run on them; otherwise the update waits for everything and takes a one-launch route - any
        # message order is fine for that
        if (self.step.sent and planes_valid(self.facts()) and self.stream is not None
                and torch.cuda.current_stream(eng.device) == self.stream):
            return self._apply_pipelined()      # (waits message by message itself)
        # bench.py: how long this stream, with this rank's gradients complete, waits for the exchange
        with eng._timed('comm_events', on=eng.reducer.active):
            eng.wait_allreduce()
        if self.shard_blocks() is not None:
            return self._apply_sharded()
        rest, self.w6_rest = self.w6_rest, None
        {'planes_f16x2': self._planes_f16x2, 'planes_f16x2_rest': lambda: self._planes_f16x2(rest),
         'planes16': self._planes16, 'planes16_rest': lambda: self._planes16(rest),
         'rowmax': self._rowmax, 'split_all': self._split_all,
         'plain': self._elementwise}[choose_route(self.facts(), rest is not None)]()
        if eng._fc is not None:
            eng._planes_dirty = False

    def sgd_f16x2(self, regions, ovf, tag, part=None):
        """The plane-writing SGD kernel (fp16x2) over the whole arena, or over `part` (an
        UpdatePart) of it; `ovf` receives `tag` when a row outgrew its bound."""
        eng = self.eng
        a, b = (0, eng.arena.total) if part is None else (part.start, part.start + part.count)
        seg = (eng.seg_end, eng.seg_lr_mult, eng.seg_wd) if part is None else part.seg
        ops.acm_sgd_update_f16x2(eng.grads[a:b], eng.momentum_buf[a:b], eng.lr, eng.params[a:b],
                                 *seg, eng.momentum, 0, eng.gpu_num, eng.sgd_iter_count, regions,
                                 ovf, tag)

    def _planes_f16x2(self, rest=None):
        """The SGD kernel writes the planes too, with scales from twice the rows' maxima before the
        update; a device-side conditional exact re-split covers a row that outgrew its bound."""
        eng, fc, tag = self.eng, self.eng._fc, self.eng.sgd_iter_count + 1
        w6, w7 = eng._weight_views()
        with eng._timed('update_events'):          # bench.py: HIP events on the update stream
            fc.begin(ALL if rest is None else None, with7=True)     # (fc6_w's half: its wgrad's)
            self.sgd_f16x2(fc.whole if rest is None else rest, fc.ovf, tag)
        eng.sgd_iter_count += 1
        if rest is None:
            fc.resplit6(w6, ALL, fc.ovf, tag)
        fc.finish7(w7, fc.ovf, tag)

    def _planes16(self, rest=None):
        """fp32x3 / bf16: the same kernel with their plane formats (exact / rounded planes)."""
        eng, fc = self.eng, self.eng._fc
        with eng._timed('update_events'):
            ops.acm_sgd_update_planes(eng.grads, eng.momentum_buf, eng.lr, eng.params, eng.seg_end,
                                      eng.seg_lr_mult, eng.seg_wd, eng.momentum, 0, eng.gpu_num,
                                      eng.sgd_iter_count, fc.whole if rest is None else rest)
        eng.sgd_iter_count += 1
        fc.convert(eng._weight_views()[1], transpose=True, out=fc.operands['w7t'])

    def _elementwise(self, maxima_of=None):
        """The element-wise kernel; maxima_of (FcPlanes): it reports max|w| of every updated fc6_w /
        fc7_w row into the scale blocks of their operand planes."""
        eng, fc = self.eng, maxima_of
        with eng._timed('update_events'):
            ops.acm_sgd_update(eng.grads, eng.momentum_buf, eng.lr, eng.params, eng.acmgrad,
                               eng.seg_end, eng.seg_lr_mult, eng.seg_wd, eng.momentum, 0,
                               eng.iter_size, eng.gpu_num, eng.sgd_iter_count,
                               rowmax=fc and fc.zeroed_rowmax(), rm_table=fc and fc.rm_table)
        eng.sgd_iter_count += 1

    def _rowmax(self):
        """... so the re-split reads the weights once (same stream as the update: hidden with it)."""
        self._elementwise(self.eng._fc)
        self.eng._fc.split_from_maxima(*self.eng._weight_views())

    def _split_all(self):
        self._elementwise()
        self.eng._fc.split_all(*self.eng._weight_views())

    # ---- NAWS.PIPELINE_UPDATE --------------------------------------------------------------------
    def seg_tables(self, start, count):
        """(seg_end, seg_lr_mult, seg_wd) device tensors of the arena range [start, start + count),
        ends relative to `start` (the SGD kernels take a base pointer + per-run hyper-parameters)."""
        (ends, lr_mult, wd), dev = self.eng._seg_host, self.eng.device
        first = next(i for i, e in enumerate(ends) if e > start)          # the runs that overlap it
        last = next((i for i, e in enumerate(ends) if e >= start + count), len(ends) - 1)
        runs = slice(first, last + 1)
        return (torch.tensor([min(e, start + count) - start for e in ends[runs]], dtype=torch.int64,
                             device=dev),
                torch.tensor(lr_mult[runs], dtype=torch.float32, device=dev),
                torch.tensor(wd[runs], dtype=torch.float32, device=dev))

    def pipe_tables(self):
        if self.pipe is None:
            def part(start, count, regions):
                return UpdatePart(start, count, self.seg_tables(start, count), regions)
            fc = self.eng._fc
            self.pipe = PipeTables([part(*fc.piece(r0, r1)) for r0, r1 in FWD_PIECES],
                                   part(fc.ob, fc.o7 - fc.ob, None), part(*fc.tail()),
                                   torch.zeros((len(FWD_PIECES) + 1,), device=self.eng.device,
                                               dtype=torch.int32))

    def _apply_pipelined(self):
        """The deferred update of an N > 1 step, piece by piece (update stream).  Messages arrive
        in the order backward handed them over: [fc6 biases][fc6_w row chunks ...][the rest].
          1. fc6's biases (element-wise kernel on their 8192 floats);
          2. per forward piece (FWD_PIECES: fc6_w rows of one branch): wait for the chunks that
             cover it, run the plane-writing SGD kernel on exactly those rows (arena slice, row
             block of the operand planes), queue the conditional exact re-split of those rows,
             record the piece's event - the next iteration's fc6 forward launches that piece
             behind it (head_forward) while the later messages are still on the links;
          3. the rest (fc7_w with planes + column maxima, fc8, biases), fc7_w's transposed planes,
             the final event.
        Per element the arithmetic is the one-launch route's (same kernels on slices: parameters,
        momentum, planes and scales bit-identical, tests/test_gpu_two_ranks.py); the one difference:
        the "a row outgrew twice its previous maximum" word is kept PER PIECE, so the exact
        re-split that answers it covers that piece's rows instead of all of fc6_w / fc7_w - the
        other rows keep their (equally valid) bound-derived scales.

        This is the form queue() leaves for a launch site after a plain forward_backward().
        train_step() queues the same three parts EARLIER, from inside backward (BackwardStep)."""
        st = self.step
        st.begin()
        st.bias()
        for i in range(len(FWD_PIECES)):
            st.piece(i)
        st.tail()

    # ---- NAWS.SHARDED_UPDATE ---------------------------------------------------------------------
    def _apply_sharded(self):
        """The deferred update of a rank under NAWS.SHARDED_UPDATE (update stream):
          1. wait for the reduces of this rank's fc6_w rows and for the small all-reduce;
          2. the plane-writing SGD kernel over [this rank's fc6_w rows | fc7_w | fc8 | biases] - the
             other owners' fc6_w rows are skip regions (neither read nor written);
          3. all-gather, in place: the updated fp32 rows (822 MB / N per rank) and, per owner, the
             rows' exact maxima, the 1/scale the owner's planes carry, and its overflow word;
          4. one split of all 8192 rows with exactly the scales the all-reduce route would hold:
             the owners' bound-derived ones, or - if ANY row of any owner outgrew its bound, which
             is what the single overflow word of the all-reduce route records - the exact maxima.
        fc7_w / fc8 / biases: as in the all-reduce route (every rank updates them)."""
        eng, sh = self.eng, self.shard
        blocks, red, fc, n6 = sh['blocks'], eng.reducer, eng._fc, 2 * HIDDEN
        b0, b1 = blocks[eng.rank]
        nb = b1 - b0
        eng.wait_allreduce()
        if eng._planes_dirty or fc is None:
            raise RuntimeError('sharded update: the operand planes are stale (blob() written '
                               'through between backward and update?)')
        if 'regions' not in sh:
            if fc.whole is None:
                raise RuntimeError('the sharded update needs the plane-writing SGD kernel '
                                   '(one hyper-parameter run over fc6_w / fc7_w)')
            sh['regions'] = fc.shard_table(b0, b1)
            # what travels back beside the fp32 rows: per owner [row maxima | 1/scale | overflow word]
            sh['meta'] = torch.zeros((len(blocks), 2 * nb + 4), device=eng.device, dtype=torch.int32)
        regions, meta = sh['regions'], sh['meta']
        max6 = fc.maxima(6)
        tag = eng.sgd_iter_count + 1
        fc.begin((b0, b1), with7=True)
        with eng._timed('update_events'):
            self.sgd_f16x2(regions, fc.ovf, tag)
        eng.sgd_iter_count += 1
        self.mom_synced = len(blocks) == 1
        # every owner's block starts from this rank's own view of those rows (what the previous
        # gather left: right for the rows this rank does not own only until the gather below
        # overwrites them - and what an exchange that moves no data, bench.py's projection, keeps)
        meta[:, :nb].copy_(max6.view(len(blocks), nb))
        meta[:, nb:2 * nb].copy_(fc.inv_scale(6).view(torch.int32).view(len(blocks), nb))
        meta[:, 2 * nb].zero_()
        meta[eng.rank, 2 * nb:2 * nb + 1].copy_(fc.ovf)
        w6, w7 = eng._weight_views()
        red.gather_blocks_async(w6.reshape(-1), eng.rank)
        red.gather_blocks_async(meta.view(-1), eng.rank)
        red.wait()
        raised = (meta[:, 2 * nb] == tag).any()
        rowmax = meta[:, :nb].reshape(n6)
        bound_scale = (meta[:, nb:2 * nb].reshape(n6).view(torch.float32) * 16384.0).view(torch.int32)
        max6.copy_(rowmax)
        eff = torch.where(raised, rowmax, bound_scale)     # 1/scale = 2^(e-14)  ->  a maximum 2^e
        fc.ovf.copy_(torch.where(raised, torch.full_like(fc.ovf, tag), fc.ovf))
        # the rows this rank does NOT own: planes from the owners' scales (always); its own rows
        # already carry the planes its SGD kernel wrote with exactly those scales - they are redone
        # (from the exact maxima) only if some owner raised the overflow word (the full
        # re-split gave back most of what the owner-only update saves)
        if b0 > 0:
            fc.resplit6(w6, (0, b0), rowmax=eff)
        if b1 < n6:
            fc.resplit6(w6, (b1, n6), rowmax=eff)
        fc.resplit6(w6, (b0, b1), fc.ovf, tag, rowmax=eff)
        fc.finish7(w7, fc.ovf, tag)
        eng._planes_dirty = False

    def gather_sharded_state(self):
        """COLLECTIVE (every rank): bring the owners' momentum rows of fc6_w to all ranks so that
        any rank can write a complete checkpoint.  The fp32 weights are complete on every rank
        after each update; the momentum of a row lives with its owner only.  No-op otherwise."""
        if self.shard_blocks() is None or self.mom_synced:
            return
        self.flush()
        eng = self.eng
        m6 = eng.arena.span(eng.momentum_buf, 'fc6_w', '_[noisy]_fc6_w')
        eng.reducer.gather_blocks_async(m6, eng.rank)
        eng.reducer.wait()
        self.mom_synced = True
