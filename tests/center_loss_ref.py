"""numpy restatement of the reference's CenterLoss / CenterLossGradient pair, written from
detectron/ops/center_loss_op.cu:33-568 (schema center_loss_op.cc:12-69).  The arbiter of
tests/test_center_loss_graph.py and tests/test_gpu_center_loss.py.

Wherever the reference sums (the distance dots, the loss, dF, the centre contribution, the
accumulators, the centre update) this computes in float64; where it only subtracts (D) it keeps
float32, so D is comparable bit for bit.  The state is the op pair's: the two iteration counters,
the gradient op's private accumulators and first-call flag, the forward op's display counters.
The three blobs CF / dCF / ndCF are the caller's and change in place, as the net's do."""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)


def select(X, P, top_k, ignore_label=-1):
    """-> picks int [C, top_k] in ascending roi index (-1 rows for inactive classes), or None when
    an active class runs out of selectable rois (the reference fails the net, :161-166)."""
    X = np.asarray(X, np.float32).reshape(-1)
    P = np.asarray(P, np.float32)
    R, C = P.shape
    picks = -np.ones((C, top_k), np.int64)
    for c in range(C):
        if c == ignore_label or R < top_k or X[c] < 0.5:           # :126-144
            continue
        # the scan `max_val < pred_val` from -FLT_MAX (:148-158): strict, so NaN, -FLT_MAX and -inf
        # never win and the first index wins ties (np.argmax returns the first maximum)
        free = P[:, c] > np.float32(-FLT_MAX)
        chosen = []
        for _ in range(top_k):
            if not free.any():
                return None
            r = int(np.argmax(np.where(free, P[:, c], -np.inf)))
            chosen.append(r)
            free[r] = False
        picks[c] = sorted(chosen)                                   # std::set order, :192
    return picks


class CenterLossRef(object):
    def __init__(self, top_k=10, update=128, lr=0.5, display=1280, max_iter=0, ignore_label=-1):
        self.top_k, self.update, self.lr = int(top_k), int(update), float(lr)
        self.display, self.max_iter, self.ignore_label = int(display), int(max_iter), int(ignore_label)
        self.cur_iter = self.cur_iter_grad = 0
        self.init_grad = True
        self.acc_dCF = self.acc_ndCF = None
        self.counts = None
        self.dots = None        # float64 [C, M] of the last forward (nan for inactive classes)

    def forward(self, X, P, F, CF):
        """-> (L float64, D float32 [C, top_k, Dm], S float32 [C], picks int [C, top_k])."""
        P, F, CF = (np.asarray(a, np.float32) for a in (P, F, CF))
        R, C = P.shape
        M, Dm = CF.shape[1:]
        D = np.zeros((C, self.top_k, Dm), np.float32)
        S = -np.ones((C,), np.float32)
        picks = -np.ones((C, self.top_k), np.int64)
        self.dots = np.full((C, M), np.nan)
        if self.cur_iter >= self.max_iter:                          # :76-78
            return 0.0, D, S, picks
        if self.counts is None:
            self.counts = np.zeros((C, M), np.int64)
        picks = select(X, P, self.top_k, self.ignore_label)
        if picks is None:
            self.cur_iter += 1
            return float('nan'), D, S, -np.ones((C, self.top_k), np.int64)
        num_gt, dot = 0, 0.0
        for c in range(C):
            if picks[c, 0] < 0:
                continue
            num_gt += 1
            rows = F[picks[c]]                                       # [top_k, Dm], ascending roi index
            c_dot, sel = FLT_MAX, -1
            for m in range(M):
                diff = rows - CF[c, m][None, :]                      # float32 subtraction
                cm = float((diff.astype(np.float64) ** 2).sum())
                self.dots[c, m] = cm
                if cm < c_dot:                                       # strict: first centre wins ties
                    c_dot, sel, D[c] = cm, m, diff
            S[c] = sel
            self.counts[c, sel] += 1
            dot += c_dot
        L = dot / num_gt / self.top_k / Dm / 2.0 if num_gt > 0 else 0.0
        self.cur_iter += 1
        return L, D, S, picks

    def gradient(self, D, S, picks, dL, R, CF, dCF, ndCF):
        """-> dF float64 [R, Dm]; CF / dCF / ndCF (float64 or float32 arrays) change in place."""
        C, top_k, Dm = D.shape
        dF = np.zeros((R, Dm), np.float64)
        if self.cur_iter_grad >= self.max_iter:                     # :329-331
            return dF
        if self.init_grad:                                          # :340-359
            self.acc_dCF = np.zeros(dCF.shape, np.float64)
            self.acc_ndCF = np.zeros(ndCF.shape, np.float64)
            dCF[...] = 0
            ndCF[...] = 0
            self.init_grad = False
        self.acc_dCF += dCF                                         # :374-379
        self.acc_ndCF += ndCF
        dCF[...] = 0                                                # :381-384
        ndCF[...] = 0
        num_gt = int((picks[:, 0] >= 0).sum())
        alpha = float(dL) / num_gt / top_k / Dm if num_gt > 0 else 0.0
        for c in range(C):
            if picks[c, 0] < 0:
                continue
            sel = int(S[c])
            ndCF[c, sel] += 1                                       # :475-486
            for k in range(top_k):
                dF[picks[c, k]] += alpha * D[c, k].astype(np.float64)
                dCF[c, sel] -= D[c, k].astype(dCF.dtype)
        self.cur_iter_grad += 1
        if self.cur_iter_grad % self.update == 0:                   # :542-565
            n = self.acc_ndCF.astype(np.int64)
            CF -= (self.lr / (n * top_k + 1))[:, :, None] * self.acc_dCF
            self.acc_dCF[...] = 0
            self.acc_ndCF[...] = 0
        return dF
