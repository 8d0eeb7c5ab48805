"""AU evaluation metric of the reference: per-AU binary F1 + accuracy.

Reference: ``MultiLabelAccF1`` (metrics/accf1.py:47-77) fed with ``round(sigmoid(logits))`` per batch
(train.py:155) and scored as ``0.5*F1 + 0.5*acc`` (train.py:163).  The reference stacks every prediction on the host
and calls sklearn per AU at the end; here the sufficient statistics (true/false positives, false negatives, correct
and labelled counts per AU) accumulate on the device, so an evaluation loop never synchronises per batch.  Results
equal sklearn's ``f1_score(average='binary')`` / ``accuracy_score(normalize=False)`` path (F1 := 0 where a class has
no positive label and no positive prediction, sklearn's zero_division default).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _cabi


class MultiLabelAccF1:
    def __init__(self, ignore_index: Optional[float] = -1, num_labels: int = 12):
        self.ignore_index = ignore_index
        self.num_labels = num_labels
        self._stats: Optional[torch.Tensor] = None  # [5, num_labels]: tp, fp, fn, correct, labelled

    def clear(self):
        self._stats = None

    @torch.no_grad()
    def update(self, y_pred: torch.Tensor, y_true: torch.Tensor):
        """y_pred: hard 0/1 predictions [B, num_labels] (``update_from_logits`` applies the reference's
        round(sigmoid(.))); y_true: labels in {0, 1, ignore_index}."""
        y_pred = y_pred.reshape(-1, self.num_labels)
        y_true = y_true.reshape(-1, self.num_labels).to(y_pred.device)
        keep = torch.ones_like(y_true, dtype=torch.bool) if self.ignore_index is None else (y_true != self.ignore_index)
        pos_p, pos_t = (y_pred == 1) & keep, (y_true == 1) & keep
        s = torch.stack([(pos_p & pos_t).sum(0), (pos_p & ~pos_t).sum(0), (~pos_p & pos_t & keep).sum(0),
                         ((y_pred == y_true) & keep).sum(0), keep.sum(0)]).to(torch.float64)
        self._stats = s if self._stats is None else self._stats + s

    def update_from_logits(self, logits: torch.Tensor, y_true: torch.Tensor):
        self.update(torch.round(torch.sigmoid(logits[:, :self.num_labels])), y_true)

    def get(self) -> Tuple[float, float]:
        """(accuracy over all labelled entries, mean of the per-AU binary F1 scores) - accf1.py:60-77"""
        if self._stats is None:
            raise RuntimeError("no samples")
        tp, fp, fn, correct, labelled = self._stats.cpu()
        denom = 2 * tp + fp + fn
        f1 = torch.where(denom > 0, 2 * tp / denom.clamp(min=1), torch.zeros_like(denom))
        return float(correct.sum() / labelled.sum()), float(f1.mean())

    def score(self) -> float:
        acc, f1 = self.get()
        return 0.5 * f1 + 0.5 * acc  # train.py:163


# ---- the whole evaluation side of train.py:106-169 ------------------------------------------------------------------
# Every metric of evaluate() is a function of plain sums over rows, so the accumulators below keep statistics, not samples:
# they can be updated batch by batch without a host copy, merged, and summed across ranks with one collective.  The layout of
# the fp64 words is the one of include/avformer_hip.h (avf_eval_update), read from there.
STATE_WORDS, EX_CONF, AU_STATS, VA_MOMENTS, LOSS_SUM, LOSS_STEPS = (
    _cabi.header()[0]["AVF_EVAL_" + n] for n in ("STATE_WORDS", "EX_CONF", "AU_STATS", "VA_MOMENTS", "LOSS_SUM", "LOSS_STEPS"))
SCORE_NAMES = ("ex_acc", "ex_f1", "ex_score", "au_acc", "au_f1", "au_score", "ccc_v", "ccc_a", "va_score", "avg_loss",
               "ex_kept_rows", "au_labelled")
AU_SWITCH = 2.0 ** -23  # round(sigmoid(x)) leaves 0 above this logit with a correctly rounded fp32 sigmoid


def _as_tensor(a) -> torch.Tensor:
    return a if torch.is_tensor(a) else torch.as_tensor(a)


def ex_confusion(pred: torch.Tensor, label: torch.Tensor, ignore_index, num_classes: int = 7) -> torch.Tensor:
    """[num_classes, num_classes] fp64 counts [label][prediction] over the rows whose label is a class and not ignore_index"""
    pred, label = pred.reshape(-1).long(), label.reshape(-1).long().to(pred.device)
    keep = (label >= 0) & (label < num_classes)
    if ignore_index is not None:
        keep = keep & (label != ignore_index)
    idx = label[keep] * num_classes + pred[keep]
    return torch.bincount(idx, minlength=num_classes * num_classes).to(torch.float64).reshape(num_classes, num_classes)


def va_moments(x: torch.Tensor, y: torch.Tensor, ignore) -> torch.Tensor:
    """[2, 6] fp64: n, sum x, sum y, sum x^2, sum y^2, sum x y per column over the rows whose label differs from ``ignore``"""
    x, y = x.reshape(-1, 2).to(torch.float64), y.reshape(-1, 2).to(x.device).to(torch.float64)
    k = (y != ignore).to(torch.float64)
    return torch.stack([k.sum(0), (k * x).sum(0), (k * y).sum(0), (k * x * x).sum(0), (k * y * y).sum(0), (k * x * y).sum(0)], 1)


def ex_scores(conf: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(accuracy, macro F1 over the classes present among labels or predictions) of a confusion matrix, fp64 scalars"""
    conf = conf.to(torch.float64)
    support = conf.sum(1) + conf.sum(0)
    present = support > 0
    f1 = torch.where(present, 2 * conf.diagonal() / support.clamp(min=1), torch.zeros_like(support))
    return conf.diagonal().sum() / conf.sum(), f1.sum() / present.sum()  # 0 / 0 = NaN without a kept row, as the reference


def au_scores(stats: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    tp, fp, fn, correct, labelled = stats.to(torch.float64)
    denom = 2 * tp + fp + fn
    f1 = torch.where(denom > 0, 2 * tp / denom.clamp(min=1), torch.zeros_like(denom))
    return correct.sum() / labelled.sum(), f1.mean()


def ccc_from_moments(mom: torch.Tensor) -> torch.Tensor:
    """cccmetric.py:4-34 from the six moments of a column: biased variances and covariance, 0 for n <= 1"""
    n, sx, sy, sxx, syy, sxy = mom.to(torch.float64).unbind(-1)
    nn = n.clamp(min=1)
    mx, my = sx / nn, sy / nn
    c = 2 * (sxy / nn - mx * my) / ((sxx / nn - mx * mx) + (syy / nn - my * my) + (mx - my) ** 2 + 1e-8)
    return torch.where(n > 1, c, torch.zeros_like(c))


def scores_from_state(state: torch.Tensor) -> torch.Tensor:
    """the twelve scores (SCORE_NAMES) of a 128-word state in plain torch, fp64 - what avf_eval_scores computes on the device"""
    s = state.detach().to("cpu", torch.float64)
    ex_acc, ex_f1 = ex_scores(s[EX_CONF:AU_STATS].reshape(7, 7))
    au_acc, au_f1 = au_scores(s[AU_STATS:VA_MOMENTS].reshape(5, 12))
    ccc = ccc_from_moments(s[VA_MOMENTS:LOSS_SUM].reshape(2, 6))
    return torch.stack([ex_acc, ex_f1, 0.67 * ex_f1 + 0.33 * ex_acc, au_acc, au_f1, 0.5 * au_f1 + 0.5 * au_acc, ccc[0], ccc[1],
                        (ccc[0] + ccc[1]) / 2, s[LOSS_SUM] / s[LOSS_STEPS], s[EX_CONF:AU_STATS].sum(), s[AU_STATS + 48:VA_MOMENTS].sum()])


class AccF1Metric:
    """accf1.py:20-42 (EX): ``update(y_pred, y_true)`` with class predictions and labels, ``get() -> (accuracy, macro F1)`` over
    the rows whose label differs from ``ignore_index``.  Keeps a confusion matrix instead of the samples; tensors on any device or
    numpy arrays.  A label outside 0..num_classes-1 is dropped (sklearn would invent a class for it)."""

    def __init__(self, ignore_index, average: str = 'macro', num_classes: int = 7):
        if average != 'macro':
            raise ValueError("AccF1Metric: only average='macro' (the one train.py uses) is implemented")
        self.ignore_index, self.average, self.num_classes = ignore_index, average, num_classes
        self._conf: Optional[torch.Tensor] = None

    def clear(self):
        self._conf = None

    @torch.no_grad()
    def update(self, y_pred, y_true):
        c = ex_confusion(_as_tensor(y_pred), _as_tensor(y_true), self.ignore_index, self.num_classes)
        self._conf = c if self._conf is None else self._conf + c

    def get(self) -> Tuple[float, float]:
        if self._conf is None:
            raise RuntimeError("no samples")
        acc, f1 = ex_scores(self._conf.cpu())
        return float(acc), float(f1)


class CCCMetric:
    """cccmetric.py:73-89 (VA): ``update(y_pred, y_true)`` with [B, 2] predictions (already through tanh, train.py:154) and
    labels, ``get() -> (ccc_v, ccc_a, their mean)``.  Keeps six fp64 moments per column instead of the samples."""

    def __init__(self, ignore_index: float = -5.0):
        self.ignore = ignore_index
        self._mom: Optional[torch.Tensor] = None

    def clear(self):
        self._mom = None

    @torch.no_grad()
    def update(self, y_pred, y_true):
        m = va_moments(_as_tensor(y_pred), _as_tensor(y_true), self.ignore)
        self._mom = m if self._mom is None else self._mom + m

    def get(self) -> Tuple[float, float, float]:
        if self._mom is None:
            raise RuntimeError("no samples")
        c = ccc_from_moments(self._mom.cpu())
        return float(c[0]), float(c[1]), float((c[0] + c[1]) / 2)


class EvalMetrics:
    """The three metrics of evaluate() and its running loss in one 128-word fp64 state (``.state``).

    ``update(result, labels, loss=None)`` takes the model's [B, 21] output and the {'EX', 'AU', 'VA'} label dict of
    train.py:127-131 (missing keys are skipped).  On a CUDA tensor it is exactly one kernel launch and no host synchronisation,
    so it can sit inside a captured graph; on a CPU tensor the same statistics come from plain torch (``update_torch``).
    ``scores()`` is the only synchronisation: one device-to-host copy of twelve doubles."""

    def __init__(self, ex_ignore: int = 7, au_ignore: float = -1.0, va_ignore: float = -5.0, ex_col: int = 12, au_col: int = 0,
                 va_col: int = 19, va_tanh: bool = True, device=None):
        self.ex_ignore, self.au_ignore, self.va_ignore = ex_ignore, au_ignore, va_ignore
        self.ex_col, self.au_col, self.va_col, self.va_tanh = ex_col, au_col, va_col, va_tanh
        self.state: Optional[torch.Tensor] = None if device is None else torch.zeros(STATE_WORDS, dtype=torch.float64, device=device)
        self._cfg_c = None

    def _cfg(self):
        if self._cfg_c is None:
            from . import _lib
            self._cfg_c = _lib.EvalCfg(self.ex_col, self.au_col, self.va_col, int(self.va_tanh),
                                       -1 if self.ex_ignore is None else int(self.ex_ignore), float(self.au_ignore), float(self.va_ignore))
        return self._cfg_c

    def _state_on(self, device) -> torch.Tensor:
        if self.state is None:
            self.state = torch.zeros(STATE_WORDS, dtype=torch.float64, device=device)
        return self.state

    def clear(self):
        if self.state is not None:
            self.state.zero_()

    @staticmethod
    def _labels(labels, device):
        def get(key, dtype):
            y = labels.get(key) if labels is not None else None
            if y is None:
                return None
            y = _as_tensor(y)
            return y if (y.dtype == dtype and y.device == device) else y.to(device=device, dtype=dtype)
        y_ex, y_au, y_va = get('EX', torch.int64), get('AU', torch.float32), get('VA', torch.float32)
        if y_ex is not None:
            y_ex = y_ex.reshape(-1).contiguous()
        if y_au is not None and y_au.stride(-1) != 1:
            y_au = y_au.contiguous()
        if y_va is not None and y_va.stride(-1) != 1:
            y_va = y_va.contiguous()
        return y_ex, y_au, y_va

    @torch.no_grad()
    def update(self, result: torch.Tensor, labels, loss: Optional[torch.Tensor] = None):
        if not result.is_cuda:
            return self.update_torch(result, labels, loss)
        from . import ops
        result = result.detach()
        if result.dtype != torch.float32 or result.stride(1) != 1:
            result = result.float().contiguous()
        y_ex, y_au, y_va = self._labels(labels, result.device)
        if loss is not None:
            loss = loss.detach()
            if loss.dtype != torch.float32 or loss.device != result.device:
                loss = loss.to(device=result.device, dtype=torch.float32)
        ops.eval_update(result, y_ex, y_au, y_va, loss, self._cfg(), self._state_on(result.device))

    def predictions_torch(self, result: torch.Tensor):
        """(EX class int64 [B], AU 0/1 uint8 [B, 12], VA fp32 [B, 2]) as train.py:150-155 takes them, in plain torch"""
        r = result.detach().float()
        va = r[:, self.va_col:self.va_col + 2]
        return (torch.argmax(r[:, self.ex_col:self.ex_col + 7], dim=1), (r[:, self.au_col:self.au_col + 12] > AU_SWITCH).to(torch.uint8),
                torch.tanh(va) if self.va_tanh else va.clone())

    @torch.no_grad()
    def update_torch(self, result: torch.Tensor, labels, loss: Optional[torch.Tensor] = None):
        """the statistics of ``update`` in plain torch, on the tensor's own device (the CPU path, and the kernel's checker)"""
        y_ex, y_au, y_va = self._labels(labels, result.device)
        p_ex, p_au, p_va = self.predictions_torch(result)
        st = self._state_on(result.device)
        if y_ex is not None:
            st[EX_CONF:AU_STATS] += ex_confusion(p_ex, y_ex, self.ex_ignore).reshape(-1)
        if y_au is not None:
            m = MultiLabelAccF1(ignore_index=self.au_ignore)
            m.update(p_au.to(y_au.dtype), y_au)
            st[AU_STATS:VA_MOMENTS] += m._stats.reshape(-1)
        if y_va is not None:
            st[VA_MOMENTS:LOSS_SUM] += va_moments(p_va, y_va, self.va_ignore).reshape(-1)
        if loss is not None:
            st[LOSS_SUM] += loss.detach().to(device=st.device, dtype=torch.float32).to(torch.float64).reshape(())
            st[LOSS_STEPS] += 1.0

    @torch.no_grad()
    def predict(self, result: torch.Tensor):
        """{'EX': int64 [B], 'AU': uint8 [B, 12], 'VA': fp32 [B, 2]} - the per-row predictions of test_aff2.py:98-117, from the same
        kernel launch as ``update`` (no statistics are touched)"""
        if not result.is_cuda:
            p_ex, p_au, p_va = self.predictions_torch(result)
            return {'EX': p_ex, 'AU': p_au, 'VA': p_va}
        from . import ops
        result = result.detach()
        if result.dtype != torch.float32 or result.stride(1) != 1:
            result = result.float().contiguous()
        B, dev = result.shape[0], result.device
        p_au = torch.empty((B, 12), dtype=torch.uint8, device=dev)
        p_ex = torch.empty(B, dtype=torch.int64, device=dev)
        p_va = torch.empty((B, 2), dtype=torch.float32, device=dev)
        ops.eval_update(result, None, None, None, None, self._cfg(), None, p_au, p_ex, p_va)
        return {'EX': p_ex, 'AU': p_au, 'VA': p_va}

    def merge(self, other: "EvalMetrics"):
        """adds another accumulator's statistics (of a disjoint set of rows) to this one"""
        if other.state is not None:
            st = self._state_on(other.state.device)
            st += other.state.to(st.device)
        return self

    def all_reduce(self, group=None):
        """one all-reduce (SUM) of the state: afterwards every rank's scores are those of the global validation set"""
        import torch.distributed as dist
        if self.state is None:
            raise RuntimeError("EvalMetrics.all_reduce: no state yet (construct with device=, or update first)")
        dist.all_reduce(self.state, op=dist.ReduceOp.SUM, group=group)
        return self

    def scores_vector(self) -> torch.Tensor:
        """the twelve scores (SCORE_NAMES) as a CPU fp64 tensor"""
        if self.state is None:
            raise RuntimeError("no samples")
        if self.state.is_cuda:
            from . import ops
            return ops.eval_scores(self.state, self._cfg()).cpu()
        return scores_from_state(self.state)

    def scores(self) -> dict:
        """the dict of train.py:160-164, with the reference's keys"""
        v = [float(t) for t in self.scores_vector()]
        self.avg_loss = v[9]
        return {'EX': {'EX:acc': v[0], 'f1': v[1], 'score': v[2]}, 'AU': {'AU:acc': v[3], 'f1': v[4], 'score': v[5]},
                'VA': {'VA:ccc_v': v[6], 'ccc_a': v[7], 'score': v[8]}}

    def total_score(self, task: str, scores: Optional[dict] = None) -> float:
        """train.py:259-270: the sum of the three task scores for task 'ALL', else the task's own"""
        scores = self.scores() if scores is None else scores
        if task == 'ALL':
            return scores['EX']['score'] + scores['AU']['score'] + scores['VA']['score']
        return scores[task]['score']


@torch.no_grad()
def evaluate(model, batches, num_step: int, task: Optional[str] = None, group=None, metrics: Optional[EvalMetrics] = None) -> dict:
    """train.py:106-169 on an EvalMetrics: ``batches`` yields (x, labels) with x what the model takes and labels the
    {'EX', 'AU', 'VA'} dict (EX already with -1 mapped to 7, train.py:125-126), all on the model's device; at most ``num_step``
    of them are consumed.  One ``update`` per batch and nothing that waits for the device inside the loop.  With ``group`` (or
    the default process group when ``group=True``) the states of all ranks are summed before scoring.  The model is left in
    train() mode, as the reference leaves it."""
    task = (task if task is not None else getattr(model, 'task', 'ALL')).upper()
    metrics = EvalMetrics() if metrics is None else metrics
    metrics.clear()
    model.eval()
    try:
        for step, (x, labels) in enumerate(batches):
            if step >= int(num_step):
                break
            result = model(x)
            if task == 'EX':
                loss = model.get_ex_loss(result, labels['EX'])
            elif task == 'AU':
                loss = model.get_au_loss(result, labels['AU'])
            elif task == 'VA':
                loss = model.get_va_loss(result, labels['VA'])
            else:
                losses = model.get_mt_loss(result, labels)
                loss = losses[0] + losses[1] + losses[2]
            metrics.update(result, labels, loss)
    finally:
        model.train()
    if group is not None:
        metrics.all_reduce(None if group is True else group)
    return metrics.scores()
