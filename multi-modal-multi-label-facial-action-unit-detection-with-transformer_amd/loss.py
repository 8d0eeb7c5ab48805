"""The task losses of the reference (models/loss.py), computed by HIP kernels that write the value and the gradient in the
same launch.

``AULoss`` - pos-weighted BCE-with-logits over the 12 action units (loss.py:63-103), on its own kernel (``au_loss_kernel``).

``CrossEntropyEX`` / ``FocalLoss_Ori`` (expression, loss.py:398-466), ``DiceAULoss`` (loss.py:149-176), ``CCCLoss`` (valence /
arousal, loss.py:271-313) and ``MultiTaskLoss`` - the three of ``get_mt_loss`` (sformer.py:423-449) at once - share ONE
single-workgroup kernel (``task_loss_kernel``, csrc/task_loss.hip): the three column blocks of the model's ``[B, 21]`` row (AU
0..11, EX 12..18, VA 19..20) are disjoint, so one launch writes the three values and one ``[B, 21]`` gradient, and backward is
one launch that scales the blocks by the three incoming gradients.  A criterion used on its own is the same kernel with the
other label pointers null.  Every criterion also has ``forward_torch``: the same formulas in plain torch, which is what CPU
tensors get and what the tests evaluate in fp64."""
from __future__ import annotations

import torch
from torch import nn
from torch.nn import functional as F

from . import _lib, ops

# reference models/loss.py:73
AU_POS_WEIGHT = (1., 1., 1., 1., 1., 1., 1., 3., 3., 3., 1., 2.)


class _AULossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y_pred, y_true, pos_weight, ignore):
        if y_pred.stride(-1) != 1:
            y_pred = y_pred.contiguous()
        if y_true.stride(-1) != 1 or y_true.dtype != torch.float32:
            y_true = y_true.to(torch.float32).contiguous()
        loss, grad = ops.au_loss(y_pred.to(torch.float32), y_true, pos_weight, ignore)
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None, None, None


class _AULossSumFn(torch.autograd.Function):
    """(sum over kept rows of the row-mean BCE, kept rows): numerator and denominator of loss.py:85-102, kept apart so
    that a data-parallel wrapper can reduce both over the ranks before dividing"""

    @staticmethod
    def forward(ctx, y_pred, y_true, pos_weight, ignore):
        if y_pred.stride(-1) != 1:
            y_pred = y_pred.contiguous()
        if y_true.stride(-1) != 1 or y_true.dtype != torch.float32:
            y_true = y_true.to(torch.float32).contiguous()
        sc, grad = ops.au_loss_sum(y_pred.to(torch.float32), y_true, pos_weight, ignore)
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(sc[1])
        return sc[0], sc[1]

    @staticmethod
    def backward(ctx, g, _gk):
        (grad,) = ctx.saved_tensors
        return grad * g, None, None, None


class _AULossRowsFn(torch.autograd.Function):
    """AULoss on slots 0..11 of the model's [B, width] output rows, the gradient returned in that layout by the loss kernel itself
    (avf_au_loss_wide): ``loss(out[:, :12], y)`` costs autograd a fill and a copy for the slice on top of the loss's own launches"""

    @staticmethod
    def forward(ctx, out, y_true, pos_weight, ignore, sum_mode):
        if y_true.stride(-1) != 1 or y_true.dtype != torch.float32:
            y_true = y_true.to(torch.float32).contiguous()
        res, grad = ops.au_loss_wide(out, y_true, pos_weight, ignore, sum_mode)
        ctx.save_for_backward(grad)
        if sum_mode:
            ctx.mark_non_differentiable(res[1])
            return res[0], res[1]
        return res

    @staticmethod
    def backward(ctx, g, *_):
        (grad,) = ctx.saved_tensors
        return grad * g, None, None, None, None


class AULoss(nn.Module):
    """Rows whose FIRST label equals ``ignore`` are dropped (loss.py:85-88); the loss is the mean of
    ``BCEWithLogits(reduction='none', pos_weight=[1,1,1,1,1,1,1,3,3,3,1,2])`` over kept rows x 12.
    With every row dropped the result is NaN, exactly like the reference's mean over an empty tensor.
    Unlike the reference ctor (loss.py:73) this does not need a current CUDA device at construction:
    ``pos_weight`` is a buffer and follows ``.to(device)``."""

    def __init__(self, ignore=-1):
        super().__init__()
        self.ignore = ignore
        self.register_buffer("pos_weight", torch.tensor(AU_POS_WEIGHT, dtype=torch.float32), persistent=False)
        # set by dp.DataParallel: callable (local_sum, local_kept) -> global mean whose backward, AVERAGED over the ranks,
        # is the gradient of that global mean (ranks may hold different numbers of ignored rows).  It is a COLLECTIVE: it
        # is taken only for a training-mode loss with gradients enabled - the one call every rank makes once per step -
        # or when ``reduce_eval`` is set (then EVERY rank must call the loss the same number of times); a validation
        # loss on one rank, or on ranks with different batch counts, stays local and cannot deadlock.
        self.global_mean = None
        self.reduce_eval = False

    def forward_torch(self, y_pred, y_true):
        """the same loss in plain torch, in the dtype of ``y_pred``"""
        return _au_bce_torch(y_pred, y_true.to(y_pred.dtype), AU_POS_WEIGHT, self.ignore)

    def forward(self, y_pred, y_true):
        if not y_pred.is_cuda:
            raise RuntimeError("AULoss (HIP) needs its inputs on the MI355X; there is no CPU fallback")
        pw = self.pos_weight if self.pos_weight.device == y_pred.device else self.pos_weight.to(y_pred.device)
        if self.global_mean is not None and ((self.training and torch.is_grad_enabled()) or self.reduce_eval):
            s, k = _AULossSumFn.apply(y_pred, y_true, pw, float(self.ignore))
            return self.global_mean(s, k)
        return _AULossFn.apply(y_pred, y_true, pw, float(self.ignore))

    def forward_rows(self, out, y_true):
        """``self(out[:, :y_true.shape[1]], y_true)`` for a contiguous fp32 [B, width] output of the model, without the slice:
        same value, same gradient (zero in the other slots), two launches fewer in backward (the task models' get_au_loss)"""
        if not (out.is_cuda and out.dim() == 2 and out.dtype == torch.float32 and out.is_contiguous() and y_true.dim() == 2
                and out.shape[0] == y_true.shape[0] and out.shape[1] >= y_true.shape[1]):
            return self(out[:, :y_true.shape[1]], y_true)
        pw = self.pos_weight if self.pos_weight.device == out.device else self.pos_weight.to(out.device)
        if self.global_mean is not None and ((self.training and torch.is_grad_enabled()) or self.reduce_eval):
            s, k = _AULossRowsFn.apply(out, y_true, pw, float(self.ignore), True)
            return self.global_mean(s, k)
        return _AULossRowsFn.apply(out, y_true, pw, float(self.ignore), False)


# =====================================================================================================================
# EX / AU / VA on the fused kernel
# =====================================================================================================================
# the reference's output row (avformer.py:101-105, sformer.py:356): AU logits, EX logits, valence and arousal
AU_COL, EX_COL, VA_COL, ROW_WIDTH = 0, 12, 19, 21
NUM_EX, NUM_AU = 7, 12
# reference models/loss.py:154
DICE_AU_POS_WEIGHT = (1., 2., 1., 1., 1., 1., 1., 6., 6., 5., 1., 5.)


def _au_bce_torch(z, y, pos_weight, ignore):
    keep = y[:, 0] != ignore
    pw = torch.tensor(pos_weight, dtype=z.dtype, device=z.device)
    return F.binary_cross_entropy_with_logits(z[keep], y[keep], pos_weight=pw, reduction='none').mean()


def _ccc_torch(x, y, ignore):
    """1 - 2 s_xy / ((var_x + var_y + (m_x - m_y)^2 + 1e-8) * B): s_xy a SUM over the rows that are left, the variances
    unbiased, B the batch size before rows labelled ``ignore`` are dropped; 0 without a gradient when at most one row is left"""
    batch = x.shape[0]
    keep = y != ignore
    x, y = x[keep], y[keep]
    if y.shape[0] <= 1:
        return (x * 0).sum()
    mx, my = x.mean(), y.mean()
    s_xy = ((x - mx) * (y - my)).sum()
    den = x.var(unbiased=True) + y.var(unbiased=True) + (mx - my) ** 2 + 1e-8
    return 1 - 2 * s_xy / (den * batch)


def _prep(t, dtype):
    if t is None:
        return None
    if t.dtype != dtype:
        t = t.to(dtype)
    return t if t.stride(-1) == 1 or t.shape[-1] == 1 else t.contiguous()


class _TaskLossFn(torch.autograd.Function):
    """(out [rows, width], y_ex | None, y_au | None, y_va | None, cfg) -> (loss_ex, loss_au, loss_va, counts [3]): one launch
    forward (avf_task_loss), one launch backward (avf_task_loss_bwd).  The loss of a task without labels is 0."""

    @staticmethod
    def forward(ctx, out, y_ex, y_au, y_va, cfg):
        if out.dtype != torch.float32 or out.stride(1) != 1:
            out = out.to(torch.float32).contiguous()
        y_ex = None if y_ex is None else _prep(y_ex.reshape(-1), torch.int64).contiguous()
        losses, counts, grad = ops.task_loss(out, y_ex, _prep(y_au, torch.float32), _prep(y_va, torch.float32), cfg)
        ctx.save_for_backward(grad)
        ctx.cfg, ctx.live = cfg, (y_ex is not None, y_au is not None, y_va is not None)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(counts)
        l_ex, l_au, l_va = losses.unbind(0)
        return l_ex, l_au, l_va, counts

    @staticmethod
    def backward(ctx, g_ex, g_au, g_va, _g_counts):
        (grad,) = ctx.saved_tensors
        gs = [g.to(torch.float32) if (g is not None and on) else None for g, on in zip((g_ex, g_au, g_va), ctx.live)]
        return ops.task_loss_bwd(grad, gs[0], gs[1], gs[2], ctx.cfg), None, None, None, None


def _new_cfg(ex_col=EX_COL, au_col=AU_COL, va_col=VA_COL, va_ncols=2, va_tanh=True, va_weights=(1.0, 1.0), va_ignore=-5.0,
             normalize=False):
    c = _lib.TaskLossCfg()
    c.ex_col, c.au_col, c.va_col, c.va_ncols, c.va_tanh, c.normalize = ex_col, au_col, va_col, va_ncols, int(va_tanh), int(normalize)
    c.va_ignore = float(va_ignore)
    c.va_weight[0], c.va_weight[1] = float(va_weights[0]), float(va_weights[1])
    c.au_ignore, c.gamma, c.smooth = -1.0, 2.0, 1e-4
    return c


class _RowCriterion(nn.Module):
    """a criterion of the fused kernel: ``_fill(cfg)`` writes its settings into an avf_task_loss_cfg"""

    def _cfg(self, key, **kw):
        cache = self.__dict__.setdefault("_cfgs", {})
        if key not in cache:
            cache[key] = self._fill(_new_cfg(**kw))
        return cache[key]


class CrossEntropyEX(_RowCriterion):
    """``nn.CrossEntropyLoss(weight=weight, ignore_index=ignore_index)`` over the 7 expression classes, as ``sformer`` /
    ``vformer`` / ``tformer`` build their ``loss_EX`` (sformer.py:359).  Every row ignored: NaN with a zero gradient."""

    def __init__(self, weight=None, ignore_index=7):
        super().__init__()
        self.weight = tuple(float(w) for w in weight) if weight is not None else (1.0,) * NUM_EX
        if len(self.weight) != NUM_EX:
            raise ValueError(f"CrossEntropyEX is built for the {NUM_EX} expression classes")
        self.ignore_index = ignore_index

    def _fill(self, c):
        c.ex_mode = _lib.EX_CROSS_ENTROPY
        c.ex_use_ignore, c.ex_ignore = int(self.ignore_index is not None), int(self.ignore_index or 0)
        for i, w in enumerate(self.weight):
            c.ex_weight[i] = w
        return c

    def forward_torch(self, logit, target):
        w = torch.tensor(self.weight, dtype=logit.dtype, device=logit.device)
        return F.cross_entropy(logit, target.reshape(-1), weight=w, ignore_index=-100 if self.ignore_index is None else self.ignore_index)

    def forward(self, logit, target):
        """logit [N, 7], target [N]"""
        if not logit.is_cuda:
            return self.forward_torch(logit, target)
        return _TaskLossFn.apply(logit, target, None, None, self._cfg("alone", ex_col=0))[0]

    def forward_rows(self, out, target):
        """``self(out[:, 12:19], target)`` on the model's [B, 21] rows without the slice"""
        if not out.is_cuda:
            return self.forward_torch(out[:, EX_COL:EX_COL + NUM_EX], target)
        return _TaskLossFn.apply(out, target, None, None, self._cfg("rows"))[0]


class FocalLoss_Ori(CrossEntropyEX):
    """loss.py:398-466 with its constructor: ``-alpha (1 - p)^gamma log p`` on ``p = softmax(logit)[target] + 1e-4``.  With an
    ``ignore_index`` the ignored rows gather class 0 and are masked, and 'mean' is sum / (rows x valid rows) (loss.py:460-463);
    no valid row gives NaN.  Built for ``num_class=7`` and ``reduction='mean'``, what ``avformer`` uses (avformer.py:89)."""

    def __init__(self, num_class, alpha=None, gamma=2, ignore_index=None, reduction='mean'):
        if num_class != NUM_EX or reduction != 'mean':
            raise ValueError(f"FocalLoss_Ori is built for num_class={NUM_EX} and reduction='mean'")
        if alpha is None:
            alpha = (1.0,) * num_class
        elif isinstance(alpha, (int, float)):
            alpha = (float(alpha),) * num_class
        if len(alpha) != num_class:
            raise RuntimeError('the length not equal to number of class')
        super().__init__(weight=alpha, ignore_index=ignore_index)
        self.num_class, self.gamma, self.reduction, self.smooth = num_class, gamma, reduction, 1e-4
        self.alpha = torch.tensor(self.weight)

    def _fill(self, c):
        super()._fill(c)
        c.ex_mode, c.gamma, c.smooth = _lib.EX_FOCAL, float(self.gamma), float(self.smooth)
        return c

    def forward_torch(self, logit, target):
        target = target.reshape(-1)
        alpha = self.alpha.to(device=logit.device, dtype=logit.dtype)
        valid = None
        if self.ignore_index is not None:
            valid = target != self.ignore_index
            target = target * valid
        p = torch.softmax(logit, dim=1).gather(1, target[:, None]).view(-1) + self.smooth
        loss = -alpha[target] * (1.0 - p) ** self.gamma * torch.log(p)
        if valid is None:
            return loss.mean()
        return (loss * valid).mean() / valid.sum()


class DiceAULoss(_RowCriterion):
    """loss.py:149-176: rows whose FIRST label equals ``ignore`` are dropped; the sum over the 12 units of the Dice loss
    ``1 - (2 sum p y + 1) / (sum p + sum y + 1)`` on ``p = sigmoid(logit)`` - unweighted: the reference hands ``pos_weight`` to
    ``MultiLabelDiceLoss`` as ``weight=``, which its ``**kwargs`` swallows - plus 5 x the mean pos-weighted BCE-with-logits.
    Every row dropped: NaN with a zero gradient."""

    def __init__(self, ignore=-1, pos_weight=DICE_AU_POS_WEIGHT):
        super().__init__()
        self.ignore = ignore
        self.pos_weight = tuple(float(w) for w in pos_weight)
        if len(self.pos_weight) != NUM_AU:
            raise ValueError(f"DiceAULoss is built for the {NUM_AU} action units")

    def _fill(self, c):
        c.au_mode, c.au_ignore = _lib.AU_DICE_BCE, float(self.ignore)
        for i, w in enumerate(self.pos_weight):
            c.pos_weight[i] = w
        return c

    def forward_torch(self, y_pred, y_true):
        y_true = y_true.to(y_pred.dtype)
        keep = y_true[:, 0] != self.ignore
        p, y = torch.sigmoid(y_pred[keep]), y_true[keep]
        dice = (1 - (2. * (p * y).sum(0) + 1.) / (p.sum(0) + y.sum(0) + 1.)).sum()
        return dice + 5 * _au_bce_torch(y_pred, y_true, self.pos_weight, self.ignore)

    def forward(self, y_pred, y_true):
        """y_pred, y_true [N, 12]"""
        if not y_pred.is_cuda:
            return self.forward_torch(y_pred, y_true)
        return _TaskLossFn.apply(y_pred, None, y_true, None, self._cfg("alone", au_col=0))[1]

    def forward_rows(self, out, y_true):
        """``self(out[:, :12], y_true)`` on the model's [B, 21] rows without the slice"""
        if not out.is_cuda:
            return self.forward_torch(out[:, :NUM_AU], y_true)
        return _TaskLossFn.apply(out, None, y_true, None, self._cfg("rows"))[1]


class _AUBCE(_RowCriterion):
    """settings of an ``AULoss`` for the fused kernel (the module itself keeps its own kernel and its data-parallel mean)"""

    def __init__(self, au_loss: AULoss):
        super().__init__()
        self.ignore, self.pos_weight = au_loss.ignore, AU_POS_WEIGHT

    def _fill(self, c):
        DiceAULoss._fill(self, c)
        c.au_mode = _lib.AU_BCE
        return c

    def forward_torch(self, y_pred, y_true):
        return _au_bce_torch(y_pred, y_true.to(y_pred.dtype), self.pos_weight, self.ignore)


class CCCLoss(_RowCriterion):
    """loss.py:271-313, Lin's concordance correlation coefficient as the reference computes it: labels equal to ``ignore`` are
    dropped; unbiased variances; the covariance term is a sum, divided by the batch size counted BEFORE the drop; at most one
    row left gives 0 without a gradient."""

    def __init__(self, ignore=-5.0):
        super().__init__()
        self.ignore = ignore

    def _fill(self, c):
        c.va_ignore = float(self.ignore)
        return c

    def forward_torch(self, y_pred, y_true):
        return _ccc_torch(y_pred, y_true.to(y_pred.dtype), self.ignore)

    def forward(self, y_pred, y_true):
        """y_pred, y_true [N]"""
        if not y_pred.is_cuda:
            return self.forward_torch(y_pred, y_true)
        cfg = self._cfg("alone", va_col=0, va_ncols=1, va_tanh=False, va_weights=(1.0, 0.0))
        return _TaskLossFn.apply(y_pred.contiguous()[:, None], None, None, y_true.contiguous()[:, None], cfg)[2]

    def forward_rows_torch(self, out, y_true, weights=(1.0, 1.0)):
        v, a = torch.tanh(out[:, VA_COL]), torch.tanh(out[:, VA_COL + 1])
        return weights[0] * self.forward_torch(v, y_true[:, 0]) + weights[1] * self.forward_torch(a, y_true[:, 1])

    def forward_rows(self, out, y_true, weights=(1.0, 1.0)):
        """``weights[0] * self(tanh(out[:, 19]), y_true[:, 0]) + weights[1] * self(tanh(out[:, 20]), y_true[:, 1])`` on the
        model's [B, 21] rows (the models' get_va_loss: avformer.py:119-123), the tanh and its derivative inside the kernel"""
        if not out.is_cuda:
            return self.forward_rows_torch(out, y_true, weights)
        cfg = self._cfg(("rows", float(weights[0]), float(weights[1])), va_weights=weights)
        return _TaskLossFn.apply(out, None, None, y_true, cfg)[2]


class MultiTaskLoss(nn.Module):
    """``[loss_ex, loss_au, loss_va]`` of ``get_mt_loss`` (sformer.py:423-449) on the model's [B, 21] rows from ONE launch, with a
    one-launch backward.  ``loss_EX``: ``CrossEntropyEX`` or ``FocalLoss_Ori``; ``loss_AU``: ``AULoss`` or ``DiceAULoss``;
    ``loss_VA``: ``CCCLoss``, applied as ``va_weights[0] * CCC(tanh valence) + va_weights[1] * CCC(tanh arousal)``.
    A label that is ``None`` leaves its task out (loss 0, no gradient).  ``normalize=True`` divides each loss by its count of
    valid labels - EX rows, AU labels != ignore, VA labels != ignore - inside the kernel, 0 for a count of 0; the reference
    counts on the host through numpy.  The values are those of the three criteria called one by one, bit for bit."""

    def __init__(self, loss_EX=None, loss_AU=None, loss_VA=None, va_weights=(1.0, 1.0)):
        super().__init__()
        self.loss_EX = loss_EX if loss_EX is not None else CrossEntropyEX(ignore_index=7)
        self.loss_AU = loss_AU if loss_AU is not None else AULoss()
        self.loss_VA = loss_VA if loss_VA is not None else CCCLoss()
        if not isinstance(self.loss_EX, CrossEntropyEX) or not isinstance(self.loss_AU, (AULoss, DiceAULoss)) \
                or not isinstance(self.loss_VA, CCCLoss):
            raise TypeError("MultiTaskLoss takes CrossEntropyEX / FocalLoss_Ori, AULoss / DiceAULoss and CCCLoss")
        self.va_weights = (float(va_weights[0]), float(va_weights[1]))
        self._cfgs = {}

    def _au(self):
        return self.loss_AU if isinstance(self.loss_AU, DiceAULoss) else _AUBCE(self.loss_AU)

    def _cfg(self, normalize):
        if normalize not in self._cfgs:
            c = _new_cfg(va_weights=self.va_weights, normalize=normalize)
            self._cfgs[normalize] = self.loss_VA._fill(self._au()._fill(self.loss_EX._fill(c)))
        return self._cfgs[normalize]

    def forward_torch(self, out, y_ex=None, y_au=None, y_va=None, normalize=False):
        zero = (out * 0).sum()
        res = [zero if y_ex is None else self.loss_EX.forward_torch(out[:, EX_COL:EX_COL + NUM_EX], y_ex),
               zero if y_au is None else self._au().forward_torch(out[:, :NUM_AU], y_au),
               zero if y_va is None else self.loss_VA.forward_rows_torch(out, y_va.to(out.dtype), self.va_weights)]
        if normalize:
            ign = self.loss_EX.ignore_index
            counts = [None if y_ex is None else (y_ex != ign).sum() if ign is not None else torch.tensor(y_ex.numel()),
                      None if y_au is None else (y_au != self.loss_AU.ignore).sum(),
                      None if y_va is None else (y_va != self.loss_VA.ignore).sum()]
            # (reads the counts on the host, as the reference does; the kernel form does not)
            res = [l if c is None else (l / c if int(c) > 0 else zero) for l, c in zip(res, counts)]
        return res

    def forward(self, out, y_ex=None, y_au=None, y_va=None, normalize=False):
        if not out.is_cuda:
            return self.forward_torch(out, y_ex, y_au, y_va, normalize)
        return list(_TaskLossFn.apply(out, y_ex, y_au, y_va, self._cfg(bool(normalize)))[:3])
