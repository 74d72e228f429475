"""Linear functionals of the logits, f(x) = sum_k c_k y_k(x), as the thing an explanation pass explains.

In explanation mode a B-cos network is linear in the head cotangent (bcos/common.py:163-181: scales, gates and variances are detached,
the LogitLayer bias is a constant), so the dynamic weights of f are W_f(x) = sum_k c_k W_k(x) and ONE input-gradient pass that starts from
c instead of a one-hot coordinate yields them (include/bcos_hip.h: bcos_head_rankm_grad, bcos_head_cotangent_grad).  The engines take a
`LogitFunctional` through `explain(x, functional=...)` and `explain_functionals(x, [f_1 ... f_T])`.

Non-linear functionals (a softmax probability, a loss) are out of scope: linearise them into a dense cotangent from the logits.
"""
from typing import Optional

import torch

from . import ops

__all__ = ["LogitFunctional"]


class LogitFunctional:
    """A value type: one functional per image of a batch.  Either SPARSE -- `classes` [N, J] int64 and `coeffs` [N, J] fp32, J <= 8 --
    or DENSE -- `cot` [N, K] fp32, the cotangent of the logits.  Tensors may live on the host or on the device; class indices given as
    lists or host tensors are validated without a device synchronisation (ops.check_functional_classes)."""

    __slots__ = ("classes", "coeffs", "cot")

    def __init__(self, classes=None, coeffs=None, cot=None):
        self.classes, self.coeffs, self.cot = classes, coeffs, cot

    # ---- constructors ------------------------------------------------------------------------------------------------------------
    @classmethod
    def sparse(cls, classes, coeffs) -> "LogitFunctional":
        """sum_j coeffs[n, j] * y[n, classes[n, j]]: `classes` [N, J] integers, `coeffs` [N, J], 1 <= J <= 8."""
        c = torch.as_tensor(classes)
        if c.dtype.is_floating_point or c.dtype == torch.bool or c.is_complex():
            raise TypeError(f"LogitFunctional.sparse: class indices must be integers, got {c.dtype}")
        w = torch.as_tensor(coeffs, dtype=torch.float32)
        if c.dim() != 2 or tuple(w.shape) != tuple(c.shape):
            raise ValueError(f"LogitFunctional.sparse: classes {tuple(c.shape)} and coeffs {tuple(w.shape)} must both be [N, J]")
        if not 1 <= c.shape[1] <= ops.HEAD_RANKM_MAX_TERMS:
            raise ValueError(f"LogitFunctional.sparse: {c.shape[1]} classes per image (1 .. {ops.HEAD_RANKM_MAX_TERMS}); use "
                             "LogitFunctional.dense for longer sums")
        return cls(classes=c.to(torch.int64), coeffs=w)

    @classmethod
    def dense(cls, cot) -> "LogitFunctional":
        """sum_k cot[n, k] * y[n, k]: `cot` [N, K]."""
        c = torch.as_tensor(cot, dtype=torch.float32)
        if c.dim() != 2:
            raise ValueError(f"LogitFunctional.dense: expected a cotangent [N, K], got {tuple(c.shape)}")
        return cls(cot=c)

    @classmethod
    def contrast(cls, pos, neg) -> "LogitFunctional":
        """y[n, pos[n]] - y[n, neg[n]]: why class `pos` rather than `neg`."""
        p, q = torch.as_tensor(pos).reshape(-1), torch.as_tensor(neg).reshape(-1)
        if p.numel() != q.numel():
            raise ValueError(f"LogitFunctional.contrast: {p.numel()} positive and {q.numel()} negative classes")
        q = q.to(p.device)
        return cls.sparse(torch.stack([p, q], 1), torch.tensor([1.0, -1.0]).expand(p.numel(), 2))

    @classmethod
    def mean_corrected(cls, targets, n_logits: int) -> "LogitFunctional":
        """y[n, t_n] - mean_k y[n, k], the explained output of OursRelative (explainers/ours.py:28-33): dense, onehot(t) - 1 / K."""
        t = ops.check_targets(torch.as_tensor(targets).reshape(-1), int(n_logits), "LogitFunctional.mean_corrected")
        cot = torch.full((t.numel(), int(n_logits)), -1.0 / int(n_logits), dtype=torch.float32, device=t.device)
        cot.scatter_add_(1, t.view(-1, 1), torch.ones((t.numel(), 1), dtype=torch.float32, device=t.device))
        return cls(cot=cot)

    # ---- what the engines read -----------------------------------------------------------------------------------------------------
    @property
    def is_sparse(self) -> bool:
        return self.cot is None

    def __len__(self) -> int:
        return int((self.classes if self.is_sparse else self.cot).shape[0])

    def checked(self, n_images: int, n_logits: int) -> "LogitFunctional":
        """The functional validated against a batch of `n_images` with `n_logits` logits: ValueError on a shape mismatch, IndexError
        where the reference's `out[0, idx]` would raise; negative class indices wrapped."""
        if len(self) != n_images:
            raise ValueError(f"LogitFunctional: {len(self)} rows for a batch of {n_images} images")
        if self.is_sparse:
            return LogitFunctional(classes=ops.check_functional_classes(self.classes, n_logits), coeffs=self.coeffs)
        if self.cot.shape[1] != n_logits:
            raise ValueError(f"LogitFunctional: a cotangent over {self.cot.shape[1]} logits for a head with {n_logits}")
        return self

    def __getitem__(self, rows: slice) -> "LogitFunctional":
        """the functional of a contiguous sub-batch"""
        if self.is_sparse:
            return LogitFunctional(classes=self.classes[rows], coeffs=self.coeffs[rows])
        return LogitFunctional(cot=self.cot[rows])

    def to(self, device) -> "LogitFunctional":
        mv = lambda t, dt: t.to(device=device, dtype=dt).contiguous()      # noqa: E731
        if self.is_sparse:
            return LogitFunctional(classes=mv(self.classes, torch.int64), coeffs=mv(self.coeffs, torch.float32))
        return LogitFunctional(cot=mv(self.cot, torch.float32))

    def as_dense(self, n_logits: int) -> torch.Tensor:
        """the cotangent [N, K] of the functional (a sparse one scattered; repeated classes add up)"""
        if not self.is_sparse:
            return self.cot
        cot = torch.zeros((len(self), int(n_logits)), dtype=torch.float32, device=self.classes.device)
        return cot.scatter_add_(1, self.classes, self.coeffs.to(cot.device))

    def value(self, logits: torch.Tensor) -> torch.Tensor:
        """sum_k c_k * logit_k per image, [N] (the `functional_value` the engines return)"""
        if self.is_sparse:
            return (logits.gather(1, self.classes) * self.coeffs).sum(1)
        return (logits * self.cot).sum(1)


def as_functional(f) -> Optional[LogitFunctional]:
    if f is None or isinstance(f, LogitFunctional):
        return f
    raise TypeError(f"expected a bcos_hip.functional.LogitFunctional, got {type(f).__name__}")
