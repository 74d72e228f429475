"""Torch interpreters of the two head entry points for linear functionals of the logits (TEST INFRASTRUCTURE, beside cpu_emulation.py):
what include/bcos_hip.h documents for bcos_head_rankm_grad and bcos_head_cotangent_grad in plain fp32, and the float64 evaluation of the
same formulas with the magnitudes the rounding bounds of tests/test_head_functional_gpu.py are built from.  The `-m "not gpu"` tests
monkeypatch bcos_hip.ops with the first two on top of cpu_emulation.install."""
import torch


def _terms(cls, coef, scale, w, inv_t, row_scale, dtype):
    """per-term factors a_j [N, R, J] (zero for a class outside [0, K)) and weight rows [N, J, D]"""
    N, R, K = scale.shape
    cls = cls.long()
    ok = (cls >= 0) & (cls < K)
    k = torch.where(ok, cls, torch.zeros_like(cls))
    c = torch.tensor(inv_t, dtype=torch.float32).to(dtype) / R              # (fp64: the exact quotient of the fp32 argument; fp32: rounded once)
    s = torch.gather(scale.to(dtype), 2, k.view(N, 1, -1).expand(N, R, -1))          # [N, R, J]
    a = c.to(scale.device) * s
    if row_scale is not None:
        a = a * row_scale.to(dtype).view(N, R, 1)
    a = a * coef.to(dtype).view(N, 1, -1)
    a = torch.where(ok.view(N, 1, -1), a, torch.zeros_like(a))
    return a, w.to(dtype)[k]


def _outputs(v, mul, want_out2, mul2, gate2, gate2_from_mul, want_absmax2):
    out = v * mul.reshape(v.shape).to(v.dtype) if mul is not None else v
    out2 = None
    if want_out2 or mul2 is not None or gate2 is not None or gate2_from_mul or want_absmax2:
        out2 = v * mul2.reshape(v.shape).to(v.dtype) if mul2 is not None else v
        if gate2_from_mul:
            out2 = out2 * (mul.reshape(v.shape).contiguous().view(torch.int32) & 1).to(out2.dtype)
        elif gate2 is not None:
            out2 = out2 * (gate2.reshape(v.shape) > 0).to(out2.dtype)
    return out, out2


def head_rankm_grad(cls, coef, scale, w, temperature=None, row_scale=None, mul=None, want_out2=False, want_absmax=False, mul2=None,
                    gate2=None, gate2_from_mul=False, want_absmax2=False):
    """ops.head_rankm_grad in fp32: v = sum_j a_j * w[cls_j] as one chain in ascending j"""
    N, R, K = scale.shape
    a, rows = _terms(cls, coef, scale, w, 1.0 if temperature is None else 1.0 / float(temperature), row_scale, torch.float32)
    v = a[:, :, 0, None] * rows[:, None, 0]
    for j in range(1, a.shape[2]):
        v = v + a[:, :, j, None] * rows[:, None, j]
    return _outputs(v.reshape(N * R, -1), mul, want_out2, mul2, gate2, gate2_from_mul, want_absmax2)


def head_rankm_grad64(cls, coef, scale, w, temperature=None, row_scale=None):
    """-> (v, sum_j |term_j|) in float64, [N R, D] each"""
    N, R, K = scale.shape
    a, rows = _terms(cls, coef, scale, w, 1.0 if temperature is None else 1.0 / float(temperature), row_scale, torch.float64)
    t = a.unsqueeze(-1) * rows.unsqueeze(1)                      # [N, R, J, D]
    return t.sum(2).reshape(N * R, -1), t.abs().sum(2).reshape(N * R, -1)


def head_cotangent_grad(cot, scale, temperature=None, want_absmax=True):
    """ops.head_cotangent_grad in fp32: (cot * scale) * (inv_t / R), K padded to a multiple of 4 with zeros"""
    N, K = scale.shape[0], scale.shape[-1]
    R = scale.numel() // (N * K)
    c = torch.tensor(1.0 if temperature is None else 1.0 / float(temperature), dtype=torch.float32) / R
    g = (cot.view((N,) + (1,) * (scale.dim() - 2) + (K,)) * scale) * c
    return torch.nn.functional.pad(g, (0, (-K) % 4))


def head_cotangent_grad64(cot, scale, temperature=None):
    N, K = scale.shape[0], scale.shape[-1]
    R = scale.numel() // (N * K)
    c = torch.tensor(1.0 if temperature is None else 1.0 / float(temperature), dtype=torch.float32).double() / R
    return cot.double().view((N,) + (1,) * (scale.dim() - 2) + (K,)) * scale.double() * c


def install(monkeypatch):
    """the two emulators over bcos_hip.ops (after cpu_emulation.install)"""
    from bcos_hip import ops
    monkeypatch.setattr(ops, "head_rankm_grad", head_rankm_grad)
    monkeypatch.setattr(ops, "head_cotangent_grad", head_cotangent_grad)
