"""Generate the SigLIP distillation-loss fixtures under tests/golden/ by RUNNING THE REFERENCE's SigLipLoss (bcos/modules/losses.py:576-694)
on CPU, with the normalisation applied outside as its training step does (bcos/training/trainer.py:673-674).  Build container only:
    python tests/golden/make_golden_siglip.py

  siglip.{json,npz}   per case of tests/siglip_emulation.py: CASES, in fp32 and in fp64 (the fp32 inputs widened): the loss, the gradients
                      w.r.t. the RAW student and teacher features (through F.normalize), w.r.t. the logit scale's logarithm (through
                      .exp(), as model.logit_scale) and w.r.t. the bias, and the reference's own fp32-vs-fp64 distance of each of them
                      (loss: relative; a gradient: largest difference over the largest magnitude).  The inputs are seeded
                      (siglip_emulation.case_inputs; a checksum is recorded); feature gradients of more than FULL_MAX elements are recorded
                      on a few rows, with the norm of every row.  The two-rank cases are the reference's _loss on the local block plus
                      _loss(..., negative_only=True) on the other rank's block, which is what its forward sums for world_size = 2.
                      Also: the parameter names and defaults of the reference's constructor and forward.
"""
import importlib
import inspect
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from oracle import refimport  # noqa: E402

refimport.setup()
RL = importlib.import_module("bcos.modules.losses")

import siglip_emulation as SE  # noqa: E402


def run_reference(case, dtype):
    s, t, log_scale, bias = SE.case_inputs(case)
    s, t = s.to(dtype).requires_grad_(True), t.to(dtype).requires_grad_(True)
    log_scale, bias = log_scale.to(dtype).requires_grad_(True), bias.to(dtype).requires_grad_(True)
    crit = RL.SigLipLoss()
    crit.set_explanation_mode(case["detach"])
    us, ut = F.normalize(s, dim=-1), F.normalize(t, dim=-1)
    scale = log_scale.exp()
    if "world" in case:
        n, r = case["N"], case["rank"]
        loss = crit._loss(us, ut[r * n:(r + 1) * n], scale, bias)
        for other in range(case["world"]):
            if other != r:
                loss = loss + crit._loss(us, ut[other * n:(other + 1) * n], scale, bias, negative_only=True)
    else:
        loss = crit(us, ut, scale, bias, output_dict=False, cos_scaling=case["p"])
    gs, gt, gls, gb = torch.autograd.grad(loss, (s, t, log_scale, bias))
    return dict(loss=loss.detach(), gs=gs, gt=gt, glogscale=gls, gbias=gb)


def distance(a, b, relative_to_max=True):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def signature_of(fn):
    return [[n, None if p.default is inspect.Parameter.empty else p.default] for n, p in inspect.signature(fn).parameters.items() if n != "self"]


def main():
    out, meta = {}, dict(cases=[], full_max=SE.FULL_MAX, torch_version=torch.__version__,
                         signature=dict(init=signature_of(RL.SigLipLoss.__init__), forward=signature_of(RL.SigLipLoss.forward)))
    for case in SE.CASES:
        name = case["name"]
        r32, r64 = run_reference(case, torch.float32), run_reference(case, torch.float64)
        s, t, _, _ = SE.case_inputs(case)
        d_ref = {k: distance(r32[k], r64[k]) for k in r32}
        for tag, res in (("f32", r32), ("f64", r64)):
            for k in ("loss", "glogscale", "gbias"):
                out[f"{name}/{tag}/{k}"] = res[k]
            for k in ("gs", "gt"):
                g = res[k].reshape(-1, case["D"])
                if g.numel() <= SE.FULL_MAX:
                    out[f"{name}/{tag}/{k}"] = g
                else:
                    out[f"{name}/{tag}/{k}_rows"] = g[SE.keep_rows(g.shape[0])]
                    out[f"{name}/{tag}/{k}_norms"] = g.norm(dim=1)
                out[f"{name}/{tag}/{k}_absmax"] = g.abs().max()
        meta["cases"].append(dict(case, d_ref=d_ref, checksum=[float(s.double().sum()), float(t.double().abs().sum())]))
        print(name, {k: f"{v:.1e}" for k, v in d_ref.items()}, float(r64["loss"]))
    np.savez_compressed(os.path.join(HERE, "siglip.npz"), **{k: v.detach().numpy() for k, v in out.items()})
    with open(os.path.join(HERE, "siglip.json"), "w") as f:
        json.dump(meta, f, indent=1)


if __name__ == "__main__":
    main()
