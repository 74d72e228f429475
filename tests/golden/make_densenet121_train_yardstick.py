"""A float64 yardstick for one training step at DenseNet-121 DEPTH, by RUNNING THE REFERENCE on CPU (beside make_golden_densenet_train.py).

Run in the build container only:   python tests/golden/make_densenet121_train_yardstick.py OUT.npz [batch, default 4]

The reference's DenseNetBcos (D121 spec, weight seed 0) inside the reference's BcosifyNetwork, calibrated on 8 images of 224 x 224
(synth.calibrate, seed 123), then ONE train()-mode BCE step of the float64 copy on `batch` images (seed 1000, labels 37 n mod 1000).
OUT.npz holds the calibrated state dict (`state/<name>`, fp32: what both fp32 paths start from), the float64 step's output and every
parameter gradient cast to fp32 (`grad/<name>`) with its float64 norm.  64 MB: NOT a committed fixture --
scripts/densenet_train_bench.py --yardstick OUT.npz measures the distance of the fused plan and of the per-layer path from it.
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_densenet as MG  # noqa: E402

synth = MG.synth


def main(out, batch=4):
    net = MG.reference_densenet(MG.D121, seed=0)
    with torch.no_grad():
        synth.calibrate(net, synth.synthetic_images(8, seed=123, size=224))
    arrays = {"state/" + k: v.detach().numpy().copy() for k, v in net.state_dict().items()}
    x = synth.synthetic_images(batch, seed=1000, size=224)
    target = torch.nn.functional.one_hot(torch.arange(batch) * 37 % 1000, 1000)
    n64 = copy.deepcopy(net).double().train()
    res = n64(x.double())
    loss = torch.nn.functional.binary_cross_entropy_with_logits(res, target.double())
    named = [(n, p) for n, p in n64.named_parameters() if p.requires_grad]
    grads = torch.autograd.grad(loss, [p for _, p in named])
    arrays.update(output=res.detach().numpy(), loss=loss.detach().numpy(), batch=np.array(batch),
                  grad_norms=np.array([float(g.norm()) for g in grads]))
    arrays.update({"grad/" + n: g.float().numpy() for (n, _), g in zip(named, grads)})
    np.savez(out, **arrays)
    print("written", out, os.path.getsize(out), "bytes; loss", float(loss))


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 4)
