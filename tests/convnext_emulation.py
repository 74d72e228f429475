"""Plain-torch fp64 restatement of the launch list of a B-cos ConvNeXt (bcos/models/convnext.py) from its state dict: the forward pass
launch by launch with what each launch keeps, and the explanation pass as the explicit reverse walk over what was kept -- no autograd.

Launches (NCHW tensors here; the layout is not part of the arithmetic):
    conv     y = s lin, lin = conv(x, w / ||w||), s = |lin| / sqrt(sum_patch x^2 + 1e-6); kept: s.        gradient: conv^T(s g)
    dw       the same with one filter and one patch norm per channel (7x7, padding 3); kept: s.          gradient: addend + dw^T(s g)
    pn       y = weight (x - mean_c x) rstd, rstd = 1 / sqrt(var_c x + eps); kept: rstd.                 gradient: h - mean_c h, h = g weight rstd
    block    dw -> pn -> conv 1x1 (C -> 4C) -> conv 1x1 (4C -> C) with ch_scale = layer_scale and addend = block input in its epilogue
    head     pn -> conv 1x1 to the classes -> mean over the positions -> + logit_bias
The reverse pass starts from the one-hot cotangent of the explained class spread over the positions (1 / HW each); a block's input
gradient is complete when its depthwise gradient launch ends (the residual gradient is that launch's addend).
"""
import torch
import torch.nn.functional as F


def _unit(w):
    return w / w.flatten(1).norm(dim=1).view(-1, 1, 1, 1)


class Conv:
    def __init__(self, w, stride=1, padding=0, groups=1):
        self.w, self.stride, self.padding, self.groups = _unit(w.double()), stride, padding, groups

    def fwd(self, x):
        lin = F.conv2d(x, self.w, stride=self.stride, padding=self.padding, groups=self.groups)
        k = self.w.shape[2]
        sq = x * x if self.groups > 1 else (x * x).sum(1, keepdim=True)
        ones = torch.ones((sq.shape[1], 1, k, k), dtype=x.dtype)
        norm = (F.conv2d(sq, ones, stride=self.stride, padding=self.padding, groups=sq.shape[1]) + 1e-6).sqrt()
        self.scale = lin.abs() / norm
        self.in_hw = x.shape[2:]
        return self.scale * lin

    def bwd(self, g, addend=None):
        gl = g * self.scale
        hw = self.in_hw
        k = self.w.shape[2]
        out_pad = [(hw[i] + 2 * self.padding - k) % self.stride for i in range(2)]
        gx = F.conv_transpose2d(gl, self.w, stride=self.stride, padding=self.padding, output_padding=out_pad, groups=self.groups)
        return gx if addend is None else addend + gx


class PositionNorm:
    def __init__(self, weight, eps=1e-6):
        self.weight, self.eps = weight.double().view(1, -1, 1, 1), eps

    def fwd(self, x):
        mean = x.mean(1, keepdim=True)
        var = ((x - mean) ** 2).mean(1, keepdim=True)
        self.rstd = 1.0 / (var + self.eps).sqrt()
        return self.weight * (x - mean) * self.rstd

    def bwd(self, g):
        h = g * self.weight * self.rstd
        return h - h.mean(1, keepdim=True)


class Block:
    def __init__(self, sd, prefix):
        C = sd[prefix + "layer_scale"].shape[0]
        self.dw = Conv(sd[prefix + "block.0.linear.weight"], padding=3, groups=C)
        self.pn = PositionNorm(sd[prefix + "block.1.weight"])
        self.c1 = Conv(sd[prefix + "block.2.linear.weight"])
        self.c2 = Conv(sd[prefix + "block.3.linear.weight"])
        self.ls = sd[prefix + "layer_scale"].double().view(1, C, 1, 1)

    def fwd(self, x):
        return x + self.ls * self.c2.fwd(self.c1.fwd(self.pn.fwd(self.dw.fwd(x))))

    def bwd(self, g):
        gb = self.pn.bwd(self.c1.bwd(self.c2.bwd(g * self.ls)))
        return self.dw.bwd(gb, addend=g)


class Plan:
    """launch list of the network with the given block setting [(C_in, C_out or None, blocks), ...]"""

    def __init__(self, sd, block_setting, logit_bias):
        self.layers = [Conv(sd["features.0.linear.weight"], stride=4), PositionNorm(sd["features.1.weight"])]
        k = 2
        for cin, cout, n in block_setting:
            self.layers += [Block(sd, f"features.{k}.{j}.") for j in range(n)]
            k += 1
            if cout is not None:
                self.layers += [PositionNorm(sd[f"features.{k}.0.weight"]), Conv(sd[f"features.{k}.1.linear.weight"], stride=2)]
                k += 1
        self.layers += [PositionNorm(sd["classifier.0.weight"]), Conv(sd["classifier.1.linear.weight"])]
        self.logit_bias = logit_bias

    def forward(self, x):
        for layer in self.layers:
            x = layer.fwd(x)
        self.head_shape = x.shape
        return x.mean((2, 3)) + self.logit_bias

    def explain(self, x, targets=None):
        """-> logits, prediction, W(x) = d logit[target] / d x with scales and variances constant, contribution map"""
        x = x.double()
        logits = self.forward(x)
        pred = logits.argmax(1)
        idx = pred if targets is None else targets
        N, K, H, W = self.head_shape
        g = torch.zeros(self.head_shape, dtype=torch.float64)
        g[torch.arange(N), idx] = 1.0 / (H * W)
        for layer in reversed(self.layers):
            g = layer.bwd(g)
        return dict(logits=logits, prediction=pred, weights=g, contribution_map=(x * g).sum(1))
