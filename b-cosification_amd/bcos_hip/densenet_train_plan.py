"""Training step of a B-cosified DenseNet as ONE launch plan (the fine-tuning side of bcos_hip/densenet_engine.py).

`net.train(); net(x)` on a network with an attached DenseNetEngine is one autograd node (train_plan._TrainStepFn) whose forward and
backward walk the engine's layer list.  The convolution units -- contraction with the dynamic scale NOT detached, BatchNormUncentered2d
behind it with batch statistics, ReLU; scale derivative, patch-norm term, ordered weight gradient on the side stream, input gradient --
are train_plan.ResNetTrainPlan's (`_unit_fwd` / `_unit_bwd`).  What is new is the pre-activation order of the topology (torchvision
_DenseLayer.norm1, _Transition.norm, norm5 on cat(features); reference standard_models.py:56-63, batchnorm_uncentered.py:36-44):

  forward   one RAW buffer X per dense block, as in the inference plan; nothing is concatenated.  When a channel slice of X is complete
            (slice 0: the pooled tensor placed; slice l: conv2 of layer l placed) bcos_slice_batch_stats runs on THAT slice and writes its
            range of the block's (mean, var) vectors.  Every reader of the concatenation sees the same columns, so its batch variance of a
            channel is the same number: a reader takes its channels from the block's vectors and adds its own weight / eps / momentum /
            running_var in one launch (bcos_bn_reader_finish) -- O(L) statistics reads instead of O(L^2) --, then bcos_slice_affine_rows
            (g, shift, ReLU) makes the dense operand of its 1 x 1 convolution.
  backward  one gradient buffer G per block.  The first reader handled (head / transition) covers every channel and WRITES G
            (bcos_slice_bn_bwd_acc, accumulate = 0).  Per layer, last to first: G[slice_l] gathered, conv2's unit, conv1's unit, then
            bcos_slice_relu_bwd_colsums (the ReLU gate rebuilt from X with the forward's rounding; norm1's weight / bias gradients and the
            variance-term coefficient from its finish; no per-element tensor) and bcos_slice_bn_bwd_acc(accumulate = 1) into G[:, :C_l].

A norm in eval() inside net.train() (frozen statistics) or with `detach` set has no variance term and leaves its running_var alone.
Scope: what DenseNetEngine attaches, minus dropout inside the dense layers, a learnable exponent and native unit-norm layers
(`supported()`; the per-layer path keeps working).  Kept for the backward pass: X, the block's mean vector, every reader's (g, rstd),
and per convolution unit what ResNetTrainPlan keeps -- the dense pre-activation operands included (conv1's weight gradient and
patch-norm term read them).  Weight banks still come from one preparation per layer, not from ops.WeightPrepBatch; conv2's output is
written dense (its scale is kept, which the epilogue writes at the output's own pitch) and placed into its slice by one more launch.
The step's forward and input-gradient contractions run with f32 products (`CONTRACTION` below).
"""
from typing import Dict, List

import torch
import torch.nn as nn

from . import ops
from .lib import BcosHipError
from .train_plan import ResNetTrainPlan


def _uses_batch_stats(bn) -> bool:
    return bn.training or (bn.running_mean is None and bn.running_var is None)


class _PreState:
    """what the backward pass of one pre-activation needs: the reader's norm, its g = weight / std, 1 / std and shift"""
    __slots__ = ("bn", "g", "rstd", "shift", "batch_stats")


class DenseNetTrainPlan(ResNetTrainPlan):
    @staticmethod
    def supported(eng):
        from bcos.modules.bcosconv2d import NormedConv2d
        # (widths: DenseNetEngine.__init__ already refuses a network whose stem / transition width or growth is no multiple of 4 --
        #  what the slice kernels need for C % 4 == 0 and 16-byte aligned slices -- so such a network never has an engine to ask)
        if not hasattr(eng, "transitions") or not hasattr(eng, "norm5"):
            return False, "not a DenseNetEngine"
        for blk in eng.blocks:
            for ly in blk:
                if float(getattr(ly.module, "drop_rate", 0.0)) > 0.0:
                    return False, "dropout inside the dense layers keeps the per-layer path"
        for p in eng._parts():
            m = getattr(p, "module", None)
            if m is None:
                continue
            if isinstance(getattr(m, "b", None), torch.Tensor) and m.b.requires_grad:
                return False, "learnable exponent"
            if isinstance(m.linear, NormedConv2d):
                return False, "native unit-norm layers"
        return True, ""

    # The forward and input-gradient contractions of the step run with f32 products (ops.contraction_override), whatever the library's
    # default; the ordered weight gradient keeps its exact bf16 planes.  With the split-f16 / split-bf16 contractions this plan's launches
    # (operands with row maxima, shapes such as 200704 rows x 160 / 192 channels) left gradients up to 0.2 from the reference's float64
    # step at DenseNet-121 depth, with f32 products within the per-layer path's distance at batches 4, 16 and 64 (DESIGN.md section
    # 3.5.1); no operand maxima are made for the pre-activations, which f32 launches do not read.
    CONTRACTION = "f32"

    def forward(self, x: torch.Tensor):
        with ops.contraction_override(self.CONTRACTION):
            return super().forward(x)

    def backward(self, st, g_logits: torch.Tensor, need_x: bool = True):
        with ops.contraction_override(self.CONTRACTION):
            return super().backward(st, g_logits, need_x)

    def _weights(self, device):
        self._wunits = {}              # (every layer prepares its own banks: module docstring)

    def parameters(self) -> List[nn.Parameter]:
        """every parameter the plan reads, in a fixed order (the autograd Function's inputs)"""
        ps, seen = [], set()
        for part in self.eng._parts():
            m, bn = getattr(part, "module", None), part.bn
            cand = (m.linear.weight, m.linear.bias) if m is not None else ()
            for p in cand + (getattr(bn, "weight", None), getattr(bn, "bias", None)):
                if isinstance(p, nn.Parameter) and id(p) not in seen:
                    seen.add(id(p))
                    ps.append(p)
        return ps

    # ------------------------------------------------------------------------------------------------------------------
    def _pre_fwd(self, pn, xs, var):
        """norm + ReLU of the channel slice `xs` of a block buffer in front of a contraction, the statistics of its channels taken from
        the block's shared vector `var` -> (dense operand, _PreState)"""
        bn, c = pn.bn, xs.shape[-1]
        ps = _PreState()
        ps.bn, ps.batch_stats = bn, _uses_batch_stats(bn)
        weight = bn.weight.detach() if bn.weight is not None else None
        if ps.batch_stats:
            momentum = 0.0 if bn.momentum is None else bn.momentum
            if bn.training and bn.track_running_stats and bn.num_batches_tracked is not None:
                if bn.momentum is None:                          # cumulative average: the count is needed on the host, now
                    bn.num_batches_tracked.add_(1)
                    momentum = 1.0 / float(bn.num_batches_tracked)
                else:
                    self._nbt.append(bn.num_batches_tracked)
            rv = bn.running_var if (bn.track_running_stats and bn.running_var is not None) else None
            ps.rstd, ps.g = ops.bn_reader_finish(var[:c], weight, bn.eps, running_var=rv, momentum=momentum)
        else:
            if bn.running_var is None:
                raise BcosHipError("densenet train plan: a BatchNormUncentered2d in eval() needs its running_var")
            ps.rstd = torch.rsqrt(bn.running_var.detach() + bn.eps)
            ps.g = (ps.rstd if weight is None else weight * ps.rstd).contiguous()
        ps.shift = bn.bias.detach().contiguous() if isinstance(bn.bias, torch.Tensor) else None
        return ops.slice_affine_rows(xs, ps.g, ps.shift, relu=True, want_absmax=False), ps

    def _pre_bwd(self, ps, d, xs, gs, mean, grads: Dict, accumulate: bool):
        """`d`: the gradient w.r.t. the pre-activation's output (dense); its input gradient goes into the slice `gs` of the block's G"""
        bn, c = ps.bn, xs.shape[-1]
        d2 = d.reshape(-1, c)
        d2 = d2 if d2.is_contiguous() else d2.contiguous()
        want_w = isinstance(bn.weight, nn.Parameter) and bn.weight.requires_grad
        want_b = isinstance(bn.bias, nn.Parameter) and bn.bias.requires_grad
        need_var = ps.batch_stats and not bn.detach           # (variance a constant in explanation mode, or for a norm in eval())
        coef = None
        if want_w or want_b or need_var:
            _, sg, gw, coef = ops.slice_relu_bwd_colsums(d2, xs, ps.g, ps.shift, rstd=ps.rstd, want_sg=want_b, want_gw=want_w,
                                                         want_coef=need_var)
            if want_w:
                grads[bn.weight] = gw
            if want_b:
                grads[bn.bias] = sg
        ops.slice_bn_bwd_acc(d2, gs, xs, scale=ps.g, shift=ps.shift, mean=mean[:c] if need_var else None, coef=coef, accumulate=accumulate)

    # ------------------------------------------------------------------------------------------------------------------
    def _forward(self, x: torch.Tensor):
        eng = self.eng
        if x.dim() != 4 or x.shape[1] not in (3, 6):
            raise ValueError(f"expected [N,6,H,W] (or [N,3,H,W] to be AddInverse-encoded), got {tuple(x.shape)}")
        ops.require_device(x, "bcos_hip.densenet_train_plan")
        xd = x.detach()
        xd = xd if xd.is_contiguous() else xd.contiguous()
        mean6, std6 = eng._consts(x.device)
        st = dict(x=xd, add_inverse=xd.shape[1] == 3, H=xd.shape[2], W=xd.shape[3], blocks=[], trans=[])
        xn = ops.prep_input(xd, mean6, std6, cpad=8, add_inverse=st["add_inverse"], want_absmax=True)
        a0, st["stem"] = self._unit_fwd(eng.stem, xn, relu=True)
        st["a0_hw"] = (a0.shape[1], a0.shape[2])
        k, s, p = eng.pool
        cur = ops.avgpool2d_fwd(a0, k, s, p, want_absmax=False)
        del a0, xn
        N = xd.shape[0]
        for bi, blk in enumerate(eng.blocks):
            H, W, c0 = cur.shape[1], cur.shape[2], cur.shape[3]
            width = c0 + sum(ly.growth for ly in blk)
            X = torch.empty((N, H, W, width), device=x.device, dtype=torch.float32)
            mean, var = (torch.empty((width,), device=x.device, dtype=torch.float32) for _ in range(2))
            ops.slice_affine_rows(cur, out=X[..., :c0], want_absmax=False)           # every stage off: the pooled tensor into slice 0
            ops.slice_batch_stats(X[..., :c0], mean[:c0], var[:c0])
            del cur
            rec = dict(X=X, mean=mean, c0=c0, pre=[], u1=[], u2=[])
            c = c0
            for ly in blk:
                pre, ps = self._pre_fwd(ly.pre, X[..., :c], var)
                y, u1 = self._unit_fwd(ly.conv1, pre, relu=True)
                new, u2 = self._unit_fwd(ly.conv2, y, relu=False)                    # (no norm, no ReLU; its scale is not detached)
                hi = c + ly.growth
                ops.slice_affine_rows(new, out=X[..., c:hi], want_absmax=False)
                ops.slice_batch_stats(X[..., c:hi], mean[c:hi], var[c:hi])           # the slice is complete: its statistics, once
                rec["pre"].append(ps)
                rec["u1"].append(u1)
                rec["u2"].append(u2)
                del pre, y, new
                c = hi
            st["blocks"].append(rec)
            if bi < len(eng.transitions):
                tr = eng.transitions[bi]
                pre, ps = self._pre_fwd(tr.pre, X, var)
                y, u = self._unit_fwd(tr.conv, pre, relu=False)
                pk, pst, pp = tr.pool
                cur = ops.avgpool2d_fwd(y, pk, pst, pp, want_absmax=False)
                st["trans"].append(dict(pre=ps, unit=u, hw=(y.shape[1], y.shape[2])))
                del pre, y
        pre, st["norm5"] = self._pre_fwd(eng.norm5, X, var)
        f, st["head"] = self._unit_fwd(eng.head, pre, relu=False)
        st["feat_hw"] = (f.shape[1], f.shape[2])
        logits = ops.global_avgpool_logits(f, eng.logit_temperature, eng.logit_bias)
        return logits, st

    def _backward(self, st, g_logits: torch.Tensor, need_x: bool = True):
        eng = self.eng
        grads: Dict = {}
        fh, fw = st["feat_hw"]
        N = g_logits.shape[0]
        inv_t = 1.0 if eng.logit_temperature is None else 1.0 / float(eng.logit_temperature)
        gf = (g_logits.to(torch.float32) * (inv_t / float(fh * fw))).view(N, 1, 1, -1).expand(N, fh, fw, g_logits.shape[1]).contiguous()
        d, _ = self._unit_bwd(st["head"], gf, grads)
        reader = st["norm5"]
        for bi in range(len(eng.blocks) - 1, -1, -1):
            blk, rec = eng.blocks[bi], st["blocks"][bi]
            X, mean = rec["X"], rec["mean"]
            # the first reader handled on the way back (head / transition) reads the whole block: it WRITES every channel of G
            G = torch.empty_like(X)
            self._pre_bwd(reader, d, X, G, mean, grads, accumulate=False)
            del d
            c = X.shape[-1]
            for li in range(len(blk) - 1, -1, -1):
                ly = blk[li]
                c -= ly.growth
                ga = ops.slice_affine_rows(G[..., c:c + ly.growth], want_absmax=False)        # every later reader has added its share
                gh, _ = self._unit_bwd(rec["u2"][li], ga, grads)
                dl, _ = self._unit_bwd(rec["u1"][li], gh, grads)
                self._pre_bwd(rec["pre"][li], dl, X[..., :c], G[..., :c], mean, grads, accumulate=True)
                rec["u1"][li] = rec["u2"][li] = rec["pre"][li] = None
                del ga, gh, dl
            g0 = ops.slice_affine_rows(G[..., :c], want_absmax=False)                # gather slice 0: the gradient of the pooled tensor
            del G
            rec["X"] = None
            if bi > 0:
                tr, trec = eng.transitions[bi - 1], st["trans"][bi - 1]
                pk, pst, pp = tr.pool
                th, tw = trec["hw"]
                gl = ops.avgpool2d_bwd(g0, th, tw, pk, pst, pp)
                d, _ = self._unit_bwd(trec["unit"], gl, grads)
                reader = trec["pre"]
                del gl, g0
        k, s, p = eng.pool
        a_h, a_w = st["a0_hw"]
        gl = ops.avgpool2d_bwd(g0, a_h, a_w, k, s, p)
        gxn, _ = self._unit_bwd(st["stem"], gl, grads, need_x=need_x)
        gx = None
        if need_x:
            _, std6 = eng._consts(g_logits.device)
            g6 = gxn.permute(0, 3, 1, 2) / std6.view(1, 6, 1, 1)            # d/dx of (x - mean) / std (bcosify.py:43)
            gx = (g6[:, :3] - g6[:, 3:]).contiguous() if st["add_inverse"] else g6.contiguous()      # AddInverse: [x, 1 - x]
        return gx, grads
