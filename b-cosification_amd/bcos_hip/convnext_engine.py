"""Fused forward / explanation engine for the native B-cos ConvNeXts (bcos/models/convnext.py; reference bcos/models/convnext.py:32-219).

`attach(net)` compiles a `BcosConvNeXt` into a launch plan; the nn.Module graph stays the source of truth for the parameters.  The plan
supplies topology only: the contractions are engine.Conv nodes, the head is engine.head_consumer, inputs and the sub-batch scheduler are
the base class's (bcos_hip/plan.py).  The network takes the 6-channel image as it is, so the prepared input is the NHWC copy of the image
(mean 0 / std 1).

Forward, per block -- four launches, no elementwise launch:
  1. bcos_dwconv7_fwd: the depthwise 7x7 B-cos convolution (its scale kept in an explanation pass);
  2. bcos_layernorm_fwd (bcos_layernorm_unc_fwd for the uncentered position norm) over the rows of the NHWC image = the position norm
     (row rstd kept);
  3. the 1x1 expansion C -> 4C (its multiplier kept);
  4. the 1x1 projection 4C -> C with ch_scale = layer_scale and addend = the block input in its epilogue (its multiplier, layer_scale
     included, kept).
Stem: 4x4 / stride-4 contraction, position norm.  Downsampling: position norm, 2x2 / stride-2 contraction.  Head: position norm, 1x1
classifier, global pool + LogitLayer (bcos_global_avgpool_logits), as the ResNet head does it.

Explanation pass, in reverse: the head's rank-one gradient, then per layer the input-gradient contraction of what was kept.  A block takes
the gradient g of its output: g times the projection's multiplier (the second output of the launch that produced g where that is a norm
gradient, one bcos_mul otherwise), the projection's input gradient times the expansion's multiplier in its epilogue, the expansion's
input gradient, the position norm's detached gradient, and bcos_dwconv7_bwd with the kept depthwise scale as `mul` and g, the residual
stream's gradient, as `addend`: the block's input gradient is complete when that launch ends.

Contraction arithmetic: every pass runs under ops.no_absmax() and the norms emit no row maxima, so in the split-f16 mode the plan's
contractions keep the exact bf16x3 loop, as the ViT plan's do and as the module path's contractions behind a norm do.  Reason (measured,
DESIGN.md "ConvNeXt"): with row maxima the K = 96 -> 384 expansion of ConvNeXt-T's first stage takes the d_128x192 tile of the LDS-DMA
loop, which returned wrong rows behind the last full 32768 rows at M > 32768 (batch 32 and up at 56^2), whichever kernel made the maxima.

Scope: position-norm variants (DetachablePositionNorm2d or PositionNormUncentered2d, with or without bias), BcosConv2d with B = 2 fixed
and max_out = 1, eval mode.  Anything else -- the `_bnu` variants, a learnable or other B, MaxOut, a model in train() -- makes attach() raise BcosHipError; the module
path keeps working for them.  `occlude=`, `perturb=`, `rise=` (forward) and `functional=` (explain), explain_targets and
explain_functionals come with the base class and the shared head and are supported; replayed `gates=` (there is no ReLU) and `cotangent=`
(no attention-pool head) are refused with a message.
"""
from typing import Dict, List, Optional

import torch
import torch.nn as nn

from . import ops, plan
from .engine import Conv, head_consumer, mul_kwargs
from .lib import BcosHipError
from .plan import FusedPlan

__all__ = ["ConvNeXtEngine", "attach", "detach", "PLAN_LOG"]

PLAN_LOG = None          # tests set this to a list: every launch of a pass appends (kind, module name)


def _log(kind, name):
    if PLAN_LOG is not None:
        PLAN_LOG.append((kind, name))


def _nhwc(t2d, like):
    """[rows, C] result of a row kernel as the NHWC tensor of `like`'s pixels"""
    return t2d.view(like.shape[0], like.shape[1], like.shape[2], t2d.shape[-1])


class _LayerScale:
    """a block's `layer_scale` [C,1,1] seen as the per-channel scale engine.Conv takes from the norm behind a contraction"""
    bias = running_var = running_mean = None
    training = False

    def __init__(self, param):
        self.weight = param

    def channel_scale_shift(self):
        return self.weight.detach().reshape(-1).contiguous(), None


def _conv(conv, name, scale=None):
    """engine.Conv of a contraction of the plan's scope: a native BcosConv2d, ungrouped, no MaxOut, B = 2 fixed"""
    from bcos.modules.bcosconv2d import BcosConv2d
    if type(conv) is not BcosConv2d:
        raise BcosHipError(f"convnext engine: `{name}` is a {type(conv).__name__}; the plan takes native BcosConv2d layers")
    if int(conv.linear.groups) != 1 or int(conv.max_out) != 1:
        raise BcosHipError(f"convnext engine: `{name}` is grouped or a MaxOut layer; the plan takes ungrouped layers with max_out = 1")
    if isinstance(conv.b, torch.Tensor) or float(conv.b) != 2.0:
        raise BcosHipError(f"convnext engine: `{name}` has B = {conv.b}; the plan takes B = 2 fixed (a learnable B runs through the module path)")
    c = Conv(conv, _LayerScale(scale) if scale is not None else None)
    c.name = name
    return c


class _PosNorm:
    """Kernel-side view of a DetachablePositionNorm2d -- LayerNorm over the rows of the NHWC image -- or of a PositionNormUncentered2d:
    the same rows, the same launches, the uncentered kernels (csrc/bcos_norms.hip, centered=False: x itself is divided, and the detached gradient
    subtracts no mean)."""

    def __init__(self, norm, name):
        if type(norm).__name__ not in ("DetachablePositionNorm2d", "PositionNormUncentered2d"):
            raise BcosHipError(f"convnext engine: `{name}` is a {type(norm).__name__}; the plan takes the position-norm variants only "
                               "(DetachablePositionNorm2d; the `_bnu` variants run through the module path)")
        self.module, self.name = norm, name
        self.unc = type(norm).__name__ == "PositionNormUncentered2d"
        self.flavour = {"centered": False} if self.unc else {}         # (keywords of ops.layernorm_*: nothing for the centred norm)
        self.refresh()

    def fingerprint(self):
        m = self.module
        return tuple((t.data_ptr(), t._version) if isinstance(t, torch.Tensor) else t for t in (m.weight, m.bias)) + (m.eps, m.training)

    def refresh(self):
        m = self.module
        self._fp = self.fingerprint()
        if m.training:
            raise BcosHipError(f"convnext engine: `{self.name}` must be in eval mode (call model.eval())")
        self.w = m.weight.detach().contiguous() if m.weight is not None else None
        self.b = m.bias.detach().contiguous() if m.bias is not None else None
        self.eps, self.C = float(m.eps), int(m.normalized_shape[0])
        if self.w is not None:
            ops.publish_cached(self.w)

    def fwd(self, x, keep):
        _log("pn", self.name)
        y, rstd = ops.layernorm_fwd(x.view(-1, self.C), self.w, self.b, self.eps, want_rstd=keep, **self.flavour)
        return _nhwc(y, x), rstd

    def bwd(self, g, rstd, mul2=None, want_out=True):
        """detached gradient of the norm -> (gradient, gradient * mul2 or None)"""
        _log("pn_bwd", self.name)
        o, o2 = ops.layernorm_bwd_detached(g.view(-1, self.C), self.w, rstd, mul2=None if mul2 is None else mul2.view(-1, self.C),
                                           want_out=want_out, want_out2=mul2 is not None, **self.flavour)
        return (None if o is None else _nhwc(o, g)), (None if o2 is None else _nhwc(o2, g))


class _DwConv:
    """Kernel-side view of the depthwise 7x7 BcosConv2d of a block."""

    def __init__(self, conv, name):
        from bcos.modules import _hipfn
        from bcos.modules.bcosconv2d import BcosConv2d
        if type(conv) is not BcosConv2d or not _hipfn.conv_is_depthwise7(conv.linear, conv.max_out):
            raise BcosHipError(f"convnext engine: `{name}` is not a depthwise 7x7 / stride 1 / padding 3 BcosConv2d")
        if isinstance(conv.b, torch.Tensor) or float(conv.b) != 2.0:
            raise BcosHipError(f"convnext engine: `{name}` has B = {conv.b}; the plan takes B = 2 fixed")
        if conv.linear.in_channels % 4:
            raise BcosHipError(f"convnext engine: `{name}` has {conv.linear.in_channels} channels; the depthwise kernel moves four at a time")
        self.module, self.name, self.C = conv, name, conv.linear.in_channels
        self.refresh()

    def fingerprint(self):
        lin = self.module.linear
        ts = (lin.weight, lin.bias, getattr(lin, "scale", None))
        return tuple((t.data_ptr(), t._version) if isinstance(t, torch.Tensor) else t for t in ts) + (getattr(lin, "use_weight_norm", None),)

    def refresh(self):
        self._fp = self.fingerprint()
        w, bias = self.module._effective_weight_and_bias()
        if bias is not None:
            raise BcosHipError(f"convnext engine: `{self.name}` has a bias; the depthwise kernel takes none")
        self.w = ops.dwconv7_weight_image(w.detach())

    def fwd(self, x, keep):
        _log("dw", self.name)
        y, s, _ = ops.dwconv7_fwd(x, self.w, b=2.0, want_scale=keep)
        return y, s

    def bwd(self, g, s, addend):
        _log("dw_bwd", self.name)
        return ops.dwconv7_bwd(g, self.w, mul=s, addend=addend)


class _Block:
    def __init__(self, blk, name):
        seq = getattr(blk, "block", None)
        if seq is None or len(seq) != 4 or not hasattr(blk, "layer_scale"):
            raise BcosHipError(f"convnext engine: `{name}` is not a CNBlock (depthwise conv, norm, two 1x1 convs, layer_scale)")
        self.dw = _DwConv(seq[0], f"{name}.block.0")
        self.pn = _PosNorm(seq[1], f"{name}.block.1")
        self.c1 = _conv(seq[2], f"{name}.block.2")
        self.c2 = _conv(seq[3], f"{name}.block.3", scale=blk.layer_scale)
        C = self.dw.C
        if (self.pn.C, self.c1.cin, self.c1.cout, self.c2.cin, self.c2.cout) != (C, C, 4 * C, 4 * C, C) or self.c1.k != (1, 1) or self.c2.k != (1, 1) \
                or blk.layer_scale.numel() != C:
            raise BcosHipError(f"convnext engine: `{name}` is not dim -> dim -> 4 dim -> dim with 1x1 contractions")
        self.C = C

    def parts(self):
        return (self.dw, self.pn, self.c1, self.c2)


class ConvNeXtEngine(FusedPlan):
    """Launch plan for a native `BcosConvNeXt` (see the module docstring for the launch list, what is kept and the scope)."""
    who = "convnext engine"

    def __init__(self, net):
        feats, cls = getattr(net, "features", None), getattr(net, "classifier", None)
        if not isinstance(feats, nn.Sequential) or not isinstance(cls, nn.Sequential) or len(feats) < 3 or len(cls) != 2 \
                or getattr(net, "logit_layer", None) is None:
            raise BcosHipError(f"convnext engine: {type(net).__name__} has no `features` / `classifier` / `logit_layer` of a BcosConvNeXt")
        if net.training:
            raise BcosHipError("convnext engine: the model must be in eval mode (call model.eval())")
        self.stem = _conv(feats[0], "features.0")
        self.stem_pn = _PosNorm(feats[1], "features.1")
        if self.stem.k != self.stem.stride or self.stem.padding != (0, 0) or self.stem.cin > 8:
            raise BcosHipError("convnext engine: the stem must be a patchifying convolution (kernel = stride, no padding) of the 6-channel image")
        self.layers: List[object] = []            # _Block | ("down", _PosNorm, Conv)
        C = self.stem.cout
        for k in range(2, len(feats)):
            mod, name = feats[k], f"features.{k}"
            if not isinstance(mod, nn.Sequential) or len(mod) == 0:
                raise BcosHipError(f"convnext engine: `{name}` is neither a stage of blocks nor a downsampling pair")
            if len(mod) == 2 and not hasattr(mod[0], "block"):          # downsampling: norm, strided convolution
                pn, conv = _PosNorm(mod[0], name + ".0"), _conv(mod[1], name + ".1")
                if pn.C != C or conv.cin != C or conv.k != conv.stride or conv.padding != (0, 0):
                    raise BcosHipError(f"convnext engine: `{name}` is not norm -> strided patch convolution over {C} channels")
                self.layers.append(("down", pn, conv))
                C = conv.cout
            else:
                for j, blk in enumerate(mod):
                    b = _Block(blk, f"{name}.{j}")
                    if b.C != C:
                        raise BcosHipError(f"convnext engine: `{name}.{j}` has {b.C} channels where the stage holds {C}")
                    self.layers.append(b)
        self.head_pn = _PosNorm(cls[0], "classifier.0")
        self.head = _conv(cls[1], "classifier.1")
        if self.head.k != (1, 1) or self.head.cin != C or self.head_pn.C != C or C % 4:
            raise BcosHipError("convnext engine: the classifier must be norm -> 1x1 convolution over the last stage's channels (a multiple of 4)")
        super().__init__(net)
        self.supports_explain = True

    # ------------------------------------------------------------------------------------------------
    def _parts(self):
        yield from (self.stem, self.stem_pn)
        for ly in self.layers:
            yield from (ly.parts() if isinstance(ly, _Block) else ly[1:])
        yield from (self.head_pn, self.head)

    def refresh(self):
        """Re-read parameters after they changed; forward() / explain() do so themselves when a parameter's storage or in-place
        version differs from what the plan was built from."""
        for p in self._parts():
            p.refresh()

    def _ensure_fresh(self):
        if self.net.training:
            raise BcosHipError("convnext engine: the model must be in eval mode (call model.eval())")
        ops.publish_pending()
        for p in self._parts():
            if p.fingerprint() != p._fp:
                p.refresh()

    def n_logits(self) -> int:
        return self.head.cout

    def _pass_context(self):
        """no operand maxima: the plan's contractions keep the bf16x3 loop in the split-f16 mode (module docstring)"""
        return ops.no_absmax()

    # ------------------------------------------------------------------------------------------------
    def _run_forward_gen(self, src, keep: bool, gates=None):
        """The forward pass over the images `src` as a generator (yields behind the stem and behind every block / downsampling, so that
        the passes of several sub-batches are issued interleaved); -> (logits, kept state)."""
        self._refuse(gates=gates)
        x, xn = self._begin(src, want_absmax=False)
        _log("conv", self.stem.name)
        a, t0 = self.stem.fwd(xn, want_scale=keep, track=False)                       # (feeds a norm)
        cur, r0 = self.stem_pn.fwd(a, keep)
        st = dict(x=x, add_inverse=src.add_inverse, H=x.shape[2], W=x.shape[3], t0=t0, r0=r0, recs=[]) if keep else None
        del a, xn
        yield
        for ly in self.layers:
            if isinstance(ly, _Block):
                d, s = ly.dw.fwd(cur, keep)
                z, rstd = ly.pn.fwd(d, keep)
                del d
                _log("conv", ly.c1.name)
                e, t1 = ly.c1.fwd(z, want_scale=keep)
                del z
                _log("conv", ly.c2.name)
                out, t2 = ly.c2.fwd(e, addend=cur, want_scale=keep, track=False)     # (feeds a depthwise launch or a norm)
                del e
                rec = dict(s=s, rstd=rstd, t1=t1, t2=t2, hw=(cur.shape[1], cur.shape[2]))
            else:
                _, pn, conv = ly
                z, rstd = pn.fwd(cur, keep)
                _log("conv", conv.name)
                out, t = conv.fwd(z, want_scale=keep, track=False)
                del z
                rec = dict(rstd=rstd, t=t, hw=(cur.shape[1], cur.shape[2]))
            cur = out
            if keep:
                st["recs"].append(rec)
            yield
        z, rstd = self.head_pn.fwd(cur, keep)
        _log("conv", self.head.name)
        f, tf = self.head.fwd(z, want_scale=keep, track=False)
        logits = ops.global_avgpool_logits(f, self.logit_temperature, self.logit_bias)
        if keep:
            st.update(tf=tf, rf=rstd, head_hw=(cur.shape[1], cur.shape[2]))
        return logits, st

    def _backward_gen(self, x, st, cls, want_weights: bool, consume: bool, outs=None, functional=None, g_head=None):
        """Input-gradient pass of logit[cls[n]] (or of `functional`) for every image n over the state `st` of a kept forward; `consume`
        frees each kept tensor as soon as it has been used (last / only pass over this state)."""
        self._refuse(cotangent=g_head)
        N = x.shape[0]
        H, W = st["head_hw"]
        d, _ = head_consumer(self.head, st["tf"], cls, functional, self.logit_temperature).run(H, W, t_main=None, td=None, gated=False, track=False)
        recs = st["recs"]

        def mul_of(i):
            """the multiplier of what produced the residual stream that layer i reads (layer i - 1, or the stem's norm: None)"""
            if i == 0:
                return None
            r = recs[i - 1]
            return r["t2"] if "t2" in r else r["t"]

        # g: gradient of the stream that the head's norm reads; gm = g times the multiplier of the layer that produced that stream
        g, gm = self.head_pn.bwd(d, st["rf"], mul2=mul_of(len(recs)), want_out=isinstance(self.layers[-1], _Block) if self.layers else True)
        if consume:
            st["tf"] = st["rf"] = None
        del d
        yield
        for i in range(len(self.layers) - 1, -1, -1):
            ly, rec = self.layers[i], recs[i]
            h, w = rec["hw"]
            if gm is None:
                gm = ops.mul(g, mul_of(i + 1))
            if isinstance(ly, _Block):
                _log("dgrad", ly.c2.name)
                gl = ly.c2.dgrad.run(gm, h, w, **mul_kwargs(rec["t1"]))
                del gm
                _log("dgrad", ly.c1.name)
                dz = ly.c1.dgrad.run(gl, h, w, track_absmax=False)
                del gl
                gd, _ = ly.pn.bwd(dz, rec["rstd"])
                del dz
                g = ly.dw.bwd(gd, rec["s"], addend=g)                                  # the block's input gradient, complete
                del gd
                gm = None
            else:
                _, pn, conv = ly
                _log("dgrad", conv.name)
                dz = conv.dgrad.run(gm, h, w, track_absmax=False)
                del gm
                below_is_block = i > 0 and isinstance(self.layers[i - 1], _Block)
                g, gm = pn.bwd(dz, rec["rstd"], mul2=mul_of(i), want_out=below_is_block or i == 0)
                del dz
            if consume:
                recs[i] = None
            yield
        # the stem: its norm's gradient times the stem's multiplier, then the patchifying convolution's input gradient
        _, gl = self.stem_pn.bwd(g, st["r0"], mul2=st["t0"], want_out=False)
        del g
        if consume:
            st["t0"] = st["r0"] = None
        gxn = torch.empty((N, st["H"], st["W"], 8), device=x.device, dtype=torch.float32)
        _log("dgrad", self.stem.name)
        self.stem.dgrad.run(gl, st["H"], st["W"], out=gxn)                             # channels 0..5 of the padded buffer
        _, std = self._consts(x.device)
        return ops.finalize_explanation(gxn, st["x"], std, add_inverse=st["add_inverse"], want_weights=want_weights, want_contrib=True,
                                        weights_out=outs[0] if outs is not None else None,
                                        contrib_out=outs[1] if outs is not None else None)

    # ------------------------------------------------------------------------------------------------
    @staticmethod
    def _refuse(**kwargs):
        for name, val in kwargs.items():
            if val is not None:
                raise BcosHipError(f"convnext engine: `{name}=` is not built for this plan (no ReLU gates to replay, no attention-pool head); "
                                   "detach() the engine and use the module path")

    @torch.no_grad()
    def explain(self, x: torch.Tensor, targets: Optional[torch.Tensor] = None, want_weights: bool = True, gates=None, cotangent=None,
                functional=None) -> Dict[str, torch.Tensor]:
        """Forward in explanation mode + input-gradient pass of the explained logit (or of `functional`) of every image."""
        self._refuse(gates=gates, cotangent=cotangent)
        return super().explain(x, targets, want_weights, functional=functional)

    explain_targets = FusedPlan._explain_targets
    explain_functionals = FusedPlan._explain_functionals


def attach(net) -> ConvNeXtEngine:
    """Compile `net` (a bcos.models.convnext.BcosConvNeXt in eval mode) into the fused plan (bcos_hip/plan.py: attach)."""
    return plan.attach(net, ConvNeXtEngine)


detach = plan.detach
