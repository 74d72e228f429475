"""Fused forward / explanation engine for B-cosified DenseNets (torchvision topology: reference standard_models.py:56-63).

`attach(net)` compiles a `BcosifyNetwork(DenseNetBcos(...))` into a launch plan; the nn.Module graph stays the source of truth for the
parameters.  What differs from the ResNet plan (bcos_hip/engine.py) is the pre-activation order -- every consumer of a dense block's
features applies ITS OWN BatchNormUncentered + ReLU to the concatenation in front of its contraction -- and the concatenation itself:

  * one RAW (pre-norm) NHWC buffer X per dense block, [N, H, W, C_block_out]; layer l reads channels [0, C_l) and its 3 x 3 conv
    appends channels [C_l, C_l + growth).  Nothing is ever concatenated or copied to grow it;
  * forward, per layer: bcos_slice_affine_rows (norm1 + ReLU of the slice -> a dense temporary with its row maxima; not kept), conv1 with
    norm2 + ReLU in its epilogue (its multiplier kept or rebuilt from the activation, as in the ResNet plan), conv2 with a plain B-cos
    epilogue.  A forward-only pass writes conv2's output straight into its slice of X (bcos_tapconv_geom.out_pitch); the explanation
    pass keeps conv2's scale, which the epilogue can only write at the output's own pitch, so there conv2 writes dense tensors and
    its output is placed into the slice by bcos_slice_affine_rows with every stage off (the same bits in X either way);
  * transition: pre-activation of the whole block -> 1 x 1 conv -> AvgPool2d(2, 2) -> placed into slice 0 of the next block's buffer;
    head: pre-activation of norm5 (the functional ReLU behind it included) -> classifier 1 x 1 -> global pool + LogitLayer;
  * explanation pass, in reverse, over one gradient buffer G per block of X's shape: the head's rank-one gradient (or a transition's
    input gradient) d goes through bcos_slice_affine_bwd_acc with accumulate = 0, which writes EVERY channel of G (no zero fill); then
    per layer, last to first: G[slice_l] * s2 (bcos_slice_affine_rows with `mul`), conv2's input gradient times conv1's multiplier,
    conv1's input gradient d [M, C_l], and bcos_slice_affine_bwd_acc(accumulate = 1) into G[:, :C_l], its ReLU gate rebuilt from X
    with the forward kernel's own rounding.  By the time layer l is handled, every later reader of its slice has added its share.

Kept between the passes: X of every block (the features AND the source of every pre-activation gate), conv2's scale and conv1's
multiplier (or what it is rebuilt from) per layer, the transition / classifier / stem scales.  Rebuilt: every pre-activation.
Scope: groups = 1, no MaxOut, B = 2 fixed, eval mode, BatchNormUncentered2d with or without bias; anything else makes attach() raise
BcosHipError (the module path keeps working).  Occlusion, perturbation, functionals, replayed gates and cotangents are not built here.
Training (net.train() + autograd with the engine attached) is bcos_hip/densenet_train_plan.py: one autograd node over this layer list.
"""
from typing import Dict, List, Optional

import torch
import torch.nn as nn

from . import ops, plan
from .engine import Conv, head_consumer, mul_kwargs, pool_params
from .lib import BCOS_CONV_EPS, BcosHipError
from .plan import FusedPlan

__all__ = ["DenseNetEngine", "attach", "detach", "PLAN_LOG"]

PLAN_LOG = None          # tests set this to a list: every contraction of a pass appends (module name, norm in front, norm behind, in / out shape)


def _log(conv, pre, x_shape, out_shape):
    if PLAN_LOG is not None:
        PLAN_LOG.append((conv.name, pre.name if pre is not None else None, conv.bn_name, tuple(x_shape), tuple(out_shape)))


def _is_bnu(m) -> bool:
    return type(m).__name__.startswith("BatchNormUncentered2d")


class _PreNorm:
    """Kernel-side view of a BatchNormUncentered2d that sits IN FRONT of a contraction: its eval-mode scale / shift."""

    def __init__(self, bn, name):
        if not _is_bnu(bn):
            raise BcosHipError(f"densenet engine: `{name}` is a {type(bn).__name__}; the plan fuses BatchNormUncentered2d only "
                               "(bcosify_args.norm_layer = 'BnUncV2' / 'BnUnc2d')")
        self.bn, self.name = bn, name
        self.refresh()

    def fingerprint(self):
        bn = self.bn
        ts = [bn.weight, bn.bias, bn.running_var]
        return tuple((t.data_ptr(), t._version) if isinstance(t, torch.Tensor) else t for t in ts) + (bn.training,)

    def refresh(self):
        self._fp = self.fingerprint()
        if self.bn.training:
            raise BcosHipError(f"densenet engine: `{self.name}` must be in eval mode (call model.eval())")
        self.scale, self.shift = self.bn.channel_scale_shift()
        ops.publish_cached(self.scale)


def _conv(conv, bn, name, bn_name=None):
    """engine.Conv of a layer of the plan's scope: ungrouped, no MaxOut, B = 2 fixed, no bias handling beyond the kernels' own"""
    lin = getattr(conv, "linear", None)
    if lin is None:
        raise BcosHipError(f"densenet engine: `{name}` is a {type(conv).__name__}, not a B-cos convolution")
    if int(lin.groups) != 1:
        raise BcosHipError(f"densenet engine: `{name}` has groups = {lin.groups}; the plan takes ungrouped layers (module path otherwise)")
    if int(getattr(conv, "max_out", 1)) != 1:
        raise BcosHipError(f"densenet engine: `{name}` is a MaxOut layer (max_out = {conv.max_out}); the plan takes max_out = 1")
    if bn is not None and not _is_bnu(bn):
        raise BcosHipError(f"densenet engine: `{bn_name}` is a {type(bn).__name__}; the plan fuses BatchNormUncentered2d only")
    c = Conv(conv, bn)
    if c.b != 2.0 or c.force_pow:
        raise BcosHipError(f"densenet engine: `{name}` has B = {c.b}{' (learnable)' if c.force_pow else ''}; the plan takes B = 2 fixed")
    c.name, c.bn_name = name, bn_name
    return c


class _Layer:
    def __init__(self, layer, name):
        for attr in ("norm1", "relu1", "conv1", "norm2", "relu2", "conv2"):
            if not hasattr(layer, attr):
                raise BcosHipError(f"densenet engine: `{name}` has no `{attr}`: not a torchvision _DenseLayer")
        if not isinstance(layer.relu1, nn.ReLU) or not isinstance(layer.relu2, nn.ReLU):
            raise BcosHipError(f"densenet engine: `{name}` without its ReLUs (act_layer = False) runs through the module path only")
        self.module = layer
        self.pre = _PreNorm(layer.norm1, f"{name}.norm1")
        self.conv1 = _conv(layer.conv1, layer.norm2, f"{name}.conv1", f"{name}.norm2")
        self.conv2 = _conv(layer.conv2, None, f"{name}.conv2")
        if self.conv1.k != (1, 1) or self.conv2.k != (3, 3) or self.conv2.stride != (1, 1) or self.conv2.padding != (1, 1):
            raise BcosHipError(f"densenet engine: `{name}` is not a 1 x 1 -> 3 x 3 / stride 1 / padding 1 dense layer")
        self.cin, self.growth = self.conv1.cin, self.conv2.cout


class _Transition:
    def __init__(self, tr, name):
        mods = list(tr.children())
        if len(mods) != 4 or not isinstance(mods[1], nn.ReLU) or not isinstance(mods[3], nn.AvgPool2d):
            raise BcosHipError(f"densenet engine: `{name}` is not norm -> ReLU -> conv -> AvgPool2d")
        self.pool = pool_params(mods[3], f"densenet engine: `{name}`")
        self.pre = _PreNorm(mods[0], f"{name}.0")
        self.conv = _conv(mods[2], None, f"{name}.2")
        if self.conv.k != (1, 1) or self.conv.stride != (1, 1):
            raise BcosHipError(f"densenet engine: `{name}`: the transition convolution must be 1 x 1 / stride 1")


class DenseNetEngine(FusedPlan):
    """Launch plan for `BcosifyNetwork(DenseNetBcos(...))` (bcosify.py:22-53 + standard_models.py:56-63)."""
    who = "densenet engine"

    def __init__(self, net):
        m = getattr(net, "model", None)
        feats = getattr(m, "features", None)
        if feats is None or not hasattr(m, "classifier"):
            raise BcosHipError(f"densenet engine: {type(m).__name__} has no `features` / `classifier`: not a torchvision-style DenseNet")
        mods = list(feats.named_children())
        if len(mods) < 6 or not isinstance(mods[2][1], nn.ReLU):
            raise BcosHipError("densenet engine: `features` does not start with conv0 / norm0 / relu0 / pool0")
        pre = "model.features."
        self.stem = _conv(mods[0][1], mods[1][1], pre + mods[0][0], pre + mods[1][0])
        pool = mods[3][1]
        if not isinstance(pool, nn.AvgPool2d):
            raise BcosHipError("densenet engine: the stem pool must be nn.AvgPool2d (the B-cosification recipe swaps MaxPool for "
                               "AvgPool2d(3, 2, 1): standard_changes = {'features[3]': ...})")
        self.pool = pool_params(pool, "densenet engine")
        self.blocks: List[List[_Layer]] = []
        self.transitions: List[_Transition] = []
        body, (last_name, last) = mods[4:-1], mods[-1]
        for name, mod in body:
            if isinstance(mod, nn.ModuleDict):
                if len(self.blocks) != len(self.transitions):
                    raise BcosHipError(f"densenet engine: dense block `{name}` does not follow a transition")
                self.blocks.append([_Layer(layer, f"{pre}{name}.{ln}") for ln, layer in mod.items()])
            else:
                if len(self.blocks) != len(self.transitions) + 1:
                    raise BcosHipError(f"densenet engine: transition `{name}` does not follow a dense block")
                self.transitions.append(_Transition(mod, pre + name))
        if not self.blocks or len(self.blocks) != len(self.transitions) + 1 or any(len(b) == 0 for b in self.blocks):
            raise BcosHipError("densenet engine: expected dense blocks separated by transitions, then the final norm")
        self.norm5 = _PreNorm(last, pre + last_name)
        self.head = _conv(m.classifier, None, "model.classifier")
        if self.head.k != (1, 1):
            raise BcosHipError("densenet engine: the classifier must be the 1 x 1 convolution in front of the global pool (bcosify_args.gap)")
        # widths: every layer reads all the channels in front of it, every transition the whole block, norm5 the last block
        c = self.stem.cout
        for bi, blk in enumerate(self.blocks):
            for ly in blk:
                if ly.cin != c or ly.pre.bn.num_features != c or c % 4 or ly.growth % 4:
                    raise BcosHipError(f"densenet engine: `{ly.conv1.name}` reads {ly.cin} channels where the block holds {c} "
                                       "(widths must chain and be multiples of 4)")
                c += ly.growth
            nxt = self.transitions[bi] if bi < len(self.transitions) else None
            reader = nxt.conv if nxt is not None else self.head
            norm = nxt.pre if nxt is not None else self.norm5
            if reader.cin != c or norm.bn.num_features != c:
                raise BcosHipError(f"densenet engine: `{reader.name}` reads {reader.cin} channels where the block holds {c}")
            if nxt is not None:
                c = nxt.conv.cout
        super().__init__(net)
        self.supports_explain = True

    @property
    def train_plan_class(self):
        """the plan `train_plan.train_forward` builds for net.train() + autograd (bcos_hip/densenet_train_plan.py)"""
        from .densenet_train_plan import DenseNetTrainPlan
        return DenseNetTrainPlan

    # ------------------------------------------------------------------------------------------------
    def _parts(self):
        yield self.stem
        for bi, blk in enumerate(self.blocks):
            for ly in blk:
                yield from (ly.pre, ly.conv1, ly.conv2)
            if bi < len(self.transitions):
                yield from (self.transitions[bi].pre, self.transitions[bi].conv)
        yield from (self.norm5, self.head)

    def refresh(self):
        """Re-read parameters after they changed (load_state_dict, calibration, ...); forward() / explain() do so themselves when a
        parameter's storage or in-place version differs from what the plan was built from."""
        for p in self._parts():
            p.refresh()

    def _ensure_fresh(self):
        ops.publish_pending()
        for p in self._parts():
            if p.fingerprint() != p._fp:
                p.refresh()

    def n_logits(self) -> int:
        return self.head.cout

    # ------------------------------------------------------------------------------------------------
    def _pre(self, pre, x_slice):
        """norm + ReLU of a channel slice of a block buffer -> the dense operand of the contraction behind it, with its row maxima"""
        return ops.slice_affine_rows(x_slice, pre.scale, pre.shift, relu=True)

    def _run_forward_gen(self, src, keep: bool, gates=None):
        """The forward pass over the images `src` (plan.Images) as a generator (yields behind the stem and behind every dense layer /
        transition, so that the passes of several sub-batches are issued interleaved); -> (logits, kept state)."""
        self._refuse(gates=gates)
        x, xn = self._begin(src)
        N = src.n
        a, t0 = self.stem.fwd(xn, relu=True, want_scale=keep, track=False)          # (feeds a pool)
        _log(self.stem, None, xn.shape, a.shape)
        st = dict(x=x, add_inverse=src.add_inverse, H=x.shape[2], W=x.shape[3], t0=t0, a0_hw=(a.shape[1], a.shape[2]), blocks=[], trans=[]) if keep else None
        k, s, p = self.pool
        cur = ops.avgpool2d_fwd(a, k, s, p, want_absmax=False)
        del a, xn
        yield
        for bi, blk in enumerate(self.blocks):
            H, W, c0 = cur.shape[1], cur.shape[2], cur.shape[3]
            width = c0 + sum(ly.growth for ly in blk)
            X = torch.empty((N, H, W, width), device=x.device, dtype=torch.float32)
            ops.slice_affine_rows(cur, out=X[..., :c0], want_absmax=False)           # every stage off: the pooled tensor into slice 0
            del cur
            rec = dict(X=X, hw=(H, W), s2=[], t1=[]) if keep else None
            c = c0
            for ly in blk:
                pre = self._pre(ly.pre, X[..., :c])
                with ops.image_range_reader(True):                                   # (the 3 x 3 conv2 reads this output)
                    y, t1 = ly.conv1.fwd(pre, relu=True, want_scale=keep, keep_act=True, track=True)
                _log(ly.conv1, ly.pre, pre.shape, y.shape)
                del pre
                c2 = ly.conv2
                g = ops.fwd_geom(N, H, W, c2.w_fwd.shape[3], c2.cout, 3, 3, 1, 1, 1, 1)
                if keep:
                    new, s2, _ = ops.conv2d_fwd(y, c2.w_fwd, stride=(1, 1), padding=(1, 1), bias=c2.bias, b=2.0, mode=BCOS_CONV_EPS,
                                                want_scale=True, track_absmax=False)
                    ops.slice_affine_rows(new, out=X[..., c:c + ly.growth], want_absmax=False)
                    rec["s2"].append(s2)
                    rec["t1"].append(t1)
                    del new
                else:
                    g["out_pitch"] = width
                    ops.tapconv(y, c2.w_fwd, g, out=X[..., c:c + ly.growth], bias=c2.bias, bcos_mode=BCOS_CONV_EPS, b=2.0, track_absmax=False)
                _log(c2, None, y.shape, (N, H, W, ly.growth))
                del y
                c += ly.growth
                yield
            if keep:
                st["blocks"].append(rec)
            if bi < len(self.transitions):
                tr = self.transitions[bi]
                pre = self._pre(tr.pre, X)
                y, tt = tr.conv.fwd(pre, relu=False, want_scale=keep, track=False)   # (feeds a pool)
                _log(tr.conv, tr.pre, pre.shape, y.shape)
                del pre
                pk, ps, pp = tr.pool
                cur = ops.avgpool2d_fwd(y, pk, ps, pp, want_absmax=False)
                if keep:
                    st["trans"].append(dict(t=tt, hw=(y.shape[1], y.shape[2])))
                del y
                yield
        pre = self._pre(self.norm5, X)
        f, tf = self.head.fwd(pre, relu=False, want_scale=keep, track=False)
        _log(self.head, self.norm5, pre.shape, f.shape)
        logits = ops.global_avgpool_logits(f, self.logit_temperature, self.logit_bias)
        if keep:
            st.update(tf=tf)
        return logits, st

    def _head_gradient(self, st, cls, H, W):
        """d logit[cls] / d (classifier input) [N, H, W, C]: rank one per image through the 1 x 1 classifier (bcos_head_rank1_grad_ex with
        mul = NULL), or the one-hot gradient and the classifier's input-gradient contraction where that launch does not apply"""
        d, _ = head_consumer(self.head, st["tf"], cls, None, self.logit_temperature).run(H, W, t_main=None, td=None, gated=False, track=False)
        return d

    def _backward_gen(self, x, st, cls, want_weights: bool, consume: bool, outs=None, functional=None, g_head=None):
        """Input-gradient pass of logit[cls[n]] for every image n over the state `st` of a kept forward; `consume` frees each kept
        tensor as soon as it has been used (last / only pass over this state)."""
        self._refuse(functional=functional, cotangent=g_head)
        N = x.shape[0]
        nb = len(self.blocks)
        d, d_pre = None, self.norm5
        for bi in range(nb - 1, -1, -1):
            blk, rec = self.blocks[bi], st["blocks"][bi]
            X, (H, W) = rec["X"], rec["hw"]
            if bi == nb - 1:
                d = self._head_gradient(st, cls, H, W)
                if consume:
                    st["tf"] = None
            # the first reader handled on the way back (head / transition) reads the whole block: it WRITES every channel of G
            G = torch.empty_like(X)
            ops.slice_affine_bwd_acc(d.view(-1, X.shape[-1]), G, x=X, scale=d_pre.scale, shift=d_pre.shift, relu=True, accumulate=False)
            del d
            yield
            c = X.shape[-1]
            for li in range(len(blk) - 1, -1, -1):
                ly = blk[li]
                c -= ly.growth
                a = ops.slice_affine_rows(G[..., c:c + ly.growth], mul=rec["s2"][li])     # (its row maxima attached; the 3 x 3 launch derives its per-image range)
                gl = ly.conv2.dgrad.run(a, H, W, track_absmax=ly.conv1.k_dgrad >= ops.F16X2_MIN_K, **mul_kwargs(rec["t1"][li]))
                del a
                dl = ly.conv1.dgrad.run(gl, H, W, track_absmax=False)
                del gl
                ops.slice_affine_bwd_acc(dl.view(-1, c), G[..., :c], x=X[..., :c], scale=ly.pre.scale, shift=ly.pre.shift, relu=True,
                                         accumulate=True)
                del dl
                if consume:
                    rec["s2"][li] = rec["t1"][li] = None
                yield
            g0 = ops.slice_affine_rows(G[..., :c], want_absmax=False)                # gather slice 0: d logit / d (pooled tensor)
            del G
            if consume:
                rec["X"] = None
            if bi > 0:
                tr, trec = self.transitions[bi - 1], st["trans"][bi - 1]
                pk, ps, pp = tr.pool
                th, tw = trec["hw"]
                gl = ops.avgpool2d_bwd(g0, th, tw, pk, ps, pp, mul=trec["t"], want_absmax=tr.conv.k_dgrad >= ops.F16X2_MIN_K)
                d = tr.conv.dgrad.run(gl, th, tw, track_absmax=False)
                d_pre = tr.pre
                if consume:
                    trec["t"] = None
                del gl, g0
                yield
        k, s, p = self.pool
        a_h, a_w = st["a0_hw"]
        gl = ops.avgpool2d_bwd(g0, a_h, a_w, k, s, p, mul=st["t0"], want_absmax=self.stem.k_dgrad >= ops.F16X2_MIN_K)
        if consume:
            st["t0"] = None
        gxn = torch.empty((N, st["H"], st["W"], 8), device=x.device, dtype=torch.float32)
        self.stem.dgrad.run(gl, st["H"], st["W"], out=gxn)                           # channels 0..5 of the padded buffer
        _, std = self._consts(x.device)
        return ops.finalize_explanation(gxn, st["x"], std, add_inverse=st["add_inverse"], want_weights=want_weights, want_contrib=True,
                                        weights_out=outs[0] if outs is not None else None,
                                        contrib_out=outs[1] if outs is not None else None)

    # ------------------------------------------------------------------------------------------------
    @staticmethod
    def _refuse(**kwargs):
        for name, val in kwargs.items():
            if val is not None:
                raise BcosHipError(f"densenet engine: `{name}=` is not built for this plan (DESIGN.md: DenseNet plan, scope); "
                                   "detach() the engine and use the module path, or a ResNet / ViT engine")

    @torch.no_grad()
    def forward(self, x: torch.Tensor, occlude=None, perturb=None, rise=None) -> torch.Tensor:
        self._refuse(occlude=occlude, perturb=perturb, rise=rise)
        return super().forward(x)

    @torch.no_grad()
    def explain(self, x: torch.Tensor, targets: Optional[torch.Tensor] = None, want_weights: bool = True, gates=None, cotangent=None,
                functional=None, occlude=None, perturb=None) -> Dict[str, torch.Tensor]:
        """Forward in explanation mode + input-gradient pass of the explained logit of every image (batched bcos/common.py:163-181).
        `targets` [N] int64 selects the logits (default: arg-max)."""
        self._refuse(occlude=occlude, perturb=perturb, functional=functional, gates=gates, cotangent=cotangent)
        return super().explain(x, targets, want_weights)

    explain_targets = FusedPlan._explain_targets


def attach(net) -> DenseNetEngine:
    """Compile `net` (a BcosifyNetwork around a torchvision-style DenseNetBcos) into the fused plan (bcos_hip/plan.py: attach)."""
    return plan.attach(net, DenseNetEngine)


detach = plan.detach
