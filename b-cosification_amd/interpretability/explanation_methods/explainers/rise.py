"""The RISE baseline explainer (reference interpretability/explanation_methods/explainers/rise.py:16-101) on the HIP path.

The reference draws n random s x s grids, upsamples each bilinearly (skimage `resize`), crops it at a random shift and keeps the float
masks [n, 1, H, W] (rise.py:34-57); it multiplies the image by all of them, moves every probability row to the host and reduces them
over the masks with one matrix product (rise.py:79-95).  A mask is its bit grid and two shifts, so here the bank is an ops.RiseBank --
int32 rows [n, 4] of (bits_lo, bits_hi, shift_r, shift_c) and s -- and the kernels evaluate the mask values (include/bcos_hip.h).  With
a fused engine attached neither masks nor copies are built: `engine.forward(img, rise=bank[lo:hi])` prepares the copies from the one
image; the logits stay on the device, the scores of the requested classes come from bcos_class_scores and ONE launch of
bcos_rise_accumulate forms their maps.  Without an engine the chunks are `img * ops.rise_masks(...)` through `self.model`; the same
accumulate call finishes.

The upsampling is the closed form of `scipy.ndimage.zoom(grid, U / s, order=1, mode="mirror", grid_mode=True)`, which current skimage
calls for the reference's arguments; skimage itself was not available, so equality with skimage's own bits is unverified.
"""
import numpy as np
import torch

from interpretability.explanation_methods.explanation_configs import explainer_configs
from interpretability.explanation_methods.utils import ExplainerBase

__all__ = ["RISE"]

ENGINE_BATCH_SIZE = 256      # masked copies per engine.forward call, as Occlusion


class RISE(ExplainerBase):
    def __init__(self, model, batch_size=2, n=6000, s=6, p1=0.1, **kwargs):
        # **kwargs as the reference: its named configuration passes "p" (explanation_configs.py), which the reference swallows here, so
        # p1 stays 0.1 under "default" -- the quirk is kept
        super().__init__(model)
        self.max_imgs_bs = 1                          # images are processed one at a time (rise.py:28)
        self.batch_size = int(batch_size)             # copies per model call on the module path
        self.engine_batch_size = max(self.batch_size, ENGINE_BATCH_SIZE)
        self.N, self.s, self.p1 = int(n), int(s), float(p1)
        if not 2 <= self.s <= 8:
            raise ValueError(f"RISE: s must be in 2..8 (the grid of a mask is one 64-bit word), got {s}")
        if self.N <= 0 or not self.p1 > 0:
            raise ValueError(f"RISE: n and p1 must be positive, got n = {n}, p1 = {p1}")
        to_prob = getattr(model, "to_probabilities", None)      # B-cos networks: sigmoid; otherwise softmax over the row (rise.py:22-24)
        self.score_mode = "softmax" if to_prob is None else "sigmoid" if to_prob is torch.sigmoid else None
        self._to_prob = to_prob
        self._banks = {}                              # (H, W) -> host bank, (H, W, device) -> device bank

    @classmethod
    def from_config(cls, model, config_name="default", **overrides):
        """the named configuration of explanation_configs.py ("default": n = 500, s = 8, batch_size = 8, and the swallowed "p")"""
        return cls(model, **{**explainer_configs["RISE"][config_name], **overrides})

    # ---------------------------------------------------------------------------------------------------------------------------------
    def make_bank(self, H, W):
        """The bank for H x W images from the random stream of the reference's `np.random.seed(42)` (a RandomState of its own: the
        global state is not touched) in the reference's order: `rand(N, s, s) < p1`, then per mask `randint(0, cell_h)` and
        `randint(0, cell_w)` (rise.py:35-51).  -> ops.RiseBank in host memory."""
        from bcos_hip import ops
        key = (int(H), int(W))
        if key not in self._banks:
            s, rs = self.s, np.random.RandomState(42)
            cell_h, cell_w = -(-key[0] // s), -(-key[1] // s)
            grid = rs.rand(self.N, s, s) < self.p1
            shifts = np.empty((self.N, 2), dtype=np.int64)
            for i in range(self.N):
                shifts[i, 0] = rs.randint(0, cell_h)
                shifts[i, 1] = rs.randint(0, cell_w)
            bits = (grid.reshape(self.N, s * s).astype(np.uint64) << np.arange(s * s, dtype=np.uint64)[None]).sum(1, dtype=np.uint64)
            rows = np.empty((self.N, 4), dtype=np.int32)
            rows[:, 0] = (bits & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
            rows[:, 1] = (bits >> np.uint64(32)).astype(np.uint32).view(np.int32)
            rows[:, 2:] = shifts
            host = torch.from_numpy(rows)
            self._banks[key] = ops.RiseBank(host, s, host)
        return self._banks[key]

    def _bank(self, img):
        H, W = int(img.shape[-2]), int(img.shape[-1])
        key = (H, W, str(img.device))
        if key not in self._banks:
            host = self.make_bank(H, W)
            self._banks[key] = host if img.device.type == "cpu" else host.to(img.device)
        return self._banks[key]

    # ---------------------------------------------------------------------------------------------------------------------------------
    def _scores(self, logits, targets):
        """logits [k, CL] on the device -> float32 scores [k, T] of `targets` (None: every class)"""
        from bcos_hip import ops
        if logits.dim() != 2:
            raise ValueError(f"RISE: the model must map k images to [k, classes], got {tuple(logits.shape)}")
        logits = logits.detach().float().contiguous()
        if targets is None or self.score_mode is None:
            prob = (self._to_prob(logits) if self.score_mode is None else torch.sigmoid(logits) if self.score_mode == "sigmoid"
                    else torch.softmax(logits, dim=1))
            return prob if targets is None else prob[:, ops.check_targets(targets, logits.shape[1], "RISE: targets").to(prob.device)]
        k = logits.shape[0]
        return torch.stack([ops.class_scores(logits, [t], group=k, mode=self.score_mode) for t in targets], dim=1)

    def _maps(self, img, targets):
        """[T, H, W] maps of ONE image for `targets` (None: every class)"""
        from bcos_hip import ops
        if img.dim() != 4 or img.shape[0] != 1:
            raise ValueError(f"RISE: one image [1, C, H, W] at a time, got {tuple(img.shape)}")
        model = self.model
        engine = getattr(model, "_bcos_engine", None)
        if engine is not None and (getattr(model, "training", False) or not hasattr(engine, "forward")):
            engine = None
        bank = self._bank(img)
        H, W = img.shape[-2:]
        n, parts = len(bank), []
        step = self.engine_batch_size if engine is not None else self.batch_size
        for lo in range(0, n, step):
            if engine is not None:
                out = engine.forward(img, rise=bank[lo:lo + step])
            else:
                masks = ops.rise_masks(bank, H, W, first=lo, n=min(step, n - lo))
                out = model(img * masks[:, None]).detach()                          # stack = masks * x (rise.py:79)
            parts.append(self._scores(out, targets))
        scores = parts[0] if len(parts) == 1 else torch.cat(parts)
        return ops.rise_accumulate(scores.contiguous(), bank, H, W, self.p1)

    @staticmethod
    def _target_list(target, n):
        if torch.is_tensor(target):
            target = target.detach().cpu().reshape(-1).tolist()
        elif isinstance(target, (list, tuple, np.ndarray)):
            target = [int(t) for t in np.asarray(target).reshape(-1)]
        else:
            target = [int(target)]
        if len(target) == 1 and n > 1:
            target = target * n
        if len(target) != n:
            raise ValueError(f"RISE: need one target per image: got {len(target)} targets for {n} images")
        return [int(t) for t in target]

    @torch.no_grad()
    def attribute(self, img, target, return_all=False):
        """-> [1, 1, H, W] per image (the map of its target), concatenated over the images; with return_all the maps of every class,
        [CL, 1, H, W] per image (rise.py:94-98); on img's device."""
        N = img.shape[0]
        if return_all:
            return torch.cat([self._maps(img[i:i + 1], None)[:, None] for i in range(N)], dim=0)
        tg = self._target_list(target, N)
        return torch.cat([self._maps(img[i:i + 1], [tg[i]])[None] for i in range(N)], dim=0)

    @torch.no_grad()
    def attribute_selection(self, img, targets):
        """ONE image and T targets -> [T, 1, H, W] (rise.py:100-101), computing the requested classes only."""
        return self._maps(img, self._target_list(targets, np.asarray(torch.as_tensor(targets).cpu()).size))[:, None]
