"""The Occlusion baseline explainer (reference interpretability/explanation_methods/explainers/occlusion.py:7-111) on the HIP path.

The reference's masks are rectangles (occlusion.py:46-49), so a mask is four integers (r0, r1, c0, c1) and the bank an int32 tensor
[n, 4].  With a fused engine attached the occluded copies are never built: `engine.forward(img, occlude=bank[lo:hi])` prepares them
from the one image (bcos_prep_input_occluded).  The logits stay on the device in one [n, classes] buffer and ONE launch of
bcos_occlusion_accumulate forms the maps of the requested classes -- where the reference stores `img * masks` as [n, 6, H, W], copies
every logit row to the host and builds [n, classes, H, W] there (occlusion.py:80-108).  Without an engine the chunks are masked with
torch ops and run through `self.model`; the same kernel finishes the call.
"""
import numpy as np
import torch

from interpretability.explanation_methods.utils import ExplainerBase

__all__ = ["Occlusion"]

ENGINE_BATCH_SIZE = 256      # occluded copies per engine.forward call (the fused plan's throughput is flat from about there)


class Occlusion(ExplainerBase):
    def __init__(self, model, stride=32, ks=32, batch_size=8, only_positive=False):
        super().__init__(model)
        self.max_imgs_bs = 1                          # images are processed one at a time (occlusion.py:13)
        if isinstance(stride, int):
            stride = (stride, stride)
        self.stride = tuple(int(s) for s in stride)
        self.ks = int(ks)
        # copies per model call.  The reference's configurations size it for the memory of the nn.Module path (8, or 1 for the "-TI"
        # ones); the fused engine takes at least ENGINE_BATCH_SIZE (`engine_batch_size`, settable).  Results do not depend on either.
        self.batch_size = int(batch_size)
        self.engine_batch_size = max(self.batch_size, ENGINE_BATCH_SIZE)
        self.only_positive = bool(only_positive)
        self.masks = None                             # int32 [n, 4] on the host: rows [r0, r1) x columns [c0, c1)
        self.n_part = None                            # int64 [n]: pixels of every mask
        self._masks_hw = None
        self._dev_masks = {}

    # ---------------------------------------------------------------------------------------------------------------------------------
    def make_masks(self, img):
        """The rectangle bank for images of img's size, by the reference's rule (occlusion.py:32-61) and with its quirks: the SLOW index
        of the position grid (`wpos`) selects the columns, and an odd `ks` gives a window of ks - 1.  ValueError where the reference
        asserts (a size that is no multiple of the stride) and where it would return NaN (an empty rectangle: 0 / 0 in its
        `influence`): non-square images and ks = 1."""
        H, W = int(img.shape[-2]), int(img.shape[-1])
        s0, s1 = self.stride
        if H % s0 or W % s1:
            raise ValueError(f"Occlusion: the image size {H}x{W} is not a multiple of the stride {self.stride}")
        ks = self.ks
        total = W // s1 * H // s0
        strided_shape = (H // s0, W // s1)
        ks2, off = ((ks - 1) // 2, 0) if ks % 2 == 1 else (ks, 1)
        # (the reference's loop over idx, occlusion.py:43-49, for all masks at once)
        wpos, hpos = np.unravel_index(np.arange(total), strided_shape)
        r0, r1 = np.maximum(0, (hpos + off) * s0 - ks2), hpos * s0 + ks2
        c0, c1 = np.maximum(0, (wpos + off) * s1 - ks2), wpos * s1 + ks2
        rects = np.stack([np.minimum(r0, H), np.minimum(r1, H), np.minimum(c0, W), np.minimum(c1, W)], axis=1).astype(np.int64)   # (what a slice keeps of the image)
        empty = (rects[:, 0] >= rects[:, 1]) | (rects[:, 2] >= rects[:, 3])
        if empty.any():
            raise ValueError(f"Occlusion: mask {int(np.argmax(empty))} of {total} is empty for a {H}x{W} image with stride {self.stride}, "
                             f"ks {ks} (the reference attributes 0 / 0 = NaN there)")
        self.masks = torch.from_numpy(rects.astype(np.int32))
        self.n_part = torch.from_numpy((rects[:, 1] - rects[:, 0]) * (rects[:, 3] - rects[:, 2]))
        self._masks_hw = (H, W)
        self._dev_masks = {}

    def _bank(self, img):
        if self.masks is None or self._masks_hw != (int(img.shape[-2]), int(img.shape[-1])):
            self.make_masks(img)
        key = str(img.device)
        if key not in self._dev_masks:
            self._dev_masks[key] = self.masks.to(img.device)
        return self._dev_masks[key]

    # ---------------------------------------------------------------------------------------------------------------------------------
    def _logits(self, img, bank):
        """-> (org [1, CL], pert [n, CL]) on img's device: the model on the image and on its n occluded copies"""
        model = self.model
        engine = getattr(model, "_bcos_engine", None)
        if engine is not None and (getattr(model, "training", False) or not hasattr(engine, "forward")):
            engine = None
        n = bank.shape[0]
        org = (engine.forward(img) if engine is not None else model(img)).detach()
        if org.dim() != 2 or org.shape[0] != 1:
            raise ValueError(f"Occlusion: the model must map one image to [1, classes], got {tuple(org.shape)}")
        org = org.float()
        pert = torch.empty((n, org.shape[1]), device=org.device, dtype=torch.float32)
        if engine is not None:
            step = self.engine_batch_size
            for lo in range(0, n, step):
                pert[lo:lo + step] = engine.forward(img, occlude=bank[lo:lo + step])
            return org, pert
        H, W = img.shape[-2:]
        rows = torch.arange(H, device=img.device)[None, :]
        cols = torch.arange(W, device=img.device)[None, :]
        step = self.batch_size
        for lo in range(0, n, step):
            r = bank[lo:lo + step].long()
            in_r = (rows >= r[:, 0:1]) & (rows < r[:, 1:2])
            in_c = (cols >= r[:, 2:3]) & (cols < r[:, 3:4])
            keep = (~(in_r[:, :, None] & in_c[:, None, :])).to(img.dtype)
            pert[lo:lo + step] = model(img * keep[:, None]).detach()               # masked_input = img * masks (occlusion.py:80)
        return org, pert

    def _maps(self, img, targets):
        """[T, H, W] maps of ONE image for `targets` (None: every class)"""
        from bcos_hip import ops
        if img.dim() != 4 or img.shape[0] != 1:
            raise ValueError(f"Occlusion: one image [1, C, H, W] at a time, got {tuple(img.shape)}")
        bank = self._bank(img)
        org, pert = self._logits(img, bank)
        H, W = img.shape[-2:]
        return ops.occlusion_accumulate(org.reshape(-1).contiguous(), pert, bank, H, W, targets=targets, only_positive=self.only_positive,
                                        rects_host=self.masks)

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
            raise ValueError(f"Occlusion: need one target per image: got {len(target)} targets for {n} images")
        return [int(t) for t in target]

    @torch.no_grad()
    def attribute(self, img, target, return_all=False):
        """-> [N, 1, H, W] (the map of `target`, one per image), or [N, classes, H, W] with return_all; on img's device."""
        N = img.shape[0]
        tg = None if return_all else self._target_list(target, N)
        return torch.stack([self._maps(img[i:i + 1], None if return_all else [tg[i]]) for i in range(N)], dim=0)

    @torch.no_grad()
    def attribute_selection(self, img, targets):
        """ONE image and T targets -> [T, 1, H, W] (occlusion.py:110-111), computing the requested classes only."""
        return self._maps(img, self._target_list(targets, np.asarray(torch.as_tensor(targets).cpu()).size))[:, None]
