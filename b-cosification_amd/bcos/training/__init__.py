"""Trainer-side pieces that touch the hot path's modules: the learnable / scheduled exponent B (`hooks`) and the
adaptive gradient clipping every B-cosification recipe runs before its optimizer step (`agc`: one `bcos_agc_clip` call per parameter list;
the recipes' losses, the CLIP recipe's SigLipLoss among them, are in `bcos.modules.losses`).  The trainer itself (PyTorch-Lightning module, optimiser factory, schedulers, EMA) is out
of scope: the recipes' Adam / AdamW is torch.optim's."""
from .hooks import Hook, forward_hook_fn, setup_b_parameters  # noqa: F401
