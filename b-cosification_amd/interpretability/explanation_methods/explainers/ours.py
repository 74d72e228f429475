"""The model-inherent B-cos explanations (reference interpretability/explanation_methods/explainers/ours.py:8-76)."""
import torch

from interpretability.explanation_methods.utils import ExplainerBase

__all__ = ["Ours", "OursRelative"]


def Ours(model):
    assert hasattr(model, "attribute_selection"), \
        "model requires a 'attribute_selection' attribute for our explanation method!"
    return model


class _MeanSubtracted(torch.nn.Module):
    def __init__(self, model):
        super().__init__()
        self.model = model

    def forward(self, *args, **kwargs):
        out = self.model(*args, **kwargs)
        assert out.dim() == 2, f"model output must be 2D (batch_size, num_classes) but is {out.ndim}D"
        return out - out.mean(dim=1, keepdim=True)


class OursRelative(ExplainerBase):
    """Mean-corrected explanations: Input x Gradient of y - mean_k y.

    With a fused engine attached to the model (bcos_hip.engine.attach / vit_engine.attach) and the model not in train(), y_t - mean_k y_k
    is explained as a linear functional of the logits by ONE fused pass (bcos_hip.functional.LogitFunctional.mean_corrected: the network is
    linear in the head cotangent in explanation mode), and `attribute_selection` runs one forward for all targets where the reference
    re-runs it per target.  Without an engine: autograd over the per-layer modules, as the reference."""

    def __init__(self, model):
        assert hasattr(model, "explanation_mode"), \
            "model requires a 'explanation_mode' attribute for our (relative) explanation method!"
        super().__init__(model)
        from interpretability.explanation_methods.explainers.captum import IxG
        self.explainer = IxG(_MeanSubtracted(model))

    def _engine(self):
        engine = getattr(self.model, "_bcos_engine", None)
        if engine is not None and getattr(engine, "supports_explain", True) and hasattr(engine, "explain_functionals") \
                and not getattr(self.model, "training", False):
            return engine
        return None

    @staticmethod
    def _functional(engine, target, n):
        from bcos_hip.functional import LogitFunctional
        t = torch.as_tensor(target).reshape(-1)
        if t.numel() == 1 and n > 1:
            t = t.expand(n)
        if t.numel() != n:
            raise ValueError(f"need one target per sample: got {t.numel()} targets for {n} samples")
        return LogitFunctional.mean_corrected(t, engine.n_logits())

    def attribute(self, image, target, **kwargs):
        engine = self._engine()
        if engine is not None:
            out = engine.explain(image, functional=self._functional(engine, target, image.shape[0]))
            return image.detach() * out["dynamic_linear_weights"]
        with self.model.explanation_mode():
            return self.explainer.attribute(image, target)

    def attribute_selection(self, image, targets, **kwargs):
        engine = self._engine()
        if engine is not None and len(targets):
            fs = [self._functional(engine, t, image.shape[0]) for t in targets]
            w = engine.explain_functionals(image, fs, want_weights=True)["dynamic_linear_weights"]      # [N, T, 6, H, W]
            return (image.detach().unsqueeze(1) * w).transpose(0, 1).reshape(-1, *image.shape[1:])       # target-major, as the cat below
        return torch.cat([self.attribute(image, t) for t in targets], dim=0)
