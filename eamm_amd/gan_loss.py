"""The adversarial loss terms of the reference (modules/model.py:505-524 ``gen_gan`` / ``feature_matching``, :575-591 ``disc_gan``)
on ``eamm_amd.discriminator.MultiScaleDiscriminator`` and the pyramids of ``eamm_amd.perceptual.ImagePyramide``.  The least-squares
terms are means over the small prediction maps; feature matching is the deterministic L1 of ``perceptual_ops.l1_pair``, with a
gradient to both sides as in the reference.  GPU only: no CPU fallback."""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch

from .perceptual_ops import l1_pair


def _detach_kp(kp):
    return None if kp is None else {key: value.detach() for key, value in kp.items()}


def _scales(discriminator):
    return [name.replace("-", ".") for name in discriminator.discs.keys()]


def generator_gan_loss(discriminator, pyramide_generated: Dict[str, torch.Tensor], pyramide_real: Dict[str, torch.Tensor], kp=None,
                       weight: float = 1.0, feature_matching_weights: Optional[Sequence[float]] = None) -> Dict[str, torch.Tensor]:
    """``{'gen_gan': weight * sum_scales mean((1 - D(generated))^2)}`` and, unless all ``feature_matching_weights`` are zero,
    ``'feature_matching': sum_scales sum_i w_i * mean|f_i(real) - f_i(generated)|`` (zero weights skipped).  ``kp``: the driving
    key points (detached here), for a discriminator with ``use_kp``.  The discriminator is called twice, as the reference does
    (with spectral norm in ``.train()``: two power iterations)."""
    if weight == 0:
        return {}
    maps_generated = discriminator(pyramide_generated, kp=_detach_kp(kp))
    maps_real = discriminator(pyramide_real, kp=_detach_kp(kp))
    values = {}
    total = 0
    for scale in _scales(discriminator):
        total = total + weight * ((1 - maps_generated["prediction_map_" + scale]) ** 2).mean()
    values["gen_gan"] = total
    fm = [float(w) for w in feature_matching_weights] if feature_matching_weights is not None else []
    if sum(fm) != 0:
        total = 0
        for scale in _scales(discriminator):
            key = "feature_maps_" + scale
            for i, (a, b) in enumerate(zip(maps_real[key], maps_generated[key])):
                if i >= len(fm) or fm[i] == 0:
                    continue
                total = total + l1_pair(a, b, fm[i])
        values["feature_matching"] = total
    return values


def discriminator_gan_loss(discriminator, pyramide_real: Dict[str, torch.Tensor], pyramide_generated: Dict[str, torch.Tensor], kp=None,
                           weight: float = 1.0) -> Dict[str, torch.Tensor]:
    """``{'disc_gan': weight * sum_scales mean((1 - D(real))^2 + D(generated.detach())^2)}``: the generated side is detached, so
    the gradient reaches the discriminator's parameters only."""
    generated = {key: value.detach() for key, value in pyramide_generated.items()}
    maps_generated = discriminator(generated, kp=_detach_kp(kp))
    maps_real = discriminator(pyramide_real, kp=_detach_kp(kp))
    total = 0
    for scale in _scales(discriminator):
        key = "prediction_map_" + scale
        total = total + weight * ((1 - maps_real[key]) ** 2 + maps_generated[key] ** 2).mean()
    return {"disc_gan": total}
