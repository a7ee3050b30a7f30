"""The reference's training loss (scripts/losses.py:155-188 `CustomMSELoss`) on the HIP loss kernel of csrc/optim.hip."""
import torch

from . import lib as _lib
from . import ops


class CustomMSELoss(torch.nn.Module):
    """The reference's CustomMSELoss with its forward semantics: `((target - input) ** 2) * weights` when `weighted`, its mean
    for reduction 'mean', the unreduced tensor otherwise.

    weights: the latitude-weight tensor itself (its shape the trailing dimensions of the input).  The reference reads it from
    `constants*.zarr` under a Hydra config (losses.py:169-173); xarray and zarr are not dependencies here, so the caller
    passes the array.  It is kept as given: a float64 tensor, the reference's case, promotes the loss to float64.

    reduction 'mean' on device tensors is ops.mse_loss: one HIP pass that also writes the input's gradient when one is wanted.
    Any other reduction (the reference's "no reduction", used in validation only) stays in torch operators."""

    def __init__(self, weights=None, reduction: str = "mean", weighted: bool = False) -> None:
        super().__init__()
        self.reduction = reduction
        self.weighted = weighted
        if weighted and weights is None:
            raise _lib.DlwpError("CustomMSELoss: weighted=True needs the weights")
        self.spatial_weights = None
        self.weights = None if weights is None else torch.nan_to_num(torch.as_tensor(weights), nan=0.0)

    def forward(self, input, target):
        if self.weighted:
            if self.spatial_weights is None or self.spatial_weights.device != input.device:      # one copy per device, not
                self.spatial_weights = torch.as_tensor(self.weights, device=input.device)        # one per step
        if self.reduction == "mean":
            return ops.mse_loss(input, target, self.spatial_weights if self.weighted else None)
        d = (target - input) ** 2
        return d * self.spatial_weights if self.weighted else d
