"""The frozen pretrained policy the `--kl_coef` penalty is measured against (KL penalty).

A second U-Net of the policy's configuration holding a copy of its flat parameters, taken right after the pretrained weights are loaded:
before LoRA adapters are attached and before a resumed run overwrites anything, so the reference is the `pretrained_model` whatever the
policy has become.  Forward-only weight planes, no gradient buffer, no optimizer state; nothing writes to it afterwards.
"""
import torch

from .. import lib as L
from ..models.unet import UNet2DCondition


def check_kl_args(kl_coef, eta):
    """The entrypoint's argument check, as a plain function: a message to exit with, or None.  With eta == 0 the DDIM step is deterministic:
    sigma_c is then the 1e-6 floor of the log-prob and a KL in its units means nothing."""
    kl_coef = float(kl_coef)
    if not kl_coef >= 0.0 or kl_coef == float("inf"):
        return f"--kl_coef must be a finite number >= 0, got {kl_coef}"
    if kl_coef > 0.0 and float(eta) == 0.0:
        return (f"--kl_coef {kl_coef} needs a stochastic sampler: with --eta 0 the policy's standard deviation is the 1e-6 floor of the "
                f"log-prob and the KL penalty is meaningless")
    return None


class KLReference:
    """`KLReference(unet)` snapshots `unet.params` now.  `forward` is the inference forward (no tape) of the snapshot."""

    def __init__(self, unet):
        if unet.lora is not None:
            raise ValueError("take the KL reference before the LoraStore is attached: it must hold the pretrained weights")
        self.unet = UNet2DCondition(unet.cfg, unet.device)
        self.unet.params.flat.copy_(unet.params.flat)
        self._packed_for = None
        self._pack()

    @property
    def params(self):
        return self.unet.params

    def _pack(self):
        """Forward-only planes for the datapath in force (none on fp32); redone if the datapath changed or the registry was emptied."""
        dp = L.current_datapath()
        probe = next(v for n, v in self.unet.params.views.items() if n.endswith(".kernel"))
        if dp == "fp32" or (self._packed_for == dp and probe.data_ptr() in L.PACKED):
            return
        self.unet.params.pack_bf16(bwd=False)
        self._packed_for = dp

    def forward(self, sample, timesteps, context):
        self._pack()
        return self.unet.forward(sample, timesteps, context, tape=None)

    def nbytes(self):
        """Device bytes of the parameters (the planes are counted by whoever measures torch.cuda.memory_allocated around the constructor)."""
        return self.unet.params.flat.numel() * 4
