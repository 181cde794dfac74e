"""Shared by the validation-step tests and tests/golden/make_golden_val.py: the model state and the inputs of val_small.json, by formula.

State: the seed-333 initialisation with EVERY parameter and running statistic moved, each tensor from a generator seeded by its position
in the state dict (so the recipe does not depend on the order in which anybody walks the keys):
  running_mean  ~ N(0, 0.1^2)                      (not 0)
  running_var   uniform in [0.8, 1.25]             (not 1)
  weights with two or more dimensions  *= WEIGHT_SCALE * (1 + 0.05 * U(-1, 1))
  one-dimensional parameters (BatchNorm weight / bias, the conv bias)  += 0.02 * N(0, 1)
The ranges of the running statistics are those tests/test_autograd_ext_gpu.py records as safe: the untrained network's eval logits reach
1e5 at 64 x 96, and wider statistics make the fp32 oracle disagree with its own fp64 evaluation by up to 6e-3.
WEIGHT_SCALE: in eval mode nothing renormalises the untrained network, and with the initialisation's own weight magnitudes its logits reach
2e5 here.  The reference and the CPU oracle, both fp32 on the same weights, then differ by up to 0.5 in single logits (5e-6 of the largest
one: summation order), which no absolute tolerance meant for O(1) logits (val_small.json is held to atol 1e-5) can meet.  A common
factor of 0.88 on every convolution weight brings the logits to O(1) (largest ~1.5, median ~0.2), where that rounding noise is below 1e-5.
Inputs: sample i is make_inputs(1, H, W, seed=INPUT_SEED + i) of tests/util_inputs.py."""
import torch

from oracle import model as omodel
from util_inputs import make_inputs

STATE_SEED = 4242
INPUT_SEED = 11500         # of the seeds 9100, 9200, ... 11900 the one whose reference output keeps the largest top-two gap over ALL pixels (1.5e-4)
N_SAMPLES = 5
H, W = 64, 96
WEIGHT_SCALE = 0.88
MIN_REL_GAP = 1e-3          # top-two logit gap of every sampled pixel, relative to the larger magnitude (checked when the fixture is made)


def perturbed_state(seed: int = STATE_SEED):
    sd = omodel.init_state(333)
    for i, (k, v) in enumerate(sd.items()):
        g = torch.Generator().manual_seed(seed * 1000 + i)
        if k.endswith("num_batches_tracked"):
            continue
        if k.endswith("running_mean"):
            v.copy_(torch.randn(v.shape, generator=g) * 0.1)
        elif k.endswith("running_var"):
            v.copy_(torch.rand(v.shape, generator=g) * 0.45 + 0.8)
        elif v.dim() >= 2:
            v.mul_(WEIGHT_SCALE * (1.0 + 0.05 * (2.0 * torch.rand(v.shape, generator=g) - 1.0)))
        else:
            v.add_(0.02 * torch.randn(v.shape, generator=g))
    return sd


def val_inputs(n: int = N_SAMPLES, h: int = H, w: int = W, seed: int = INPUT_SEED):
    """(x [n,16,h,w] fp32, y [n,h,w] int64): sample i from its own seed."""
    xs, ys = zip(*(make_inputs(1, h, w, seed=seed + i) for i in range(n)))
    return torch.cat(xs), torch.cat(ys)


def rel_gap(logits: torch.Tensor) -> torch.Tensor:
    """[B,3,H,W] -> [B,H,W]: (top1 - top2) / max(|top1|, |top2|)."""
    top = torch.topk(logits.double(), 2, dim=1).values
    return (top[:, 0] - top[:, 1]) / top.abs().amax(dim=1).clamp_min(1e-30)
