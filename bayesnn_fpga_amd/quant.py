"""The fixed-point codes of the quantised LeNet-5 (csrc/qlenet5.hip; the contract is in include/bayesnn_fpga_amd.h): what QKeras'
``quantized_bits(W, I, alpha=1)`` and ``quantized_relu(W)`` of Hardware_Artifact/bayes_hw/models/t_qmodels_bayes.py keep of a value.  Both
round half to even and return int32 tensors; the arithmetic is float64, so a float32 input times a power of two is exact before rounding."""
import torch


def _check(W, I=0):
    if not (isinstance(W, int) and isinstance(I, int) and 2 <= W <= 8 and 0 <= I < W):
        raise ValueError(f"quant_tbit must be an int in [2, 8] and quant_ibit one in [0, quant_tbit - 1], got {W!r}, {I!r}")


def weight_codes(w, W, I=0):
    """Kernel / bias codes q = clip(rne(w * 2^F), -2^(W-1), 2^(W-1) - 1), F = W - 1 - I; the value is q * 2^-F."""
    _check(W, I)
    return torch.round(w.detach().double() * 2.0 ** (W - 1 - I)).clamp_(-2 ** (W - 1), 2 ** (W - 1) - 1).to(torch.int32)


def act_codes(v, W):
    """Activation codes a = clip(rne(v * 2^W), 0, 2^W - 1) (no integer bits); the value is a * 2^-W.  W = 8 is the kernel's input format."""
    _check(W)
    return torch.round(v.detach().double() * 2.0 ** W).clamp_(0, 2 ** W - 1).to(torch.int32)
