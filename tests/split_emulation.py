"""CPU emulation of the f16x3 arithmetic (CCN_DTYPE_F16X3), for the oracle.

``SplitFunctional`` is a drop-in for ``torch.nn.functional``: handed to ``oracle.ref_unet`` (``with emulated(): ...``) it replaces the
convolutions the mode runs on split operands and leaves everything else to torch.

  scope   a 3x3 stride-1 conv with Cin == Cout (the ResBlock convs) or a ConvTranspose, with Cout >= ``min_cout`` (64: the N tiles of
          64 and 128 that the ws / fr kernels carry; narrower layers, stem, head and stride-2 convs run the fp32 kernels).
          ``min_cout=0`` splits every ResBlock conv and ConvTranspose, ``every_conv=True`` every convolution.
  split   hi = RNE_T(x), lo = RNE_T(x - hi) with torch's casts, T = fp16 (or bf16); fp16 hi saturates at +-65504 like the kernel
  weights scaled per tensor by the power of two s with max|w| s in [2^13, 2^14) before the split (fp16 only), undone on the result
  product a_lo w_hi + a_hi w_lo + a_hi w_hi: three fp32 convolutions by torch's CPU kernels, summed in fp32, then / s, then + bias
  ``flush=True`` zeroes fp16-subnormal hi / lo operands (what an MFMA that flushed them would see).
"""
from __future__ import annotations

import contextlib

import torch
import torch.nn.functional as TF


def weight_scale(w: torch.Tensor) -> float:
    mx = float(w.abs().max())
    if mx == 0.0 or not torch.isfinite(torch.tensor(mx)):
        return 1.0
    e = torch.frexp(torch.tensor(mx, dtype=torch.float32))[1].item()      # mx in [2^(e-1), 2^e)
    return float(2.0 ** min(14 - e, 126))


def split(x: torch.Tensor, T=torch.float16, flush: bool = False):
    if T == torch.float16:
        x = x.clamp(-65504.0, 65504.0)
    hi = x.to(T).float()
    lo = (x - hi).to(T).float()
    if flush and T == torch.float16:
        tiny = 2.0 ** -14
        hi = torch.where(hi.abs() < tiny, torch.zeros_like(hi), hi)
        lo = torch.where(lo.abs() < tiny, torch.zeros_like(lo), lo)
    return hi, lo


class SplitFunctional:
    def __init__(self, T=torch.float16, min_cout: int = 64, every_conv: bool = False, flush: bool = False, scale: bool = True):
        self.T, self.min_cout, self.every_conv, self.flush, self.scale = T, min_cout, every_conv, flush, scale
        self.n_split = self.n_plain = 0

    def __getattr__(self, name):
        return getattr(TF, name)

    def _three(self, conv, x, w, bias, **kw):
        s = weight_scale(w) if (self.scale and self.T == torch.float16) else 1.0
        wh, wl = split(w * s, self.T, self.flush)
        ah, al = split(x, self.T, self.flush)
        y = conv(al, wh, None, **kw) + conv(ah, wl, None, **kw)
        y = y + conv(ah, wh, None, **kw)
        y = y * (1.0 / s)
        self.n_split += 1
        return y if bias is None else y + bias.view(1, -1, 1, 1)

    def conv2d(self, x, w, bias=None, stride=1, padding=0, **kw):
        in_scope = stride == 1 and tuple(w.shape[2:]) == (3, 3) and w.shape[0] == w.shape[1] and w.shape[0] >= self.min_cout
        if in_scope or self.every_conv:
            return self._three(TF.conv2d, x, w, bias, stride=stride, padding=padding, **kw)
        self.n_plain += 1
        return TF.conv2d(x, w, bias, stride=stride, padding=padding, **kw)

    def conv_transpose2d(self, x, w, bias=None, stride=1, padding=0, **kw):
        if w.shape[1] >= self.min_cout or self.every_conv:
            return self._three(TF.conv_transpose2d, x, w, bias, stride=stride, padding=padding, **kw)
        self.n_plain += 1
        return TF.conv_transpose2d(x, w, bias, stride=stride, padding=padding, **kw)


@contextlib.contextmanager
def emulated(**kw):
    """Inside the block ``oracle.ref_unet`` computes with the emulated arithmetic; yields the SplitFunctional (its counters)."""
    from oracle import ref_unet
    f = SplitFunctional(**kw)
    old = ref_unet.F
    ref_unet.F = f
    try:
        yield f
    finally:
        ref_unet.F = old
