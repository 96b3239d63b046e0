#!/usr/bin/env python3
"""Golden fixture of the reference's default training objective (MSE + recon_w L1 + tv_w TV), made by RUNNING THE REFERENCE.

Run where the reference is available only (the GPU tests read the .npz, never the reference):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_objective_golden.py --reference-src <reference checkout>/src

Taken from the reference, unmodified: ``clip_feature_codec.diffusion.scheduler.NoiseScheduler`` (imported: ``q_sample`` and
``predict_x0_from_eps``) and ``total_variation`` of ``train/diffusion_train.py``.  That file cannot be imported (``open_clip`` is
absent), so its source is parsed with ``ast`` and the one function definition is compiled at run time --
nothing of it is restated here.  The terms are combined as its lines 124-129 do (``F.mse_loss`` / ``F.l1_loss``), in fp32 on the CPU.

Stored (data only, all from the fp32 run): x0, t, noise, eps_hat, x_t, the gathered coefficients a / s, raw (= predict_x0_from_eps
before the clamp), the four loss terms (total, mse, l1, tv; l1 and tv unweighted), d loss / d eps_hat from ``loss.backward()``, and
the clamp mask ``-1 <= raw <= 1``.

Before writing, the script asserts that the inputs exercise what the tests are about: clamped and unclamped samples, exact ties
(sgn(0) in the L1 and the TV term) and an auxiliary gradient that is not negligible next to the MSE part.
"""
from __future__ import annotations

import argparse
import ast
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

HERE = Path(__file__).resolve().parent
B, C, S = 6, 3, 32
T_STEPS = (0, 120, 400, 700, 930, 999)
RECON_W, TV_W = 0.05, 1e-4


def reference_total_variation(src: Path):
    """``total_variation`` exactly as the reference's train/diffusion_train.py defines it."""
    path = src / "clip_feature_codec" / "train" / "diffusion_train.py"
    tree = ast.parse(path.read_text(encoding="utf-8"))
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "total_variation"]
    assert len(fn) == 1, "total_variation not found in the reference"
    ns = {"torch": torch}
    exec(compile(ast.Module(body=fn, type_ignores=[]), str(path), "exec"), ns)
    return ns["total_variation"]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference-src", required=True, help="the reference checkout's src/ directory")
    ap.add_argument("--out", default=str(HERE / "train_objective.npz"))
    args = ap.parse_args()
    src = Path(args.reference_src).resolve()
    sys.path.insert(0, str(src))
    import clip_feature_codec
    assert str(src) in clip_feature_codec.__file__, clip_feature_codec.__file__
    from clip_feature_codec.diffusion.scheduler import NoiseScheduler
    total_variation = reference_total_variation(src)

    g = torch.Generator().manual_seed(20250)
    x0 = torch.randint(0, 256, (B, C, S, S), generator=g).float() / 127.5 - 1.0
    x0[0, :, 4:8, :] = 1.0             # exact +1 / -1: with eps_hat != noise the clamp then gives p == x0 exactly
    x0[1, :, 20:24, :] = -1.0
    t = torch.tensor(T_STEPS, dtype=torch.long)
    noise = torch.randn(B, C, S, S, generator=g)
    eps_hat = (noise + 0.3 * torch.randn(B, C, S, S, generator=g)).requires_grad_(True)

    sch = NoiseScheduler(timesteps=1000, schedule="cosine", device="cpu")
    x_t = sch.q_sample(x0, t, noise)
    raw = sch.predict_x0_from_eps(x_t, t, eps_hat)
    x0_pred = raw.clamp(-1, 1)
    mse = F.mse_loss(eps_hat, noise)
    l1 = F.l1_loss(x0_pred, x0)
    tv = total_variation(x0_pred)
    loss = mse
    loss = loss + RECON_W * l1
    loss = loss + TV_W * tv
    loss.backward()
    d_eps = eps_hat.grad.detach()
    raw = raw.detach(); p = x0_pred.detach(); eps = eps_hat.detach()
    mask = (raw >= -1) & (raw <= 1)

    # ---- the fixture must not go blind ----------------------------------------------------------------------------------------
    share = mask.float().mean(dim=(1, 2, 3))
    print("unclamped share per sample:", [round(float(v), 3) for v in share])
    assert int((share > 0.9).sum()) >= 2 and int(((share > 0.1) & (share < 0.9)).sum()) >= 1 and int((share == 0).sum()) >= 1, share
    tie_l1 = float((p == x0).float().mean())
    tie_tv = float(((p[:, :, 1:, :] - p[:, :, :-1, :]) == 0).float().mean())
    print(f"p == x0 share {tie_l1:.4f}; vertical TV differences equal to 0: {tie_tv:.4f}")
    assert tie_l1 > 0.01 and tie_tv > 0.05, (tie_l1, tie_tv)
    n = eps.numel()
    g_mse = 2.0 * (eps - noise) / n
    aux = d_eps - g_mse
    ratio = aux.abs().amax(dim=(1, 2, 3)) / g_mse.abs().amax(dim=(1, 2, 3))
    print("max|aux| / max|mse part| per sample:", [round(float(v), 3) for v in ratio])
    assert float(ratio.max()) > 0.1, ratio

    a = sch.sqrt_alphas_cumprod[t].contiguous()
    s = sch.sqrt_one_minus_alphas_cumprod[t].contiguous()
    np.savez_compressed(
        args.out, x0=x0.numpy(), t=t.numpy(), noise=noise.numpy(), eps_hat=eps.numpy(), x_t=x_t.numpy(), a=a.numpy(), s=s.numpy(),
        raw=raw.numpy(), loss_terms=np.array([float(v.detach()) for v in (loss, mse, l1, tv)], dtype=np.float32),
        d_eps=d_eps.numpy(), mask=mask.numpy(), weights=np.array([RECON_W, TV_W], dtype=np.float64))
    print("wrote", args.out, Path(args.out).stat().st_size, "bytes")


if __name__ == "__main__":
    main()
