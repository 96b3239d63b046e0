"""The training-step oracle (oracle/ref_train.py) against the fixture made by the reference's own modules
(tests/golden/train_step.npz, tests/golden/make_train_golden.py).  CPU only."""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "clip-neural-image-conpression_amd")]

from clip_feature_codec.utils import synth  # noqa: E402
from oracle import ref_unet, ref_train  # noqa: E402

GOLD = np.load(ROOT / "tests" / "golden" / "train_step.npz")
SCHED = np.load(ROOT / "tests" / "golden" / "scheduler.npz")


def _sample(t, n=64):
    f = t.detach().flatten()
    step = max(1, f.numel() // n)
    return f[::step][:n].numpy()


def test_oracle_training_step_matches_reference_loss_gradients_and_adamw():
    sd = ref_unet.as_torch_sd(synth.synth_state_dict(synth.unet_param_spec(512, 32, (1, 2))))
    # the reference's cosine tables as stored with the fixtures (tests/test_oracle_golden.py checks the oracle's own against them):
    # torch's CPU cos rounds differently in the last bit on some host CPUs, and q_sample's elementwise ops are exact on every host
    tables = {k.split(".", 1)[1]: torch.from_numpy(SCHED[k]) for k in SCHED.files if k.startswith("cosine.")}
    x0, z, t, noise = (torch.from_numpy(GOLD[k]) for k in ("x0", "z", "t", "noise"))
    loss, grads, eps, x_t = ref_train.train_step_grads(sd, tables, x0, z, t, noise)
    assert np.array_equal(x_t.numpy(), GOLD["x_t"])                     # q_sample: same fp32 ops, bit-exact
    assert abs(float(loss) - float(GOLD["loss"])) < 1e-6
    names = [str(k) for k in GOLD["names"]]
    assert set(names) == set(grads)
    for k in names:
        g = grads[k]
        scale = max(float(g.abs().max()), 1e-12)
        assert np.abs(_sample(g) - GOLD[f"gsample/{k}"]).max() <= 2e-5 * scale + 1e-9, k
        s = GOLD[f"gsum/{k}"]
        assert abs(float(g.double().abs().sum()) - s[1]) <= 1e-4 * s[1] + 1e-9, k
        if f"gfull/{k}" in GOLD.files:
            assert np.abs(g.numpy() - GOLD[f"gfull/{k}"]).max() <= 2e-5 * scale + 1e-9, k
        # one AdamW(lr=2e-4) step from zero moments
        p1, _, _ = ref_train.adamw_update(sd[k], g, torch.zeros_like(g), torch.zeros_like(g), 1)
        assert np.abs(_sample(p1) - GOLD[f"psample/{k}"]).max() <= 2e-6, k
