"""bench.py's plain run: the contract fields of its line, none of the `--full` measurements, and `--dump-outputs` writing what the
timed path computed in its last step -- equal bit for bit to the same sample run in this process (the kernels are run-to-run
deterministic)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
PKG = REPO / "clip-neural-image-conpression_amd"


def test_bench_plain_run_and_dump_outputs(tmp_path, synth):
    from clip_feature_codec import _native
    from clip_feature_codec.models.unet import CLIPCondUNet
    from clip_feature_codec.diffusion.scheduler import NoiseScheduler
    from clip_feature_codec.diffusion.ddim import DDIMSampler

    B, S, T, steps = 8, 64, 4, 3
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "CCN_LAUNCH_DEPTH")}
    env["PYTHONPATH"] = os.pathsep.join([str(PKG), str(REPO)] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    r = subprocess.run([sys.executable, str(REPO / "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--size", str(S),
                        "--ddim-steps", str(T), "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["unit"] == "images/sec" and line["higher_is_better"] is True and line["dtype"] == "bf16" and line["metric"].startswith("images/sec")
    assert line["steps"] == steps and line["warmup"] == 1
    assert line["value"] > 0 and abs(line["value"] * line["ms_per_step"] / 1e3 - B) < 0.01     # one timed step = one batch of B images
    assert line["roofline"] is None and line["parity"] is None and line["parity_mode"] is None and line["cpu_baseline"] is None
    assert line["config"]["value_with_two_steps_in_flight"] is None

    got = np.load(tmp_path / "out" / "x_final.npy", allow_pickle=False)
    assert got.dtype == np.float32 and got.shape == (B, 3, S, S)

    _native.load_library()
    dev = "cuda:0"
    sd = synth.synth_state_dict(synth.unet_param_spec(512, 128, (1, 2, 2)))
    net = CLIPCondUNet(512, 128, (1, 2, 2), dtype="bf16").to(dev).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    z = torch.from_numpy(synth.synth_z(B)).to(dev)
    x_T = torch.from_numpy(synth.start_noise(list(range(B)), S, seed_base=100)).to(dev)
    want = DDIMSampler(NoiseScheduler(1000, "cosine", dev), eta=0.0).sample(net, z, (B, 3, S, S), steps=T, x_T=x_T).cpu().numpy()
    assert np.array_equal(got, want), float(np.abs(got - want).max())
