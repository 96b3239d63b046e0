"""``--dynamic_threshold`` of ``cli.reconstruct_diffusion`` on the GPU, together with ``--cfg_scale 3``: the reconstruction is finite
and is another one than without the flag.  Synthetic store at 64 px, the C1-sized checkpoint, 6 steps.

The reconstruction is taken where the CLI gets it, at ``sampler.sample``'s return: the PNG is ``clamp(x, -1, 1)`` in eight bits, which
would hide a non-finite value."""
import json

import numpy as np
import pytest
import torch

from clip_feature_codec.cli import reconstruct_diffusion as cli_recon
from clip_feature_codec.io import bitstream
from clip_feature_codec.utils import synth

pytestmark = pytest.mark.gpu
SIZE, STEPS, SEED = 64, 6, 7
BUILD_SAMPLER = cli_recon.build_sampler


@pytest.fixture(scope="module")
def store(tmp_path_factory):
    d = tmp_path_factory.mktemp("store_thr")
    synth.write_synth_store(d, 2, SIZE, write_clp=bitstream.write_bitstream)
    sd = synth.synth_state_dict(synth.unet_param_spec(512, 32, (1, 2)))
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, d / "ckpt.pt")
    return d


def reconstruct(store, monkeypatch, tag, extra):
    """The CLI in this process; returns (the sampler it built, the float reconstruction, the PNG)."""
    from PIL import Image
    seen = {}

    def build_and_tap(*a, **kw):
        sampler = BUILD_SAMPLER(*a, **kw)
        sample = sampler.sample

        def tapped(*sa, **skw):
            x = sample(*sa, **skw)
            seen["x"] = x.detach().cpu().numpy().copy()
            return x
        sampler.sample = tapped
        seen["sampler"] = sampler
        return sampler
    monkeypatch.setattr(cli_recon, "build_sampler", build_and_tap)
    manifest = json.loads((store / "manifest.json").read_text())
    out = store / f"recon_{tag}.png"
    cli_recon.main(["--store_dir", str(store), "--bitstream", manifest[1]["bitstream"], "--weights", str(store / "ckpt.pt"), "--out", str(out),
                    "--steps", str(STEPS), "--size", str(SIZE), "--seed", str(SEED), "--cfg_scale", "3", "--device", "cuda"] + extra)
    return seen["sampler"], seen["x"], np.array(Image.open(out))


def test_reconstruct_cli_dynamic_threshold(store, monkeypatch, capsys):
    s0, plain, png0 = reconstruct(store, monkeypatch, "plain", [])
    s1, thr, png1 = reconstruct(store, monkeypatch, "thr", ["--dynamic_threshold", "0.995"])
    s2, capped, _ = reconstruct(store, monkeypatch, "cap", ["--dynamic_threshold", "0.995", "--threshold_max", "1"])
    assert "Saved to" in capsys.readouterr().out
    assert s0.dynamic_threshold is None and (s1.dynamic_threshold, s1.threshold_max) == (0.995, None) and s2.threshold_max == 1.0
    assert s0.guided and s1.guided
    assert plain.shape == thr.shape == (1, 3, SIZE, SIZE) and png1.shape == (SIZE, SIZE, 3)
    assert np.isfinite(plain).all() and np.isfinite(thr).all()
    diff = float(np.abs(plain - thr).max())
    print(f"--dynamic_threshold 0.995 against the static clamp at cfg_scale 3: max-abs difference {diff:.3e}")
    assert diff > 0 and not np.array_equal(png0, png1)
    assert np.array_equal(capped, plain)                            # a maximum of 1 is the static clamp, bit for bit


def test_threshold_flag_errors(store):
    manifest = json.loads((store / "manifest.json").read_text())
    base = ["--store_dir", str(store), "--bitstream", manifest[0]["bitstream"], "--weights", str(store / "ckpt.pt"), "--out", str(store / "x.png"),
            "--size", str(SIZE), "--steps", str(STEPS), "--device", "cuda"]
    for extra in (["--dynamic_threshold", "0"], ["--dynamic_threshold", "1.5"], ["--threshold_max", "2"],
                  ["--dynamic_threshold", "0.9", "--threshold_max", "0.5"]):
        with pytest.raises(SystemExit) as e:
            cli_recon.main(base + extra)
        assert e.value.code not in (0, None)
