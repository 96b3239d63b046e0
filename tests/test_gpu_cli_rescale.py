"""``--guidance_rescale`` and ``--zero_snr`` of the two hot-path CLIs on the GPU: with ``--cfg_scale 3`` the rescaled reconstruction is
finite and another one than without the flag; ``--zero_snr --prediction v`` runs; each flag without its prerequisite exits with the
flag error.  Synthetic store at 16 px, the C1-sized checkpoint, 6 steps.

The reconstructions are taken where the CLIs get them, at ``sampler.sample``'s return."""
import json

import numpy as np
import pytest
import torch

from clip_feature_codec.cli import eval as cli_eval, reconstruct_diffusion as cli_recon, _common
from clip_feature_codec.io import bitstream
from clip_feature_codec.utils import synth

pytestmark = pytest.mark.gpu
SIZE, N, STEPS, SEED = 16, 3, 6, 7
BUILD_SAMPLER = _common.build_sampler


@pytest.fixture(scope="module")
def store(tmp_path_factory):
    d = tmp_path_factory.mktemp("store_rs")
    synth.write_synth_store(d, N, SIZE, write_clp=bitstream.write_bitstream)
    sd = synth.synth_state_dict(synth.unet_param_spec(512, 32, (1, 2)))
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, d / "ckpt.pt")
    return d


def tap(monkeypatch, module, seen):
    def build_and_tap(*a, **kw):
        sampler = BUILD_SAMPLER(*a, **kw)
        sample = sampler.sample

        def tapped(*sa, **skw):
            x = sample(*sa, **skw)
            seen.setdefault("x", []).append(x.detach().cpu().numpy().copy())
            return x
        sampler.sample = tapped
        seen["sampler"] = sampler
        return sampler
    monkeypatch.setattr(module, "build_sampler", build_and_tap)


def reconstruct(store, monkeypatch, tag, extra):
    seen = {}
    tap(monkeypatch, cli_recon, seen)
    manifest = json.loads((store / "manifest.json").read_text())
    cli_recon.main(["--store_dir", str(store), "--bitstream", manifest[1]["bitstream"], "--weights", str(store / "ckpt.pt"), "--out",
                    str(store / f"recon_{tag}.png"), "--steps", str(STEPS), "--size", str(SIZE), "--seed", str(SEED), "--device", "cuda"] + extra)
    return seen["sampler"], np.concatenate(seen["x"])


def evaluate(store, monkeypatch, tag, extra):
    seen = {}
    tap(monkeypatch, _common, seen)
    out_json = store / f"metrics_{tag}.json"
    cli_eval.main(["--store_dir", str(store), "--weights", str(store / "ckpt.pt"), "--size", str(SIZE), "--steps", str(STEPS), "--batch", "2",
                   "--seed", str(SEED), "--device", "cuda", "--out_json", str(out_json)] + extra)
    assert out_json.exists()
    return seen["sampler"], np.concatenate(seen["x"])


@pytest.mark.parametrize("cli", ["reconstruct", "eval"])
def test_guidance_rescale_flag(store, monkeypatch, cli):
    run = reconstruct if cli == "reconstruct" else evaluate
    s0, plain = run(store, monkeypatch, "plain", ["--cfg_scale", "3"])
    s1, rs = run(store, monkeypatch, "rs", ["--cfg_scale", "3", "--guidance_rescale", "0.7"])
    assert s0.guidance_rescale is None and s1.guidance_rescale == 0.7 and s0.guided and s1.guided
    assert plain.shape == rs.shape == ((1 if cli == "reconstruct" else N), 3, SIZE, SIZE)
    assert np.isfinite(plain).all() and np.isfinite(rs).all()
    diff = float(np.abs(plain - rs).max())
    print(f"{cli}: --guidance_rescale 0.7 against the plain guided run at cfg_scale 3: max-abs difference {diff:.3e}")
    assert diff > 0
    # with the multistep sampler too
    _, ms = run(store, monkeypatch, "ms", ["--cfg_scale", "3", "--sampler", "dpmpp2m"])
    _, ms_rs = run(store, monkeypatch, "ms_rs", ["--cfg_scale", "3", "--sampler", "dpmpp2m", "--guidance_rescale", "0.7"])
    assert np.isfinite(ms_rs).all() and not np.array_equal(ms, ms_rs)


@pytest.mark.parametrize("cli", ["reconstruct", "eval"])
def test_zero_snr_flag(store, monkeypatch, cli):
    run = reconstruct if cli == "reconstruct" else evaluate
    s0, plain = run(store, monkeypatch, "v", ["--prediction", "v"])
    s1, zero = run(store, monkeypatch, "zero", ["--prediction", "v", "--zero_snr"])
    assert not s0.sch.rescale_zero_snr and s1.sch.rescale_zero_snr and float(s1.sch.alphas_cumprod[-1]) == 0.0
    assert np.isfinite(zero).all() and not np.array_equal(plain, zero)
    _, both = run(store, monkeypatch, "both", ["--prediction", "v", "--zero_snr", "--sampler", "dpmpp2m", "--cfg_scale", "3", "--guidance_rescale", "0.7"])
    assert np.isfinite(both).all()


def test_flag_errors(store):
    manifest = json.loads((store / "manifest.json").read_text())
    recon = ["--store_dir", str(store), "--bitstream", manifest[0]["bitstream"], "--weights", str(store / "ckpt.pt"), "--out", str(store / "x.png"),
             "--size", str(SIZE), "--steps", str(STEPS), "--device", "cuda"]
    ev = ["--store_dir", str(store), "--weights", str(store / "ckpt.pt"), "--size", str(SIZE), "--steps", str(STEPS), "--device", "cuda"]
    for main, base in ((cli_recon.main, recon), (cli_eval.main, ev)):
        for extra in (["--guidance_rescale", "0.7"], ["--guidance_rescale", "0.7", "--cfg_scale", "1"], ["--guidance_rescale", "0", "--cfg_scale", "3"],
                      ["--guidance_rescale", "1.5", "--cfg_scale", "3"], ["--zero_snr"], ["--zero_snr", "--prediction", "eps"]):
            with pytest.raises(SystemExit) as e:
                main(base + extra)
            assert e.value.code not in (0, None), extra
            assert "--guidance_rescale" in str(e.value.code) or "--zero_snr" in str(e.value.code)
