"""``--lowres_guide`` of the two hot-path CLIs on the GPU, on a 4-record synthetic store at 32 px with the C1-sized checkpoint and
6 steps: the guided reconstruction is finite, another one than without the flag and -- with ``--sampler dpmpp2m``, whose last step
returns its x0 (the DDIM table keeps the reference's last row, which adds ``e``) -- carries the thumbnail it was given; ``eval``
writes ``side_bytes_per_record``; without the flags each CLI writes, byte for byte, what the same sampler call without any guide
argument gives -- the call both CLIs made before they knew the flag.

The reconstructions are taken where the CLIs get them, at ``sampler.sample``'s return."""
import json

import numpy as np
import pytest
import torch
from PIL import Image

import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
import guide_ref  # noqa: E402

from clip_feature_codec import _native  # noqa: E402
from clip_feature_codec.cli import eval as cli_eval, reconstruct_diffusion as cli_recon, _common
from clip_feature_codec.io import bitstream
from clip_feature_codec.utils import synth

pytestmark = pytest.mark.gpu
SIZE, RECORDS, STEPS, SEED, N = 32, 4, 6, 7, 8
BUILD_SAMPLER = _common.build_sampler


@pytest.fixture(scope="module")
def store(tmp_path_factory):
    d = tmp_path_factory.mktemp("store_guide")
    synth.write_synth_store(d, RECORDS, SIZE, write_clp=bitstream.write_bitstream)
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
            seen.setdefault("kw", []).append({k: v for k, v in skw.items() if k.startswith("guide")})
            return x
        sampler.sample = tapped
        return sampler
    monkeypatch.setattr(module, "build_sampler", build_and_tap)


def reconstruct(store, monkeypatch, tag, extra, record=1):
    seen = {}
    tap(monkeypatch, cli_recon, seen)
    manifest = json.loads((store / "manifest.json").read_text())
    out = store / f"recon_{tag}.png"
    cli_recon.main(["--store_dir", str(store), "--bitstream", manifest[record]["bitstream"], "--weights", str(store / "ckpt.pt"), "--out", str(out),
                    "--steps", str(STEPS), "--size", str(SIZE), "--seed", str(SEED), "--device", "cuda"] + extra)
    return seen, out


def evaluate(store, monkeypatch, tag, extra):
    seen = {}
    tap(monkeypatch, _common, seen)
    out_json = store / f"metrics_{tag}.json"
    cli_eval.main(["--store_dir", str(store), "--weights", str(store / "ckpt.pt"), "--size", str(SIZE), "--steps", str(STEPS), "--batch", "2",
                   "--seed", str(SEED), "--device", "cuda", "--out_json", str(out_json)] + extra)
    return seen, out_json


def test_eval_with_the_guide(store, monkeypatch):
    _, ddim_json = evaluate(store, monkeypatch, "ddim", ["--lowres_guide", str(N)])
    assert all(r["side_bytes_per_record"] == 3 * (SIZE // N) ** 2 and np.isfinite(r["psnr"]) for r in json.loads(ddim_json.read_text()))
    _, plain_json = evaluate(store, monkeypatch, "plain", ["--sampler", "dpmpp2m"])
    seen, guided_json = evaluate(store, monkeypatch, "guided", ["--sampler", "dpmpp2m", "--lowres_guide", str(N)])
    plain, guided = json.loads(plain_json.read_text()), json.loads(guided_json.read_text())
    assert len(plain) == len(guided) == RECORDS
    assert all("side_bytes_per_record" not in r for r in plain)
    assert all(r["side_bytes_per_record"] == 3 * (SIZE // N) ** 2 for r in guided)
    x = np.concatenate(seen["x"])
    assert x.shape == (RECORDS, 3, SIZE, SIZE) and np.isfinite(x).all()
    assert all(set(kw) == {"guide", "guide_strength", "guide_t_min"} and kw["guide_strength"] == 1.0 and kw["guide_t_min"] == 0 for kw in seen["kw"])
    # each batch got the thumbnails of its own originals, and (lambda = 1, every step) the result carries them
    manifest = json.loads((store / "manifest.json").read_text())
    want = np.stack([_common.derive_guide(cli_eval.original_u8(r["image"], SIZE), N) for r in manifest])
    got = np.concatenate([kw["guide"].cpu().numpy() for kw in seen["kw"]])
    assert got.shape == (RECORDS, 3, SIZE // N, SIZE // N)
    alt = np.stack([_common.derive_guide(cli_eval.load_original(r["image"], SIZE), N) for r in manifest])
    assert np.array_equal(got, want) or np.array_equal(got, alt)     # (from the uint8 or the float original, whichever this run scores on)
    thumb = _native.block_mean(torch.from_numpy(x).cuda(), N).cpu().numpy()
    # (ccn_block_mean clamps and x0' is not clamped again: its bound holds on the blocks inside [-1, 1], tests/test_gpu_guide.py)
    err_all, err_in, inside = guide_ref.thumbnail_errors(x, thumb, got, N)
    print(f"eval --lowres_guide {N}: max |float64 block mean of the result - thumbnail| = {err_all:.3e}, ccn_block_mean on the {inside:.0%} of "
          f"blocks inside [-1, 1] {err_in:.3e}, on all blocks {np.abs(thumb - got).max():.3e}")
    assert err_all <= 3 * 2.0 ** -23 and err_in <= 3 * 2.0 ** -23
    assert any(a["psnr"] != b["psnr"] for a, b in zip(plain, guided))
    # fewer bits and a partial guide run too, and say so
    _, j = evaluate(store, monkeypatch, "bits", ["--lowres_guide", "4", "--guide_bits", "4", "--guide_strength", "0.5", "--guide_t_min", "300",
                                                 "--cfg_scale", "3", "--sampler", "dpmpp2m"])
    assert all(r["side_bytes_per_record"] == 3 * 64 // 2 and np.isfinite(r["psnr"]) for r in json.loads(j.read_text()))


def test_reconstruct_with_the_guide(store, monkeypatch):
    rng = np.random.default_rng(3)
    thumb = rng.integers(64, 192, (SIZE // N, SIZE // N, 3), dtype=np.uint8)
    np.save(store / "thumb.npy", thumb)
    Image.fromarray(thumb).save(store / "thumb.png")
    _, ddim_plain = reconstruct(store, monkeypatch, "ddim_plain", [])
    _, ddim_png = reconstruct(store, monkeypatch, "ddim", ["--lowres_guide", str(store / "thumb.npy")])
    assert ddim_plain.read_bytes() != ddim_png.read_bytes()
    ms = ["--sampler", "dpmpp2m"]
    _, plain_png = reconstruct(store, monkeypatch, "plain", ms)
    seen, npy_png = reconstruct(store, monkeypatch, "npy", ms + ["--lowres_guide", str(store / "thumb.npy")])
    _, img_png = reconstruct(store, monkeypatch, "img", ms + ["--lowres_guide", str(store / "thumb.png")])
    assert npy_png.read_bytes() == img_png.read_bytes() != plain_png.read_bytes()
    x = seen["x"][0]
    g = (thumb.astype(np.float32) / np.float32(127.5) - np.float32(1.0)).transpose(2, 0, 1)[None]
    assert np.isfinite(x).all() and np.array_equal(seen["kw"][0]["guide"].cpu().numpy(), g)
    got = _native.block_mean(torch.from_numpy(x).cuda(), N).cpu().numpy()
    err_all, err_in, inside = guide_ref.thumbnail_errors(x, got, g, N)
    print(f"reconstruct --lowres_guide: max |float64 block mean of the result - thumbnail| = {err_all:.3e}, ccn_block_mean on the {inside:.0%} "
          f"of blocks inside [-1, 1] {err_in:.3e}, on all blocks {np.abs(got - g).max():.3e}")
    assert err_all <= 3 * 2.0 ** -23 and err_in <= 3 * 2.0 ** -23
    seen, _ = reconstruct(store, monkeypatch, "half", ["--lowres_guide", str(store / "thumb.npy"), "--guide_strength", "0.5", "--guide_t_min", "400"])
    assert seen["kw"][0]["guide_strength"] == 0.5 and seen["kw"][0]["guide_t_min"] == 400 and np.isfinite(seen["x"][0]).all()


def test_without_the_flags_nothing_changes(store, monkeypatch):
    """Each CLI without the flags against the sampler call it made before it knew them -- ``sample`` with no guide argument at all,
    on the inputs the CLI builds: the same PNG bytes, the same metrics, no new key."""
    seen, png = reconstruct(store, monkeypatch, "noflag", [])
    assert seen["kw"] == [{}]                                       # no guide argument reaches the sampler
    manifest = json.loads((store / "manifest.json").read_text())
    scale, zero = _common.load_codec_meta(store)
    z = torch.from_numpy(_common.load_embedding(manifest[1]["bitstream"], scale, zero)).to("cuda:0")
    net = _common.build_model(str(store / "ckpt.pt"), "cuda:0", z.shape[1], "fp32")
    sampler = BUILD_SAMPLER(0.0, "cuda:0")
    with torch.no_grad():
        x = sampler.sample(net, z, shape=(1, 3, SIZE, SIZE), steps=STEPS, cfg_scale=1.0, x_T=_common.start_noise([0], SIZE, SEED).to("cuda:0"))
    assert np.array_equal(seen["x"][0], x.cpu().numpy())
    img = x[0].clamp(-1, 1).cpu().numpy().transpose(1, 2, 0)
    Image.fromarray(((img + 1.0) * 127.5).astype(np.uint8)).save(store / "direct.png")
    assert png.read_bytes() == (store / "direct.png").read_bytes()

    seen, out_json = evaluate(store, monkeypatch, "noflag", [])
    assert all(kw == {} for kw in seen["kw"])
    recs = json.loads(out_json.read_text())
    assert all(set(r) == {"image", "psnr", "ssim", "lpips", "clip_sim"} for r in recs)
    zs = np.concatenate([_common.load_embedding(r["bitstream"], scale, zero) for r in manifest])
    for lo in range(0, RECORDS, 2):                                 # --batch 2: records lo, lo + 1 with the start noise of their indices
        with torch.no_grad():
            x = sampler.sample(net, torch.from_numpy(zs[lo:lo + 2]).to("cuda:0"), shape=(2, 3, SIZE, SIZE), steps=STEPS, cfg_scale=1.0,
                               x_T=torch.cat([_common.start_noise([i], SIZE, SEED) for i in (lo, lo + 1)]).to("cuda:0"), slot=(lo // 2) & 1)
        assert np.array_equal(seen["x"][lo // 2], x.cpu().numpy()), lo


def test_flag_errors(store):
    manifest = json.loads((store / "manifest.json").read_text())
    recon = ["--store_dir", str(store), "--bitstream", manifest[0]["bitstream"], "--weights", str(store / "ckpt.pt"), "--out", str(store / "x.png"),
             "--size", str(SIZE), "--steps", str(STEPS), "--device", "cuda"]
    ev = ["--store_dir", str(store), "--weights", str(store / "ckpt.pt"), "--size", str(SIZE), "--steps", str(STEPS), "--device", "cuda"]
    np.save(store / "bad.npy", np.zeros((5, 5, 3), np.uint8))
    cases = [(cli_eval.main, ev, e) for e in (["--lowres_guide", "3"], ["--lowres_guide", "64"], ["--lowres_guide", "8", "--guide_strength", "0"],
                                               ["--lowres_guide", "8", "--guide_bits", "9"], ["--guide_strength", "0.5"], ["--guide_bits", "4"])]
    cases += [(cli_recon.main, recon, e) for e in (["--lowres_guide", str(store / "bad.npy")], ["--guide_t_min", "3"],
                                                    ["--lowres_guide", str(store / "bad.npy"), "--guide_t_min", "-1"])]
    for main, base, extra in cases:
        with pytest.raises(SystemExit) as e:
            main(base + extra)
        assert e.value.code not in (0, None) and ("--lowres_guide" in str(e.value.code) or "--guide" in str(e.value.code)), extra
