"""``--device_noise`` of the two hot-path CLIs on the GPU: a record's reconstruction does not depend on the batch it sat in, also
with ``--eta > 0``; the flag needs ``--seed``.  Synthetic store of 5 records at 16 px, the C1-sized checkpoint.

The reconstructions are taken where the CLI gets them, at ``sampler.sample``'s return (cli.eval itself only writes metrics), keyed
by the record seed the CLI passed.  They are compared within 1e-5 max-abs, the suite's tolerance for one fp32 reconstruction
computed through launch forms that differ (TOL_COND_PATHS of test_gpu_guidance.py / test_gpu_parity.py): the UNet's kernels may
depend on B; the draws themselves are pinned bit for bit in test_gpu_rng.py."""
import json

import numpy as np
import pytest
import torch

from clip_feature_codec.cli import eval as cli_eval, reconstruct_diffusion as cli_recon, _common
from clip_feature_codec.io import bitstream
from clip_feature_codec.utils import synth

pytestmark = pytest.mark.gpu
SIZE, N, STEPS, SEED = 16, 5, 6, 7
TOL_CROSS_BATCH_FP32 = 1e-5
# Under the CLI's cosine table the reference's direction coefficient sqrt(ab_s - sigma^2) is real at t = 999 only for
# eta <= 1.5e-3 (sigma_0 = 0.99995 eta against sqrt(ab_s) = 1.558e-3): at ETA = 0.03 the unseeded sampler reproduces the reference's
# NaN, the seeded one caps sigma on that step (ddim_coefficients(cap_sigma=True)).  ETA_REAL: every row is the reference's own.
ETA, ETA_REAL = 0.03, 0.001
BUILD_SAMPLER = _common.build_sampler


@pytest.fixture(scope="module")
def store(tmp_path_factory):
    d = tmp_path_factory.mktemp("store_dn")
    synth.write_synth_store(d, N, SIZE, write_clp=bitstream.write_bitstream)
    sd = synth.synth_state_dict(synth.unet_param_spec(512, 32, (1, 2)))
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, d / "ckpt.pt")
    return d


def run_eval(store, monkeypatch, batch, eta, tag):
    """cli.eval in this process; returns ({record seed: reconstruction}, the JSON rows, the x_T arguments seen)."""
    recons, x_ts = {}, []
    build = BUILD_SAMPLER

    def build_and_tap(*a, **kw):
        sampler = build(*a, **kw)
        sample = sampler.sample

        def tapped(*sa, **skw):
            x = sample(*sa, **skw)
            x_ts.append(skw.get("x_T"))
            for k, s in enumerate(skw["seeds"]):
                recons[int(s)] = x[k].detach().cpu().numpy().copy()
            return x
        sampler.sample = tapped
        return sampler
    monkeypatch.setattr(_common, "build_sampler", build_and_tap)
    out_json = store / f"metrics_{tag}.json"
    cli_eval.main(["--store_dir", str(store), "--weights", str(store / "ckpt.pt"), "--size", str(SIZE), "--steps", str(STEPS), "--batch", str(batch),
                   "--seed", str(SEED), "--device_noise", "--eta", str(eta), "--device", "cuda", "--out_json", str(out_json)])
    return recons, json.loads(out_json.read_text()), x_ts


def compare(store, monkeypatch, eta):
    two, rows2, x_ts = run_eval(store, monkeypatch, 2, eta, f"b2_{eta}")
    three, rows3, _ = run_eval(store, monkeypatch, 3, eta, f"b3_{eta}")
    assert sorted(two) == sorted(three) == [SEED + i for i in range(N)]        # record i draws from seed + i
    assert all(x is None for x in x_ts)                                        # no start noise was made on the host or uploaded
    diff = max(float(np.abs(two[s].astype(np.float64) - three[s]).max()) for s in two)
    finite = all(np.isfinite(two[s]).all() and np.isfinite(three[s]).all() for s in two)
    print(f"eta {eta}: batch 2 vs batch 3, max-abs difference of the {N} reconstructions {diff:.3e} (all finite: {finite})")
    return diff, finite, rows2, rows3


def test_eval_device_noise_record_is_independent_of_the_batch(store, monkeypatch, capsys):
    """``cli.eval --seed 7 --device_noise --eta 0.03`` with ``--batch 2`` against ``--batch 3``: numbers, and the same ones."""
    diff, finite, rows2, rows3 = compare(store, monkeypatch, ETA)
    out = capsys.readouterr().out
    print(out)                                                                 # (the figure above stays in the test's output)
    assert "Average PSNR:" in out
    assert finite and diff <= TOL_CROSS_BATCH_FP32, diff
    assert all(np.isfinite(r["psnr"]) and np.isfinite(r["ssim"]) for r in rows2 + rows3)


def test_eval_device_noise_record_is_independent_of_the_batch_real_table(store, monkeypatch):
    """The same comparison at an eta whose cosine table is real on every step: no row of the table is capped."""
    diff, finite, rows2, rows3 = compare(store, monkeypatch, ETA_REAL)
    assert finite and diff <= TOL_CROSS_BATCH_FP32, diff
    assert all(np.isfinite(r["psnr"]) and np.isfinite(r["ssim"]) for r in rows2 + rows3)


def test_device_noise_needs_a_seed(store):
    base = ["--store_dir", str(store), "--weights", str(store / "ckpt.pt"), "--size", str(SIZE), "--steps", str(STEPS), "--device", "cuda"]
    with pytest.raises(SystemExit) as e:
        cli_eval.main(base + ["--device_noise"])
    assert e.value.code not in (0, None) and "--seed" in str(e.value.code)
    manifest = json.loads((store / "manifest.json").read_text())
    with pytest.raises(SystemExit) as e:
        cli_recon.main(base + ["--bitstream", manifest[0]["bitstream"], "--out", str(store / "x.png"), "--device_noise"])
    assert e.value.code not in (0, None)


def test_reconstruct_cli_device_noise_is_reproducible(store, capsys):
    from PIL import Image
    manifest = json.loads((store / "manifest.json").read_text())
    imgs = []
    for tag in ("a", "b"):
        out = store / f"recon_{tag}.png"
        cli_recon.main(["--store_dir", str(store), "--bitstream", manifest[2]["bitstream"], "--weights", str(store / "ckpt.pt"), "--out", str(out),
                        "--steps", str(STEPS), "--size", str(SIZE), "--seed", str(SEED), "--device_noise", "--eta", str(ETA_REAL), "--device", "cuda"])
        imgs.append(np.array(Image.open(out)))
    assert f"Saved to {store / 'recon_b.png'}" in capsys.readouterr().out
    assert imgs[0].shape == (SIZE, SIZE, 3) and np.array_equal(imgs[0], imgs[1])
