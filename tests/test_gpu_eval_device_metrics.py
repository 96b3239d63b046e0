"""``cli.eval --device_metrics`` against the same command without the flag, on the synthetic store of tests/test_gpu_cli.py.

Repeated fused samples are bit-equal in this build (tests/test_gpu_plan_cache.py), so both runs score the same bytes: per record PSNR
may differ by the host's float32 mean (about 1e-6 relative, 5e-6 dB; bound 1e-4 dB) and SSIM by fp64 rounding (bound 1e-10)."""
import json
import math

import pytest
import torch

from clip_feature_codec.cli import eval as cli_eval
from clip_feature_codec.io import bitstream
from clip_feature_codec.utils import synth

pytestmark = pytest.mark.gpu
SIZE, N, STEPS, SEED = 32, 5, 6, 11                                # batch 2: the last batch is ragged
AVERAGES = ("Average PSNR:", "Average SSIM:", "Average LPIPS:", "Average CLIP similarity:")


@pytest.fixture(scope="module")
def store(tmp_path_factory):
    d = tmp_path_factory.mktemp("store")
    synth.write_synth_store(d, N, SIZE, write_clp=bitstream.write_bitstream)
    sd = synth.synth_state_dict(synth.unet_param_spec(512, 32, (1, 2)))
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, d / "ckpt.pt")
    return d


def run(d, capsys, name, *extra):
    out_json = d / name
    cli_eval.main(["--store_dir", str(d), "--weights", str(d / "ckpt.pt"), "--size", str(SIZE), "--steps", str(STEPS),
                   "--batch", "2", "--seed", str(SEED), "--device", "cuda", "--out_json", str(out_json), *extra])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Average")]
    return lines, json.loads(out_json.read_text())


def compare(host, device):
    (h_lines, h_recs), (d_lines, d_recs) = host, device
    assert len(h_lines) == len(d_lines) == 4
    assert all(h.startswith(k) and g.startswith(k) for h, g, k in zip(h_lines, d_lines, AVERAGES))
    assert [list(r) for r in d_recs] == [list(r) for r in h_recs] and len(d_recs) == N
    assert [set(r) for r in d_recs] == [{"image", "psnr", "ssim", "lpips", "clip_sim"}] * N
    for h, g in zip(h_recs, d_recs):
        print(f"{g['image']}: psnr {g['psnr']!r} (host {h['psnr']!r}), ssim {g['ssim']!r} (host {h['ssim']!r})")
        assert g["image"] == h["image"]
        assert math.isfinite(h["psnr"]) and math.isfinite(h["ssim"])
        assert abs(g["psnr"] - h["psnr"]) <= 1e-4
        assert abs(g["ssim"] - h["ssim"]) <= 1e-10
        for k in ("lpips", "clip_sim"):
            assert (math.isnan(g[k]) and math.isnan(h[k])) or g[k] == h[k]


def test_device_metrics_match_host_metrics(store, capsys):
    compare(run(store, capsys, "host.json"), run(store, capsys, "device.json", "--device_metrics"))


def test_device_metrics_on_the_multistep_route(store, capsys):
    compare(run(store, capsys, "host_ms.json", "--sampler", "dpmpp2m"),
            run(store, capsys, "device_ms.json", "--sampler", "dpmpp2m", "--device_metrics"))


def test_device_metrics_on_the_sequential_route(store, capsys):
    """eta > 0 draws noise step by step from the seeded device generator state; the flag must run there too (same helper)."""
    lines, recs = run(store, capsys, "device_eta.json", "--eta", "0.5", "--device_metrics")
    assert len(lines) == 4 and len(recs) == N
    assert all(math.isfinite(r["psnr"]) and -1.0 <= r["ssim"] <= 1.0 and math.isnan(r["lpips"]) for r in recs)
