"""Classifier-free guidance, the parts that need no GPU: the exported symbols, the embedding dropout of the training step, the
``--cfg_scale`` flag of both CLIs, and the guided sampler's refusal of host tensors."""
import ctypes
import math

import pytest
import torch

from clip_feature_codec import _native
from clip_feature_codec.diffusion.ddim import DDIMSampler
from clip_feature_codec.diffusion.scheduler import NoiseScheduler


def test_library_exports_the_guidance_entry_points():
    if not _native.LIB_PATH.exists():
        pytest.fail(f"{_native.LIB_PATH} is not built: run `python __graft_entry__.py`")
    lib = ctypes.CDLL(str(_native.LIB_PATH))
    for name in ("ccn_sample_guided", "ccn_cfg_ddim_step"):
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _native.SIGNATURES, f"{name} has no ctypes prototype"
    assert len(_native.SIGNATURES["ccn_sample_guided"][1]) == 19
    assert len(_native.SIGNATURES["ccn_cfg_ddim_step"][1]) == 13


def rows_kept_or_zero(z, zd, keep):
    assert zd.shape == z.shape and zd.dtype == z.dtype and keep.shape == (z.shape[0],) and keep.dtype == torch.bool
    for b in range(z.shape[0]):
        if bool(keep[b]):
            assert torch.equal(zd[b].view(torch.int32), z[b].view(torch.int32)), f"row {b} was kept but is not bit-identical"
        else:
            assert torch.equal(zd[b].view(torch.int32), torch.zeros_like(z[b]).view(torch.int32)), f"row {b} was dropped but is not all +0"


def test_z_dropout_rows_are_unchanged_or_zero():
    from clip_feature_codec.train.diffusion_train import z_dropout
    g = torch.Generator().manual_seed(5)
    z = torch.randn((64, 512), generator=g)
    z[3, 7] = -0.0
    zd, keep = z_dropout(z, 0.5, generator=g)
    rows_kept_or_zero(z, zd, keep)
    assert 0 < int(keep.sum()) < 64                    # (2^-63 that a fair coin gives neither)


def test_z_dropout_p0_keeps_all_and_draws_nothing():
    from clip_feature_codec.train.diffusion_train import z_dropout
    z = torch.randn((8, 512), generator=torch.Generator().manual_seed(1))
    g = torch.Generator().manual_seed(9)
    before, before_default = g.get_state().clone(), torch.get_rng_state().clone()
    zd, keep = z_dropout(z, 0.0, generator=g)
    assert bool(keep.all()) and torch.equal(zd, z)
    assert torch.equal(g.get_state(), before)
    zd, keep = z_dropout(z, 0.0)
    assert bool(keep.all()) and torch.equal(zd, z)
    assert torch.equal(torch.get_rng_state(), before_default)


def test_z_dropout_p1_zeroes_all_and_draws_once():
    from clip_feature_codec.train.diffusion_train import z_dropout
    z = torch.randn((8, 512), generator=torch.Generator().manual_seed(1))
    g, g2 = torch.Generator().manual_seed(9), torch.Generator().manual_seed(9)
    zd, keep = z_dropout(z, 1.0, generator=g)
    assert not bool(keep.any()) and not bool(zd.any())
    rows_kept_or_zero(z, zd, keep)
    torch.rand(8, generator=g2)                        # one torch.rand(B) draw, nothing else
    assert torch.equal(g.get_state(), g2.get_state())


def test_z_dropout_default_generator_and_bad_p():
    from clip_feature_codec.train.diffusion_train import z_dropout
    z = torch.ones((16, 4))
    torch.manual_seed(123)
    _, keep = z_dropout(z, 0.5)
    torch.manual_seed(123)
    assert torch.equal(keep, torch.rand(16) >= 0.5)
    for p in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            z_dropout(z, p)


def test_z_dropout_rate():
    """N = 4096 rows, p = 0.1, seeded: the dropped count is within 5 binomial standard deviations of N p."""
    from clip_feature_codec.train.diffusion_train import z_dropout
    n, p = 4096, 0.1
    z = torch.ones((n, 2))
    zd, keep = z_dropout(z, p, generator=torch.Generator().manual_seed(2024))
    dropped = n - int(keep.sum())
    assert dropped == int((zd[:, 0] == 0).sum())
    assert abs(dropped - n * p) <= 5 * math.sqrt(n * p * (1 - p)), dropped


def test_clis_parse_cfg_scale():
    from clip_feature_codec.cli import eval as cli_eval, reconstruct_diffusion as cli_rec
    a = cli_eval.build_parser().parse_args(["--store_dir", "s", "--weights", "w"])
    assert a.cfg_scale == 1.0
    a = cli_eval.build_parser().parse_args(["--store_dir", "s", "--weights", "w", "--cfg_scale", "3.5"])
    assert a.cfg_scale == 3.5
    a = cli_rec.build_parser().parse_args(["--store_dir", "s", "--bitstream", "b", "--weights", "w"])
    assert a.cfg_scale == 1.0
    a = cli_rec.build_parser().parse_args(["--store_dir", "s", "--bitstream", "b", "--weights", "w", "--cfg_scale", "2"])
    assert a.cfg_scale == 2.0


def test_build_sampler_guided_flag():
    import inspect
    from clip_feature_codec.cli._common import build_sampler
    assert inspect.signature(build_sampler).parameters["guided"].default is False
    s = build_sampler(0.0, "cpu")
    assert s.guided is False and s.null_z is None
    assert build_sampler(0.0, "cpu", guided=True).guided is True


def test_guided_sampler_refuses_cpu_tensors():
    sampler = DDIMSampler(NoiseScheduler(1000, "cosine", "cpu"), guided=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sampler.sample(lambda x, z, t: x, torch.zeros(2, 512), (2, 3, 32, 32), steps=4, cfg_scale=3.0)
