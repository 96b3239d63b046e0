"""The exact-integer restatement of the score kernel (tests/score_ref.py) against the host metrics it stands for (no GPU needed)."""
import warnings

import numpy as np
import pytest

import score_ref
from clip_feature_codec.eval import metrics


@pytest.mark.parametrize("shape", score_ref.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restatement_matches_host_metrics(shape):
    B, C, H, W = shape
    for content in score_ref.CONTENTS:
        a, b = score_ref.images(shape, content)
        sse, ssim = score_ref.score(a, b)
        want = score_ref.plane_mean_ssim(a, b)
        for i in range(B):
            assert sse[i] == int(((a[i].astype(np.int64) - b[i].astype(np.int64)) ** 2).sum())
            # psnr_u8 takes its mean in float32 (good to about 1e-6 relative, 5e-6 dB); the SSE itself is exact
            p_host, p_ref = metrics.psnr_u8(a[i], b[i]), metrics.psnr_from_sse(sse[i], a[i].size)
            assert (np.isinf(p_host) and np.isinf(p_ref)) if sse[i] == 0 else abs(p_host - p_ref) <= 1e-4, (content, p_host, p_ref)
            if H < score_ref.WIN or W < score_ref.WIN:
                assert np.isnan(ssim[i])
            else:
                # measured: 2.8e-15 at worst over these cases (a handful of fp64 roundings per position, a mean over positions)
                assert abs(ssim[i] - want[i]) <= 1e-12, (content, ssim[i], want[i])
        if content == "identical":
            assert (sse == 0).all() and (np.isnan(ssim).all() or (ssim == 1.0).all())
        if content == "checker" and H >= score_ref.WIN and W >= score_ref.WIN:
            assert (ssim < 0).all()


def test_host_crop_is_empty_without_a_window():
    a, b = score_ref.images((1, 1, 6, 20), "random")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert np.isnan(metrics._ssim_plane(a[0, 0], b[0, 0]))


def test_to_uint8_restatement_is_the_host_conversion():
    x = np.random.default_rng(3).uniform(-1.5, 1.5, 4096).astype(np.float32)
    x[:4] = (-1.0, 1.0, 0.0, -0.0)
    assert np.array_equal(score_ref.to_uint8(x), metrics._to_uint8(x))
