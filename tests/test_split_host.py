"""f16x3 mode (CCN_DTYPE_F16X3), everything that needs no GPU: the public surface accepts the dtype, the commit-time weight split
keeps what the mode's accuracy rests on, and the CPU emulation of the arithmetic (tests/split_emulation.py) meets the C1 gate."""
import ctypes
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from clip_feature_codec import _native
from oracle import ref_unet, ref_diffusion

HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))
import split_emulation  # noqa: E402

REPO = HERE.parent
TOL_E2E_FP32 = 1e-3       # tests/test_gpu_parity.py: north_star's max-abs gate on the reconstructed tensor


def test_dtype_is_part_of_the_public_surface():
    assert _native.dtype_code("f16x3") == 2 and _native.DTYPE_F16X3 == 2
    header = (REPO / "include" / "ccn_hip.h").read_text()
    assert re.search(r"#define\s+CCN_DTYPE_F16X3\s+2\b", header)
    from clip_feature_codec.models.unet import CLIPCondUNet
    from clip_feature_codec.models.blocks import ResBlock
    net = CLIPCondUNet(z_dim=512, base=32, ch_mult=(1, 2), dtype="f16x3")
    assert net.compute_dtype == "f16x3"
    assert net.set_compute_dtype("fp32").set_compute_dtype("f16x3").compute_dtype == "f16x3"
    with pytest.raises(KeyError):
        net.set_compute_dtype("f16x2")
    rb = ResBlock(32, 256)
    rb.compute_dtype = "f16x3"
    assert _native.dtype_code(rb.compute_dtype) == 2


@pytest.mark.parametrize("module", ["eval", "reconstruct_diffusion"])
def test_cli_parsers_accept_the_dtype(module, capsys):
    import importlib
    cli = importlib.import_module(f"clip_feature_codec.cli.{module}")
    ap = cli.build_parser()
    required = []
    for a in ap._actions:
        if a.required:
            required += [a.option_strings[0], "x"]
    assert ap.parse_args(required).dtype == "fp32"                      # the default stays the parity mode
    assert ap.parse_args(required + ["--dtype", "f16x3"]).dtype == "f16x3"
    assert ap.parse_args(required + ["--dtype", "bf16"]).dtype == "bf16"
    with pytest.raises(SystemExit):
        ap.parse_args(required + ["--dtype", "fp16"])
    capsys.readouterr()


def _split(w):
    lib = ctypes.CDLL(str(_native.LIB_PATH))
    fn = lib.ccn_internal_split_weights
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    w = np.ascontiguousarray(w, dtype=np.float32).ravel()
    s = np.zeros(1, np.float32); hi = np.zeros(w.size, np.uint16); lo = np.zeros(w.size, np.uint16)
    assert fn(w.ctypes.data, w.size, s.ctypes.data, hi.ctypes.data, lo.ctypes.data) == 0
    return float(s[0]), hi.view(np.float16), lo.view(np.float16)


def _check_split(w, what):
    w = np.asarray(w, np.float32).ravel()
    s, hi, lo = _split(w)
    mant, _ = np.frexp(np.float64(s))
    assert mant == 0.5 and s > 0, (what, s)                              # a power of two
    ws = w.astype(np.float64) * s
    if np.abs(w).max() == 0:
        assert s == 1.0, (what, s)
    else:
        assert 2.0 ** 13 <= np.abs(ws).max() < 2.0 ** 14, (what, s, np.abs(ws).max())
    assert np.isfinite(hi).all() and np.isfinite(lo).all(), what
    err = np.abs(hi.astype(np.float64) + lo.astype(np.float64) - ws)
    bound = 2.0 ** -22 * np.abs(ws) + 2.0 ** -25
    assert (err <= bound).all(), (what, float((err / bound).max()))
    # and the split is the emulation's split: hi = RNE(w s), lo = RNE(w s - hi)
    eh, el = split_emulation.split(torch.from_numpy(w) * s)
    assert np.array_equal(eh.numpy(), hi.astype(np.float32)) and np.array_equal(el.numpy(), lo.astype(np.float32)), what
    assert s == split_emulation.weight_scale(torch.from_numpy(w)), what
    return s


def test_weight_split_on_the_c1_weights(tiny_sd):
    n = 0
    for name, w in tiny_sd.items():
        if w.ndim == 4:
            _check_split(w, name)
            n += 1
    assert n >= 20


def test_weight_split_over_a_wide_range_and_on_zeros():
    rng = np.random.default_rng(11)
    mag = np.exp2(rng.uniform(-30.0, 3.0, 4096)).astype(np.float32)
    mag[0], mag[1] = 2.0 ** -30, 2.0 ** 3 * 0.999
    w = mag * rng.choice([-1.0, 1.0], mag.size).astype(np.float32)
    s = _check_split(w, "2^-30..2^3")
    assert s == 2.0 ** 11                                                # max|w| in [2^2, 2^3) -> [2^13, 2^14)
    assert _check_split(np.zeros(100, np.float32), "zeros") == 1.0


def test_emulated_arithmetic_meets_the_c1_gate(golden, tiny_sd):
    """The emulation on C1 (64 px, base 32, (1,2), 10 steps) against the reference's x_final, in the scope the GPU runs (N tiles
    of 64 and 128) and with every ResBlock conv and ConvTranspose split (the wider scope measured 8.7e-6 when the mode was designed)."""
    g = golden("c1_sample.npz")
    sd = ref_unet.as_torch_sd(tiny_sd)
    for kw in (dict(), dict(min_cout=0)):
        with split_emulation.emulated(**kw) as f:
            x = ref_diffusion.ddim_sample(ref_unet.make_model(sd), torch.from_numpy(g["z"]), torch.from_numpy(g["x_T"]), steps=10)
        err = float(np.abs(x.numpy() - g["x_final"]).max())
        print(f"f16x3 emulation, C1 10 steps, {kw or 'GPU scope'}: max-abs {err:.2e} ({f.n_split} split / {f.n_plain} plain convs)")
        assert f.n_split > 0 and f.n_plain > 0
        assert err < TOL_E2E_FP32, err
    assert ref_unet.F is torch.nn.functional
