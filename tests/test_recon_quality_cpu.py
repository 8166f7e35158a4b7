"""CPU: the C ABI of csrc/recon_quality.hip as far as the host alone can tell, the argument checks of
`ops.recon_quality`, the fp64 restatement of tests/_recon_refs.py against closed forms (it is the reference of the GPU
tests), the MS-SSIM scale rule and weights, and the glue of recon_quality.report / Accumulator over that restatement."""
import ctypes
import math
import os
import re

import pytest
import torch

import _recon_refs as R
from conftest import ROOT


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vaegan_hip.h")).read(), flags=re.S)


@pytest.fixture(scope="module")
def lib_path():
    from disentangle_mlp_amd import build
    return build.build(verbose=False)


def test_entries_are_declared_bound_and_exported(lib_path):
    from disentangle_mlp_amd import _lib, ops
    P, I, Z, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_double
    want = {"vg_recon_quality_workspace_bytes": (Z, [I] * 5),
            "vg_recon_quality": (I, [P, P, P] + [I] * 5 + [D] * 4 + [P, Z, P])}
    text = _header()
    lib = ctypes.CDLL(lib_path)
    for name, sig in want.items():
        assert _lib.SIGNATURES[name] == sig, name
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, text)
        assert decl and len(decl.group(1).split(",")) == len(sig[1]), name
        assert getattr(lib, name) is not None, name
    for define, value in (("VG_RECON_BAND_ROWS", ops.RECON_BAND_ROWS), ("VG_RECON_TILE_COLS", ops.RECON_TILE_COLS)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % define, text).group(1)) == value
    assert re.search(r"#define\s+VG_ABI_VERSION\s+(\d+)", text).group(1) == str(_lib.ABI_VERSION) == "7"      # only added


def test_workspace_query_rejects_what_the_kernel_rejects(lib_path):
    from disentangle_mlp_amd import _lib
    lib = ctypes.CDLL(lib_path)
    size = lib.vg_recon_quality_workspace_bytes
    size.restype, size.argtypes = _lib.SIGNATURES["vg_recon_quality_workspace_bytes"]
    for bad in ((0, 3, 64, 64, 11), (2, 0, 64, 64, 11), (2, 3, 0, 64, 11), (2, 3, 64, 0, 11), (-1, 3, 64, 64, 11),
                (2, 3, 64, 64, 10), (2, 3, 64, 64, 4), (2, 3, 64, 64, 1), (2, 3, 64, 64, 13), (2, 3, 64, 64, 0),
                (2, 3, 64, 64, -3), (2, 3, 10, 64, 11), (2, 3, 64, 10, 11), (2, 3, 2, 2, 3)):
        assert size(*bad) == 0, bad
    assert size(1, 1, 3, 3, 3) > 0 and size(65536, 3, 256, 256, 11) > 0
    assert size(2, 3, 11, 11, 11) > 0 and size(2, 3, 64, 64, 5) > 0
    assert size(4, 3, 64, 64, 11) >= 2 * size(2, 3, 64, 64, 11) - 256      # one slot per workgroup, per image


def test_ops_refuse_cpu_tensors_and_bad_arguments(monkeypatch):
    from disentangle_mlp_amd import ops
    x = torch.zeros(2, 3, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.recon_quality(x, x)
    # the remaining checks come before any launch: let every tensor pass for a device tensor
    monkeypatch.setattr(ops, "_req", lambda t, name: t)
    with pytest.raises(RuntimeError, match="one shape"):
        ops.recon_quality(x, torch.zeros(2, 3, 16, 17))
    with pytest.raises(RuntimeError, match="one shape"):
        ops.recon_quality(x[0], x[0])
    for window in (0, 1, 4, 10, 13, -3):
        with pytest.raises(ValueError, match="window must be odd and in 3..11"):
            ops.recon_quality(x, x, window=window)
    with pytest.raises(RuntimeError, match="H, W >= 11"):
        ops.recon_quality(torch.zeros(2, 3, 10, 16), torch.zeros(2, 3, 10, 16))
    with pytest.raises(RuntimeError, match="H, W >= 5"):
        ops.recon_quality(torch.zeros(2, 3, 16, 4), torch.zeros(2, 3, 16, 4), window=5)
    for kw in ({"sigma": 0.0}, {"sigma": float("nan")}, {"data_range": 0.0}, {"data_range": float("inf")}, {"k1": -1.0},
               {"k2": float("nan")}):
        with pytest.raises(ValueError, match="must be finite"):
            ops.recon_quality(x, x, **kw)


def test_the_restatement_checks_out():
    worst = R.check_self()
    print(f"[_recon_refs] direct 2-D window against separable, fp64: max per-pixel difference {worst:.3e}")


def test_the_textbook_fp32_form_is_what_the_kernel_avoids():
    """The issue's measurement, restated: the separable form in fp32 is off by ~1e-4 per pixel on a nearly flat input."""
    x, y, _ = R.pair("near_flat", (1, 1, 32, 32), seed=1)
    w = R.taps().float()
    m = lambda v: R.moments_separable(v, w)
    mx, my = m(x), m(y)
    c2 = torch.tensor((0.03 * 2.0) ** 2, dtype=torch.float32)
    cs32 = (2 * (m(x * y) - mx * my) + c2) / ((m(x * x) - mx * mx) + (m(y * y) - my * my) + c2)
    err = float((cs32.double() - R.maps(x, y)[1]).abs().max())
    print(f"[fp32 textbook] worst per-pixel cs error on the near-flat input: {err:.3e}")
    assert err > 1e-6                                          # four orders above the GPU tests' 1e-10


def test_ms_ssim_scale_rule_and_weights():
    from disentangle_mlp_amd import recon_quality as rq
    assert [rq.ms_ssim_scales(s, s) for s in (64, 128, 256)] == [3, 4, 5]
    assert rq.ms_ssim_scales(176, 176) == 5 and rq.ms_ssim_scales(175, 300) == 4 and rq.ms_ssim_scales(11, 40) == 1
    assert rq.ms_ssim_scales(64, 64, window=3) == 5
    with pytest.raises(ValueError, match="does not hold"):
        rq.ms_ssim_scales(10, 64)
    for s in (1, 2, 3, 4, 5):
        w = rq.ms_ssim_weights(s)
        assert len(w) == s and abs(sum(w) - 1.0) <= 1e-15
        assert all(abs(a / w[0] - b / R.WEIGHTS[0]) <= 1e-14 for a, b in zip(w, R.WEIGHTS))     # truncated, rescaled
    for size in (11, 21, 22, 43, 44, 64, 87, 88, 128, 175, 176, 256, 1000):
        assert rq.ms_ssim_scales(size, 999) == R.default_scales(size, 999), size
    # (the five published weights sum to 1.0001: at S = 5 the renormalisation divides by that)
    assert rq.ms_ssim_weights(5) == pytest.approx([w / sum(R.WEIGHTS) for w in R.WEIGHTS], abs=1e-15)
    assert rq.ms_ssim_weights(2, [0.3, 0.9]) == [0.3, 0.9]
    with pytest.raises(ValueError, match="weights for"):
        rq.ms_ssim_weights(3, [0.5, 0.5])
    with pytest.raises(ValueError, match="1..5"):
        rq.ms_ssim_weights(6)
    assert "NOT" in rq.ms_ssim.__doc__ and "published" in rq.ms_ssim.__doc__


# ---- the glue, over the restatement ----------------------------------------------------------------------------------
@pytest.fixture
def restated(monkeypatch):
    from disentangle_mlp_amd import ops
    calls = []

    def recon_quality(x, y, data_range=2.0, window=11, sigma=1.5, k1=0.01, k2=0.03):
        calls.append((tuple(x.shape), window))
        return R.recon_quality(x, y, data_range, window, sigma, k1, k2)
    monkeypatch.setattr(ops, "recon_quality", recon_quality)
    return calls


SCALARS = ("mse", "psnr", "ssim", "ms_ssim", "ssim_std")


def test_report_matches_the_restatement(restated):
    from disentangle_mlp_amd import recon_quality as rq
    x, y, _ = R.pair("noisy_copy", (5, 3, 64, 64), seed=2)
    got, want = rq.report(x, y, per_image=True), R.report(x, y)
    assert set(got) == {"n", "ms_ssim_scales", *SCALARS, "sse_per_image", "psnr_per_image", "ssim_per_image",
                        "ms_ssim_per_image"}
    assert got["n"] == 5 and got["ms_ssim_scales"] == 3 == want["ms_ssim_scales"]
    for k in SCALARS:
        assert got[k].dtype == torch.float64 and got[k].dim() == 0, k
        assert abs(float(got[k]) - float(want[k])) <= 1e-12 * max(1.0, abs(float(want[k]))), k
    assert restated == [((5, 3, 64, 64), 11), ((5, 3, 32, 32), 11), ((5, 3, 16, 16), 11)]      # the finest scale ONCE
    assert torch.allclose(got["ssim_per_image"], rq.ssim(x, y), rtol=0, atol=0)
    assert torch.allclose(got["psnr_per_image"], rq.psnr(x, y), rtol=0, atol=1e-12)
    assert torch.allclose(got["psnr_per_image"], R.psnr(x, y), rtol=0, atol=1e-12)
    assert torch.allclose(got["ms_ssim_per_image"], R.ms_ssim(x, y), rtol=0, atol=1e-14)
    assert torch.allclose(rq.ms_ssim(x, y, scales=2), R.ms_ssim(x, y, scales=2), rtol=0, atol=1e-14)
    assert float(got["mse"]) == float(got["sse_per_image"].mean()) > 0.0
    assert set(rq.report(x, y)) == {"n", "ms_ssim_scales", *SCALARS}


def test_psnr_is_pinned_when_an_image_comes_back_identical(restated):
    from disentangle_mlp_amd import recon_quality as rq
    x, y, _ = R.pair("noisy_copy", (3, 1, 16, 16), seed=4)
    y[1] = x[1]
    got = rq.report(x, y, per_image=True)
    assert math.isinf(float(got["psnr_per_image"][1])) and float(got["psnr_per_image"][1]) > 0
    assert torch.isfinite(got["psnr_per_image"][[0, 2]]).all()
    assert float(got["psnr"]) == float("inf")                  # documented: +inf, never NaN; `mse` stays finite
    assert math.isfinite(float(got["mse"])) and float(got["ssim_per_image"][1]) == pytest.approx(1.0, abs=1e-12)
    assert "inf" in rq.report.__doc__


def test_accumulator_equals_one_report(restated):
    from disentangle_mlp_amd import recon_quality as rq
    x, y, _ = R.pair("uniform", (7, 2, 24, 30), seed=6)
    whole = rq.report(x, y, per_image=True)
    acc = rq.Accumulator(per_image=True)
    assert acc.update(x[:4], y[:4]) is acc
    parts = acc.update(x[4:], y[4:]).result()
    assert parts["n"] == 7 and parts["ms_ssim_scales"] == 2
    for k in ("sse_per_image", "ssim_per_image", "ms_ssim_per_image", "psnr_per_image"):
        assert torch.equal(parts[k], whole[k]), k
    for k in SCALARS:
        assert torch.equal(parts[k], whole[k]), k
    with pytest.raises(ValueError, match="one size"):
        acc.update(x[:, :, :20], y[:, :, :20])
    with pytest.raises(ValueError, match="no batch"):
        rq.Accumulator().result()
    with pytest.raises(ValueError, match="one shape"):
        rq.report(x, y[:3])


def test_negative_coarse_cs_is_clamped(restated):
    """y = -x: every contrast-structure term is negative, each factor clamps at 0 and the product is exactly 0."""
    from disentangle_mlp_amd import recon_quality as rq
    x, _, _ = R.pair("uniform", (2, 1, 32, 32), seed=7)
    assert bool((R.coarse_cs(x, -x, 2) < 0).all())
    assert rq.ms_ssim(x, -x).tolist() == [0.0, 0.0] == R.ms_ssim(x, -x).tolist()


def test_a_trainer_without_an_encoder_has_nothing_to_reconstruct():
    from disentangle_mlp_amd import trainer as T
    tr = T.GANTrainer(device="cpu")
    with pytest.raises(TypeError, match="no encoder"):
        tr.reconstruction_report([(torch.zeros(2, 3, 64, 64), None)])
    with pytest.raises(TypeError, match="no discriminator"):
        T.VAETrainer(device="cpu").reconstruction_report([], dis_l=True)
    for cls in (T.BetaVAEGANTrainer, T.VAETrainer):
        assert "running" in cls.reconstruction_report.__doc__
