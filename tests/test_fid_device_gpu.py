"""MI355X: the device-resident FID route against the oracle -- ``features_u8`` and the "hip" pooling of
``InceptionV3.forward`` against ``oracle.inception`` on seeded random weights (the pretrained file cannot be obtained:
absolute FID stays unpinned), the sample-level parity of HIP decoder + quantiser + network + Frechet arithmetic against
``oracle.modules`` / ``oracle.inception`` / ``oracle.fid`` on identical latents, ``get_fid_of_generator`` and
``fit(fid_on_device=True)``.  The oracle runs on the CPU; its results are computed once per module."""
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle import fid as ofid
from oracle.inception import random_fid_inception
from test_fid_device_cpu import LEVEL_CAP, N_HIDDEN, N_LATENTS, SAMPLE_SEED, latents, level_report, oracle_generator, \
    quantize_restated

pytestmark = pytest.mark.gpu


def record(key, value):
    """Measured figures go to the JSON-lines file VG_FID_RECORD names (the profile run sets it); printed always."""
    print(f"[fid_device] {key}: {value}")
    path = os.environ.get("VG_FID_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({key: value}) + "\n")


def oracle_features(ref, images_u8):
    torch.set_num_threads(16)
    with torch.no_grad():
        return ref(images_u8.float().permute(0, 3, 1, 2) / 255.0).reshape(images_u8.shape[0], -1)


@pytest.fixture(scope="module")
def ref():
    return random_fid_inception(0)


@pytest.fixture(scope="module")
def extractor(ref):
    from disentangle_mlp_amd.inception import InceptionFeatureExtractor
    return InceptionFeatureExtractor(ref.state_dict(), device="cuda", batch_size=4)        # 6 images: a ragged 2nd chunk


@pytest.fixture(scope="module")
def six(ref):
    imgs = torch.randint(0, 256, (6, 64, 64, 3), generator=torch.Generator().manual_seed(2), dtype=torch.uint8)
    return imgs, oracle_features(ref, imgs)


@pytest.fixture(scope="module")
def generator():
    """The HIP decoder with the oracle generator's seeded weights."""
    from disentangle_mlp_amd import model as M
    from disentangle_mlp_amd.trainer import ModelOpt
    g = M.Generator_celeba(ModelOpt(n_hidden=N_HIDDEN))
    g.load_state_dict(oracle_generator().state_dict())
    return g.cuda().train()


@pytest.fixture(scope="module")
def reference_statistics(ref):
    """Fixed, seeded: 8 other images through the oracle network and the oracle statistics."""
    imgs = torch.randint(0, 256, (8, 64, 64, 3), generator=torch.Generator().manual_seed(41), dtype=torch.uint8)
    return ofid.activation_statistics(oracle_features(ref, imgs).double().numpy())


def rel_l2(got, want):
    return float((got - want).norm() / want.norm())


def test_features_u8_match_the_oracle(extractor, six):
    imgs, want = six
    got = extractor.features_u8(imgs.cuda())
    assert got.shape == (6, 2048) and got.is_cuda and got.dtype == torch.float32
    e = rel_l2(got.cpu(), want)
    record("features_u8_rel_l2", e)
    assert e <= 1e-4, e
    assert torch.equal(got, extractor.features_u8(imgs.cuda()))                         # no atomics in any sum
    assert torch.equal(got[4:], extractor.features_u8(imgs[4:].cuda()))                 # the ragged chunk alone


def test_forward_with_hip_pooling_matches_the_oracle(extractor, six, monkeypatch):
    from disentangle_mlp_amd import inception
    imgs, want = six
    monkeypatch.setattr(inception, "POOL_LOWERING", "hip")
    e = rel_l2(extractor(imgs.float()).cpu(), want)
    record("forward_pool_hip_rel_l2", e)
    assert e <= 1e-4, e


def test_default_lowering_never_reaches_the_new_kernels(extractor, six, monkeypatch):
    """``POOL_LOWERING = "aten"`` (the default) changes no existing behaviour: with the four new wrappers made
    unreachable the existing entry point gives the same bits."""
    from disentangle_mlp_amd import inception, ops
    imgs, want = six
    assert inception.POOL_LOWERING == "aten"
    before = extractor(imgs.float())

    def unreachable(*a, **k):
        raise AssertionError("a csrc/fid_front.hip kernel on the default path")
    for name in ("pool3x3", "global_avg_pool", "resize_bilinear_u8", "quantize_each_u8"):
        monkeypatch.setattr(ops, name, unreachable)
    after = extractor(imgs.float())
    assert torch.equal(before, after)
    assert rel_l2(after.cpu(), want) <= 1e-4


def test_sample_parity_a_quantised_decoder_output(generator):
    """Half (a): ``ops.quantize_each_u8`` of the HIP decode against the restated quantisation of the oracle's fp64
    decode of the same latents and weights: at most one level apart, in at most 1 % of the pixels (trunc flips a level
    only where v * 255 lies within ~255 * 3e-6 / (max - min) of an integer: ~0.1 % expected; the oracle's own fp32
    decode is held to the same cap in tests/test_fid_device_cpu.py)."""
    from disentangle_mlp_amd import ops
    z = latents()
    with torch.no_grad():
        got = ops.quantize_each_u8(generator(z.cuda()).float().contiguous()).cpu()
        want = quantize_restated(oracle_generator().double()(z.double()))
    worst, share = level_report(got, want)
    record("sample_parity_a", {"max_level_difference": worst, "share_of_pixels": share})
    assert got.shape == (N_LATENTS, 64, 64, 3)
    assert worst <= 1 and share <= LEVEL_CAP, (worst, share)


def test_sample_parity_b_fid_of_the_same_images(generator, extractor, ref, reference_statistics):
    """Half (b): the device-produced uint8 images on both sides -- ``sample_statistics`` + ``calculate_frechet_distance``
    on the device, the oracle network + ``oracle.fid`` on the CPU.  |dFID| <= 1e-3 S, S = |mu1|^2 + |mu2|^2 + tr s1 +
    tr s2: every term is quadratic in features that agree to 1e-4 (~2e-4 S to first order, margin 5)."""
    from disentangle_mlp_amd import fid
    seen = []

    def capture(u8):
        seen.append(u8.cpu())
        return extractor.features_u8(u8)
    torch.manual_seed(SAMPLE_SEED)
    mu1, s1 = fid.sample_statistics(generator, N_LATENTS, N_HIDDEN, capture)
    mu2, s2 = reference_statistics
    assert mu1.is_cuda and s1.is_cuda and mu1.dtype == s1.dtype == torch.float64 and s1.shape == (2048, 2048)
    got = fid.calculate_frechet_distance(mu1, s1, mu2, s2)
    assert len(seen) == 1 and seen[0].shape == (N_LATENTS, 64, 64, 3)                    # decoded as ONE batch
    o_mu1, o_s1 = ofid.activation_statistics(oracle_features(ref, seen[0]).double().numpy())
    want = float(ofid.frechet_distance(o_mu1, o_s1, mu2, s2))
    S = float(o_mu1 @ o_mu1 + mu2 @ mu2 + np.trace(o_s1) + np.trace(s2))
    record("sample_parity_b", {"fid_device": got, "fid_oracle": want, "S": S, "abs_dfid_over_S": abs(got - want) / S})
    assert math.isfinite(got) and abs(got - want) <= 1e-3 * S, (got, want, S)


def test_get_fid_of_generator_is_its_pieces(generator, extractor, reference_statistics, tmp_path):
    from disentangle_mlp_amd import fid
    npz = tmp_path / "reference.npz"
    fid.save_statistics(npz, *reference_statistics)
    torch.manual_seed(5)
    got = fid.get_fid_of_generator(generator, N_LATENTS, N_HIDDEN, str(npz), feature_extractor=extractor)
    torch.manual_seed(5)
    mu1, s1 = fid.sample_statistics(generator, N_LATENTS, N_HIDDEN, extractor)
    want = fid.calculate_frechet_distance(mu1, s1, *fid.load_statistics(npz))
    assert isinstance(got, float) and math.isfinite(got) and got == want, (got, want)
    assert list(tmp_path.iterdir()) == [npz]


class _FourImages:
    def __init__(self):
        self.batch = torch.tanh(torch.randn(4, 3, 64, 64, generator=torch.Generator().manual_seed(9))).cuda()
        self.dataset, self.last_global_batch = list(range(4)), None

    def __iter__(self):
        self.last_global_batch = 4
        yield self.batch, None


def test_fit_scores_the_decoder_on_the_device_and_writes_no_file(extractor, reference_statistics, tmp_path):
    from disentangle_mlp_amd import fid
    from disentangle_mlp_amd.trainer import BetaVAEGANTrainer, ModelOpt
    npz, out = tmp_path / "reference.npz", tmp_path / "samples"
    out.mkdir()
    fid.save_statistics(npz, *reference_statistics)
    tr = BetaVAEGANTrainer(device="cuda", opt=ModelOpt(n_hidden=N_HIDDEN))
    logged = []
    rows = tr.fit(_FourImages(), epochs=1, calc_fid=True, n_samples=4, fid_path_recons=str(out), fid_path_pretrained=str(npz),
                  log=logged.append, max_iterations=1, verbose=False, fid_on_device=True, fid_feature_extractor=extractor)
    assert len(rows) == 1 and isinstance(logged[0]["FID"], float) and math.isfinite(logged[0]["FID"])
    assert list(out.iterdir()) == [] and sorted(p.name for p in tmp_path.iterdir()) == ["reference.npz", "samples"]
