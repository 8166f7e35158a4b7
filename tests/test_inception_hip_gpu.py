"""MI355X: the FID Inception network on the general fp16x3 convolution kernel (csrc/conv_general.hip) -- no im2col on the
device path, features against the fp64 oracle, the slice writes of every block type, memory against the forced
``unfold`` lowering, and get_fid end to end.

The feature bound: e_ref = the relative L2 error of the fp32 CPU oracle against the same network in fp64, computed here;
the device features must be within 8 x e_ref of the fp64 run.  Why 8: DESIGN.md section 2's measured per-convolution
errors on this hardware are 4e-7 ... 6e-7 for fp16x3 and 5e-7 ... 1e-6 for the fp32 MFMA, 2-4 x the CPU fp32
convolution's 0.7e-7 ... 2.5e-7 (the MFMA's K sum truncates); a further factor 2 covers the spread between inputs."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import fid as ofid
from oracle.inception import random_fid_inception

pytestmark = pytest.mark.gpu
FACTOR = 8


@pytest.fixture(scope="module")
def ref():
    torch.set_num_threads(16)
    return random_fid_inception(3)


@pytest.fixture(scope="module")
def ref64(ref):
    return copy.deepcopy(ref).double()


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def six_images():
    return torch.randint(0, 256, (6, 64, 64, 3), generator=torch.Generator().manual_seed(2)).float()


def oracle_blocks(m, x):
    """The four block outputs of InceptionV3.forward (scoring/inception.py:130-160) on the oracle's modules, no resize."""
    x = 2 * x - 1
    b0 = F.max_pool2d(m.Conv2d_2b_3x3(m.Conv2d_2a_3x3(m.Conv2d_1a_3x3(x))), kernel_size=3, stride=2)
    b1 = F.max_pool2d(m.Conv2d_4a_3x3(m.Conv2d_3b_1x1(b0)), kernel_size=3, stride=2)
    x = b1
    for name in ("Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
        x = getattr(m, name)(x)
    b2 = x
    for name in ("Mixed_7a", "Mixed_7b", "Mixed_7c"):
        x = getattr(m, name)(x)
    return [b0, b1, b2, F.adaptive_avg_pool2d(x, (1, 1))]


def test_no_im2col_on_the_device_path(ref, monkeypatch):
    from disentangle_mlp_amd.inception import InceptionFeatureExtractor

    def forbidden(*a, **k):
        raise AssertionError("im2col lowering on the device path")

    monkeypatch.setattr(torch.nn.functional, "unfold", forbidden)
    monkeypatch.setattr(torch, "baddbmm", forbidden)
    ex = InceptionFeatureExtractor(ref.state_dict(), device="cuda", batch_size=4)
    got = ex(six_images())
    assert got.shape == (6, 2048) and bool(torch.isfinite(got).all())


def test_features_against_the_fp64_oracle(ref, ref64):
    from disentangle_mlp_amd.inception import InceptionFeatureExtractor
    imgs = six_images()
    x = imgs.permute(0, 3, 1, 2) / 255.0
    with torch.no_grad():
        want64 = ref64(x.double()).reshape(6, -1)
        want32 = ref(x).reshape(6, -1)
    e_ref = rel_l2(want32, want64)
    got = InceptionFeatureExtractor(ref.state_dict(), device="cuda", batch_size=4)(imgs).cpu()
    e = rel_l2(got, want64)
    print(f"inception pool_3 features: device vs fp64 {e:.3e}, fp32 CPU vs fp64 (e_ref) {e_ref:.3e}, bound {FACTOR * e_ref:.3e}")
    assert e <= FACTOR * e_ref, (e, e_ref)


def test_all_four_blocks_against_the_fp64_oracle(ref, ref64):
    """75 x 75 inputs without resize: every block type writes its branches as channel slices of one output."""
    from disentangle_mlp_amd.inception import InceptionV3
    m = InceptionV3([0, 1, 2, 3], resize_input=False, weights=ref.state_dict()).cuda()
    x = torch.rand(2, 3, 75, 75, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        got = [o.cpu() for o in m(x.cuda())]
        want64 = oracle_blocks(ref64, x.double())
        want32 = oracle_blocks(ref, x)
    assert [o.shape[1] for o in got] == [64, 192, 768, 2048]
    bad = []
    for i in range(4):
        assert got[i].shape == want64[i].shape
        e_ref, e = rel_l2(want32[i], want64[i]), rel_l2(got[i], want64[i])
        print(f"inception block {i}: device vs fp64 {e:.3e}, e_ref {e_ref:.3e}, bound {FACTOR * e_ref:.3e}")
        if not e <= FACTOR * e_ref:
            bad.append((i, e, e_ref))
    assert not bad, bad


def test_default_and_unfold_paths_agree(ref, ref64, monkeypatch):
    from disentangle_mlp_amd import inception
    imgs = six_images()
    x = imgs.permute(0, 3, 1, 2) / 255.0
    with torch.no_grad():
        e_ref = rel_l2(ref(x).reshape(6, -1), ref64(x.double()).reshape(6, -1))
    ex = inception.InceptionFeatureExtractor(ref.state_dict(), device="cuda", batch_size=4)
    new = ex(imgs).cpu()
    monkeypatch.setattr(inception, "CONV_LOWERING", "unfold")
    old = ex(imgs).cpu()
    e = rel_l2(new, old)
    print(f"inception pool_3 features: kernel path vs unfold path {e:.3e}, bound {2 * FACTOR * e_ref:.3e}")
    assert e <= 2 * FACTOR * e_ref, (e, e_ref)


def test_peak_memory_is_below_the_unfold_lowering(ref, monkeypatch):
    from disentangle_mlp_amd import inception
    imgs = torch.randint(0, 256, (50, 64, 64, 3), generator=torch.Generator().manual_seed(5)).float()
    ex = inception.InceptionFeatureExtractor(ref.state_dict(), device="cuda", batch_size=50)

    def peak():
        ex(imgs)                                     # folds, packs, allocator warm-up
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        ex(imgs)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated(), base

    new, base_new = peak()
    monkeypatch.setattr(inception, "CONV_LOWERING", "unfold")
    old, base_old = peak()
    print(f"inception batch 50 peak memory: kernel path {new / 2**20:.0f} MiB (resident {base_new / 2**20:.0f}), "
          f"unfold path {old / 2**20:.0f} MiB (resident {base_old / 2**20:.0f})")
    assert new < old, (new, old)


def test_get_fid_on_the_device_end_to_end(ref, tmp_path):
    """tests/test_inception.py's CPU end-to-end construction with device="cuda"; relative 1e-4, the figure the project
    holds device features to."""
    from PIL import Image
    from disentangle_mlp_amd import fid
    rng = np.random.RandomState(4)
    folders = []
    for name, shift in (("a", 0), ("b", 40)):
        d = tmp_path / name
        d.mkdir()
        for i in range(6):
            img = np.clip(rng.randint(0, 200, size=(32, 32, 3)) + shift, 0, 255).astype(np.uint8)
            Image.fromarray(img).save(d / f"{i}.png")
        folders.append(d)
    wpath = tmp_path / "pt_inception-2015-12-05-rand.pth"
    torch.save(ref.state_dict(), wpath)
    got = fid.get_fid(str(folders[0]), str(folders[1]), inception=str(tmp_path), device="cuda")
    stats = []
    for d in folders:
        files = list(d.glob("*.jpg")) + list(d.glob("*.png"))
        x = torch.from_numpy(np.stack([np.asarray(Image.open(f).convert("RGB"), dtype=np.float32) for f in files]))
        with torch.no_grad():
            act = ref(x.permute(0, 3, 1, 2) / 255.0).reshape(len(files), -1).double().numpy()
        stats.append(ofid.activation_statistics(act))
    want = ofid.frechet_distance(*stats[0], *stats[1])
    print(f"get_fid on the device {got!r}, oracle {want!r}")
    assert abs(got - want) <= 1e-4 * max(abs(want), 1.0), (got, want)
