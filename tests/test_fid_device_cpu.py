"""CPU: the host side of the device-resident FID route -- the argument and error contract of
``fid.sample_statistics`` / ``fid.get_fid_of_generator``, the latent stream they share with
``image_io.generate_fid_samples``, the new ``ops`` wrappers' refusal of CPU tensors, the ``fid_on_device`` switch of
``fit`` / ``evaluate`` (kernels stubbed: which route is called, with what, how often), and the one premise of the
sample-level parity test (tests/test_fid_device_gpu.py) that needs no device."""
import numpy as np
import pytest
import torch

import oracle

SAMPLE_SEED, N_LATENTS, N_HIDDEN = 1234, 8, 16        # shared with tests/test_fid_device_gpu.py
LEVEL_CAP = 0.01                                      # share of pixels that may differ by one 8-bit level


def oracle_generator():
    """The smallest 64 x 64 option set the model accepts (n_z stays [256, 8, 8]: the decoder's first layer takes 256
    channels), seeded ``weights_init``; train mode, as the reference never calls ``.eval()``."""
    torch.manual_seed(999)
    g = oracle.Generator_celeba(oracle.OracleOpt(n_hidden=N_HIDDEN))
    g.apply(oracle.weights_init)
    return g.train()


def latents():
    return torch.randn(N_LATENTS, N_HIDDEN, generator=torch.Generator().manual_seed(SAMPLE_SEED))


def quantize_restated(x):
    """``save_image(x[i], normalize=True)`` per image, restated (torchvision 0.2.1: clamp to [min, max], subtract min,
    divide by max - min + 1e-5; times 255, clamp, truncate) in the precision of x."""
    out = []
    for img in x:
        lo, hi = img.min(), img.max()
        v = (img.clamp(lo, hi) - lo) / (hi - lo + 1e-5)
        out.append((v * 255).clamp(0, 255).to(torch.uint8).permute(1, 2, 0))
    return torch.stack(out)


def level_report(a, b):
    d = (a.to(torch.int16) - b.to(torch.int16)).abs()
    return int(d.max()), float((d != 0).float().mean())


def test_oracle_fp32_decode_stays_under_the_level_cap_for_the_chosen_seed():
    """trunc flips a level only where v * 255 lies within ~255 * 3e-6 / (max - min) of an integer (~0.1 % of the
    pixels): the oracle's own fp32 decode against its fp64 decode must respect the cap the HIP decode is held to."""
    g = oracle_generator()
    z = latents()
    with torch.no_grad():
        u32 = quantize_restated(g(z))
        u64 = quantize_restated(g.double()(z.double()))
    worst, share = level_report(u32, u64)
    print(f"[fid_device] oracle fp32 vs fp64 decode: max level difference {worst}, share of pixels {share:.5f}")
    assert u32.shape == (N_LATENTS, 64, 64, 3)
    assert worst <= 1 and share <= LEVEL_CAP, (worst, share)


def test_error_contract_of_the_generator_entry_points(tmp_path):
    from disentangle_mlp_amd import fid
    fn = lambda z: pytest.fail("the decoder must not run")            # noqa: E731
    ex = lambda u8: pytest.fail("the network must not run")           # noqa: E731
    with pytest.raises(ValueError, match="at least 2 samples"):
        fid.sample_statistics(fn, 1, 8, ex, device="cpu")
    with pytest.raises(RuntimeError, match="Inception pool_3"):
        fid.sample_statistics(fn, 8, 8, None, device="cpu")
    with pytest.raises(ValueError, match="decode_batch"):
        fid.sample_statistics(fn, 8, 8, ex, device="cpu", decode_batch=0)
    npz = tmp_path / "ref.npz"
    fid.save_statistics(npz, np.zeros(4), np.eye(4))
    with pytest.raises(RuntimeError, match="Inception pool_3"):       # neither an extractor nor weights: the loud error
        fid.get_fid_of_generator(fn, 8, 8, str(npz), device="cpu")
    with pytest.raises(RuntimeError, match="pt_inception-2015-12-05"):
        fid.get_fid_of_generator(fn, 8, 8, str(npz), inception=str(tmp_path), device="cpu")    # a directory without weights
    with pytest.raises(ValueError, match="at least 2 samples"):
        fid.get_fid_of_generator(fn, 1, 8, str(npz), feature_extractor=ex, device="cpu")
    with pytest.raises(RuntimeError, match="Invalid path"):
        fid.get_fid_of_generator(fn, 8, 8, str(tmp_path / "missing.npz"), feature_extractor=ex, device="cpu")


def test_latent_stream_is_the_one_generate_fid_samples_draws(monkeypatch, tmp_path):
    from disentangle_mlp_amd import fid, image_io
    seen = {}

    class Stop(Exception):
        pass

    def writer_fn(z):
        seen["files"] = z.clone()
        return torch.zeros(z.shape[0], 3, 4, 4)
    monkeypatch.setattr(image_io, "save_image", lambda *a, **k: None)
    torch.manual_seed(77)
    image_io.generate_fid_samples(writer_fn, 0, 6, 10, str(tmp_path), device="cpu")

    def device_fn(z):
        seen["device"] = z.clone()
        raise Stop                                             # what follows needs the GPU
    torch.manual_seed(77)
    with pytest.raises(Stop):
        fid.sample_statistics(device_fn, 6, 10, lambda u8: None, device="cpu")
    assert seen["files"].shape == (6, 10) and torch.equal(seen["files"], seen["device"])
    # decode_batch (the documented deviation) cuts the same stream into pieces
    pieces = []

    def piece_fn(z):
        pieces.append(z.clone())
        raise Stop
    torch.manual_seed(77)
    with pytest.raises(Stop):
        fid.sample_statistics(piece_fn, 6, 10, lambda u8: None, device="cpu", decode_batch=4)
    assert torch.equal(pieces[0], seen["files"][:4])


def test_new_ops_refuse_cpu_tensors():
    from disentangle_mlp_amd import ops
    x = torch.zeros(2, 3, 8, 8)
    for call in (lambda: ops.quantize_each_u8(x), lambda: ops.pool3x3(x, 1, 1, "max"), lambda: ops.global_avg_pool(x),
                 lambda: ops.resize_bilinear_u8(torch.zeros(2, 8, 8, 3, dtype=torch.uint8))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    from disentangle_mlp_amd.inception import InceptionFeatureExtractor
    ex = InceptionFeatureExtractor.__new__(InceptionFeatureExtractor)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ex.features_u8(torch.zeros(2, 8, 8, 3, dtype=torch.uint8))


def test_pool_lowering_switch_defaults_to_aten():
    from disentangle_mlp_amd import inception
    assert inception.POOL_LOWERING == "aten" and inception._force_hip_pool is False
    assert not inception._hip_pool(torch.zeros(1))                     # CPU tensors never take the HIP pooling


def _stubbed_trainer(monkeypatch, calls):
    from disentangle_mlp_amd import fid, image_io
    from disentangle_mlp_amd.trainer import BetaVAEGANTrainer
    tr = BetaVAEGANTrainer(device="cpu")
    tr.train_epoch = lambda loader, label_rng=None, max_iterations=None: (calls.append(("train", loader)) or (3.0, 3.0, 0.5, 0.5))
    tr.load = lambda m: 5
    monkeypatch.setattr(image_io, "generate_fid_samples",
                        lambda fn, epoch, n, nh, path, device="cuda": calls.append(("fid_samples", fn, epoch, n, nh, path, str(device))))
    monkeypatch.setattr(fid, "get_fid_of_generator",
                        lambda fn, n, nh, pre, inception="", feature_extractor=None, device="cuda":
                        calls.append(("on_device", fn, n, nh, pre, feature_extractor, str(device))) or 7.25)
    return tr


def test_fid_on_device_off_keeps_the_file_route_exactly(monkeypatch):
    calls = []
    tr = _stubbed_trainer(monkeypatch, calls)
    score = lambda a, b: calls.append(("get_fid", a, b)) or 12.5      # noqa: E731
    for kw in ({}, {"fid_on_device": False}):
        calls.clear()
        rows = tr.fit("LOADER", epochs=2, calc_fid=True, n_samples=7, fid_path_recons="FIDDIR", fid_path_pretrained="PRE",
                      get_fid=score, verbose=False, **kw)
        assert [r["FID"] for r in rows] == [12.5, 12.5]
        assert calls == [("train", "LOADER"), ("fid_samples", tr.netEG.decode, 0, 7, 128, "FIDDIR", "cpu"), ("get_fid", "FIDDIR", "PRE"),
                         ("train", "LOADER"), ("fid_samples", tr.netEG.decode, 1, 7, 128, "FIDDIR", "cpu"), ("get_fid", "FIDDIR", "PRE")]
        calls.clear()
        res = tr.evaluate(["A"], calc_fid=True, n_samples=4, fid_path_samples="S", fid_path_pretrained="PRE", get_fid=score, **kw)
        assert res[0]["FID"] == 12.5
        assert calls == [("fid_samples", tr.netEG.decode, 5, 4, 128, "S", "cpu"), ("get_fid", "S", "PRE")]
    calls.clear()
    assert tr.fit("LOADER", epochs=1, fid_on_device=True, verbose=False)[0]["FID"] == "N/A"      # calc_fid stays the master switch
    assert calls == [("train", "LOADER")]


def test_fid_on_device_on_scores_the_decoder_and_writes_nothing(monkeypatch, tmp_path):
    calls = []
    tr = _stubbed_trainer(monkeypatch, calls)
    ex = object()
    rows = tr.fit("LOADER", epochs=2, calc_fid=True, n_samples=7, fid_path_recons=str(tmp_path), fid_path_pretrained="PRE",
                  get_fid=lambda a, b: pytest.fail("the file route must not run"), verbose=False, fid_on_device=True,
                  fid_feature_extractor=ex)
    assert [r["FID"] for r in rows] == [7.25, 7.25]
    on = ("on_device", tr.netEG.decode, 7, 128, "PRE", ex, "cpu")
    assert calls == [("train", "LOADER"), on, ("train", "LOADER"), on]            # one extractor for the whole fit
    assert list(tmp_path.iterdir()) == []
    calls.clear()
    res = tr.evaluate(["A", "B"], calc_fid=True, n_samples=4, fid_path_pretrained="PRE", fid_on_device=True, fid_feature_extractor=ex)
    assert [r["FID"] for r in res] == [7.25, 7.25] and calls == [("on_device", tr.netEG.decode, 4, 128, "PRE", ex, "cpu")] * 2
    with pytest.raises(RuntimeError, match="Inception pool_3"):                  # neither weights nor an extractor: before any epoch
        tr.fit("LOADER", epochs=1, calc_fid=True, fid_on_device=True, fid_path_pretrained="PRE", verbose=False)
    assert calls[2:] == []
