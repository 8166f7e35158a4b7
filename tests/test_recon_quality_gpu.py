"""MI355X: `ops.recon_quality` (csrc/recon_quality.hip) per image against the fp64 direct-2-D-window restatement of
tests/_recon_refs.py, its exactness / independence / NaN contracts to the bit, MS-SSIM and graph capture, and the routes
through the trainers (`reconstruction_report`, `evaluate(reconstruction_report=...)`).

The tolerance is derived, not measured: a window moment is 22 fp64 roundings (two chains of 11 FMAs) on |v| <= (L/2)^2,
sigma^2 is a difference of two such moments divided by at least C2 = (0.03 L)^2 = 3.6e-3 at the defaults, which bounds the
per-pixel error near 3e-12; the means are asserted to 1e-10 per image (about 30 x the bound, six orders below the fp32
textbook form).  The sum of squared errors is n = C H W non-negative fp64 terms: relative 4 n 2^-53.  MS-SSIM is a product
of at most five factors, each within 1e-10: 1e-9."""
import functools

import pytest
import torch

import _recon_refs as R

pytestmark = pytest.mark.gpu

TOL, TOL_MS = 1e-10, 1e-9


def _ops():
    from disentangle_mlp_amd import ops
    return ops


def _shapes(window):
    """The issue's five shapes, then one shape on each side of every band / column-tile boundary of the launcher: the
    SSIM map has H - window + 1 rows in bands of RECON_BAND_ROWS and W - window + 1 columns in tiles of RECON_TILE_COLS."""
    ops = _ops()
    rb, ct, h = ops.RECON_BAND_ROWS, ops.RECON_TILE_COLS, window - 1
    return [(2, 3, 11, 11), (3, 1, 12, 75), (1, 2, 37, 29), (2, 3, 64, 64), (1, 1, 176, 176),
            (1, 2, rb + h, ct + h),                # exactly one band, one tile
            (1, 1, rb + h - 1, ct + h + 1),        # a row short of the band; one column into the second tile
            (2, 1, rb + h + 1, ct + h - 1),        # one row into the second band; a column short of the tile
            (1, 1, 2 * rb + h, 2 * ct + h),        # two whole bands, two whole tiles
            (1, 1, 2 * rb + h + 1, 2 * ct + h + 1)]


CASES = [(i, window, kind) for window in (11, 3) for i in range(10) for kind in R.KINDS]


@functools.lru_cache(maxsize=None)
def _case(i, window, kind):
    """(x, y, data_range, reference [B, 3]) -- computed once, shared."""
    shape = _shapes(window)[i]
    x, y, L = R.pair(kind, shape, seed=17 * i + window)
    return x.cuda(), y.cuda(), L, R.recon_quality(x, y, data_range=L, window=window)


def _assert_close(got, want, n, what):
    got, want = got.cpu(), want.cpu()
    err = (got - want).abs()
    rel = float((err[:, 0] / want[:, 0].clamp(min=1e-300)).max())
    print(f"[recon_quality] {what}: sse rel {rel:.2e} (bound {4 * n * 2.0 ** -53:.2e}), ssim {float(err[:, 1].max()):.2e}, "
          f"cs {float(err[:, 2].max()):.2e} (bound {TOL:.0e})")
    assert bool((err[:, 0] <= 4 * n * 2.0 ** -53 * want[:, 0]).all()), what
    assert float(err[:, 1].max()) <= TOL and float(err[:, 2].max()) <= TOL, what


@pytest.mark.parametrize("i,window,kind", CASES, ids=lambda v: str(v))
def test_per_image_parity(i, window, kind):
    x, y, L, want = _case(i, window, kind)
    got = _ops().recon_quality(x, y, data_range=L, window=window)
    assert got.shape == (x.shape[0], 3) and got.dtype == torch.float64 and got.is_cuda
    _assert_close(got, want, x[0].numel(), f"{tuple(x.shape)} w={window} {kind}")


@pytest.mark.parametrize("window,sigma,k1,k2", [(5, 1.0, 0.01, 0.03), (7, 2.5, 0.02, 0.05), (9, 1.5, 0.0, 0.03)])
def test_other_windows_and_constants(window, sigma, k1, k2):
    x, y, L = R.pair("noisy_copy", (2, 2, 45, 70), seed=window)
    got = _ops().recon_quality(x.cuda(), y.cuda(), window=window, sigma=sigma, k1=k1, k2=k2)
    _assert_close(got, R.recon_quality(x, y, window=window, sigma=sigma, k1=k1, k2=k2), x[0].numel(), f"w={window}")


@pytest.mark.parametrize("window", (11, 3))
def test_an_image_against_itself_is_exact(window):
    from disentangle_mlp_amd import recon_quality as rq
    for i in (0, 3, 7, 9):
        for kind in ("uniform", "near_flat", "unit_range"):
            x, _, L, _ = _case(i, window, kind)
            got = _ops().recon_quality(x, x.clone(), data_range=L, window=window)
            assert bool((got[:, 0] == 0.0).all()) and bool((got[:, 1] == 1.0).all()) and bool((got[:, 2] == 1.0).all()), (i, kind)
            assert bool(torch.isposinf(rq.psnr(x, x.clone(), data_range=L)).all())
            assert bool((rq.ssim(x, x, data_range=L, window=window) == 1.0).all())


def _bits(t):
    return t.contiguous().view(torch.int64)


@pytest.mark.parametrize("shape", [(5, 3, 64, 64), (5, 1, 49, 91)], ids=str)
def test_an_image_has_the_same_bits_wherever_it_stands(shape):
    ops = _ops()
    x, y, _ = R.pair("noisy_copy", shape, seed=5)
    x, y = x.cuda(), y.cuda()
    whole = ops.recon_quality(x, y)
    assert torch.equal(_bits(whole), _bits(ops.recon_quality(x, y)))                      # a second run
    for b in (0, 2, 4):                                                                   # first, mid-batch, last
        alone = ops.recon_quality(x[b:b + 1].contiguous(), y[b:b + 1].contiguous())
        assert torch.equal(_bits(alone[0]), _bits(whole[b])), b
    moved = ops.recon_quality(x.flip(0).contiguous(), y.flip(0).contiguous())
    assert torch.equal(_bits(moved.flip(0)), _bits(whole))
    swapped = ops.recon_quality(y, x)
    assert torch.equal(_bits(swapped[:, 0]), _bits(whole[:, 0]))
    assert float((swapped[:, 1:] - whole[:, 1:]).abs().max()) <= 1e-12


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_a_non_finite_pixel_stays_in_its_image(bad):
    ops = _ops()
    x, y, _ = R.pair("noisy_copy", (3, 2, 40, 50), seed=8)
    x, y = x.cuda(), y.cuda()
    clean = ops.recon_quality(x, y)
    for at in ((0, 0, 0), (1, 20, 33), (1, 39, 49)):           # a corner, the seam of four workgroups, the last pixel
        dirty = y.clone()
        dirty[(1, *at)] = bad
        got = ops.recon_quality(x, dirty)
        assert not bool(torch.isfinite(got[1]).any()), (at, got[1])
        assert torch.equal(_bits(got[[0, 2]]), _bits(clean[[0, 2]])), at


def test_arguments_are_checked_on_the_device_too():
    ops = _ops()
    x = torch.zeros(2, 3, 16, 16, device="cuda")
    with pytest.raises(RuntimeError, match="expected float32"):
        ops.recon_quality(x.double(), x.double())
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.recon_quality(x.transpose(2, 3), x.transpose(2, 3))
    with pytest.raises(RuntimeError, match="one shape"):
        ops.recon_quality(x, x[:1])
    with pytest.raises(RuntimeError, match="H, W >= 11"):
        ops.recon_quality(x[:, :, :10].contiguous(), x[:, :, :10].contiguous())
    with pytest.raises(ValueError, match="window"):
        ops.recon_quality(x, x, window=4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.recon_quality(x, x.cpu())


# ---- composite metrics and capture -------------------------------------------------------------------------------------
def test_ms_ssim_against_the_restatement():
    from disentangle_mlp_amd import recon_quality as rq
    x, y, _ = R.pair("noisy_copy", (2, 3, 64, 64), seed=12)
    y[1] = -x[1]                                               # every contrast-structure term of image 1 is negative
    assert bool((R.coarse_cs(x, y, 3)[1] < 0).all()) and bool((R.coarse_cs(x, y, 3)[0] > 0).all())
    got, want = rq.ms_ssim(x.cuda(), y.cuda()).cpu(), R.ms_ssim(x, y)
    print(f"[ms_ssim] 64^2, S = 3: {got.tolist()} against {want.tolist()}")
    assert float((got - want).abs().max()) <= TOL_MS and float(got[1]) == 0.0 and 0.0 < float(got[0]) < 1.0
    x, y, _ = R.pair("noisy_copy", (1, 1, 176, 176), seed=13)
    got, want = rq.ms_ssim(x.cuda(), y.cuda()).cpu(), R.ms_ssim(x, y)
    print(f"[ms_ssim] 176^2, S = 5: {got.tolist()} against {want.tolist()}")
    assert rq.ms_ssim_scales(176, 176) == 5 and float((got - want).abs().max()) <= TOL_MS
    rep = rq.report(x.cuda(), y.cuda())
    assert rep["ms_ssim_scales"] == 5 and rep["ssim"].is_cuda and rep["ssim"].dtype == torch.float64 and rep["ssim"].dim() == 0
    assert abs(float(rep["ms_ssim"]) - float(want[0])) <= TOL_MS


def test_one_capture_replays_the_eager_bits():
    ops = _ops()
    x, y, _ = R.pair("noisy_copy", (4, 3, 64, 64), seed=14)
    x, y = x.cuda(), y.cuda()
    eager = ops.recon_quality(x, y).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.recon_quality(x, y)                                # warm-up on the capture stream: its workspace exists
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = ops.recon_quality(x, y)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(eager))
    x2, y2, _ = R.pair("uniform", (4, 3, 64, 64), seed=15)     # the replay reads the inputs where they are
    x.copy_(x2), y.copy_(y2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(ops.recon_quality(x, y)))


# ---- the trainers ------------------------------------------------------------------------------------------------------
N_HIDDEN = 16
REPORT_KEYS = {"n", "mse", "psnr", "ssim", "ms_ssim", "ms_ssim_scales", "ssim_std"}


@pytest.fixture(scope="module")
def trainer():
    from disentangle_mlp_amd.trainer import BetaVAEGANTrainer, ModelOpt
    torch.manual_seed(41)
    return BetaVAEGANTrainer(device="cuda", opt=ModelOpt(n_hidden=N_HIDDEN), graph=False)


@pytest.fixture(scope="module")
def loader():
    g = torch.Generator().manual_seed(42)
    return [(torch.rand(4, 3, 64, 64, generator=g) * 2 - 1, None), (torch.rand(3, 3, 64, 64, generator=g) * 2 - 1, None)]


def test_reconstruction_report_is_the_decode_of_mu_scored_by_hand(trainer, loader):
    from disentangle_mlp_amd import model as M
    net = trainer.netEG
    before = {k: v.clone() for k, v in net.state_dict().items()}
    got = trainer.reconstruction_report(loader, eval_mode=True)
    assert set(got) == REPORT_KEYS and got["n"] == 7 and got["ms_ssim_scales"] == 3 and net.training
    net.load_state_dict(before)
    xs, recons = [], []
    with torch.no_grad(), M.eval_mode(net):
        for data, _ in loader:
            x = data.cuda()
            xs.append(x)
            recons.append(net.decode(net.encode(x)[0]))
    want = R.report(torch.cat(recons), torch.cat(xs))
    print("[reconstruction_report]", {k: float(v) for k, v in got.items()}, "against", {k: float(v) for k, v in want.items()})
    n = 3 * 64 * 64
    assert abs(float(got["mse"]) - float(want["mse"])) <= 4 * n * 2.0 ** -53 * float(want["mse"])
    assert abs(float(got["psnr"]) - float(want["psnr"])) <= 1e-10
    assert abs(float(got["ssim"]) - float(want["ssim"])) <= TOL and abs(float(got["ssim_std"]) - float(want["ssim_std"])) <= TOL
    assert abs(float(got["ms_ssim"]) - float(want["ms_ssim"])) <= TOL_MS
    for k in ("mse", "psnr", "ssim", "ms_ssim", "ssim_std"):
        assert got[k].is_cuda and got[k].dtype == torch.float64 and got[k].dim() == 0, k


def test_sampled_reconstructions_follow_the_generator(trainer, loader):
    runs = [trainer.reconstruction_report(loader, sample=True, eval_mode=True,
                                          generator=torch.Generator(device="cuda").manual_seed(3)) for _ in range(2)]
    for k in ("mse", "psnr", "ssim", "ms_ssim", "ssim_std"):
        assert torch.equal(_bits(runs[0][k]), _bits(runs[1][k])), k
    other = trainer.reconstruction_report(loader, sample=True, eval_mode=True,
                                          generator=torch.Generator(device="cuda").manual_seed(4))
    mean = trainer.reconstruction_report(loader, eval_mode=True)
    assert float(other["mse"]) != float(runs[0]["mse"]) != float(mean["mse"])


def test_dis_l_is_added_on_request(trainer, loader):
    got = trainer.reconstruction_report(loader, dis_l=True)
    assert set(got) == REPORT_KEYS | {"dis_l"}
    assert got["dis_l"].dtype == torch.float64 and got["dis_l"].dim() == 0
    assert bool(torch.isfinite(got["dis_l"])) and float(got["dis_l"]) >= 0.0
    assert "dis_l" not in trainer.reconstruction_report(loader)


def test_evaluate_carries_the_report_only_when_asked(trainer, loader, tmp_path):
    path = str(tmp_path / "ck.pth")
    trainer.save(path, 2)
    rows = trainer.evaluate([path])
    assert len(rows) == 1 and "reconstruction" not in rows[0]
    asked = trainer.evaluate([path], reconstruction_report=loader, reconstruction_args={"dis_l": True}, eval_mode=True)
    assert {k: v for k, v in asked[0].items() if k != "reconstruction"} == rows[0]
    assert set(asked[0]["reconstruction"]) == REPORT_KEYS | {"dis_l"} and asked[0]["reconstruction"]["n"] == 7


def test_a_vae_trainer_reports_too(loader):
    from disentangle_mlp_amd.trainer import ModelOpt, VAETrainer
    torch.manual_seed(43)
    tr = VAETrainer(opt=ModelOpt(n_hidden=N_HIDDEN), graph=False)
    got = tr.reconstruction_report(loader)
    assert set(got) == REPORT_KEYS and got["n"] == 7 and 0.0 <= float(got["ms_ssim"]) <= 1.0
    with pytest.raises(TypeError, match="no discriminator"):
        tr.reconstruction_report(loader, dis_l=True)
