"""GPU: the aggregate-posterior kernels (csrc/agg_posterior.hip) against the fp64 restatement of tests/_latent_refs.py,
and through metrics.py and the trainers' `latent_report`.

Bound of every parity check, per tensor: max error over the reference's largest magnitude <= max(1e-6, 5 x the same
figure of the restatement evaluated in fp32) -- `_tc_refs.bound`, the project's convention.  Each check prints its figures
before it asserts (``pytest -s``).

Shapes (M, N, D): the issue's six; one point more than a wavefront's tile of points, one more than a workgroup's four
tiles and one row more than a row tile (a second, nearly empty wavefront, workgroup and tile); D one above the 16
dimensions a wavefront of the per-dimension kernel owns."""
import math

import pytest
import torch

import _latent_refs as L

pytestmark = pytest.mark.gpu

from disentangle_mlp_amd import ops  # noqa: E402

SHAPES = [(1, 1, 1), (3, 5, 7), (17, 65, 65), (64, 1000, 128), (130, 1100, 128), (40, 300, 200),
          (ops.AGG_POINT_TILE + 1, 50, 20), (ops.AGG_WORKGROUP_WAVES * ops.AGG_POINT_TILE + 1, 50, 20),
          (50, ops.AGG_ROW_TILE + 1, 20), (9, 20, 17)]
SPLITS = (0, 1, 2, 3, 7)

_cache = {}


def _case(shape, kind):
    """inputs and the (fp64, fp32) restatement of one case: computed once, shared, never modified"""
    k = (shape, kind)
    if k not in _cache:
        i = L.make_inputs(*shape, kind=kind)
        _cache[k] = (i, L.lse(i["z"], i["mu"], i["lv"], torch.float64), L.lse(i["z"], i["mu"], i["lv"], torch.float32))
    return _cache[k]


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _check(what, got, r32, r64):
    e, b = L.rel_err(got, r64), L.bound(r32, r64)
    print(f"{what}: error {e:.3e}  bound {b:.3e}  (fp32 restatement {L.rel_err(r32, r64):.3e})")
    assert torch.isfinite(torch.as_tensor(got)).all(), what
    assert e <= b, (what, e, b)


def _check_lse(what, got, r64, r32):
    assert got[0].dtype == torch.float64 and got[1].dtype == torch.float32
    _check(f"{what} lse_joint", got[0], r32[0], r64[0])
    _check(f"{what} lse_dim", got[1], r32[1], r64[1])


@pytest.mark.parametrize("kind", ["own", "far"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_lse_against_fp64(shape, kind):
    i, r64, r32 = _case(shape, kind)
    z, mu, lv = (i[k].cuda() for k in ("z", "mu", "lv"))
    for splits in SPLITS:
        a = ops.agg_posterior_lse(z, mu, lv, splits=splits or None)
        b = ops.agg_posterior_lse(z, mu, lv, splits=splits or None)
        _check_lse(f"{shape} {kind} splits={splits}", a, r64, r32)
        assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1])), splits


def test_splits_above_the_row_tiles_are_clamped():
    """The documented choice: a request above ceil(N / AGG_ROW_TILE) runs that many ranges -- the bits of asking for them."""
    shape = (17, 65, 65)
    i, r64, r32 = _case(shape, "own")
    z, mu, lv = (i[k].cuda() for k in ("z", "mu", "lv"))
    tiles = math.ceil(65 / ops.AGG_ROW_TILE)
    assert ops.agg_posterior_splits(17, 65, 65, tiles + 91) == tiles
    assert ops.agg_posterior_splits(17, 65, 65, 1) == 1
    a, b = ops.agg_posterior_lse(z, mu, lv, splits=tiles + 91), ops.agg_posterior_lse(z, mu, lv, splits=tiles)
    _check_lse(f"{shape} clamped", a, r64, r32)
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))
    with pytest.raises(RuntimeError):
        ops.agg_posterior_lse(z, mu, lv, splits=-1)


def _edge(name):
    if name not in _cache:
        i = dict(L.make_inputs(33, 33, 5, seed=7))
        if name == "shifted":        # every pair term far below log(FLT_MIN) = -87: a fixed shift would give log(0)
            i["z"] = i["mu"] + 40.0
        elif name == "on_a_narrow_row":
            i["lv"][3] = -6.0
            i["z"][0] = i["mu"][3]
        elif name == "one_row":
            i = dict(L.make_inputs(5, 1, 7, seed=7))
        _cache[name] = (i, L.lse(i["z"], i["mu"], i["lv"], torch.float64), L.lse(i["z"], i["mu"], i["lv"], torch.float32))
    return _cache[name]


@pytest.mark.parametrize("name", ["shifted", "on_a_narrow_row", "one_row"])
def test_edges(name):
    i, r64, r32 = _edge(name)
    if name == "shifted":
        lq = L.pair_terms(i["z"].double(), i["mu"].double(), i["lv"].double())
        assert float(lq.max()) < -87.0
    got = ops.agg_posterior_lse(*(i[k].cuda() for k in ("z", "mu", "lv")))
    _check_lse(name, got, r64, r32)


def test_rejected_arguments():
    from disentangle_mlp_amd import _lib
    lib = _lib.load()
    M, N, D = 5, 9, 7
    z, mu, lv = torch.zeros(M, D, device="cuda"), torch.zeros(N, D, device="cuda"), torch.zeros(N, D, device="cuda")
    lj, ld = torch.full((M,), 7.0, dtype=torch.float64, device="cuda"), torch.full((M, D), 7.0, device="cuda")
    need = lib.vg_agg_posterior_workspace_bytes(M, N, D, 0)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(m, n, d, nbytes, splits=0):
        return lib.vg_agg_posterior_lse(z.data_ptr(), mu.data_ptr(), lv.data_ptr(), lj.data_ptr(), ld.data_ptr(), m, n, d,
                                        splits, ws.data_ptr(), nbytes, st)

    assert call(M, N, D, need - 1) == -2                                  # VG_ERR_WORKSPACE
    for bad in ((M, N, 1025), (0, N, D), (M, 0, D)):
        assert call(*bad, need) == -1, bad                                # VG_ERR_BAD_ARG
    assert call(M, N, D, need, splits=-1) == -1
    torch.cuda.synchronize()
    assert bool((lj == 7.0).all()) and bool((ld == 7.0).all())            # nothing ran
    assert call(M, N, D, need) == 0
    torch.cuda.synchronize()
    assert torch.allclose(ld, torch.full_like(ld, math.log(N) - 0.5 * L.LOG_2PI), rtol=0, atol=1e-5)


# ---- metrics.py -----------------------------------------------------------------------------------------------------------
def _metric_inputs():
    """(N, D) = (600, 16); two factors that the code does carry: the sign of mu_0 (2 values) and the tercile of mu_1 (3)."""
    if "metrics" not in _cache:
        i = L.make_inputs(1, 600, 16, seed=5)
        mu = i["mu"]
        cuts = torch.quantile(mu[:, 1], torch.tensor([1 / 3, 2 / 3]))
        factors = torch.stack([(mu[:, 0] > 0).long(), torch.bucketize(mu[:, 1].contiguous(), cuts)], dim=1)
        assert factors[:, 0].unique().numel() == 2 and factors[:, 1].unique().numel() == 3
        _cache["metrics"] = (mu, i["lv"], factors)
    return _cache["metrics"]


def _compare(what, got, r64, r32):
    assert set(got) == set(r64) - {"identity"}, what
    for k, v in got.items():
        assert v.is_cuda, k
        if k == "active_units":
            assert int(v) == int(r64[k]), k
        else:
            assert v.dtype == torch.float64 and v.shape == r64[k].shape, k
            _check(f"{what} {k}", v, r32[k], r64[k])


@pytest.mark.parametrize("n_eval", [None, 100])
def test_elbo_decomposition_against_fp64(n_eval):
    from disentangle_mlp_amd import metrics
    mu, lv, _ = _metric_inputs()
    mu_d, lv_d = mu.cuda(), lv.cuda()
    got = metrics.elbo_decomposition(mu_d, lv_d, n_eval=n_eval, generator=torch.Generator("cuda").manual_seed(21))
    g = torch.Generator("cuda").manual_seed(21)              # the module's draws, in its order
    rows = torch.arange(600) if n_eval is None else torch.randperm(600, device="cuda", generator=g)[:n_eval].cpu()
    eps = torch.randn((rows.numel(), 16), device="cuda", generator=g)
    z = (mu_d[rows.cuda()] + eps * torch.exp(0.5 * lv_d[rows.cuda()])).cpu()
    r64, r32 = (L.elbo_decomposition(mu, lv, z, rows=rows, dtype=dt) for dt in (torch.float64, torch.float32))
    _compare(f"elbo n_eval={n_eval}", got, r64, r32)
    total = got["mi"] + got["tc"] + got["dwkl"]
    assert abs(float(total - r64["identity"])) <= 1e-9 * abs(float(r64["identity"]))


@pytest.mark.parametrize("n_eval_per_value", [None, 60])
def test_mig_against_fp64(n_eval_per_value):
    from disentangle_mlp_amd import metrics
    mu, lv, factors = _metric_inputs()
    mu_d, lv_d = mu.cuda(), lv.cuda()
    got = metrics.mig(mu_d, lv_d, factors.cuda(), n_eval_per_value=n_eval_per_value,
                      generator=torch.Generator("cuda").manual_seed(22))
    g = torch.Generator("cuda").manual_seed(22)
    z = (mu_d + torch.randn(mu_d.shape, device="cuda", generator=g) * torch.exp(0.5 * lv_d)).cpu()
    r64, r32 = (L.mig(mu, lv, z, factors, n_eval_per_value=n_eval_per_value, dtype=dt) for dt in (torch.float64, torch.float32))
    assert set(got) == set(r64)
    for k in got:
        assert got[k].shape == r64[k].shape, k
        _check(f"mig n={n_eval_per_value} {k}", got[k], r32[k], r64[k])
    assert int(got["mi_matrix"][:, 0].argmax()) == 0 and int(got["mi_matrix"][:, 1].argmax()) == 1


# ---- the trainers ---------------------------------------------------------------------------------------------------------
def _loader(labels=True):
    from disentangle_mlp_amd.data import DeviceImageDataset, DeviceLoader
    g = torch.Generator().manual_seed(9)
    images = torch.randint(0, 256, (16, 64, 64, 3), dtype=torch.uint8, generator=g)
    return DeviceLoader(DeviceImageDataset(images, (torch.arange(16) % 2).numpy() if labels else None), 4)


ELBO_KEYS = {"mi", "tc", "dwkl", "kl", "h_joint", "h_dim", "kl_dim", "active_units"}
MIG_KEYS = {"mig", "mig_per_factor", "mi_matrix"}


def test_latent_report_of_a_vae_trainer():
    from disentangle_mlp_amd import metrics, trainer as T
    tr = T.VAETrainer(graph=False)
    loader = _loader()
    torch.manual_seed(5)
    rep = tr.latent_report(loader)
    assert set(rep) == ELBO_KEYS | MIG_KEYS
    for k, v in rep.items():
        assert torch.isfinite(v.double()).all(), k
    assert rep["h_dim"].shape == (tr.opt.n_hidden,) and rep["mi_matrix"].shape == (tr.opt.n_hidden, 1)
    torch.manual_seed(5)
    mu, logvar, labels = metrics.encode_dataset(tr.model, loader)
    assert mu.shape == (16, tr.opt.n_hidden) and torch.equal(labels.cpu(), torch.arange(16) % 2)
    direct = metrics.elbo_decomposition(mu, logvar)
    for k in ELBO_KEYS:
        assert torch.equal(rep[k], direct[k]), k
    plain = tr.latent_report(_loader(labels=False), n_eval=8)          # constant labels: no factor, no MIG
    assert set(plain) == ELBO_KEYS
    given = tr.latent_report(_loader(labels=False), factors=torch.arange(16) % 4)
    assert set(given) == ELBO_KEYS | MIG_KEYS


def test_evaluate_carries_the_report_only_when_asked(tmp_path):
    from disentangle_mlp_amd import trainer as T
    tr = T.BetaVAEGANTrainer(graph=False)
    path = str(tmp_path / "ck.pth")
    tr.save(path, 3)
    rows = tr.evaluate([path])
    assert len(rows) == 1 and "latent" not in rows[0]
    asked = tr.evaluate([path], latent_report=_loader())
    assert {k: v for k, v in asked[0].items() if k != "latent"} == rows[0]
    assert set(asked[0]["latent"]) == ELBO_KEYS | MIG_KEYS
    assert all(torch.isfinite(v.double()).all() for v in asked[0]["latent"].values())
