"""FID on the device: the arithmetic of /root/reference/scoring/fid.py.

What the reference does on the CPU with NumPy / SciPy -- mean and covariance of the Inception
pool_3 activations (fid.py:181-183) and the Frechet distance with a Schur-based
``scipy.linalg.sqrtm`` of a 2048 x 2048 product (:132-160) -- runs here in fp64 on the GPU:

* statistics are accumulated batch by batch (``ActivationStatistics.update``) as shifted sums
  ``sum(x - c)`` and ``(x - c)^T (x - c)`` (rocBLAS dgemm), so 10k x 2048 activations never have
  to exist at once and the generator's samples can stream straight from the decoder;
* ``Tr sqrt(C1 C2)`` is the sum of the square roots of the eigenvalues of the symmetric
  ``C1^{1/2} C2 C1^{1/2}`` (two ``eigh``): always real and finite, where the reference's sqrtm of
  the non-symmetric product needs its "singular product" and "imaginary component" branches.
  For non-singular inputs the two agree to ~1e-9 relative (tests/golden/fid_kat.npz, generated
  with the imported reference).  ``singular_offset=True`` applies the reference's eps*I offset
  (fid.py:146-150) explicitly -- the reference applies it only when sqrtm went non-finite.

File contract kept: ``.npz`` statistics with keys ``mu`` and ``sigma`` (fid.py:287-290),
``get_fid(path_data, path_pretrained, inception="", lowprofile=False)`` (fid.py:320-323).
The Inception pool_3 network is disentangle_mlp_amd/inception.py (the FID Inception-v3 of scoring/inception.py
on the device).  Its pretrained weights (fid.py:268-283 downloads a TensorFlow GraphDef; scoring/inception.py:13
the PyTorch port of the same weights) are NOT part of this repo and cannot be fetched here: pass the
``pt_inception-2015-12-05`` state_dict file as ``inception=`` (the reference's ``inception_path`` argument), or any
``feature_extractor`` callable (images [n,h,w,3] with values 0..255 -> [n,2048]); without either ``get_fid`` accepts
``.npz`` statistics on both sides and raises otherwise.  Absolute FID of images: unpinned (no weights, no reference
statistics offline).

Scoring a generator without files: ``get_fid_of_generator`` / ``sample_statistics`` take the decoder itself.  The
reference's route (utils.py:23-29 -> scoring/fid.py:286-300) writes one file per sample and reads them back; here the
decoder's output is quantised to the very bytes ``save_image(x[i], normalize=True)`` would have encoded
(``ops.quantize_each_u8``: bit-identical to the per-image writer) and goes to the network as a device uint8 tensor
(``InceptionFeatureExtractor.features_u8``) -- no PIL, no PCIe copy, no file.  Differences from the file route that are
NOT arithmetic: the lossy JPEG-in-PDF encoding of the reference's ``.pdf`` samples is skipped (a PNG would round-trip
these bytes exactly), and all ``n_samples`` are scored (scoring/fid.py:88 drops the remainder of the last batch of 50).

Keeping the activations: ``sample_features`` / ``path_features`` return the [n, d] activations themselves (the same loops
as ``sample_statistics`` / the folder route, unfolded), ``save_features`` writes them beside ``mu`` and ``sigma`` -- what
the metrics of sample_quality.py (precision / recall, density / coverage, KID) need and the statistics cannot give.
"""
import os
import pathlib

import numpy as np
import torch


def _dev64(a, device):
    if isinstance(a, torch.Tensor):
        return a.to(device=device, dtype=torch.float64)
    return torch.as_tensor(np.asarray(a, dtype=np.float64), device=device)


class ActivationStatistics:
    """Streaming mean / covariance (np.mean(axis=0), np.cov(rowvar=False)) in fp64 on the device."""

    def __init__(self, dim=2048, device="cuda"):
        self.device = torch.device(device)
        self.dim, self.n = int(dim), 0
        self.shift = None
        self.s1 = torch.zeros(dim, dtype=torch.float64, device=self.device)
        self.s2 = torch.zeros(dim, dim, dtype=torch.float64, device=self.device)

    def update(self, act):
        act = _dev64(act, self.device).reshape(-1, self.dim)
        if self.shift is None:                      # centre on the first batch: no cancellation later
            self.shift = act.mean(dim=0)
        x = act - self.shift
        self.s1 += x.sum(dim=0)
        self.s2.addmm_(x.t(), x)
        self.n += act.size(0)
        return self

    def finalize(self):
        """(mu [d], sigma [d,d]) as fp64 device tensors."""
        if self.n < 2:
            raise ValueError("covariance needs at least 2 samples")
        m = self.s1 / self.n
        sigma = (self.s2 - self.n * torch.outer(m, m)) / (self.n - 1)
        return m + self.shift, sigma


def calculate_activation_statistics(act, device="cuda", batch_size=4096):
    """fid.py:163-183 for precomputed activations [n, d] (numpy or tensor)."""
    d = act.shape[1]
    st = ActivationStatistics(d, device)
    for s in range(0, act.shape[0], batch_size):
        st.update(act[s:s + batch_size])
    return st.finalize()


def _sym_sqrt(c):
    w, v = torch.linalg.eigh((c + c.t()) * 0.5)
    return (v * w.clamp_min(0).sqrt()) @ v.t()


def calculate_frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6, device="cuda", singular_offset=False):
    """fid.py:109-160.  Accepts numpy arrays or tensors; returns a Python float."""
    device = torch.device(device)
    mu1, mu2 = _dev64(mu1, device).reshape(-1), _dev64(mu2, device).reshape(-1)
    sigma1, sigma2 = _dev64(sigma1, device), _dev64(sigma2, device)
    sigma1 = sigma1.reshape(mu1.numel(), -1)
    sigma2 = sigma2.reshape(mu2.numel(), -1)
    if mu1.shape != mu2.shape:
        raise AssertionError("Training and test mean vectors have different lengths")
    if sigma1.shape != sigma2.shape:
        raise AssertionError("Training and test covariances have different dimensions")
    diff = mu1 - mu2
    a, b = sigma1, sigma2
    if singular_offset:
        off = torch.eye(a.size(0), dtype=torch.float64, device=device) * eps
        a, b = a + off, b + off
    ra = _sym_sqrt(a)
    m = ra @ b @ ra
    lam = torch.linalg.eigvalsh((m + m.t()) * 0.5)
    tr_covmean = lam.clamp_min(0).sqrt().sum()
    val = diff.dot(diff) + torch.trace(sigma1) + torch.trace(sigma2) - 2 * tr_covmean
    return float(val)


def save_statistics(path, mu, sigma):
    """The .npz layout fid.py:287-290 reads."""
    to_np = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    np.savez(path, mu=to_np(mu), sigma=to_np(sigma))


def load_statistics(path):
    with np.load(path) as f:
        return f["mu"][:], f["sigma"][:]


def _load_images(files):
    from PIL import Image
    return np.stack([np.asarray(Image.open(str(fn)).convert("RGB"), dtype=np.float32) for fn in files])


_NO_EXTRACTOR = (
    "FID of an image folder needs the Inception pool_3 network; its weights "
    "(classify_image_graph_def.pb, fid.py:268-283) are not distributed with this package and cannot be "
    "downloaded here.  Pass feature_extractor=callable(images[n,h,w,3] float 0..255) -> [n,2048], or "
    "precomputed .npz statistics.")


def _path_activations(path, feature_extractor, batch_size=50):
    """The activations [n_i, d] of a folder of *.jpg / *.png images, batch by batch (fid.py:88: the remainder of the
    last batch is never propagated)."""
    if feature_extractor is None:
        raise RuntimeError(_NO_EXTRACTOR)
    p = pathlib.Path(path)
    files = list(p.glob("*.jpg")) + list(p.glob("*.png"))
    n_batches = len(files) // min(batch_size, max(len(files), 1))   # fid.py:88: the remainder is never propagated
    bs = min(batch_size, len(files))
    for i in range(n_batches):
        act = feature_extractor(_load_images(files[i * bs:(i + 1) * bs]))
        act = torch.as_tensor(np.asarray(act) if not isinstance(act, torch.Tensor) else act)
        yield act.reshape(act.shape[0], -1)


def _handle_path(path, feature_extractor, device, batch_size=50):
    """fid.py:286-300: .npz statistics or a folder of *.jpg / *.png images."""
    if str(path).endswith(".npz"):
        return load_statistics(path)
    st = None
    for act in _path_activations(path, feature_extractor, batch_size):
        st = st or ActivationStatistics(act.shape[1], device)
        st.update(act)
    if st is None:
        raise RuntimeError(f"no *.jpg / *.png images under {path}")
    return st.finalize()


def path_features(path, feature_extractor=None, device="cuda"):
    """[n, d] fp32 on ``device``: the ``features`` array of an ``.npz`` written by `save_features`, or the activations of
    an image folder -- the same files and the same remainder rule as the FID of that folder (`_handle_path`)."""
    if str(path).endswith(".npz"):
        with np.load(path) as f:
            if "features" not in f.files:
                raise RuntimeError(f"{path} holds no `features` array (keys: {sorted(f.files)}): statistics alone "
                                   "(mu, sigma) cannot serve the sample-quality metrics; write the file with "
                                   "fid.save_features")
            feats = f["features"][:]
        return torch.as_tensor(feats).to(device=device, dtype=torch.float32).contiguous()
    acts = [act.to(device=device, dtype=torch.float32) for act in _path_activations(path, feature_extractor)]
    if not acts:
        raise RuntimeError(f"no *.jpg / *.png images under {path}")
    return torch.cat(acts).contiguous()


def save_features(path, features):
    """`save_statistics` plus the activations themselves: ``mu``, ``sigma`` (fp64, of all rows) and ``features`` (fp32
    [n, d]) in one ``.npz``, which then serves `get_fid`, `get_fid_of_generator` and `path_features` alike."""
    feats = features.detach() if isinstance(features, torch.Tensor) else torch.as_tensor(np.asarray(features))
    if feats.dim() != 2 or feats.shape[0] < 2:
        raise ValueError("save_features: features must be [n, d] with n >= 2")
    mu, sigma = calculate_activation_statistics(feats, device=feats.device)
    np.savez(path, mu=mu.cpu().numpy(), sigma=sigma.cpu().numpy(), features=feats.float().cpu().numpy())


def _find_inception_weights(inception_path):
    """The reference's ``inception_path`` is a directory or file of the Inception model (fid.py:268-283); here: the
    ``pt_inception-2015-12-05*.pth`` state_dict, given directly or looked up in a directory."""
    if not inception_path:
        return None
    p = pathlib.Path(inception_path)
    if p.is_file():
        return str(p)
    if p.is_dir():
        hits = sorted(p.glob("pt_inception-2015-12-05*.pth"))
        if hits:
            return str(hits[0])
    raise RuntimeError(f"no Inception state_dict (pt_inception-2015-12-05*.pth) at {inception_path!r}")


def calculate_fid_given_paths(paths, inception_path="", low_profile=False, feature_extractor=None, device="cuda"):
    """fid.py:303-317."""
    for p in paths:
        if not os.path.exists(p):
            raise RuntimeError("Invalid path: %s" % p)
    if feature_extractor is None and not all(str(p).endswith(".npz") for p in paths):
        weights = _find_inception_weights(inception_path)
        if weights is not None:
            from .inception import InceptionFeatureExtractor
            feature_extractor = InceptionFeatureExtractor(weights, device=device)
    m1, s1 = _handle_path(paths[0], feature_extractor, device)
    m2, s2 = _handle_path(paths[1], feature_extractor, device)
    return calculate_frechet_distance(m1, s1, m2, s2, device=device)


def get_fid(path_data, path_pretrained, inception="", lowprofile=False, feature_extractor=None, device="cuda"):
    """fid.py:320-323."""
    return calculate_fid_given_paths([path_data, path_pretrained], inception, lowprofile, feature_extractor, device)


def _eval_nets(fn, eval_mode):
    """The networks ``eval_mode=True`` puts into eval mode around ``fn``: ``fn`` itself when it is a module, the module
    it is a bound method of (``netEG.decode``) otherwise.  () for False."""
    if not eval_mode:
        return ()
    net = fn if isinstance(fn, torch.nn.Module) else getattr(fn, "__self__", None)
    if not isinstance(net, torch.nn.Module):
        raise ValueError("eval_mode=True needs fn to be a module or a bound method of one (netEG.decode); wrap a "
                         "plain function's call in model.eval_mode(net) yourself")
    return (net,)


def _sample_activations(fn, n_samples, n_hidden, feature_extractor, device, decode_batch, eval_mode):
    """The one loop behind `sample_statistics` and `sample_features`: yields the activations [n_i, d] of each decoded
    piece, in order -- the CPU draw, the decoding, the quantisation and the extractor calls documented there."""
    if feature_extractor is None:
        raise RuntimeError(_NO_EXTRACTOR)
    if decode_batch is not None and int(decode_batch) < 1:
        raise ValueError("decode_batch must be positive")
    extract = getattr(feature_extractor, "features_u8", feature_extractor)
    from . import model, ops
    with torch.no_grad(), model.eval_mode(*_eval_nets(fn, eval_mode)):
        z = torch.randn(n_samples, n_hidden)                 # CPU draw, like the reference
        step = n_samples if decode_batch is None else int(decode_batch)
        for s in range(0, n_samples, step):
            sample = fn(z[s:s + step].to(device))
            act = extract(ops.quantize_each_u8(sample.detach().float().contiguous()))
            yield act.reshape(act.shape[0], -1)


def sample_statistics(fn, n_samples, n_hidden, feature_extractor, device="cuda", decode_batch=None, eval_mode=False):
    """(mu, sigma), fp64 device tensors, of the pool_3 activations of ``n_samples`` decoded N(0, 1) codes -- what
    utils.py:23-29 + scoring/fid.py:286-300 compute through files, without leaving the device.

    The codes are drawn as ``image_io.generate_fid_samples`` draws them (``torch.randn(n_samples, n_hidden)`` on the
    CPU: the same seed gives the same latents) and decoded by ``fn`` (``netEG.decode``) as ONE batch, like the
    reference.  ``decode_batch`` decodes them in pieces instead: under the default train-mode BatchNorm a DEVIATION,
    because the reference never calls ``.eval()`` and batch statistics make a sample depend on the batch it is decoded
    with; it is opt-in, for ``n_samples`` whose activations do not fit.  ``eval_mode=True`` wraps the decoding in
    ``model.eval_mode(net)``, ``net`` the module ``fn`` is (or is a bound method of): BatchNorm on its running
    statistics, every sample a function of its own latent alone -- ``decode_batch`` is then no deviation, only a memory
    setting -- and the network is back in its previous mode afterwards.  The default keeps the reference's train-mode
    behaviour.
    Each decoded image is quantised as ``save_image(x[i], normalize=True)``
    would (``ops.quantize_each_u8``); ``feature_extractor`` is an ``InceptionFeatureExtractor`` (its ``features_u8`` is
    used) or any callable on device uint8 images [n,h,w,3] -> [n,d]."""
    n_samples = int(n_samples)
    if n_samples < 2:
        raise ValueError("covariance needs at least 2 samples")
    st = None
    for act in _sample_activations(fn, n_samples, n_hidden, feature_extractor, device, decode_batch, eval_mode):
        st = st or ActivationStatistics(act.shape[1], device)
        st.update(act)
    return st.finalize()


def sample_features(fn, n_samples, n_hidden, feature_extractor, device="cuda", decode_batch=None, eval_mode=False):
    """The activations themselves, [n_samples, d] fp32 on ``device``: the same draw, decoding, quantisation and extractor
    calls as `sample_statistics` (one loop serves both), kept instead of folded into the statistics -- what
    `sample_quality` needs (``ActivationStatistics(d, device).update(features).finalize()`` of an undivided decode is
    `sample_statistics` of the same seed)."""
    n_samples = int(n_samples)
    if n_samples < 1:
        raise ValueError("n_samples must be positive")
    acts = [act.to(device=device, dtype=torch.float32)
            for act in _sample_activations(fn, n_samples, n_hidden, feature_extractor, device, decode_batch, eval_mode)]
    return (acts[0] if len(acts) == 1 else torch.cat(acts)).contiguous()


def get_fid_of_generator(fn, n_samples, n_hidden, path_pretrained, inception="", feature_extractor=None, device="cuda",
                         eval_mode=False):
    """FID of the generator ``fn`` (``netEG.decode``) against ``path_pretrained`` (``.npz`` statistics, or an image
    folder: `_handle_path`): ``generate_fid_samples`` + ``get_fid`` (new_betavaegan.py:231-235) with nothing written.
    ``inception`` as in `get_fid`; ``feature_extractor`` and ``eval_mode`` as in `sample_statistics`."""
    if int(n_samples) < 2:
        raise ValueError("covariance needs at least 2 samples")
    if not os.path.exists(path_pretrained):
        raise RuntimeError("Invalid path: %s" % path_pretrained)
    if feature_extractor is None:
        weights = _find_inception_weights(inception)
        if weights is None:
            raise RuntimeError(_NO_EXTRACTOR)
        from .inception import InceptionFeatureExtractor
        feature_extractor = InceptionFeatureExtractor(weights, device=device)
    m2, s2 = _handle_path(path_pretrained, feature_extractor, device)
    m1, s1 = sample_statistics(fn, n_samples, n_hidden, feature_extractor, device, eval_mode=eval_mode)
    return calculate_frechet_distance(m1, s1, m2, s2, device=device)
