"""The reference of the differentiable augmentation, restated in plain torch: fp64 on the CPU,
differentiable by autograd, nothing imported from the package.  The integer mappings -- a uniform to a shift or to a cut
centre -- are done in fp32 exactly as the kernel's contract states them: ONE fp32 product, floor, clamp.

For one image x[C, H, W] and one row u[0..7] of uniforms in [0, 1), in this fixed order:
  colour       b = u0 - 1/2: x1 = x + b;  s = 2 u1: x2 = (x1 - mean_C x1) s + mean_C x1;  c = u2 + 1/2, m = mean_CHW x2:
               x3 = (x2 - m) c + m
  translation  r_h = int(H/8 + 1/2), t_r = min(floor(u3 (2 r_h + 1)), 2 r_h) - r_h, t_c alike from u4 and W:
               y[c, i, j] = x3[c, i + t_r, j + t_c] inside the image, 0 elsewhere
  cutout       k_h = int(H/2 + 1/2), n_h = H + 1 - (k_h mod 2), o_r = min(floor(u5 n_h), n_h - 1): rows o_r - k_h // 2 ..
               o_r - k_h // 2 + k_h - 1 are cut, columns alike from u6; a position whose row AND column are cut is 0
  gate         transformed iff u7 < p, else the image as it is.
"""
import numpy as np
import torch

COLOR, TRANSLATION, CUTOUT = 1, 2, 4
POLICIES = {1: "color", 2: "translation", 3: "color,translation", 4: "cutout", 5: "color,cutout", 6: "translation,cutout",
            7: "color,translation,cutout"}


def pick(u, n):
    """min(floor(u * n), n - 1) with the product in fp32."""
    return min(int(np.floor(np.float32(u) * np.float32(n))), n - 1)


def radius(size):
    return int(size / 8 + 0.5)


def shift_of(u, size):
    r = radius(size)
    return pick(u, 2 * r + 1) - r


def cut_size(size):
    return int(size / 2 + 0.5)


def cut_count(size):
    """n: the number of cut centres."""
    return size + 1 - cut_size(size) % 2


def cut_range(u, size):
    """(first, last) cut index along an axis of ``size``, clipped to the image."""
    k = cut_size(size)
    o = pick(u, cut_count(size))
    return max(o - k // 2, 0), min(o - k // 2 + k - 1, size - 1)


def geometry(u, H, W, policy):
    """(t_r, t_c, keep): ``keep`` [H, W] bool -- the output positions that take a source pixel (not cut, source inside)."""
    u = [float(v) for v in u]
    t_r, t_c = (shift_of(u[3], H), shift_of(u[4], W)) if policy & TRANSLATION else (0, 0)
    i, j = torch.arange(H)[:, None], torch.arange(W)[None, :]
    keep = (i + t_r >= 0) & (i + t_r < H) & (j + t_c >= 0) & (j + t_c < W)
    if policy & CUTOUT:
        (r0, r1), (c0, c1) = cut_range(u[5], H), cut_range(u[6], W)
        keep = keep & ~((i >= r0) & (i <= r1) & (j >= c0) & (j <= c1))
    return t_r, t_c, keep


def is_open(u_row, p):
    return bool(np.float32(u_row[7]) < np.float32(p))


def factors(u_row):
    """(b, s, c) in fp64 from the fp32 uniforms."""
    u = u_row.double()
    return u[0] - 0.5, 2.0 * u[1], u[2] + 0.5


def _shifted(v, t_r, t_c, keep):
    """out[c, i, j] = v[c, i + t_r, j + t_c] where keep[i, j], else 0 (a select: what is dropped is 0 whatever it held)."""
    C, H, W = v.shape
    i = (torch.arange(H)[:, None] + t_r).clamp(0, H - 1).expand(H, W)
    j = (torch.arange(W)[None, :] + t_c).clamp(0, W - 1).expand(H, W)
    return torch.where(keep[None], v[:, i, j], torch.zeros((), dtype=v.dtype))


def augment_one(x, u_row, policy, p):
    """One image, fp64, differentiable in x."""
    if not is_open(u_row, p):
        return x.clone()
    C, H, W = x.shape
    if policy & COLOR:
        b, s, c = factors(u_row)
        x = x + b
        xbar = x.mean(dim=0, keepdim=True)
        x = (x - xbar) * s + xbar
        m = x.mean()
        x = (x - m) * c + m
    t_r, t_c, keep = geometry(u_row, H, W, policy)
    return _shifted(x, t_r, t_c, keep)


def augment(x, u, policy, p=1.0):
    """x [B, C, H, W] (any float dtype, computed in fp64), u [B, 8] fp32 -> fp64 [B, C, H, W]."""
    x = x.double()
    return torch.stack([augment_one(x[b], u[b], policy, p) for b in range(x.shape[0])])


def transpose_one(gy, u_row, policy, p):
    """The explicit transpose of the linear part: g3 = gy masked and shifted back; g2 = c g3 + (1 - c) mean_CHW g3;
    gx = s g2 + (1 - s) mean_C g2."""
    if not is_open(u_row, p):
        return gy.clone()
    C, H, W = gy.shape
    t_r, t_c, keep = geometry(u_row, H, W, policy)
    masked = torch.where(keep[None], gy, torch.zeros((), dtype=gy.dtype))
    # source (i', j') was read by output (i' - t_r, j' - t_c), if that lies inside
    i, j = torch.arange(H)[:, None] - t_r, torch.arange(W)[None, :] - t_c
    inside = (i >= 0) & (i < H) & (j >= 0) & (j < W)
    g = torch.where(inside[None], masked[:, i.clamp(0, H - 1).expand(H, W), j.clamp(0, W - 1).expand(H, W)],
                    torch.zeros((), dtype=gy.dtype))
    if policy & COLOR:
        b, s, c = factors(u_row)
        g = c * g + (1.0 - c) * g.mean()
        g = s * g + (1.0 - s) * g.mean(dim=0, keepdim=True)
    return g


def transpose(gy, u, policy, p=1.0):
    gy = gy.double()
    return torch.stack([transpose_one(gy[b], u[b], policy, p) for b in range(gy.shape[0])])


def dropped_sources(u_row, H, W, policy):
    """[H, W] bool: the source pixels no output position reads -- shifted out of the frame or under the cut."""
    t_r, t_c, keep = geometry(u_row, H, W, policy)
    i, j = torch.arange(H)[:, None] - t_r, torch.arange(W)[None, :] - t_c
    inside = (i >= 0) & (i < H) & (j >= 0) & (j < W)
    read = inside & keep[i.clamp(0, H - 1).expand(H, W), j.clamp(0, W - 1).expand(H, W)]
    return ~read


# ---- rows of u for the tests ------------------------------------------------------------------------------------------------
ALMOST_ONE = float(np.nextafter(np.float32(1.0), np.float32(0.0)))


def edges(n):
    """fp32 values on both sides of every k / n, k = 1 .. n - 1, and the ends of [0, 1)."""
    out = [0.0, ALMOST_ONE]
    for k in range(1, n):
        t = np.float32(k) / np.float32(n)
        out += [float(np.nextafter(t, np.float32(0.0))), float(t), float(np.nextafter(t, np.float32(1.0)))]
    return out


def extreme_rows(p):
    """Hand-made rows: the largest shifts in all four directions, cut centres at 0 and n - 1 on both axes, s = 0, c at both
    ends, and u7 below, at and above ``p`` (at: closed).  [b, s/2, c - 1/2, shift row, shift col, cut row, cut col, gate]"""
    lo, hi = 0.0, ALMOST_ONE
    below = float(np.nextafter(np.float32(p), np.float32(0.0))) if p > 0 else 0.0
    rows = [
        [0.3, 0.7, 0.4, lo, lo, 0.5, 0.5, lo],          # up and left
        [0.3, 0.7, 0.4, hi, hi, 0.5, 0.5, lo],          # down and right
        [0.3, 0.7, 0.4, lo, hi, lo, lo, lo],            # mixed; cut centre 0, 0
        [0.3, 0.7, 0.4, hi, lo, hi, hi, lo],            # mixed; cut centre n - 1, n - 1
        [0.3, 0.7, 0.4, 0.5, 0.5, lo, hi, lo],          # cut centre 0, n - 1
        [0.3, 0.7, 0.4, 0.5, 0.5, hi, lo, lo],          # cut centre n - 1, 0
        [0.9, 0.0, lo, 0.2, 0.8, 0.3, 0.6, lo],         # s = 0, c = 1/2
        [0.1, hi, hi, 0.8, 0.2, 0.6, 0.3, lo],          # s ~ 2, c ~ 3/2
        [0.6, 0.4, 0.7, 0.1, 0.9, 0.4, 0.7, below],     # gate: just open
        [0.6, 0.4, 0.7, 0.1, 0.9, 0.4, 0.7, p],         # u7 == p: closed
        [0.6, 0.4, 0.7, 0.1, 0.9, 0.4, 0.7, hi],        # closed (unless p = 1)
    ]
    return torch.tensor(rows, dtype=torch.float32)
