"""numpy (float64) restatement of the sky_sampling distribution (include/rfwhip.h, csrc/sky_sampling.h) and of the texel
mapping of the pt integrator's sky lookup (rt_core.h pt_sky) — test infrastructure for tests/test_sky_sampling*.py."""
import numpy as np


def luminance(rgb):
    """A texel's weight per steradian: max(0, 0.2126 r + 0.7152 g + 0.0722 b); NaN and negative texels weigh 0."""
    rgb = np.asarray(rgb, np.float64)
    l = 0.2126 * rgb[..., 0] + 0.7152 * rgb[..., 1] + 0.0722 * rgb[..., 2]
    return np.where(l > 0, l, 0.0)


def solid_angles(W, H):
    """Omega_j of every texel of row j: (2 pi / W) (cos(pi j / H) - cos(pi (j + 1) / H)), shape (H, 1)."""
    j = np.arange(H, dtype=np.float64)
    return (2 * np.pi / W) * (np.cos(np.pi * j / H) - np.cos(np.pi * (j + 1) / H))[:, None]


def distribution(px, W, H):
    """(P, lum, S): texel probabilities (H, W), luminances (H, W) and S = sum lum * Omega."""
    lum = luminance(np.asarray(px, np.float64).reshape(H, W, 3))
    w = lum * solid_angles(W, H)
    S = w.sum()
    return w / S, lum, S


def texel_of(D, W, H):
    """pt_sky's texel index of directions D (n, 3): u = W (1 + atan2(x, -z) / pi) / 2, v = H acos(y) / pi; -1 out of range."""
    D = np.asarray(D, np.float64)
    u = np.floor(W * 0.5 * (1.0 + np.arctan2(D[:, 0], -D[:, 2]) / np.pi)).astype(np.int64)
    v = np.floor(H * np.arccos(np.clip(D[:, 1], -1, 1)) / np.pi).astype(np.int64)
    idx = u + v * W
    return np.where((u >= 0) & (v >= 0) & (idx < W * H), idx, -1)


def pdf(D, px, W, H):
    """Sampling density per steradian: lum(texel(D)) / S (0 where pt_sky reads black)."""
    _, lum, S = distribution(px, W, H)
    t = texel_of(D, W, H)
    return np.where(t >= 0, lum.reshape(-1)[np.maximum(t, 0)] / S, 0.0)


def texel_centre_directions(W, H):
    """The direction through the middle (in phi and cos theta) of every texel, row-major (W H, 3)."""
    j, i = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    phi = -np.pi + 2 * np.pi * (i + 0.5) / W
    c0, c1 = np.cos(np.pi * j / H), np.cos(np.pi * (j + 1) / H)
    ct = 0.5 * (c0 + c1)
    st = np.sqrt(1 - ct * ct)
    return np.stack([st * np.sin(phi), ct, -st * np.cos(phi)], -1).reshape(-1, 3)


def local_coordinates(D, texel, W, H):
    """(a, b) of directions D inside texel (i, j): phi = -pi + 2 pi (i + a) / W, cos theta = cos theta_j - b (cos theta_j -
    cos theta_{j+1})."""
    D = np.asarray(D, np.float64)
    i, j = texel % W, texel // W
    phi = np.arctan2(D[:, 0], -D[:, 2])
    a = (phi + np.pi) * W / (2 * np.pi) - i
    c0, c1 = np.cos(np.pi * j / H), np.cos(np.pi * (j + 1) / H)
    b = (c0 - D[:, 1]) / (c0 - c1)
    return a, b
