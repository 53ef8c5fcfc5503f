"""3D LUTs for the display stage's colour grading (include/rfwhip.h, rfwhip_set_display_lut): an n x n x n x 3 float array indexed
[b][g][r] — red fastest, the order of a .cube file — and the .cube text that rfwhip_set_display_lut_cube reads."""
import numpy as np


def identity(n):
    """The LUT that maps every colour to itself."""
    g = np.linspace(0.0, 1.0, n, dtype=np.float64)
    b, gg, r = np.meshgrid(g, g, g, indexing="ij")
    return np.stack([r, gg, b], -1).astype(np.float32)


def cube_text(lut, title=None):
    """The text of a .cube file: every float32 entry with nine significant digits, so that it reads back bit for bit."""
    a = np.asarray(lut, dtype=np.float32)
    n = a.shape[0]
    if a.shape != (n, n, n, 3):
        raise ValueError("a LUT is n x n x n x 3, got %s" % (a.shape,))
    lines = ["# %d^3 entries, red fastest" % n]
    if title is not None:
        lines.append('TITLE "%s"' % title)
    lines += ["LUT_3D_SIZE %d" % n, "DOMAIN_MIN 0 0 0", "DOMAIN_MAX 1 1 1"]
    lines += ["%.9g %.9g %.9g" % (float(r), float(g), float(b)) for r, g, b in a.reshape(-1, 3)]
    return "\n".join(lines) + "\n"


def write_cube(path, lut, title=None):
    with open(path, "w") as f:
        f.write(cube_text(lut, title))
