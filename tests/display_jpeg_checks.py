"""What tests/test_display_jpeg.py (host emulation) and tests/test_display_jpeg_gpu.py (the HIP kernels) both ask of a context: the
stream of rfwhip_jpeg_image equals the numpy model's (tests/jpeg_model.py) byte for byte, the coefficients, the record and the
capacity contract.  The model's streams are computed once per process and shared."""
import ctypes as C

import numpy as np
import pytest

import jpeg_model as jm

_MODEL = {}


def model(name, w, h, quality, sub, ri):
    """(image, stream, facts, coefficients) of one case, computed once."""
    key = (name, w, h, quality, sub, ri)
    if key not in _MODEL:
        img = getattr(jm, name)(w, h)
        stream, facts = jm.encode(img, quality, sub, ri)
        _MODEL[key] = (img, stream, facts, jm.coefficients(img, quality, sub))
    return _MODEL[key]


def configure(c, quality, sub, ri):
    c.set_setting("display_jpeg_quality", quality)
    c.set_setting("display_jpeg_subsampling", sub)
    c.set_setting("display_jpeg_restart", ri)


def matrix(w, h):
    """The cases of one size: every subsampling x quality x Ri, the three plain inputs in rotation."""
    k = 0
    for sub in jm.SUBS:
        for quality in jm.QUALITIES:
            for ri in jm.RESTARTS:
                yield ("constant", "smooth", "noise")[k % 3], quality, sub, ri
                k += 1


def stream_matches_the_model(c, name, w, h, quality, sub, ri):
    """c: a context initialised to w x h."""
    img, want, facts, coef = model(name, w, h, quality, sub, ri)
    configure(c, quality, sub, ri)
    got = c.jpeg_image(img)
    label = (name, w, h, quality, sub, ri)
    assert len(got) == len(want), (label, len(got), len(want))
    assert got == want, (label, "first difference at byte %d" % next(i for i in range(len(want)) if got[i] != want[i]))
    assert np.array_equal(c.jpeg_coefficients(), coef), label
    assert c.get_setting("display_jpeg_bytes") == str(len(want)), label
    rec = c.jpeg_record()
    assert rec == dict(bytes=len(want), intervals=facts["intervals"], mcus=facts["mcus"], blocks=facts["blocks"],
                       stuffed_bytes=facts["stuffed"], overflow=0, header_bytes=jm.HEADER_BYTES), (label, rec)
    assert len(want) <= c.jpeg_bound() == jm.bound(w, h, sub, ri), label


def cap_one_byte_short_is_refused(c, name, w, h, quality, sub, ri):
    """A cap one byte short: refused with the needed size, and nothing is written — the byte behind cap least of all."""
    img, want, _, _ = model(name, w, h, quality, sub, ri)
    configure(c, quality, sub, ri)
    fn = c._fn("jpeg_image")
    buf = np.full(len(want) + 8, 0xA5, np.uint8)
    n = C.c_size_t()
    assert fn(c._ctx, img.ctypes.data, buf.ctypes.data, len(want) - 1, C.byref(n)) != 0
    assert n.value == len(want) and str(len(want)) in c._fn("last_error")().decode()
    assert (buf == 0xA5).all()
    with pytest.raises(RuntimeError, match="%d bytes" % len(want)):
        c.jpeg_image(img, cap=0)
    assert fn(c._ctx, img.ctypes.data, buf.ctypes.data, len(want), C.byref(n)) == 0  # exactly enough
    assert bytes(buf[:len(want)]) == want and (buf[len(want):] == 0xA5).all()
