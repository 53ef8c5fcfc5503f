"""The denoiser on the MI355X (setting "denoise", csrc/denoise.h): the HIP guide pass and filter against the numpy model and the
host emulation, groups / a one-rank communicator against the single context, and the quality bound of the CPU tier."""
import numpy as np
import pytest

import denoise_model
from test_denoise import QUALITY, _mse

pytestmark = pytest.mark.gpu


def _render(pkg, c, scene, w, h, spp=1, frames=1, **settings):
    c.init(w, h)
    scene.upload(c)
    for k, v in dict(integrator="pt", spp=spp, **settings).items():
        c.set_setting(k, v)
    for f in range(frames):
        c.render_frame(scene.camera, pkg.RESET if f == 0 else pkg.CONVERGE)
    return c


def _model(img, g):
    return denoise_model.denoise(img, g["albedo"], g["valid"], g["normal"], g["z"])


@pytest.mark.parametrize("name", ["cornell", "cards"])
def test_hip_filter_and_guides_match_the_model_and_the_emulation(pkg, make_hip, make_emu, name):
    w, h = 480, 270
    scene = pkg.scenes.cornell(w, h, geometric_emitter=True) if name == "cornell" else pkg.scenes.cards(w, h)
    hip = _render(pkg, make_hip(), scene, w, h)
    emu = _render(pkg, make_emu(), scene, w, h)
    raw = hip.framebuffer()
    g, ge = hip.read_denoise_guides(), emu.read_denoise_guides()
    # the guides: the same surfaces (a pixel whose centre ray grazes an edge may differ by rounding)
    same = g["valid"] == ge["valid"]
    assert same.mean() > 0.999
    both = g["valid"] & ge["valid"]
    assert np.mean(np.abs(g["z"][both] - ge["z"][both]) <= 1e-4 * ge["z"][both]) > 0.999
    assert np.mean(np.abs(g["albedo"][both] - ge["albedo"][both]).max(-1) <= 1e-3) > 0.99
    out = hip.denoise_image(raw)
    np.testing.assert_allclose(out, _model(raw, g), rtol=1e-4, atol=1e-6)
    # the emulation's filter on the same image with ITS guides: the same model (guides that differ by rounding in a few pixels
    # move the weights of their neighbourhoods, so the two filters are compared through the model, each with its own guides)
    np.testing.assert_allclose(emu.denoise_image(raw), _model(raw, ge), rtol=1e-4, atol=1e-6)
    hip.set_setting("denoise", 1)
    assert np.array_equal(hip.framebuffer(), out)


def test_full_size_terrain_matches_the_model(pkg, make_hip):
    scene = pkg.scenes.terrain()
    c = _render(pkg, make_hip(), scene, 1920, 1080)
    raw = c.framebuffer()
    g = c.read_denoise_guides()
    assert 0.3 < g["valid"].mean() < 1.0
    c.set_setting("denoise", 1)
    out = c.framebuffer()
    np.testing.assert_allclose(out, _model(raw, g), rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("n", [2, 4])
def test_groups_on_one_device_equal_the_single_context(pkg, make_hip, n):
    scene = pkg.scenes.terrain()
    ref = _render(pkg, make_hip(), scene, 1920, 1080, denoise=1)
    g = pkg.render_group([0] * n, "peer")
    g.init(1920, 1080)
    scene.upload(g)
    for k, v in dict(integrator="pt", spp=1, denoise=1).items():
        g.set_setting(k, v)
    g.render_frame(scene.camera, pkg.RESET)
    want = ref.framebuffer()
    assert np.array_equal(g.framebuffer(), want)
    # frames in flight hand out denoised frames too
    for f in range(3):
        ref.render_frame(scene.camera, pkg.CONVERGE)
        g.render_async(scene.camera, pkg.CONVERGE)
        g.present_async(f % 2)
        assert np.array_equal(g.present_wait(f % 2), ref.framebuffer()), f
    g.destroy()


def test_one_rank_comm_gather_is_denoised(pkg, make_hip):
    import torch
    scene = pkg.scenes.terrain()
    ref = _render(pkg, make_hip(), scene, 1920, 1080, denoise=1)
    c = _render(pkg, make_hip(), scene, 1920, 1080, denoise=1)
    comm = pkg.RenderComm(c, None)
    out = torch.zeros((1080, 1920, 4), dtype=torch.float32, device="cuda:0")
    comm.gather(out.data_ptr())
    comm.wait()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), ref.framebuffer())
    comm.destroy()


@pytest.mark.parametrize("spp", [1, 4])
def test_quality_on_the_gpu(pkg, make_hip, spp):
    w, h = 480, 270
    scene = pkg.scenes.cornell(w, h, geometric_emitter=True)
    ref = _render(pkg, make_hip(), scene, w, h, spp=1024).framebuffer()
    c = _render(pkg, make_hip(), scene, w, h, spp=spp)
    raw = c.framebuffer()
    c.set_setting("denoise", 1)
    den = c.framebuffer()
    gain = _mse(raw, ref) / _mse(den, ref)
    print("gpu quality spp=%d: gain %.2f" % (spp, gain))
    assert gain >= QUALITY[spp]
