"""The denoiser's temporal stage on the MI355X (setting "denoise_temporal", csrc/denoise.h dn_temporal_item): the HIP stage against
the numpy model and the host emulation over a moving sequence, groups / a one-rank communicator against the single context with
frames in flight, and the quality bound of the CPU tier."""
import numpy as np
import pytest

import denoise_temporal_model as M
from test_denoise_temporal import QUALITY, _bits, _cut, _mse, check_frame

pytestmark = pytest.mark.gpu


def _ctx(pkg, c, scene, w, h, spp=1, **settings):
    c.init(w, h)
    scene.upload(c)
    for k, v in dict(integrator="pt", spp=spp, **settings).items():
        c.set_setting(k, v)
    return c


def _run_against_the_model(pkg, den, raw_ctx, scene, cams):
    changed = np.zeros(len(scene.instances), bool)
    prev, outs = None, []
    for f, cam in enumerate(cams):
        den.render_frame(cam, pkg.RESET)
        raw_ctx.render_frame(cam, pkg.RESET)
        raw = raw_ctx.framebuffer()
        out = den.framebuffer()
        assert np.array_equal(_bits(den.framebuffer()), _bits(out)), f
        hist = den.read_denoise_history()
        want, st = M.model_frame(den, cam, raw, prev, changed)
        check_frame(out, hist, want, st)
        v = st["valid"]
        assert f > 0 or (hist["length"][v] == 1).all()
        if (hist["length"][v] == 1).all():  # a fresh frame: the spatial filter bit for bit
            assert np.array_equal(_bits(out), _bits(den.denoise_image(raw))), f
        prev = dict(st, history=hist["history"], moments=hist["moments"], length=hist["length"])
        outs.append((out, hist["length"]))
    return outs


def test_hip_stage_matches_the_model_and_the_emulation(pkg, make_hip, make_emu):
    w, h = 480, 270
    scene = pkg.scenes.cornell(w, h, geometric_emitter=True)
    cams = [M.panned(scene.camera, 0.03 * k) for k in range(5)] + [_cut(scene)]
    hip = _run_against_the_model(pkg, _ctx(pkg, make_hip(), scene, w, h, denoise=1, denoise_temporal=1),
                                 _ctx(pkg, make_hip(), scene, w, h, denoise_temporal=1), scene, cams)
    emu = _run_against_the_model(pkg, _ctx(pkg, make_emu(), scene, w, h, denoise=1, denoise_temporal=1),
                                 _ctx(pkg, make_emu(), scene, w, h, denoise_temporal=1), scene, cams)
    for f, ((ho, hn), (eo, en)) in enumerate(zip(hip, emu)):
        # the same history lengths almost everywhere (a pixel whose tap is borderline may round the other way)
        assert np.mean(np.abs(hn - en) < 1e-3) > 0.995, f
    assert hip[-2][1].max() >= 5


def test_full_size_terrain_matches_the_model(pkg, make_hip):
    scene = pkg.scenes.terrain()
    cams = [M.panned(scene.camera, 0.3 * k) for k in range(3)]
    outs = _run_against_the_model(pkg, _ctx(pkg, make_hip(), scene, 1920, 1080, denoise=1, denoise_temporal=1),
                                  _ctx(pkg, make_hip(), scene, 1920, 1080, denoise_temporal=1), scene, cams)
    assert np.median(outs[-1][1][outs[-1][1] > 0]) > 2.5  # (the third frame: most pixels have two frames of history)


@pytest.mark.parametrize("n", [2, 4])
def test_groups_on_one_device_equal_the_single_context_in_flight(pkg, make_hip, n):
    scene = pkg.scenes.terrain()
    ref = _ctx(pkg, make_hip(), scene, 1920, 1080, denoise=1, denoise_temporal=1)
    g = pkg.render_group([0] * n, "peer")
    g.init(1920, 1080)
    scene.upload(g)
    for k, v in dict(integrator="pt", spp=1, denoise=1, denoise_temporal=1).items():
        g.set_setting(k, v)
    frames, slots = 8, 4
    want = []
    for f in range(frames):
        cam = M.panned(scene.camera, 0.3 * f)
        ref.render_frame(cam, pkg.RESET)
        want.append(ref.framebuffer())
    got = {}
    for f in range(frames):  # 4 frames in flight: render(k), present_async(k % 4), present_wait((k + 1) % 4)
        g.render_async(M.panned(scene.camera, 0.3 * f), pkg.RESET)
        g.present_async(f % slots)
        if f + 1 >= slots:
            k = f + 1 - slots
            got[k] = g.present_wait(k % slots).copy()
    for k in range(frames - slots + 1, frames):
        got[k] = g.present_wait(k % slots).copy()
    for f in range(frames):
        assert np.array_equal(_bits(got[f]), _bits(want[f])), f
    g.destroy()


def test_one_rank_comm_gather_runs_the_stage(pkg, make_hip):
    import torch
    scene = pkg.scenes.terrain()
    ref = _ctx(pkg, make_hip(), scene, 1920, 1080, denoise=1, denoise_temporal=1)
    c = _ctx(pkg, make_hip(), scene, 1920, 1080, denoise=1, denoise_temporal=1)
    comm = pkg.RenderComm(c, None)
    out = torch.zeros((1080, 1920, 4), dtype=torch.float32, device="cuda:0")
    for f in range(3):
        cam = M.panned(scene.camera, 0.3 * f)
        ref.render_frame(cam, pkg.RESET)
        c.render_frame(cam, pkg.RESET)
        comm.gather(out.data_ptr())
        comm.wait()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(ref.framebuffer())), f
    comm.destroy()


@pytest.mark.parametrize("motion", ["static", "pan"])
def test_quality_on_the_gpu(pkg, make_hip, motion):
    w, h = 64, 64
    scene = pkg.scenes.cornell(w, h, geometric_emitter=True)
    cams = [M.panned(scene.camera, (0.02 * k) if motion == "pan" else 0.0) for k in range(8)]
    ref = _ctx(pkg, make_hip(), scene, w, h, spp=1024)
    ref.render_frame(cams[-1], pkg.RESET)
    ref = ref.framebuffer()
    t = _ctx(pkg, make_hip(), scene, w, h, denoise=1, denoise_temporal=1)
    r = _ctx(pkg, make_hip(), scene, w, h, denoise_temporal=1)
    for cam in cams:
        t.render_frame(cam, pkg.RESET)
        r.render_frame(cam, pkg.RESET)
        temporal = t.framebuffer()
    spatial = t.denoise_image(r.framebuffer())
    gain = _mse(spatial, ref) / _mse(temporal, ref)
    print("gpu temporal quality %s: gain %.2f" % (motion, gain))
    assert gain >= QUALITY[motion]
