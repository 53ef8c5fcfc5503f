"""Motion in the denoiser's temporal stage on the MI355X (setting "denoise_motion"; kernels k_dn_guides_surf and
k_dn_temporal_motion): the HIP stage against the model and the host emulation over the rigid sequences of the CPU tier, the
previous positions of a character posed on the device against the fixture's float64 poses, groups / a one-rank communicator
against the single context with frames in flight, and the quality bound of the CPU tier."""
import numpy as np
import pytest

import denoise_motion_model as MM
from test_denoise_motion import (CAMERAS, ON, QUALITY_FLOOR, _asset, _bits, _cornell, _move, deformed_frame, mover_transform,
                                 quality_gain, rigid_sequence)

pytestmark = pytest.mark.gpu


def _ctx(c, scene, w, h, spp=1, **settings):
    c.init(w, h)
    scene.upload(c)
    for k, v in dict(integrator="pt", spp=spp, **settings).items():
        c.set_setting(k, v)
    return c


def _rigid(pkg, make, scene, w, h, turn):
    # (the panning camera of the CPU tier's sequences: see CAMERAS there for what a still one does to check_frame at this size)
    return rigid_sequence(pkg, _ctx(make(), scene, w, h, **ON), _ctx(make(), scene, w, h, denoise_temporal=1), scene, turn, CAMERAS["pan"])


@pytest.mark.parametrize("turn", [False, True], ids=["translate", "translate_turn"])
def test_hip_stage_matches_the_model_and_the_emulation(pkg, make_hip, make_emu, turn):
    w, h = 480, 270
    scene = _cornell(pkg, w, h)
    hip = _rigid(pkg, make_hip, scene, w, h, turn)
    emu = _rigid(pkg, make_emu, scene, w, h, turn)
    for f, (hn, en) in enumerate(zip(hip, emu)):
        # the same history lengths almost everywhere (a pixel whose tap is borderline may round the other way)
        assert np.mean(np.abs(hn - en) < 1e-3) > 0.995, f


def test_cesiumman_posed_on_the_gpu_is_reprojected(pkg, make_hip):
    fx, scene, c, poses = _asset(pkg, make_hip, "cesiumman", 360, 480)
    prev_state, prev_pos = None, None
    for f, (apply, pos) in enumerate(poses):
        apply()
        c.update()
        c.render_frame(scene.camera, pkg.RESET)
        prev_state = deformed_frame(c, scene, fx, pos, prev_pos, prev_state, f)
        prev_pos = pos


def _frames(scene, n):
    return [mover_transform(scene, f, turn=True) for f in range(n)]


@pytest.mark.parametrize("n", [2, 4])
def test_groups_on_one_device_equal_the_single_context_in_flight(pkg, make_hip, n):
    w, h = 480, 270
    scene = _cornell(pkg, w, h)
    ref = _ctx(make_hip(), scene, w, h, **ON)
    g = pkg.render_group([0] * n, "peer")
    g.init(w, h)
    scene.upload(g)
    for k, v in dict(integrator="pt", spp=1, **ON).items():
        g.set_setting(k, v)
    frames, slots = 8, 4
    want = []
    for f, t in enumerate(_frames(scene, frames)):
        if f:
            _move((ref,), scene, t)
        ref.render_frame(scene.camera, pkg.RESET)
        want.append(ref.framebuffer())
    assert (ref.read_denoise_motion()["state"] == MM.MOVED).sum() > 500
    got = {}
    for f, t in enumerate(_frames(scene, frames)):  # 4 frames in flight: render(k), present_async(k % 4), present_wait((k + 1) % 4)
        if f:
            _move((g,), scene, t)
        g.render_async(scene.camera, pkg.RESET)
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
    w, h = 480, 270
    scene = _cornell(pkg, w, h)
    ref, c = _ctx(make_hip(), scene, w, h, **ON), _ctx(make_hip(), scene, w, h, **ON)
    comm = pkg.RenderComm(c, None)
    out = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
    for f, t in enumerate(_frames(scene, 4)):
        if f:
            _move((ref, c), scene, t)
        ref.render_frame(scene.camera, pkg.RESET)
        c.render_frame(scene.camera, pkg.RESET)
        comm.gather(out.data_ptr())
        comm.wait()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(ref.framebuffer())), f
    comm.destroy()


def test_quality_on_the_gpu(pkg, make_hip):
    gain, mse, n = quality_gain(pkg, make_hip, 480, 270)
    print("gpu motion quality: %d mover pixels, MSE motion=0 %.5g motion=1 %.5g gain %.2f" % (n, mse[0], mse[1], gain))
    assert gain >= QUALITY_FLOOR
