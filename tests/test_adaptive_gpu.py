"""Adaptive sampling on the device (k_primary_packet_masked, k_extend_masked, k_resolve_adaptive, k_present_adaptive,
k_noise_tiles_adaptive, k_adaptive_step, k_adaptive_connections; work items: csrc/adaptive.h): the checks of tests/test_adaptive.py
on the HIP kernels at the same small shapes, held bit for bit to a reference of their own kind — the HIP build with the setting off,
not the emulation — one 1920 x 1080 terrain case with a forced checkerboard, and a group of two contexts on one device."""
import pytest

import test_adaptive as ta

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("scene_name,w,h,every,min_samples,look,monotone", ta.ORACLE_CASES)
def test_oracle(pkg, make_hip, scene_name, w, h, every, min_samples, look, monotone):
    ta.check_oracle(pkg, make_hip, "hip", scene_name, w, h, every, min_samples, look, monotone)[0].destroy()


@pytest.mark.parametrize("spp,calls,settings", ta.FORMS, ids=lambda v: str(v).replace(" ", ""))
def test_kernel_forms(pkg, make_hip, spp, calls, settings):
    ta.check_form(pkg, make_hip, "hip", spp, calls, settings)


@pytest.mark.parametrize("settings", ta.SCHEDULES, ids=lambda v: str(v).replace(" ", ""))
def test_scheduling_changes_no_bit(pkg, make_hip, settings):
    ta.check_schedule(pkg, make_hip, "hip", settings)


@pytest.mark.parametrize("name", ["checkerboard", "one tile", "all retired"])
def test_forced_masks(pkg, make_hip, name):
    ta.check_forced(pkg, make_hip, "hip", name)


def test_forced_mask_without_group_flags_per_lane(pkg, make_hip):
    ta.check_forced(pkg, make_hip, "hip", "checkerboard", refill=7, group_flags=0)


def test_forced_mask_packet_form_without_group_flags(pkg, make_hip):
    ta.check_forced(pkg, make_hip, "hip", "checkerboard", group_flags=0)


def test_primary_rays_of_a_half_retired_frame(pkg, make_hip):
    ta.check_primary_count(pkg, make_hip)


@pytest.mark.parametrize("spp", (1, 3, 8, 64))
def test_setting_on_nothing_retired(pkg, make_hip, spp):
    ta.check_nothing_retired(pkg, make_hip, "hip", spp)


def test_state_and_errors(pkg, make_hip):
    ta.check_state(pkg, make_hip)


def test_presented_paths(pkg, make_hip):
    ta.check_presented_paths(pkg, make_hip, "hip")


def test_full_size_checkerboard(pkg, make_hip):
    """1920 x 1080 terrain, 60 x 135 tiles: every other tile retires after the first call; the per-tile property against a
    non-adaptive run of the same process."""
    ta.check_forced(pkg, make_hip, "hip", "checkerboard", scene_name="terrain", w=1920, h=1080, spp=4, before=1, calls=2)


def test_group_on_one_device_equals_the_single_context(pkg, make_hip):
    g = pkg.render_group([0, 0], "peer")
    ta.check_group(pkg, make_hip, g)
    g.destroy()
