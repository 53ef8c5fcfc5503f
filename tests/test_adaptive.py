"""Adaptive sampling (include/rfwhip.h, rfwhip_get_adaptive; csrc/adaptive.h), CPU tier: the host-emulation build runs the work items
of the masked primary wave, k_resolve_adaptive, k_present_adaptive, k_noise_tiles_adaptive and k_adaptive_step in plain loops, on
emulated streams that replay out of order.

The oracle is the product with the setting off, bit for bit: a pixel's samples depend on pixel and sample index only and a retired
tile stops accumulating, so the adaptive image on a tile that retired after call r is the reference's framebuffer after call r.
The reference R (noise_estimate = 1, adaptive off) is rendered once per (library, scene, size, spp, calls) and shared; each
tile's retirement call is predicted from R's own tile records (max_e <= threshold is `converged == pixels`) before the adaptive
context is looked at.  tests/test_adaptive_gpu.py runs the same checks on the HIP kernels, against an R of their own kind."""
import ctypes

import numpy as np
import pytest

TX, TY = 32, 8  # the noise tile
_REF = {}


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def upload(pkg, c, scene_name, w, h, spp, **settings):
    scene = getattr(pkg.scenes, scene_name)(w, h) if scene_name != "terrain" else pkg.scenes.terrain(width=w, height_px=h)
    c.init(w, h)
    scene.upload(c)
    for k, v in dict(dict(integrator="pt", spp=spp, noise_estimate=1), **settings).items():
        c.set_setting(k, v)
    return scene


def reference(pkg, make, kind, scene_name, w, h, spp, calls, **settings):
    """R: framebuffer, moments and the tiles' max_e / pixels after every call (index k - 1 holds call k)."""
    key = (kind, scene_name, w, h, spp, calls, tuple(sorted(settings.items())))
    if key not in _REF:
        c = make()
        scene = upload(pkg, c, scene_name, w, h, spp, **settings)
        F, M, E, px = [], [], [], None
        for k in range(calls):
            c.render_frame(scene.camera, pkg.CONVERGE if k else pkg.RESET)
            F.append(c.framebuffer())
            M.append(c.read_noise_moments())
            if (k + 1) * spp >= 2:
                t = c.read_noise_tiles()
                E.append(t["max_e"].copy())
                px = t["pixels"].copy()
            else:
                E.append(None)
        E = [np.full(px.shape, np.inf, np.float32) if e is None else e for e in E]
        st = c.get_noise()
        c.destroy()
        for a in F + E + [px] + [m for pair in M for m in pair]:
            a.setflags(write=False)
        _REF[key] = {"F": F, "M": M, "E": E, "pixels": px, "noise": st}
    return _REF[key]


def threshold_of(ref, call):
    """The median of R's tile max_e after `call`, over the tiles that have pixels: a float32."""
    e = ref["E"][call - 1][ref["pixels"] > 0]
    return np.float32(np.median(e))


def predict(ref, thr, spp, every, min_samples, calls, forced=None):
    """Per tile the call after which it retires (0: never).  forced = (call, flags): the tiles whose flag is false retire after `call`."""
    r = np.zeros(ref["pixels"].shape, np.int64)
    for k in range(1, calls + 1):
        if k % every == 0 and k * spp >= min_samples:
            r[(r == 0) & (ref["E"][k - 1] <= thr)] = k
        if forced is not None and forced[0] == k:
            r[(r == 0) & ~forced[1]] = k
    return r


def per_pixel(tiles, h, w):
    return np.repeat(np.repeat(tiles, TY, 0), TX, 1)[:h, :w]


def compose(ref, r, calls, h, w):
    """What the adaptive context must hold: framebuffer, (sumY, M2), n_tile / spp."""
    k = per_pixel(np.where(r == 0, calls, r), h, w) - 1
    yy, xx = np.mgrid[:h, :w]
    F = np.stack(ref["F"])[k, yy, xx]
    s = np.stack([m[0] for m in ref["M"]])[k, yy, xx]
    m2 = np.stack([m[1] for m in ref["M"]])[k, yy, xx]
    return F, s, m2


def judge(c, ref, r, spp, calls, h, w, label=""):
    F, s, m2 = compose(ref, r, calls, h, w)
    n, active = c.read_adaptive_tiles()
    got, (gs, gm) = c.framebuffer(), c.read_noise_moments()
    print("%s retired tiles %d of %d, calls %s" % (label, int((r > 0).sum()), r.size, sorted(set(r[r > 0].tolist()))))
    assert np.array_equal(n, np.where(r == 0, calls, r) * spp), label
    assert np.array_equal(active, r == 0), label
    assert np.array_equal(u32(got), u32(F)), label
    assert np.array_equal(u32(gs), u32(s)) and np.array_equal(u32(gm), u32(m2)), label
    px = ref["pixels"].astype(np.int64)
    st = c.get_adaptive()
    assert st == {"tiles": int((px > 0).sum()), "active_tiles": int(((r == 0) & (px > 0)).sum()), "pixels": int(px.sum()),
                  "active_pixels": int(px[r == 0].sum()), "samples_taken": int((px * n.astype(np.int64)).sum()),
                  "samples_uniform": int(px.sum()) * calls * spp}, label
    assert st["pixels"] == h * w


def run_adaptive(pkg, c, scene, calls, pipelined=False):
    for k in range(calls):
        (c.render_async if pipelined else c.render_frame)(scene.camera, pkg.CONVERGE if k else pkg.RESET)
    c.wait()


def adaptive_on(c, thr, every, min_samples):
    for k, v in (("noise_threshold", repr(float(thr))), ("adaptive_sampling", 1), ("adaptive_every", every), ("adaptive_min_samples", min_samples)):
        c.set_setting(k, v)


# ---- the oracle -------------------------------------------------------------------------------------------------------------------
S, K = 4, 12
# (scene, width, height, adaptive_every, adaptive_min_samples, look, monotone).  look: the threshold is the median of R's tile max_e
# after that call.  monotone: the PREDICTION has a tile that retires and is above the threshold again at a later DECISION call —
# what shows that retired tiles stay retired; asserted from R alone, and asserted absent where the flag is False, so that the table
# says what each case exercises.  With adaptive_every = 3 the decisions fall on calls 3, 6, 9, 12, and at the threshold of call 6 no
# tile of either scene that retired at one of them is above it at a later one (R's records say so; the tiles that cross back do it
# between two decisions): those two rows check the decision rule and the counts,
# and the two Cornell rows with the threshold of call 5 are there for monotone retirement at adaptive_every = 3.
ORACLE_CASES = [("cornell", 96, 64, 1, 2, 6, True), ("cornell", 96, 64, 1, 16, 6, True), ("cards", 96, 64, 1, 2, 6, True),
                ("cornell", 96, 64, 3, 2, 6, False), ("cards", 96, 64, 3, 16, 6, False),
                ("cornell", 96, 64, 3, 2, 5, True), ("cornell", 96, 64, 3, 16, 5, True),
                ("cards", 100, 60, 1, 2, 6, True)]  # (partial tiles at the right edge, the padded last strip)


def check_oracle(pkg, make, kind, scene_name, w, h, every, min_samples, look=6, monotone=True, pipelined=False, **settings):
    ref = reference(pkg, make, kind, scene_name, w, h, S, K)
    thr = threshold_of(ref, look)
    real = ref["pixels"] > 0
    below = np.stack([e <= thr for e in ref["E"]])[:, real]
    first = np.where(below.any(0), below.argmax(0) + 1, 0)
    r = predict(ref, thr, S, every, min_samples, K)
    # from R alone, before the adaptive context exists: the case retires tiles at three calls or more, keeps some, and (monotone) has
    # a tile that retired and whose record is above the threshold at a later decision call
    back = np.zeros(r.shape, bool)
    for k in range(1, K + 1):
        if k % every == 0:
            back |= (r > 0) & (r < k) & (ref["E"][k - 1] > thr)
    back &= real
    print("%s %dx%d threshold %.4g (call %d): first call below it %s, never %d; predicted: retired and above it at a later decision %d" %
          (scene_name, w, h, thr, look, sorted(set(first[first > 0].tolist())), int((first == 0).sum()), int(back.sum())))
    rr = r[real]
    assert len(set(rr[rr > 0].tolist())) >= 3 and (rr == 0).any()
    assert back.any() == monotone
    c = make()
    scene = upload(pkg, c, scene_name, w, h, S, **settings)
    adaptive_on(c, thr, every, min_samples)
    run_adaptive(pkg, c, scene, K, pipelined)
    judge(c, ref, r, S, K, h, w, "%s every %d min %d %s:" % (scene_name, every, min_samples, settings))
    return c, scene, ref, r


# ---- kernel forms: the per-lane primary kernel, the packet form, odd groups, one pixel per wave, the scan without group flags ------
FORMS = [(1, 6, {"sample_group": 1}), (4, 6, {}), (4, 6, {"refill": 7}), (4, 6, {"group_flags": 0}), (64, 3, {}), (3, 6, {})]


def check_form(pkg, make, kind, spp, calls, settings):
    ref = reference(pkg, make, kind, "cornell", 96, 64, spp, calls)
    look = max(2, -(-2 // spp))  # the first call with two samples or the second call
    thr = threshold_of(ref, look)
    r = predict(ref, thr, spp, 1, 2, calls)
    assert (r == 0).any() and (r > 0).any() and (r[r > 0] < calls).any()  # (some tiles sit calls out, some never do)
    c = make()
    scene = upload(pkg, c, "cornell", 96, 64, spp, **settings)
    adaptive_on(c, thr, 1, 2)
    run_adaptive(pkg, c, scene, calls)
    judge(c, ref, r, spp, calls, 64, 96, "spp %d %s:" % (spp, settings))


# ---- scheduling independence ---------------------------------------------------------------------------------------------------------
SCHEDULES = [{"ring": 1}, {"ring": 3}, {"streams": 1}, {"streams": 4, "sub_batch_paths": 1}, {"streams": 3, "sub_batch_paths": 1, "overlap": 1},
             {"overlap": 0}, {"overlap": 1, "ring": 3}, {"fuse": 0}, {"fuse": 0, "ring": 3}]


def check_schedule(pkg, make, kind, settings):
    check_oracle(pkg, make, kind, "cornell", 96, 64, 1, 2, 6, True, pipelined=True, **settings)[0].destroy()


# ---- forced masks ----------------------------------------------------------------------------------------------------------------------
def patterns(shape):
    yy, xx = np.mgrid[:shape[0], :shape[1]]
    one = np.ones(shape, bool)
    one[shape[0] // 2, shape[1] // 2] = False
    return {"checkerboard": (yy + xx) % 2 == 0, "one tile": one, "all retired": np.zeros(shape, bool)}


def check_forced(pkg, make, kind, name, scene_name="cornell", w=96, h=64, spp=4, before=3, calls=6, **settings):
    ref = reference(pkg, make, kind, scene_name, w, h, spp, calls, **settings)
    flags = patterns(ref["pixels"].shape)[name]
    c = make()
    scene = upload(pkg, c, scene_name, w, h, spp, count_traversal=1, **settings)
    adaptive_on(c, 1e-12, 1, 2)  # (nothing retires by itself)
    run_adaptive(pkg, c, scene, before)
    c.adaptive_set_tiles(flags)
    c.get_counters(reset=True)
    for _ in range(calls - before):
        c.render_frame(scene.camera, pkg.CONVERGE)
    r = predict(ref, np.float32(1e-12), spp, 1, 2, calls, forced=(before, flags))
    judge(c, ref, r, spp, calls, h, w, name + ":")
    cnt = c.get_counters()
    hits = c.primary_hits()
    retired = per_pixel(r > 0, h, w)
    assert (hits["prim"][retired] == -2).all() and (hits["prim"][~retired] >= -1).all()
    if name == "all retired":
        print("counters of the calls with every tile retired:", cnt)
        # (every traversal and shade counter; "samples" counts the calls' nominal samples, and the HIP build's extend_ticks /
        # extend_launches_timed are the clock of the launches, which still run)
        assert all(cnt[k] == 0 for k in ("rays_extend", "rays_shadow", "inner_extend", "tris_extend", "inner_shadow", "tris_shadow",
                                         "shaded", "lds_extend", "lds_shadow")), cnt
        # flags only clear: nothing comes back
        c.adaptive_set_tiles(np.ones(flags.shape, bool))
        assert not c.read_adaptive_tiles()[1].any()
    c.destroy()


def check_primary_count(pkg, make):
    """max_depth = 0: the primary rays of a half-retired frame are the active real pixels x spp."""
    c = make()
    scene = upload(pkg, c, "cornell", 100, 60, 4, count_traversal=1, max_depth=0)
    adaptive_on(c, 1e-12, 1, 2)
    c.render_frame(scene.camera, pkg.RESET)
    n, _ = c.read_adaptive_tiles()
    c.adaptive_set_tiles(patterns(n.shape)["checkerboard"])
    c.get_counters(reset=True)
    c.render_frame(scene.camera, pkg.CONVERGE)
    st, cnt = c.get_adaptive(), c.get_counters()
    assert 0 < st["active_pixels"] < st["pixels"] and cnt["rays_extend"] == st["active_pixels"] * 4, (st, cnt)
    c.destroy()


# ---- setting on, nothing retired ---------------------------------------------------------------------------------------------------------
def check_nothing_retired(pkg, make, kind, spp):
    ref = reference(pkg, make, kind, "cornell", 96, 64, spp, 4)
    c = make()
    scene = upload(pkg, c, "cornell", 96, 64, spp)
    adaptive_on(c, 1e-12, 1, 2)
    for k in range(4):
        c.render_frame(scene.camera, pkg.CONVERGE if k else pkg.RESET)
        assert np.array_equal(u32(c.framebuffer()), u32(ref["F"][k]))
        s, m2 = c.read_noise_moments()
        assert np.array_equal(u32(s), u32(ref["M"][k][0])) and np.array_equal(u32(m2), u32(ref["M"][k][1]))
    c.set_setting("noise_threshold", repr(float(ref["noise"]["threshold"])))
    assert c.get_noise() == ref["noise"]
    assert c.read_adaptive_tiles()[1].all()
    c.destroy()


# ---- state and errors ------------------------------------------------------------------------------------------------------------------
def check_state(pkg, make):
    c = make()
    scene = upload(pkg, c, "cornell", 96, 64, 2, noise_estimate=0)
    with pytest.raises(RuntimeError, match="needs noise_estimate=1"):
        c.set_setting("adaptive_sampling", 1)
    c.set_setting("noise_estimate", 1)
    c.render_frame(scene.camera, pkg.RESET)
    for call in (c.get_adaptive, c.read_adaptive_tiles, lambda: c.adaptive_set_tiles(np.ones(24))):
        with pytest.raises(RuntimeError, match="adaptive_sampling is off"):
            call()
    c.set_setting("adaptive_sampling", 1)
    with pytest.raises(RuntimeError, match="adaptive_sampling is on"):
        c.set_setting("noise_estimate", 0)
    c.render_frame(scene.camera, pkg.CONVERGE)  # (the setting begins with the next RESET)
    with pytest.raises(RuntimeError, match="RESET first"):
        c.get_adaptive()
    c.set_setting("integrator", "parity")
    with pytest.raises(RuntimeError, match="needs integrator=pt"):
        c.render_frame(scene.camera, pkg.RESET)
    c.set_setting("integrator", "pt")
    for key, bad in (("adaptive_sampling", "2"), ("adaptive_min_samples", "1"), ("adaptive_every", "0"), ("adaptive_every", "65")):
        with pytest.raises(RuntimeError):
            c.set_setting(key, bad)
    assert [c.get_setting(k) for k in ("adaptive_sampling", "adaptive_min_samples", "adaptive_every")] == ["1", "16", "4"]
    assert not any(k.startswith("adaptive") for k in c.get_settings())
    # generous threshold: everything retires at the first decision; RESET re-activates everything
    adaptive_on(c, 1e3, 1, 2)
    c.render_frame(scene.camera, pkg.RESET)
    first = c.framebuffer()
    assert c.get_adaptive()["active_tiles"] == 0
    c.render_frame(scene.camera, pkg.CONVERGE)
    assert np.array_equal(u32(c.framebuffer()), u32(first)) and (c.read_adaptive_tiles()[0] == 2).all()
    c.render_frame(scene.camera, pkg.RESET)
    c.wait()
    n, a = c.read_adaptive_tiles()
    assert np.array_equal(u32(c.framebuffer()), u32(first)) and (n == 2).all() and not a.any()
    with pytest.raises(RuntimeError, match="24 tiles"):
        c.adaptive_set_tiles(np.ones(23))
    with pytest.raises(RuntimeError, match="adaptive one"):
        c.set_setting("adaptive_sampling", 0) or c.set_setting("noise_estimate", 0)
    # off: with the next RESET the image is the plain one again — no stale mask, no per-tile scale
    plain = make()
    upload(pkg, plain, "cornell", 96, 64, 2)
    for ctx in (c, plain):
        ctx.render_frame(scene.camera, pkg.RESET)
        ctx.render_frame(scene.camera, pkg.CONVERGE)
    assert np.array_equal(u32(c.framebuffer()), u32(plain.framebuffer()))
    with pytest.raises(RuntimeError, match="adaptive_sampling is off"):
        c.get_adaptive()
    # ... and on again
    c.set_setting("adaptive_sampling", 1)
    c.set_setting("noise_threshold", "1e-12")
    c.render_frame(scene.camera, pkg.RESET)
    c.render_frame(scene.camera, pkg.CONVERGE)
    assert np.array_equal(u32(c.framebuffer()), u32(plain.framebuffer())) and c.get_adaptive()["active_tiles"] == 24
    # null pointers and a capacity too small, through the C ABI
    INVALID = 1
    buf, u = (ctypes.c_uint32 * 64)(), ctypes.c_uint32()
    assert c._fn("get_adaptive")(c._ctx, None) == INVALID
    assert c._fn("read_adaptive_tiles")(c._ctx, buf, buf, ctypes.c_size_t(23), ctypes.byref(u), ctypes.byref(u)) == INVALID
    assert c._fn("read_adaptive_tiles")(c._ctx, None, buf, ctypes.c_size_t(24), ctypes.byref(u), ctypes.byref(u)) == INVALID
    assert c._fn("adaptive_set_tiles")(c._ctx, None, ctypes.c_size_t(24)) == INVALID
    c.destroy(), plain.destroy()


# ---- the other presented-image paths -----------------------------------------------------------------------------------------------------
def check_presented_paths(pkg, make, kind):
    c, scene, ref, r = check_oracle(pkg, make, kind, "cornell", 96, 64, 1, 2)
    raw = compose(ref, r, K, 64, 96)[0]
    assert np.array_equal(c.display("rgba32f"), c.display_image(raw, scene.camera.brightness, scene.camera.contrast, "rgba32f"))
    c.set_setting("denoise", 1)
    assert np.array_equal(u32(c.framebuffer()), u32(c.denoise_image(raw)))
    c.set_setting("denoise", 0)
    # render_until needs no change: the tiles that retire keep e <= threshold, and their samples stop
    c.set_setting("adaptive_every", 1)
    c.set_setting("spp", 2)
    st = c.render_until(scene.camera, threshold=0.9, max_samples=32)
    ad, (n, active) = c.get_adaptive(), c.read_adaptive_tiles()
    print("render_until:", st, ad)
    assert ad["samples_uniform"] == st["samples"] * 96 * 64 and 0 < ad["samples_taken"] < ad["samples_uniform"]
    assert (c.read_noise_map()[per_pixel(~active, 64, 96)] <= np.float32(0.9)).all()
    assert st["converged"] >= ad["pixels"] - ad["active_pixels"]
    c.destroy()


# ---- groups --------------------------------------------------------------------------------------------------------------------------------
def check_group(pkg, make, group):
    """`group`: a RenderGroup of n ranks.  Its image and its stats are the world-1 adaptive context's."""
    one = make()
    scene = upload(pkg, one, "cornell", 70, 51, 3)
    adaptive_on(one, 0.75, 2, 2)
    run_adaptive(pkg, one, scene, 6)
    want = one.get_adaptive()
    assert 0 < want["active_tiles"] < want["tiles"], want
    group.init(70, 51)
    scene.upload(group)
    for k, v in dict(integrator="pt", spp=3, noise_estimate=1, noise_threshold=0.75, adaptive_sampling=1, adaptive_every=2, adaptive_min_samples=2).items():
        group.set_setting(k, v)
    run_adaptive(pkg, group, scene, 6)
    assert np.array_equal(u32(group.framebuffer()), u32(one.framebuffer()))
    assert group.get_adaptive() == want
    one.destroy()


# ---- CPU tier ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene_name,w,h,every,min_samples,look,monotone", ORACLE_CASES)
def test_oracle(pkg, make_emu, scene_name, w, h, every, min_samples, look, monotone):
    check_oracle(pkg, make_emu, "emu", scene_name, w, h, every, min_samples, look, monotone)[0].destroy()


@pytest.mark.parametrize("spp,calls,settings", FORMS, ids=lambda v: str(v).replace(" ", ""))
def test_kernel_forms(pkg, make_emu, spp, calls, settings):
    check_form(pkg, make_emu, "emu", spp, calls, settings)


@pytest.mark.parametrize("settings", SCHEDULES, ids=lambda v: str(v).replace(" ", ""))
def test_scheduling_changes_no_bit(pkg, make_emu, settings):
    check_schedule(pkg, make_emu, "emu", settings)


@pytest.mark.parametrize("name", ["checkerboard", "one tile", "all retired"])
def test_forced_masks(pkg, make_emu, name):
    check_forced(pkg, make_emu, "emu", name)


def test_forced_mask_without_group_flags_per_lane(pkg, make_emu):
    check_forced(pkg, make_emu, "emu", "checkerboard", refill=7, group_flags=0)


def test_primary_rays_of_a_half_retired_frame(pkg, make_emu):
    check_primary_count(pkg, make_emu)


@pytest.mark.parametrize("spp", (1, 3, 8, 64))
def test_setting_on_nothing_retired(pkg, make_emu, spp):
    check_nothing_retired(pkg, make_emu, "emu", spp)


def test_state_and_errors(pkg, make_emu):
    check_state(pkg, make_emu)


def test_presented_paths(pkg, make_emu):
    check_presented_paths(pkg, make_emu, "emu")


@pytest.mark.parametrize("n", [2, 3])
def test_group_equals_the_single_context(pkg, make_emu, emu_lib, n):
    g = pkg._binding.RenderGroup(emu_lib, "rfwhip_", [0] * n, "peer")
    check_group(pkg, make_emu, g)
    g.destroy()
