"""Host-side mirror of rfw::RenderContext (RFW/system/context/rfw/context/context.h:74-111) over a C ABI.

`CoreBinding` speaks to any shared library that exports the entry points of include/rfwhip.h under a given prefix.
The product instantiates it with librfwhip.so / "rfwhip_" (context.py); the test oracle re-uses it with its own
library and prefix.  Method names, argument meaning and error behaviour follow the reference interface: failures
raise RuntimeError (the reference throws std::runtime_error across the plugin boundary, context.h:84-91).
"""
import ctypes as C

import numpy as np

from . import abi


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _texture_source_array(textures):
    """The rfwhip_texture_source array of a list of texture dicts (CoreBinding.set_textures) and the arrays it points into."""
    arr = (abi.TextureSource * max(1, len(textures)))()
    keep = []
    for i, t in enumerate(textures):
        kind = t.get("kind", "texels")
        flags = int(t.get("flags", 0))
        if kind == "jpeg":
            data = np.frombuffer(bytes(t["data"]), np.uint8)
            arr[i] = abi.TextureSource(abi.TEXSRC_JPEG, flags, data.ctypes.data, data.size, 0, 0, abi.TEX_UINT, 0)
        elif kind == "rgba8":
            data = np.ascontiguousarray(t["data"], dtype=np.uint8)
            h, w = data.shape[:2]
            arr[i] = abi.TextureSource(abi.TEXSRC_RGBA8, flags, data.ctypes.data, data.size, w, h, abi.TEX_UINT, 0)
        elif kind == "texels":
            data = np.ascontiguousarray(t["data"])
            per = 4 if t["type"] == abi.TEX_FLOAT4 else 1
            arr[i] = abi.TextureSource(abi.TEXSRC_TEXELS, 0, data.ctypes.data, data.nbytes, t["width"], t["height"], t["type"], data.size // per)
        else:
            raise ValueError("texture %d: unknown kind %r" % (i, kind))
        keep.append(data)
    return arr, keep


def _texture_source_types(textures):
    return [t["type"] if t.get("kind", "texels") == "texels" else abi.TEX_UINT for t in textures]


class CoreBinding:
    def __init__(self, lib, prefix, device=0, rank=0, world=1, borrowed=None):
        """borrowed: an existing context pointer owned by somebody else (a RenderGroup): used, never destroyed."""
        self._lib = lib
        self._p = prefix
        self._ctx = C.c_void_p()
        self._borrowed = borrowed is not None
        self._declare()
        if borrowed is not None:
            self._ctx = C.c_void_p(borrowed)
        else:
            self._check(self._fn("create")(int(device), int(rank), int(world), C.byref(self._ctx)))
        self.rank, self.world = rank, world
        self.width = self.height = 0

    # ---- plumbing -------------------------------------------------------------------------------------------------
    def _fn(self, name):
        return getattr(self._lib, self._p + name)

    def _has(self, name):
        return hasattr(self._lib, self._p + name)

    def _declare(self):
        vp, sz, u32, i32, fp = C.c_void_p, C.c_size_t, C.c_uint32, C.c_int, C.c_float
        sig = {
            "last_error": (C.c_char_p, []),
            "create": (i32, [i32, i32, i32, C.POINTER(vp)]),
            "cleanup": (i32, [vp]),
            "destroy": (None, [vp]),
            "init": (i32, [vp, u32, u32]),
            "set_sky": (i32, [vp, vp, sz, sz]),
            "set_blue_noise": (i32, [vp, vp, sz]),
            "set_textures": (i32, [vp, vp, sz]),
            "set_materials": (i32, [vp, vp, vp, sz]),
            "set_mesh": (i32, [vp, sz, C.POINTER(abi.Mesh)]),
            "set_instance": (i32, [vp, sz, sz, vp, vp]),
            "set_lights": (i32, [vp, abi.LightCount, vp, vp, vp, vp]),
            "update": (i32, [vp]),
            "camera_get_view": (None, [C.POINTER(abi.CameraPOD), C.POINTER(abi.CameraView)]),
            "render": (i32, [vp, C.POINTER(abi.CameraPOD), i32]),
            "wait": (i32, [vp]),
            "read_framebuffer": (i32, [vp, vp]),
            "local_rows": (u32, [vp]),
            "set_probe_index": (i32, [vp, u32, u32]),
            "get_probe_results": (i32, [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(fp)]),
            "get_stats": (i32, [vp, C.POINTER(abi.RenderStats)]),
            "set_setting": (i32, [vp, C.c_char_p, C.c_char_p]),
            "read_primary_hits": (i32, [vp, vp, vp, vp, vp, vp]),
            "get_bvh": (i32, [vp, sz, vp, sz, vp, sz, C.POINTER(sz), C.POINTER(sz)]),
            "trace_rays": (i32, [vp, sz, vp, vp, fp, fp, vp, vp, vp, vp, vp]),
        }
        for name, (res, args) in sig.items():
            f = self._fn(name)
            f.restype, f.argtypes = res, args
        # device-side presents: only the rendercore (and its emulation build) export these
        for name, (res, args) in {"set_mesh_skin": (i32, [vp, sz, vp, vp, vp, sz]),
                                  "pose_mesh": (i32, [vp, sz, vp, sz]),
                                  "set_mesh_morph": (i32, [vp, sz, vp, vp, vp, sz, sz]),
                                  "morph_mesh": (i32, [vp, sz, vp, sz]),
                                  "set_rig": (i32, [vp, sz, C.POINTER(abi.Rig)]),
                                  "bind_rig": (i32, [vp, sz, sz, sz, sz]),
                                  "animate": (i32, [vp, vp, vp, vp, sz]),
                                  "read_rig": (i32, [vp, sz, i32, sz, vp, sz]),
                                  "read_framebuffer_device": (i32, [vp, vp]),
                                  "read_local_framebuffer_stream": (i32, [vp, vp, vp]),
                                  "deinterleave_stream": (i32, [vp, vp, vp, vp]),
                                  "read_local_framebuffer_device": (i32, [vp, vp]),
                                  "deinterleave_device": (i32, [vp, vp, vp]),
                                  "kat": (i32, [vp, i32, sz, vp, vp]),
                                  "trace_rays_form": (i32, [vp, i32, u32, u32, sz, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp, vp, vp,
                                                            vp, vp, vp]),
                                  "get_bvh4": (i32, [vp, sz, vp, vp, vp, sz, vp, sz, C.POINTER(abi.Bvh4Info)]),
                                  "get_light_tree": (i32, [vp, vp, sz, vp, sz]),
                                  "read_area_lights": (i32, [vp, vp, sz]),
                                  "light_tree_refit": (i32, [vp, vp, sz, vp, sz, vp]),
                                  "read_denoise_guides": (i32, [vp, vp, vp]),
                                  "denoise_image": (i32, [vp, vp, vp]),
                                  "display_image": (i32, [vp, vp, fp, fp, i32, vp]),
                                  "read_display": (i32, [vp, i32, vp]),
                                  "read_display_device": (i32, [vp, i32, vp]),
                                  "display_stream": (i32, [vp, vp, vp, i32, vp]),
                                  "get_meter": (i32, [vp, C.POINTER(abi.MeterStats)]),
                                  "read_meter_histogram": (i32, [vp, vp, C.POINTER(u32)]),
                                  "meter_reset": (i32, [vp]),
                                  "meter_image": (i32, [vp, vp, C.POINTER(abi.MeterStats), vp]),
                                  "meter_histogram": (i32, [vp, vp, u32, C.POINTER(abi.MeterStats)]),
                                  "bloom_image": (i32, [vp, vp, C.c_float, vp]),
                                  "read_bloom_level": (i32, [vp, i32, vp, sz, C.POINTER(u32), C.POINTER(u32)]),
                                  "set_display_lut": (i32, [vp, vp, u32]),
                                  "set_display_lut_cube": (i32, [vp, C.c_char_p, sz]),
                                  "get_display_lut": (i32, [vp, vp, sz, C.POINTER(u32)]),
                                  "grade_colors": (i32, [vp, i32, sz, vp, vp]),
                                  "display_jpeg_bound": (i32, [vp, C.POINTER(sz)]),
                                  "read_display_jpeg": (i32, [vp, vp, sz, C.POINTER(sz)]),
                                  "display_jpeg_stream": (i32, [vp, vp, vp, sz, vp, vp]),
                                  "get_jpeg": (i32, [vp, C.POINTER(abi.JpegStats)]),
                                  "jpeg_image": (i32, [vp, vp, vp, sz, C.POINTER(sz)]),
                                  "read_jpeg_coefficients": (i32, [vp, vp, sz, C.POINTER(u32)]),
                                  "set_texture_sources": (i32, [vp, vp, sz]),
                                  "image_info": (i32, [vp, sz, C.POINTER(abi.ImageInfo)]),
                                  "get_texture_decode": (i32, [vp, sz, C.POINTER(abi.TextureDecodeRecord)]),
                                  "read_texture": (i32, [vp, sz, vp, sz, C.POINTER(sz)]),
                                  "png_unfilter": (i32, [vp, sz, sz, sz, vp]),
                                  "decode_image": (i32, [vp, vp, sz, u32, vp, sz, C.POINTER(u32), C.POINTER(u32)]),
                                  "read_texture_coefficients": (i32, [vp, vp, sz, C.POINTER(u32)]),
                                  "set_sky_hdr": (i32, [vp, vp, sz, u32]),
                                  "hdr_info": (i32, [vp, sz, C.POINTER(abi.HdrInfo)]),
                                  "read_sky": (i32, [vp, vp, sz, C.POINTER(u32), C.POINTER(u32)]),
                                  "read_sky_table": (i32, [vp, vp, sz, C.POINTER(sz), C.POINTER(abi.SkyTableRecord)]),
                                  "sky_alias_from_weights": (i32, [vp, vp, sz, vp, C.POINTER(abi.SkyTableRecord)]),
                                  "get_noise": (i32, [vp, C.POINTER(abi.NoiseStats)]),
                                  "read_noise_map": (i32, [vp, vp]),
                                  "read_noise_tiles": (i32, [vp, vp, sz, C.POINTER(u32), C.POINTER(u32)]),
                                  "read_noise_moments": (i32, [vp, vp, vp]),
                                  "noise_merge": (i32, [vp, sz, u32, vp, vp, u32, vp, vp, vp]),
                                  "noise_image": (i32, [vp, u32, u32, u32, vp, vp, C.POINTER(abi.NoiseStats), vp, vp]),
                                  "get_adaptive": (i32, [vp, C.POINTER(abi.AdaptiveStats)]),
                                  "read_adaptive_tiles": (i32, [vp, vp, vp, sz, C.POINTER(u32), C.POINTER(u32)]),
                                  "adaptive_set_tiles": (i32, [vp, vp, sz]),
                                  "read_denoise_history": (i32, [vp, vp, vp, vp, vp, vp]),
                                  "read_denoise_motion": (i32, [vp, vp, vp, vp]),
                                  "get_counters": (i32, [vp, C.POINTER(abi.Counters), i32]),
                                  "get_kernel_time": (i32, [vp, i32, C.POINTER(fp), C.POINTER(u32), i32]),
                                  "get_setting": (i32, [vp, C.c_char_p, C.c_char_p, sz]),
                                  "get_settings": (i32, [vp, C.POINTER(C.c_char_p), sz]),
                                  "version": (C.c_char_p, [])}.items():
            if self._has(name):
                f = self._fn(name)
                f.restype, f.argtypes = res, args

    def _check(self, code):
        if code != 0:
            msg = self._fn("last_error")()
            raise RuntimeError((msg or b"unknown error").decode(errors="replace"))

    # ---- rfw::RenderContext ------------------------------------------------------------------------------------------
    def get_supported_targets(self):
        return ["BUFFER"]  # RenderTarget::BUFFER, context.h:27-34

    def init(self, width, height):
        self._check(self._fn("init")(self._ctx, int(width), int(height)))
        self.width, self.height = int(width), int(height)

    def cleanup(self):
        if self._ctx:
            self._check(self._fn("cleanup")(self._ctx))

    def destroy(self):
        if self._ctx and not self._borrowed:
            self._fn("destroy")(self._ctx)
        self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    def render_frame(self, camera, status=abi.RESET):
        """render_frame(const Camera&, RenderStatus): synchronous like the reference (glFinish at the end)."""
        self.render_async(camera, status)
        self.wait()

    def render_async(self, camera, status=abi.RESET):
        pod = camera.pod() if hasattr(camera, "pod") else camera
        self._check(self._fn("render")(self._ctx, C.byref(pod), int(status)))

    def wait(self):
        self._check(self._fn("wait")(self._ctx))

    def set_materials(self, materials, tex_ids=None):
        m = np.ascontiguousarray(materials, dtype=abi.MATERIAL_DTYPE)
        if tex_ids is None:
            tex_ids = np.full(len(m), -1, dtype=np.int32).repeat(11).reshape(len(m), 11).view(abi.MATERIAL_TEX_IDS_DTYPE)
        t = np.ascontiguousarray(tex_ids)
        self._check(self._fn("set_materials")(self._ctx, m.ctypes.data, t.ctypes.data, len(m)))

    def set_textures(self, textures):
        """textures: list of dicts {type, width, height, data(np.ndarray)}; data may include appended mip levels.  A dict with a
        "kind" (images.texture_from_file: "jpeg" with the file's bytes, "rgba8" with H x W x 4 pixels in file order; "flags") is an
        image the device decodes and mips: with one in the list the whole list goes through rfwhip_set_texture_sources."""
        if any("kind" in t for t in textures):
            return self._set_texture_sources(textures)
        self._texture_types = [t["type"] for t in textures]  # (read_texture)
        arr = (abi.Texture * max(1, len(textures)))()
        keep = []
        for i, t in enumerate(textures):
            data = np.ascontiguousarray(t["data"])
            keep.append(data)
            per = 4 if t["type"] == abi.TEX_FLOAT4 else 1
            arr[i] = abi.Texture(t["type"], t["width"], t["height"], data.size // per, 0, 0, data.ctypes.data)
        self._check(self._fn("set_textures")(self._ctx, C.cast(arr, C.c_void_p), len(textures)))

    def _set_texture_sources(self, textures):
        arr, keep = _texture_source_array(textures)
        self._check(self._fn("set_texture_sources")(self._ctx, C.cast(arr, C.c_void_p), len(textures)))
        self._texture_types = _texture_source_types(textures)
        del keep

    # ---- image textures (include/rfwhip.h, rfwhip_set_texture_sources; rendering_fw_amd.images) ------------------------------
    def decode_image(self, data, flags=0):
        """Known-answer hook: a JPEG stream decoded on the device -> H x W x 4 uint8 (level 0 alone; needs no scene)."""
        src = np.frombuffer(bytes(data), np.uint8)
        w, h = C.c_uint32(), C.c_uint32()
        self._check(self._fn("decode_image")(self._ctx, src.ctypes.data, src.size, int(flags), None, 0, C.byref(w), C.byref(h)))
        out = np.empty((h.value, w.value, 4), np.uint8)
        self._check(self._fn("decode_image")(self._ctx, src.ctypes.data, src.size, int(flags), out.ctypes.data, w.value * h.value, C.byref(w), C.byref(h)))
        return out

    def read_texture(self, index):
        """All levels of texture `index` of the current table, back to back: uint32 texels (float32 x 4 for a FLOAT4 texture)."""
        n = C.c_size_t()
        self._check(self._fn("read_texture")(self._ctx, int(index), None, 0, C.byref(n)))
        raw = np.empty(n.value * 16, np.uint8)
        self._check(self._fn("read_texture")(self._ctx, int(index), raw.ctypes.data, n.value, C.byref(n)))
        if self._texture_types[int(index)] == abi.TEX_FLOAT4:
            return raw.view(np.float32).reshape(-1, 4)
        return raw[:n.value * 4].view(np.uint32).copy()

    def texture_record(self, index=None):
        """The decode record of texture `index` as a dict (abi.TextureDecodeRecord); None: of the last decode_image."""
        r = abi.TextureDecodeRecord()
        self._check(self._fn("get_texture_decode")(self._ctx, C.c_size_t(-1).value if index is None else int(index), C.byref(r)))
        return r.as_dict()

    def texture_coefficients(self):
        """The coefficients of the last decode: blocks x 64 int16 in zigzag order, in stream order (MCU by MCU)."""
        n = C.c_uint32()
        self._check(self._fn("read_texture_coefficients")(self._ctx, None, 0, C.byref(n)))
        out = np.empty((n.value, 64), np.int16)
        self._check(self._fn("read_texture_coefficients")(self._ctx, out.ctypes.data, n.value, C.byref(n)))
        return out

    def set_mesh(self, index, vertices, triangles, indices=None):
        v = _f32(vertices).reshape(-1, 4)
        tr = np.ascontiguousarray(triangles, dtype=abi.TRIANGLE_DTYPE)
        idx = None if indices is None else np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1, 3)
        m = abi.Mesh(v.ctypes.data, None, None, tr.ctypes.data, None if idx is None else idx.ctypes.data, len(v), len(tr))
        self._check(self._fn("set_mesh")(self._ctx, int(index), C.byref(m)))

    def set_instance(self, i, mesh_idx, transform, normal_matrix=None):
        """transform: 4x4 in maths (row, col) convention; sent column-major like glm::mat4.  normal_matrix defaults to
        the inverse-transpose of the upper 3x3 (system.cpp:347)."""
        t = np.asarray(transform, dtype=np.float64).reshape(4, 4)
        if normal_matrix is None:
            normal_matrix = np.linalg.inv(t[:3, :3]).T
        n = np.asarray(normal_matrix, dtype=np.float64).reshape(3, 3)
        tc, nc = _f32(t.T).ravel(), _f32(n.T).ravel()
        self._check(self._fn("set_instance")(self._ctx, int(i), int(mesh_idx), tc.ctypes.data, nc.ctypes.data))

    def set_sky(self, pixels, width, height):
        p = _f32(pixels).reshape(-1, 3)
        assert len(p) == width * height
        self._check(self._fn("set_sky")(self._ctx, p.ctypes.data, int(width), int(height)))

    # ---- the sky's loaders (include/rfwhip.h, rfwhip_set_sky_hdr; rendering_fw_amd.images.load_hdr) ----------------------------
    def set_sky_hdr(self, data, flip=False):
        """The bytes of a Radiance .hdr file become the sky: the device decodes them.  All or nothing: a refused file raises
        RuntimeError and the previous sky stays."""
        src = np.frombuffer(bytes(data), np.uint8)
        self._check(self._fn("set_sky_hdr")(self._ctx, src.ctypes.data, src.size, abi.SKYSRC_FLIP_ROWS if flip else 0))

    def read_sky(self):
        """The sky's texels: H x W x 4 float32 (r, g, b, 0); a context without a sky: 0 x 0 x 4."""
        w, h = C.c_uint32(), C.c_uint32()
        self._check(self._fn("read_sky")(self._ctx, None, 0, C.byref(w), C.byref(h)))
        out = np.empty((h.value, w.value, 4), np.float32)
        if out.size:
            self._check(self._fn("read_sky")(self._ctx, out.ctypes.data, w.value * h.value, C.byref(w), C.byref(h)))
        return out

    def read_sky_table(self):
        """The alias table of sky_sampling = 1 as (entries of abi.SKY_ALIAS_DTYPE, the record as a dict); no entries without a table."""
        n, rec = C.c_size_t(), abi.SkyTableRecord()
        self._check(self._fn("read_sky_table")(self._ctx, None, 0, C.byref(n), C.byref(rec)))
        out = np.empty(n.value, abi.SKY_ALIAS_DTYPE)
        if n.value:
            self._check(self._fn("read_sky_table")(self._ctx, out.ctypes.data, n.value, C.byref(n), C.byref(rec)))
        return out, rec.as_dict()

    def sky_alias_from_weights(self, weights):
        """Known-answer hook: the device's alias table over the given float64 weights -> (entries, record)."""
        w = np.ascontiguousarray(weights, np.float64).reshape(-1)
        out, rec = np.empty(len(w), abi.SKY_ALIAS_DTYPE), abi.SkyTableRecord()
        self._check(self._fn("sky_alias_from_weights")(self._ctx, w.ctypes.data, len(w), out.ctypes.data, C.byref(rec)))
        return out, rec.as_dict()

    def set_mesh_skin(self, index, joints, weights, base_normals):
        """Device skinning: per-vertex joints (V x 4 uint32), weights (V x 4) and bind-pose normals (V x 3|4) of mesh
        `index`, whose last set_mesh vertices are the bind pose."""
        j = np.ascontiguousarray(joints, dtype=np.uint32).reshape(-1, 4)
        w = _f32(weights).reshape(-1, 4)
        n = _f32(base_normals).reshape(len(j), -1)
        n4 = np.zeros((len(j), 4), np.float32)
        n4[:, :3] = n[:, :3]
        self._keep = (j, w, n4)
        self._check(self._fn("set_mesh_skin")(self._ctx, int(index), j.ctypes.data, w.ctypes.data, n4.ctypes.data, len(j)))

    def pose_mesh(self, index, joint_matrices):
        """joint_matrices: (J, 4, 4) row-major numpy matrices acting on column vectors (object -> posed)."""
        m = _f32(joint_matrices).reshape(-1, 4, 4)
        cm = np.ascontiguousarray(np.transpose(m, (0, 2, 1)))  # column-major storage
        self._check(self._fn("pose_mesh")(self._ctx, int(index), cm.ctypes.data, len(cm)))

    def set_mesh_morph(self, index, base_normals, target_positions, target_normals):
        """Device morph targets of mesh `index` (whose last set_mesh vertices are the base pose): base normals (V x 3|4) and
        per target the position / normal displacements, (T, V, 3|4) each."""
        def f4(a, lead):
            a = _f32(a).reshape(lead + (-1,))
            out = np.zeros(lead + (4,), np.float32)
            out[..., :3] = a[..., :3]
            return out
        tp = _f32(target_positions)
        t, v = tp.shape[0], tp.shape[1]
        bn, tp4, tn4 = f4(base_normals, (v,)), f4(tp, (t, v)), f4(target_normals, (t, v))
        self._check(self._fn("set_mesh_morph")(self._ctx, int(index), bn.ctypes.data, tp4.ctypes.data, tn4.ctypes.data, t, v))

    def morph_mesh(self, index, weights):
        w = _f32(weights).reshape(-1)
        self._check(self._fn("morph_mesh")(self._ctx, int(index), w.ctypes.data, len(w)))

    # ---- animations on the device (include/rfwhip.h, rfwhip_set_rig; rendering_fw_amd.gltf.Gltf.rig packs a file's tables) -------
    def set_rig(self, index, rig):
        """rig: the tables of abi.RIG_TABLES by name (a missing one is empty); inverse_bind holds 16 floats, column-major, per joint."""
        pod, keep = _rig_pod(rig)
        self._check(self._fn("set_rig")(self._ctx, int(index), C.byref(pod)))
        if not hasattr(self, "_rigs"):
            self._rigs = {}
        self._rigs[int(index)] = (len(keep["nodes"]), keep["skins"]["joint_count"].copy(), keep["nodes"]["weight_count"].copy())

    def bind_rig(self, rig, mesh, skin=0, node=0):
        """Mesh `mesh` follows rig `rig`: a skinned mesh takes the joint matrices of `skin`, a morphed one the weights of `node`."""
        self._check(self._fn("bind_rig")(self._ctx, int(rig), int(skin), int(node), int(mesh)))

    def animate(self, rigs, times, animations=0):
        """Evaluate the listed rigs at their times (one launch), pose / morph and refit every mesh bound to them.  animations: one
        index for all or one per rig; None or abi.RIG_BASE_POSE: the base pose.  update() afterwards."""
        r, t, a = _rig_calls(rigs, times, animations)
        self._check(self._fn("animate")(self._ctx, r.ctypes.data, a.ctypes.data, t.ctypes.data, len(r)))

    def read_rig(self, rig, what, index=0):
        """Values of the rig's last evaluation: "trs" (N, 10), "world" (N, 4, 4) and "joints" of skin `index` (J, 4, 4) as row-major
        matrices acting on column vectors (what pose_mesh takes), "weights" of node `index`, "status" a dict."""
        nodes, joint_counts, weight_counts = self._rigs[int(rig)]
        n = {"trs": nodes * 10, "world": nodes * 16, "status": 8}.get(what)
        if what == "joints":
            n = int(joint_counts[index]) * 16
        elif what == "weights":
            n = int(weight_counts[index])
        out = np.zeros(max(n, 1), np.float32)
        self._check(self._fn("read_rig")(self._ctx, int(rig), abi.RIG_READ[what], int(index), out.ctypes.data, n))
        out = out[:n]
        if what == "trs":
            return out.reshape(-1, 10)
        if what in ("world", "joints"):
            return np.ascontiguousarray(out.reshape(-1, 4, 4).transpose(0, 2, 1))
        if what == "status":
            w = out.view(np.uint32)
            return {"time": float(out[0]), "rotation_fallbacks": int(w[1]), "inverse_fallbacks": int(w[2]), "serial": int(w[3]),
                    "animation": int(w[4])}
        return out

    def set_blue_noise(self, table):
        """The reference's 5 x 65536-word blue-noise table (createBlueNoiseBuffer()); see scenes.synthetic_blue_noise."""
        t = np.ascontiguousarray(table, dtype=np.uint32).reshape(-1)
        self._check(self._fn("set_blue_noise")(self._ctx, t.ctypes.data, int(t.size)))

    def set_lights(self, area=None, point=None, spot=None, directional=None):
        def prep(a, dt):
            a = np.zeros(0, dtype=dt) if a is None else np.ascontiguousarray(a, dtype=dt)
            return a, (a.ctypes.data if len(a) else None)

        a, pa = prep(area, abi.AREA_LIGHT_DTYPE)
        p, pp = prep(point, abi.POINT_LIGHT_DTYPE)
        s, ps = prep(spot, abi.SPOT_LIGHT_DTYPE)
        d, pd = prep(directional, abi.DIRECTIONAL_LIGHT_DTYPE)
        self._check(self._fn("set_lights")(self._ctx, abi.LightCount(len(a), len(p), len(s), len(d)), pa, pp, ps, pd))
        self._light_count = len(a) + len(p) + len(s) + len(d)

    def get_probe_results(self):
        inst, prim, dist = C.c_uint32(), C.c_uint32(), C.c_float()
        self._check(self._fn("get_probe_results")(self._ctx, C.byref(inst), C.byref(prim), C.byref(dist)))
        return inst.value, prim.value, dist.value

    def set_probe_index(self, x, y):
        self._check(self._fn("set_probe_index")(self._ctx, int(x), int(y)))

    def set_setting(self, key, value):
        self._check(self._fn("set_setting")(self._ctx, str(key).encode(), str(value).encode()))

    def update(self):
        self._check(self._fn("update")(self._ctx))

    def get_stats(self):
        s = abi.RenderStats()
        self._check(self._fn("get_stats")(self._ctx, C.byref(s)))
        return s

    # ---- headless BUFFER target + test hooks ----------------------------------------------------------------------
    def camera_view(self, camera):
        v = abi.CameraView()
        pod = camera.pod() if hasattr(camera, "pod") else camera
        self._fn("camera_get_view")(C.byref(pod), C.byref(v))
        return v

    def framebuffer(self):
        out = np.empty((self.height, self.width, 4), dtype=np.float32)
        self._check(self._fn("read_framebuffer")(self._ctx, out.ctypes.data))
        return out

    def read_framebuffer_device(self, device_ptr):
        self._check(self._fn("read_framebuffer_device")(self._ctx, C.c_void_p(device_ptr)))

    def read_local_framebuffer_device(self, device_ptr):
        """This rank's strips (local_rows() x width float4) into caller-owned device memory (a torch tensor's
        data_ptr())."""
        self._check(self._fn("read_local_framebuffer_device")(self._ctx, C.c_void_p(device_ptr)))

    def deinterleave_device(self, gathered_ptr, out_ptr):
        """Root side of the multi-GPU gather: [world][local_rows][width] float4 -> [height][width] float4."""
        self._check(self._fn("deinterleave_device")(self._ctx, C.c_void_p(gathered_ptr), C.c_void_p(out_ptr)))

    def read_local_framebuffer_stream(self, device_ptr, stream):
        """Stream-ordered present of this rank's strips on the caller's hipStream_t (an int, e.g.
        torch.cuda.current_stream().cuda_stream); no host synchronisation."""
        self._check(self._fn("read_local_framebuffer_stream")(self._ctx, C.c_void_p(device_ptr), C.c_void_p(stream)))

    def deinterleave_stream(self, gathered_ptr, out_ptr, stream):
        self._check(self._fn("deinterleave_stream")(self._ctx, C.c_void_p(gathered_ptr), C.c_void_p(out_ptr),
                                                    C.c_void_p(stream)))

    def local_rows(self):
        return int(self._fn("local_rows")(self._ctx))

    def primary_hits(self):
        n = self.width * self.height
        t, u, v = (np.empty(n, np.float32) for _ in range(3))
        prim, inst = np.empty(n, np.int32), np.empty(n, np.int32)
        self._check(self._fn("read_primary_hits")(self._ctx, t.ctypes.data, prim.ctypes.data, inst.ctypes.data,
                                                   u.ctypes.data, v.ctypes.data))
        shp = (self.height, self.width)
        return {"t": t.reshape(shp), "prim": prim.reshape(shp), "inst": inst.reshape(shp), "u": u.reshape(shp),
                "v": v.reshape(shp)}

    def trace_rays(self, org, dir, t_min=1e-5, t_max=1e34):
        """Closest hits of arbitrary world-space rays (n x 3 each) against the resident scene."""
        o, d = _f32(org).reshape(-1, 3), _f32(dir).reshape(-1, 3)
        n = len(o)
        t, u, v = (np.empty(n, np.float32) for _ in range(3))
        prim, inst = np.empty(n, np.int32), np.empty(n, np.int32)
        self._check(self._fn("trace_rays")(self._ctx, n, o.ctypes.data, d.ctypes.data, t_min, t_max, t.ctypes.data,
                                            prim.ctypes.data, inst.ctypes.data, u.ctypes.data, v.ctypes.data))
        return {"t": t, "prim": prim, "inst": inst, "u": u, "v": v}

    FORMS = {"lane_closest": 0, "stream_closest": 1, "lane_any": 2, "stream_any": 3, "fused": 4, "packet_any": 5}
    RAY_VOID = 0xFFFFFFFF        # tag of a void queue entry
    HIT_VOID = -2                # prim of a void entry's hit record
    FORM_UNTOUCHED = -777.0      # visibility of a slot no queue entry named
    FORM_SENTINEL_PRIM = 0x5E5E5E5E  # prim of a hit record no kernel wrote

    def trace_rays_form(self, form, org=None, dir=None, tag=None, org_any=None, dir_any=None, t_max_any=None, tag_any=None,
                        bins=0, grid_items=0):
        """The given rays through one form of the traversal, launched by the product's own launchers (include/rfwhip.h,
        rfwhip_trace_rays_form).  form: a key of FORMS.  The closest-hit forms ("lane_closest", "stream_closest", "fused") take
        org / dir (n x 3) and tag (n uint32 slot words below 2^31, RAY_VOID for a void entry; None: the ray index) and return
        t / u / v / prim / inst; the occlusion forms ("lane_any", "stream_any", "fused", "packet_any") take org_any / dir_any /
        t_max_any and tag_any (the slot, unique and below the ray count, RAY_VOID for void; "packet_any": bin << (31 - bins) |
        slot) and return "visible", indexed by SLOT: 1 visible, 0 occluded, FORM_UNTOUCHED for a slot no entry named.
        grid_items: what the launcher sizes its grid by (0: the ray count).  "counters": rays_extend, rays_shadow, sp_runs,
        stack_overflow of this launch.  In the host-emulation build the forms collapse to the same per-item loops: the lane
        and stream forms, "fused" and "packet_any" run identical code there."""
        if form not in self.FORMS:
            code = int(form)  # (an unknown number goes to the library, which refuses it)
        else:
            code = self.FORMS[form]
        e_o = _f32(org if org is not None else np.zeros((0, 3))).reshape(-1, 3)
        e_d = _f32(dir if dir is not None else np.zeros((0, 3))).reshape(-1, 3)
        a_o = _f32(org_any if org_any is not None else np.zeros((0, 3))).reshape(-1, 3)
        a_d = _f32(dir_any if dir_any is not None else np.zeros((0, 3))).reshape(-1, 3)
        n, na = len(e_o), len(a_o)
        if len(e_d) != n or len(a_d) != na:
            raise ValueError("origins and directions differ in number")
        a_t = _f32(np.full(na, 1e34) if t_max_any is None else t_max_any).reshape(-1)
        e_tag = None if tag is None else np.ascontiguousarray(tag, np.uint32).reshape(-1)
        a_tag = None if tag_any is None else np.ascontiguousarray(tag_any, np.uint32).reshape(-1)
        if len(a_t) != na or (e_tag is not None and len(e_tag) != n) or (a_tag is not None and len(a_tag) != na):
            raise ValueError("per-ray arrays differ in length")
        t, u, v = (np.empty(n, np.float32) for _ in range(3))
        prim, inst = np.empty(n, np.int32), np.empty(n, np.int32)
        vis = np.empty(na, np.float32)
        cnt = np.zeros(4, np.uint64)
        ptr = lambda x: None if x is None else x.ctypes.data
        self._check(self._fn("trace_rays_form")(self._ctx, code, int(grid_items), int(bins), n, ptr(e_o), ptr(e_d), ptr(e_tag),
                                                 ptr(t), ptr(prim), ptr(inst), ptr(u), ptr(v), na, ptr(a_o), ptr(a_d), ptr(a_t),
                                                 ptr(a_tag), ptr(vis), ptr(cnt)))
        return {"t": t, "prim": prim, "inst": inst, "u": u, "v": v, "visible": vis,
                "counters": dict(zip(("rays_extend", "rays_shadow", "sp_runs", "stack_overflow"), (int(x) for x in cnt)))}

    def read_denoise_guides(self):
        """The denoiser's guides of the full image for the camera of the last render (include/rfwhip.h, "denoise"):
        {"albedo": H x W x 3, "valid": H x W bool, "normal": H x W x 3, "z": H x W (-1 where invalid)}."""
        shp = (self.height, self.width, 4)
        a, nd = np.empty(shp, np.float32), np.empty(shp, np.float32)
        self._check(self._fn("read_denoise_guides")(self._ctx, a.ctypes.data, nd.ctypes.data))
        return {"albedo": a[..., :3], "valid": a[..., 3] > 0.5, "normal": nd[..., :3], "z": nd[..., 3]}

    def denoise_image(self, rgba):
        """Filter an H x W x 4 float32 image with the current guides and the context's denoise_* settings."""
        src = np.ascontiguousarray(rgba, dtype=np.float32).reshape(self.height, self.width, 4)
        out = np.empty_like(src)
        self._check(self._fn("denoise_image")(self._ctx, src.ctypes.data, out.ctypes.data))
        return out

    # ---- display stage (include/rfwhip.h, rfwhip_read_display) ----------------------------------------------------
    DISPLAY_FORMATS = {"rgba8": 0, "rgba32f": 1}

    @classmethod
    def display_format(cls, format):
        """(code, numpy dtype) of a display format: "rgba8" | "rgba32f", or the C ABI's number (an unknown number goes to
        the library, which refuses it)."""
        code = cls.DISPLAY_FORMATS[format] if format in cls.DISPLAY_FORMATS else int(format)
        return code, (np.uint8 if code == 0 else np.float32)

    def display(self, format="rgba8"):
        """The presented image after the display stage — tone map, FXAA, encoding, with the display_* settings and the
        last render's camera: H x W x 4 uint8 ("rgba8") or float32 ("rgba32f")."""
        code, dt = self.display_format(format)
        out = np.empty((self.height, self.width, 4), dtype=dt)
        self._check(self._fn("read_display")(self._ctx, code, out.ctypes.data))
        return out

    def read_display_device(self, device_ptr, format="rgba8"):
        self._check(self._fn("read_display_device")(self._ctx, self.display_format(format)[0], C.c_void_p(device_ptr)))

    def display_stream(self, rgba_device_ptr, out_device_ptr, format="rgba8", stream=0):
        """Stream-ordered display stage on a full float4 image in device memory (rfwhip_display_stream)."""
        self._check(self._fn("display_stream")(self._ctx, C.c_void_p(rgba_device_ptr or None), C.c_void_p(out_device_ptr or None),
                                               self.display_format(format)[0], C.c_void_p(stream or None)))

    def display_image(self, rgba, brightness=0.05, contrast=1.0, format="rgba8"):
        """The display stage on a given H x W x 4 float32 image with the context's display_* settings."""
        src = np.ascontiguousarray(rgba, dtype=np.float32).reshape(self.height, self.width, 4)
        code, dt = self.display_format(format)
        out = np.empty((self.height, self.width, 4), dtype=dt)
        self._check(self._fn("display_image")(self._ctx, src.ctypes.data, float(brightness), float(contrast), code,
                                              out.ctypes.data))
        return out

    # ---- exposure meter (include/rfwhip.h, rfwhip_get_meter; setting display_exposure = auto) -----------------------
    def meter(self):
        """The exposure meter's record as a dict: exposure (E), log2_exposure, log2_target, log2_luminance, valid, excluded,
        steps."""
        st = abi.MeterStats()
        self._check(self._fn("get_meter")(self._ctx, C.byref(st)))
        return st.as_dict()

    def meter_histogram(self):
        """(bins: 256 uint32, excluded) of the last metered image."""
        bins, ex = np.zeros(abi.METER_BINS, np.uint32), C.c_uint32()
        self._check(self._fn("read_meter_histogram")(self._ctx, bins.ctypes.data, C.byref(ex)))
        return bins, int(ex.value)

    def meter_image(self, rgba):
        """Known-answer hook: one step of the meter on an H x W x 4 float32 image under the current display_exposure*
        settings -> (record dict, bins)."""
        src = np.ascontiguousarray(rgba, dtype=np.float32).reshape(self.height, self.width, 4)
        st, bins = abi.MeterStats(), np.zeros(abi.METER_BINS, np.uint32)
        self._check(self._fn("meter_image")(self._ctx, src.ctypes.data, C.byref(st), bins.ctypes.data))
        return st.as_dict(), bins

    def meter_from_histogram(self, bins, excluded=0):
        """Known-answer hook: the meter's reduce alone on a histogram of 256 counts -> record dict."""
        b = np.ascontiguousarray(bins, dtype=np.uint32).reshape(-1)
        if len(b) != abi.METER_BINS:
            raise ValueError("a meter histogram has %d bins, got %d" % (abi.METER_BINS, len(b)))
        st = abi.MeterStats()
        self._check(self._fn("meter_histogram")(self._ctx, b.ctypes.data, int(excluded), C.byref(st)))
        return st.as_dict()

    def meter_reset(self):
        """E = 1, steps = 0: the next step is a first step."""
        self._check(self._fn("meter_reset")(self._ctx))

    # ---- bloom (include/rfwhip.h, rfwhip_bloom_image; setting display_bloom = 1) -----------------------------------
    def bloom_image(self, rgba, exposure=1.0):
        """Known-answer hook: the bloom chain on an H x W x 4 float32 image under the exposure E = `exposure` and the current
        display_bloom_* settings -> the linear H x W x 4 float32 image the display kernel would read."""
        src = np.ascontiguousarray(rgba, dtype=np.float32).reshape(self.height, self.width, 4)
        out = np.empty_like(src)
        self._check(self._fn("bloom_image")(self._ctx, src.ctypes.data, float(exposure), out.ctypes.data))
        return out

    def read_bloom_level(self, level):
        """U_level of the last bloom chain as an h x w x 4 float32 array (level 1 = half the image's size)."""
        w, h = C.c_uint32(), C.c_uint32()
        self._check(self._fn("read_bloom_level")(self._ctx, int(level), None, 0, C.byref(w), C.byref(h)))
        out = np.empty((h.value, w.value, 4), np.float32)
        self._check(self._fn("read_bloom_level")(self._ctx, int(level), out.ctypes.data, out.size, C.byref(w), C.byref(h)))
        return out

    # ---- colour grading and dither (include/rfwhip.h, rfwhip_set_display_lut; setting display_grade = 1) ------------
    def set_display_lut(self, lut):
        """The display stage's 3D LUT: an n x n x n x 3 array indexed [b][g][r] (red fastest, the order of a .cube file) or any
        array of 3 n^3 floats in that order; None removes it."""
        a, n = _lut_array(lut)
        self._check(self._fn("set_display_lut")(self._ctx, a.ctypes.data if n else None, n))

    def set_display_lut_cube(self, text):
        """The LUT from the text of a .cube file (str or bytes)."""
        raw = _cube_bytes(text)
        self._check(self._fn("set_display_lut_cube")(self._ctx, raw, len(raw)))

    def load_cube(self, path):
        self.set_display_lut_cube(_read_file(path))

    def get_display_lut(self):
        """The LUT as an n x n x n x 3 float32 array indexed [b][g][r], or None."""
        n = C.c_uint32()
        self._check(self._fn("get_display_lut")(self._ctx, None, 0, C.byref(n)))
        if not n.value:
            return None
        out = np.empty((n.value, n.value, n.value, 3), np.float32)
        self._check(self._fn("get_display_lut")(self._ctx, out.ctypes.data, out.size, C.byref(n)))
        return out

    def grade_colors(self, which, rgb):
        """Known-answer hook: colours (... x 3) through k_kat_grade under the current settings — which = 0: white balance, CDL and
        saturation on linear colours; 1: the LUT on display colours."""
        src = np.ascontiguousarray(rgb, dtype=np.float32)
        out = np.empty_like(src)
        self._check(self._fn("grade_colors")(self._ctx, int(which), src.size // 3, src.ctypes.data, out.ctypes.data))
        return out

    # ---- baseline JPEG of the display image (include/rfwhip.h, rfwhip_read_display_jpeg; settings display_jpeg_*) -------------
    def jpeg_bound(self):
        """The capacity in bytes that always suffices for the target size under the current display_jpeg_* settings."""
        n = C.c_size_t()
        self._check(self._fn("display_jpeg_bound")(self._ctx, C.byref(n)))
        return int(n.value)

    def _jpeg_call(self, call, cap):
        """call(buffer address, cap, byref(bytes)) -> the stream as bytes; cap None: the bound."""
        cap = self.jpeg_bound() if cap is None else int(cap)
        buf, n = np.empty(max(cap, 1), np.uint8), C.c_size_t()
        self._check(call(buf.ctypes.data, cap, C.byref(n)))
        return buf[:n.value].tobytes()

    def display_jpeg(self, cap=None):
        """The presented image after the display stage as a baseline JPEG (bytes), encoded on the device: what display()
        returns as RGBA8, compressed under display_jpeg_quality / _subsampling / _restart.  cap: the host buffer's size
        (default: the bound); a stream longer than cap raises and names its length."""
        return self._jpeg_call(lambda p, c, n: self._fn("read_display_jpeg")(self._ctx, p, c, n), cap)

    def save_jpeg(self, path):
        """display_jpeg() into a file; returns the bytes written."""
        data = self.display_jpeg()
        with open(path, "wb") as f:
            f.write(data)
        return len(data)

    def display_jpeg_stream(self, rgba8_device_ptr, out_device_ptr, cap, record_device_ptr, stream=0):
        """Stream-ordered encode of a W x H RGBA8 image in device memory (rfwhip_display_jpeg_stream)."""
        self._check(self._fn("display_jpeg_stream")(self._ctx, C.c_void_p(rgba8_device_ptr or None), C.c_void_p(out_device_ptr or None),
                                                    int(cap), C.c_void_p(record_device_ptr or None), C.c_void_p(stream or None)))

    def jpeg_record(self):
        """The record of the last stream read back, as a dict (abi.JpegStats)."""
        st = abi.JpegStats()
        self._check(self._fn("get_jpeg")(self._ctx, C.byref(st)))
        return st.as_dict()

    def jpeg_image(self, rgba8, cap=None):
        """Known-answer hook: an H x W x 4 uint8 image through the encoder under the current settings -> bytes."""
        src = np.ascontiguousarray(rgba8, dtype=np.uint8).reshape(self.height, self.width, 4)
        return self._jpeg_call(lambda p, c, n: self._fn("jpeg_image")(self._ctx, src.ctypes.data, p, c, n), cap)

    def jpeg_coefficients(self):
        """The quantised blocks of the last encode: blocks x 64 int16 in zigzag order, in stream order (MCU by MCU)."""
        n = C.c_uint32()
        self._check(self._fn("read_jpeg_coefficients")(self._ctx, None, 0, C.byref(n)))
        out = np.empty((n.value, 64), np.int16)
        self._check(self._fn("read_jpeg_coefficients")(self._ctx, out.ctypes.data, n.value, C.byref(n)))
        return out

    # ---- noise estimate (include/rfwhip.h, rfwhip_get_noise; setting noise_estimate = 1) ---------------------------
    def get_noise(self):
        """The noise of the accumulated image as a dict: samples, pixels, converged, mean_error, max_error, threshold.
        Two small kernels and a wait for 32 bytes; raises while noise_estimate is off or fewer than 2 samples are in."""
        st = abi.NoiseStats()
        self._check(self._fn("get_noise")(self._ctx, C.byref(st)))
        return st.as_dict()

    def read_noise_map(self):
        """H x W float32: every pixel's relative standard error of the mean."""
        out = np.empty((self.height, self.width), np.float32)
        self._check(self._fn("read_noise_map")(self._ctx, out.ctypes.data))
        return out

    def read_noise_tiles(self):
        """This rank's tile records (abi.NOISE_TILE_DTYPE), tiles_y x tiles_x."""
        cap = -(-self.width // abi.NOISE_TILE_X) * (int(self._fn("local_rows")(self._ctx)) // abi.NOISE_TILE_Y)
        rec = np.zeros(max(cap, 1), abi.NOISE_TILE_DTYPE)
        tx, ty = C.c_uint32(), C.c_uint32()
        self._check(self._fn("read_noise_tiles")(self._ctx, rec.ctypes.data, cap, C.byref(tx), C.byref(ty)))
        return rec[:tx.value * ty.value].reshape(ty.value, tx.value)

    def read_noise_moments(self):
        """(sumY, M2), H x W float32 each (test hook)."""
        a, b = np.empty((self.height, self.width), np.float32), np.empty((self.height, self.width), np.float32)
        self._check(self._fn("read_noise_moments")(self._ctx, a.ctypes.data, b.ctypes.data))
        return a, b

    def noise_merge(self, n_a, sumY_a, m2_a, samples_rgb):
        """Known-answer hook: one call's update of P pixels on samples_rgb (P x S x 3) -> (sumY, M2)."""
        c = np.ascontiguousarray(samples_rgb, dtype=np.float32)
        a, b = _f32(sumY_a).ravel(), _f32(m2_a).ravel()
        assert c.ndim == 3 and c.shape[2] == 3 and len(a) == len(b) == c.shape[0]
        oa, ob = np.empty_like(a), np.empty_like(b)
        self._check(self._fn("noise_merge")(self._ctx, c.shape[0], int(n_a), a.ctypes.data, b.ctypes.data, c.shape[1], c.ctypes.data,
                                            oa.ctypes.data, ob.ctypes.data))
        return oa, ob

    def noise_image(self, n, sumY, m2):
        """Known-answer hook: the metric on given H x W moments -> (stats dict, error map H x W, tile records)."""
        a, b = _f32(sumY), _f32(m2)
        assert a.ndim == 2 and a.shape == b.shape
        h, w = a.shape
        st, e = abi.NoiseStats(), np.empty((h, w), np.float32)
        tiles = np.zeros((-(-h // abi.NOISE_TILE_Y), -(-w // abi.NOISE_TILE_X)), abi.NOISE_TILE_DTYPE)
        self._check(self._fn("noise_image")(self._ctx, w, h, int(n), a.ctypes.data, b.ctypes.data, C.byref(st), e.ctypes.data,
                                            tiles.ctypes.data))
        return st.as_dict(), e, tiles

    def render_until(self, camera, threshold=None, max_samples=4096, check_every=1):
        """Render until every pixel's noise is at most `threshold` (None: the noise_threshold setting as it stands) or
        max_samples samples per pixel are in: a RESET call, then CONVERGE calls of the `spp` setting's samples each; the
        stats are asked for every check_every calls — a query waits for the device, so a larger check_every lets the calls
        in between overlap and stops up to check_every - 1 calls late.  Returns the last stats (a dict, see get_noise)."""
        self.set_setting("noise_estimate", 1)
        if threshold is not None:
            self.set_setting("noise_threshold", repr(float(threshold)))
        spp, cap, calls = int(self.get_setting("spp")), max(2, int(max_samples)), 0
        while True:
            for _ in range(max(1, int(check_every))):
                if calls * spp < cap:
                    self.render_async(camera, abi.CONVERGE if calls else abi.RESET)
                    calls += 1
            if calls * spp < 2:  # (the estimate needs two samples)
                continue
            st = self.get_noise()
            if st["converged"] == st["pixels"] or calls * spp >= cap:
                break
        self.wait()
        return st

    # ---- adaptive sampling (include/rfwhip.h, rfwhip_get_adaptive; setting adaptive_sampling = 1) ------------------
    def get_adaptive(self):
        """Adaptive sampling so far as a dict: tiles, active_tiles, pixels, active_pixels, samples_taken, samples_uniform."""
        st = abi.AdaptiveStats()
        self._check(self._fn("get_adaptive")(self._ctx, C.byref(st)))
        return st.as_dict()

    def read_adaptive_tiles(self):
        """(n_tile uint32, active bool), tiles_y x tiles_x each: this rank's tiles in the order of read_noise_tiles."""
        cap = -(-self.width // abi.NOISE_TILE_X) * (int(self._fn("local_rows")(self._ctx)) // abi.NOISE_TILE_Y)
        n, a = np.zeros(max(cap, 1), np.uint32), np.zeros(max(cap, 1), np.uint8)
        tx, ty = C.c_uint32(), C.c_uint32()
        self._check(self._fn("read_adaptive_tiles")(self._ctx, n.ctypes.data, a.ctypes.data, cap, C.byref(tx), C.byref(ty)))
        k = tx.value * ty.value
        return n[:k].reshape(ty.value, tx.value), a[:k].reshape(ty.value, tx.value).astype(bool)

    def adaptive_set_tiles(self, active):
        """Known-answer hook: retire the tiles whose flag is false (flags only clear; tiles in the order of read_adaptive_tiles)."""
        a = np.ascontiguousarray(np.asarray(active).ravel() != 0, dtype=np.uint8)
        self._check(self._fn("adaptive_set_tiles")(self._ctx, a.ctypes.data, len(a)))

    def read_denoise_history(self):
        """The temporal stage of the last presented frame (include/rfwhip.h, "denoise_temporal"; world-1 contexts):
        {"pre": H x W x 4 (I~, lum), "var": H x W, "history": H x W x 4 (colour history, lum), "moments": H x W x 2,
        "length": H x W (n; 0 at invalid pixels)} — abi.DENOISE_HISTORY_KEYS."""
        h, w = self.height, self.width
        out = dict(zip(abi.DENOISE_HISTORY_KEYS, (np.empty(s, np.float32) for s in
                                                   ((h, w, 4), (h, w), (h, w, 4), (h, w, 2), (h, w)))))
        self._check(self._fn("read_denoise_history")(self._ctx, *(out[k].ctypes.data for k in abi.DENOISE_HISTORY_KEYS)))
        return out

    def read_denoise_motion(self):
        """The motion part of the temporal stage of the last presented frame (include/rfwhip.h, "denoise_motion"; world-1
        contexts): {"state": H x W int32 (0 invalid, 1 still, 2 moved, 3 restart), "position": H x W x 3 (X_P),
        "normal": H x W x 3 (n'_p)}."""
        h, w = self.height, self.width
        state, pos, nrm = np.empty((h, w), np.int32), np.empty((h, w, 3), np.float32), np.empty((h, w, 3), np.float32)
        self._check(self._fn("read_denoise_motion")(self._ctx, state.ctypes.data, pos.ctypes.data, nrm.ctypes.data))
        return {"state": state, "position": pos, "normal": nrm}

    # ---- measurement hooks -------------------------------------------------------------------------------------------
    KERNELS = ("generate", "extend", "shade", "connect", "finalize", "refit")
    DENOISE = 6  # kernel family of the denoiser (guide pass + filter), outside KERNELS: the render's stages
    DISPLAY = 7  # ... and of the display stage (one launch per displayed image)
    NOISE = 8  # ... and of the noise metric (two launches per get_noise)
    METER_HIST, METER_REDUCE = 9, 10  # ... and of the exposure meter's two kernels (one launch each per step)
    PRIMARY_ORDER = 11  # ... and of the primary wave's ordering pass (one count per rewrite of the camera-ordered node table)
    BLOOM = 12  # ... and of bloom (one count per launch of a chain: 2 x the levels it ran)
    GRADE = 13  # ... and of the graded display kernel (one launch per displayed image with display_grade = 1)
    JPEG = 14  # ... and of the JPEG encoder (four launches per stream)
    TEXDEC = 15  # ... and of the image-texture decoder (one count per launch of a decode or mip chain)
    PRIMARY_ENTRY = 16  # ... and of the primary wave's entry snapshot pass (one count per rewrite of the records)
    SKY_LOAD = 17  # ... and of the sky's loaders (one count per launch of an HDR decode or of the alias table's chain)
    RIG = 18  # ... and of the rig kernel (one launch per animate, however many rigs it lists)

    def get_kernel_time(self, which, reset=False):
        ms, n = C.c_float(), C.c_uint32()
        idx = self.DENOISE if which == "denoise" else self.DISPLAY if which == "display" else self.NOISE if which == "noise" else self.METER_HIST if which == "meter_hist" else self.METER_REDUCE if which == "meter_reduce" else self.PRIMARY_ORDER if which == "primary_order" else self.BLOOM if which == "bloom" else self.GRADE if which == "grade" else self.JPEG if which == "jpeg" else self.TEXDEC if which == "texture_decode" else self.PRIMARY_ENTRY if which == "primary_entry" else self.SKY_LOAD if which == "sky_load" else self.RIG if which == "rig" else self.KERNELS.index(which) if isinstance(which, str) else int(which)
        self._check(self._fn("get_kernel_time")(self._ctx, idx, C.byref(ms), C.byref(n), int(reset)))
        return ms.value, n.value

    def get_setting(self, key):
        buf = C.create_string_buffer(128)
        self._check(self._fn("get_setting")(self._ctx, str(key).encode(), buf, 128))
        return buf.value.decode()

    def get_settings(self):
        keys = (C.c_char_p * 32)()
        n = self._fn("get_settings")(self._ctx, keys, 32)
        return {keys[i].decode(): self.get_setting(keys[i].decode()) for i in range(n)}

    def version(self):
        return self._fn("version")().decode()

    # known-answer hook: RFWHIP_KAT_* (include/rfwhip_abi.h)
    KAT = {"bsdf_eval": 0, "bsdf_pdf": 1, "bsdf_sample": 2, "tangent_space": 3, "pack_normal": 4,
           "random_barycentrics": 5, "point_on_light": 6, "light_pick_prob": 7, "blue_noise": 8, "hash": 9, "half_to_float": 10, "fastdiv": 11, "tex_wrap": 12,
           "sky_sample": 13, "sky_pdf": 14, "tex_fetch": 15, "surface_layers": 16, "lt_sample": 17, "lt_pick_prob": 18, "meter_bin": 19, "surface_maps": 20}

    def kat(self, function, records):
        """One of the path tracer's functions on n records (n x 24 float32, integers as bit patterns) -> n x 8 float32."""
        rec = np.ascontiguousarray(records, dtype=np.float32).reshape(-1, 24)
        out = np.zeros((len(rec), 8), np.float32)
        self._check(self._fn("kat")(self._ctx, int(self.KAT[function]), len(rec), rec.ctypes.data, out.ctypes.data))
        return out

    def get_counters(self, reset=False):
        """Traversal statistics since the last reset (count_traversal=1): rays, popped inner nodes, triangle tests."""
        c = abi.Counters()
        self._check(self._fn("get_counters")(self._ctx, C.byref(c), int(reset)))
        return c.as_dict()

    def get_bvh(self, mesh_index):
        nn, np_ = C.c_size_t(), C.c_size_t()
        self._check(self._fn("get_bvh")(self._ctx, int(mesh_index), None, 0, None, 0, C.byref(nn), C.byref(np_)))
        nodes = np.zeros(nn.value, dtype=abi.BVH_NODE_DTYPE)
        prims = np.zeros(np_.value, dtype=np.uint32)
        self._check(self._fn("get_bvh")(self._ctx, int(mesh_index), nodes.ctypes.data, len(nodes), prims.ctypes.data,
                                        len(prims), C.byref(nn), C.byref(np_)))
        return nodes, prims

    def get_light_tree(self, lights=None):
        """The light tree of light_sampling=tree as the next render would use it: (nodes LIGHT_TREE_NODE_DTYPE, paths
        LIGHT_TREE_PATH_DTYPE — one per light of all four kinds; `lights`: how many the scene has, by default the count of
        this binding's last set_lights).  No nodes: the mode is not tree, or no light has a position."""
        if lights is None:
            lights = getattr(self, "_light_count", 0)
        f = self._fn("get_light_tree")
        n = f(self._ctx, None, 0, None, 0)
        if n < 0:
            self._check(-n)
        nodes = np.zeros(n, abi.LIGHT_TREE_NODE_DTYPE)
        paths = np.zeros(int(lights), abi.LIGHT_TREE_PATH_DTYPE)
        n = f(self._ctx, nodes.ctypes.data, len(nodes), paths.ctypes.data, len(paths))
        if n < 0:
            self._check(-n)
        return nodes, paths

    def read_area_lights(self):
        """The area lights as the next render would read them (AREA_LIGHT_DTYPE): with lights_follow_geometry=1 the bound ones
        are what the last update() derived on the device, every other one holds the bytes of set_lights."""
        f = self._fn("read_area_lights")
        n = f(self._ctx, None, 0)
        if n < 0:
            self._check(-n)
        out = np.zeros(n, abi.AREA_LIGHT_DTYPE)
        n = f(self._ctx, out.ctypes.data if len(out) else None, len(out))
        if n < 0:
            self._check(-n)
        return out

    def light_tree_refit(self, nodes, area, bound=None):
        """Known-answer hook: the refit kernels of lights_follow_geometry on a tree get_light_tree returned (for the same
        light counts) and the given area lights (lights 0 .. len(area) - 1 of the tree); bound: per area light 1 = refit its
        leaf (None: all).  Returns the refitted nodes."""
        nd = np.array(nodes, dtype=abi.LIGHT_TREE_NODE_DTYPE, copy=True)
        a = np.ascontiguousarray(area, dtype=abi.AREA_LIGHT_DTYPE)
        b = None if bound is None else np.ascontiguousarray(bound, dtype=np.uint8).reshape(-1)
        assert b is None or len(b) == len(a)
        self._check(self._fn("light_tree_refit")(self._ctx, nd.ctypes.data, len(nd), a.ctypes.data if len(a) else None, len(a),
                                                 None if b is None else b.ctypes.data))
        return nd

    def get_bvh4(self, mesh_index):
        """The traversed tree of a resident mesh as it sits on the device (entries absolute): {"nodes4c": NODE4C_DTYPE,
        "nodes4f": NODE4F_DTYPE, "src4": n4 x 4 uint32, "tri_verts": tri_count x 3 x 4 float32, plus the fields of
        abi.Bvh4Info (device_built as a bool)}."""
        info = abi.Bvh4Info()
        f = self._fn("get_bvh4")
        self._check(f(self._ctx, int(mesh_index), None, None, None, 0, None, 0, C.byref(info)))
        n4, nt = info.n4_count, info.tri_count
        c4 = np.zeros(n4, abi.NODE4C_DTYPE)
        f4 = np.zeros(n4, abi.NODE4F_DTYPE)
        src = np.zeros((n4, 4), np.uint32)
        tv = np.zeros((nt, 3, 4), np.float32)
        self._check(f(self._ctx, int(mesh_index), c4.ctypes.data, f4.ctypes.data, src.ctypes.data, n4, tv.ctypes.data, nt,
                      C.byref(info)))
        out = {name: getattr(info, name) for name, _ in abi.Bvh4Info._fields_}
        out["device_built"] = bool(info.device_built)
        out.update(nodes4c=c4, nodes4f=f4, src4=src, tri_verts=tv)
        return out


# ---- what CoreBinding and RenderGroup share of the display stage's LUT (rfwhip_set_display_lut / rfwhip_group_set_display_lut) ----
def _lut_array(lut):
    """(the LUT as a contiguous float32 array, n); (None, 0) for None: the call that removes the LUT."""
    if lut is None:
        return None, 0
    a = np.ascontiguousarray(lut, dtype=np.float32)
    n = a.shape[0] if a.ndim == 4 else int(round((a.size / 3.0) ** (1.0 / 3.0)))
    if a.size != 3 * n ** 3:
        raise ValueError("a LUT holds 3 n^3 floats, got %d" % a.size)
    return a, n


def _cube_bytes(text):
    return text.encode() if isinstance(text, str) else bytes(text)


def _read_file(path):
    with open(path, "rb") as f:
        return f.read()


def _rig_pod(rig):
    """abi.Rig over contiguous copies of a rig's tables -> (pod, the arrays it points into)."""
    keep = {name: np.ascontiguousarray(rig.get(name, ()), dtype=dt).reshape(-1) for name, dt in abi.RIG_TABLES}
    if len(keep["inverse_bind"]) != 16 * len(keep["joints"]):
        raise ValueError("inverse_bind holds %d floats for %d joints (16 each)" % (len(keep["inverse_bind"]), len(keep["joints"])))
    pod = abi.Rig()
    for name, _ in abi.RIG_TABLES:
        setattr(pod, name, keep[name].ctypes.data if len(keep[name]) else None)
        if name != "inverse_bind":
            setattr(pod, name[:-1] + "_count", len(keep[name]))
    return pod, keep


def _rig_calls(rigs, times, animations):
    r = np.ascontiguousarray(np.atleast_1d(rigs), dtype=np.uint32)
    t = np.ascontiguousarray(np.broadcast_to(_f32(np.atleast_1d(times)), r.shape))
    a = np.full(r.shape, abi.RIG_BASE_POSE, np.uint32) if animations is None else \
        np.ascontiguousarray(np.broadcast_to(np.atleast_1d(animations), r.shape), dtype=np.uint32)
    return r, t, a


class RenderGroup:
    """n devices driven by ONE host thread through rfwhip_group_* (include/rfwhip.h): context i renders the strips of rank i
    of world n, one gather per presented frame lands the image on the root's device.  Looks like one RenderContext to the
    scene code: every set_* is repeated per context (each device holds the whole scene)."""
    TRANSPORTS = {"auto": 0, "rccl": 1, "peer": 2}

    def __init__(self, lib, prefix, devices, transport="auto"):
        self._lib, self._p = lib, prefix
        vp, u32, i32 = C.c_void_p, C.c_uint32, C.c_int
        for name, res, args in [("group_create", i32, [C.POINTER(i32), i32, i32, C.POINTER(vp)]), ("group_destroy", None, [vp]),
                                ("group_size", i32, [vp]), ("group_transport", i32, [vp]), ("group_context", vp, [vp, i32]),
                                ("group_init", i32, [vp, u32, u32]), ("group_update", i32, [vp]),
                                ("group_set_setting", i32, [vp, C.c_char_p, C.c_char_p]),
                                ("group_render", i32, [vp, C.POINTER(abi.CameraPOD), i32]), ("group_gather", i32, [vp]),
                                ("group_wait", i32, [vp]), ("group_read_framebuffer", i32, [vp, vp]),
                                ("group_framebuffer_device", i32, [vp, C.POINTER(vp), C.POINTER(i32)]),
                                ("group_present_async", i32, [vp, i32]), ("group_present_wait", i32, [vp, i32, C.POINTER(vp)]),
                                ("last_error", C.c_char_p, [])]:
            f = self._fn(name)
            f.restype, f.argtypes = res, args
        for name, res, args in [("group_read_display", i32, [vp, i32, vp]), ("group_present_display_async", i32, [vp, i32, i32]),
                                ("group_present_display_wait", i32, [vp, i32, C.POINTER(vp), C.POINTER(i32)]),
                                ("group_get_noise", i32, [vp, C.POINTER(abi.NoiseStats)]),
                                ("group_get_adaptive", i32, [vp, C.POINTER(abi.AdaptiveStats)]),
                                ("group_get_meter", i32, [vp, C.POINTER(abi.MeterStats)]),
                                ("group_set_display_lut", i32, [vp, vp, u32]),
                                ("group_set_display_lut_cube", i32, [vp, C.c_char_p, C.c_size_t]),
                                ("group_read_display_jpeg", i32, [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
                                ("group_present_jpeg_async", i32, [vp, i32]),
                                ("group_present_jpeg_wait", i32, [vp, i32, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
                                ("group_set_texture_sources", i32, [vp, vp, C.c_size_t]),
                                ("group_set_sky_hdr", i32, [vp, vp, C.c_size_t, u32]),
                                ("group_set_rig", i32, [vp, C.c_size_t, C.POINTER(abi.Rig)]),
                                ("group_bind_rig", i32, [vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t]),
                                ("group_animate", i32, [vp, vp, vp, vp, C.c_size_t])]:
            if hasattr(lib, prefix + name):
                f = self._fn(name)
                f.restype, f.argtypes = res, args
        devs = (i32 * len(devices))(*[int(d) for d in devices])
        self._g = vp()
        self._check(self._fn("group_create")(devs, len(devices), self.TRANSPORTS[transport], C.byref(self._g)))
        n = self._fn("group_size")(self._g)
        self.contexts = [CoreBinding(lib, prefix, rank=i, world=n, borrowed=self._fn("group_context")(self._g, i)) for i in range(n)]
        self.world, self.width, self.height = n, 0, 0
        self.transport = {v: k for k, v in self.TRANSPORTS.items()}[self._fn("group_transport")(self._g)]

    def _fn(self, name):
        return getattr(self._lib, self._p + name)

    def _check(self, code):
        if code != 0:
            raise RuntimeError((self._fn("last_error")() or b"unknown error").decode(errors="replace"))

    # the display stage's LUT belongs to the root's context (include/rfwhip.h, rfwhip_group_set_display_lut)
    def set_display_lut(self, lut):
        a, n = _lut_array(lut)
        self._check(self._fn("group_set_display_lut")(self._g, a.ctypes.data if n else None, n))

    def set_display_lut_cube(self, text):
        raw = _cube_bytes(text)
        self._check(self._fn("group_set_display_lut_cube")(self._g, raw, len(raw)))

    def load_cube(self, path):
        self.set_display_lut_cube(_read_file(path))

    def set_textures(self, textures):
        """CoreBinding.set_textures on every member; a list with image sources goes through rfwhip_group_set_texture_sources: every
        member decodes its own replica."""
        if not any("kind" in t for t in textures):
            for c in self.contexts:
                c.set_textures(textures)
            return
        arr, keep = _texture_source_array(textures)
        self._check(self._fn("group_set_texture_sources")(self._g, C.cast(arr, C.c_void_p), len(textures)))
        for c in self.contexts:
            c._texture_types = _texture_source_types(textures)
        del keep

    def set_sky_hdr(self, data, flip=False):
        """CoreBinding.set_sky_hdr through rfwhip_group_set_sky_hdr: every member decodes its own replica of the sky."""
        src = np.frombuffer(bytes(data), np.uint8)
        self._check(self._fn("group_set_sky_hdr")(self._g, src.ctypes.data, src.size, abi.SKYSRC_FLIP_ROWS if flip else 0))

    # animations (CoreBinding.set_rig / bind_rig / animate through rfwhip_group_*): every member evaluates its own copy
    def set_rig(self, index, rig):
        pod, keep = _rig_pod(rig)
        self._check(self._fn("group_set_rig")(self._g, int(index), C.byref(pod)))
        for c in self.contexts:
            if not hasattr(c, "_rigs"):
                c._rigs = {}
            c._rigs[int(index)] = (len(keep["nodes"]), keep["skins"]["joint_count"].copy(), keep["nodes"]["weight_count"].copy())

    def bind_rig(self, rig, mesh, skin=0, node=0):
        self._check(self._fn("group_bind_rig")(self._g, int(rig), int(skin), int(node), int(mesh)))

    def animate(self, rigs, times, animations=0):
        r, t, a = _rig_calls(rigs, times, animations)
        self._check(self._fn("group_animate")(self._g, r.ctypes.data, a.ctypes.data, t.ctypes.data, len(r)))

    def __getattr__(self, name):
        # scene setters and friends: the same call on every context (set_sky, set_mesh, set_lights, set_blue_noise, ...)
        if name.startswith("set_") or name in ("pose_mesh", "morph_mesh"):
            def every(*a, **k):
                for c in self.contexts:
                    getattr(c, name)(*a, **k)
            return every
        raise AttributeError(name)

    def init(self, width, height):
        self._check(self._fn("group_init")(self._g, int(width), int(height)))
        self.width, self.height = int(width), int(height)
        for c in self.contexts:
            c.width, c.height = self.width, self.height

    def update(self):
        self._check(self._fn("group_update")(self._g))

    def set_setting(self, key, value):
        self._check(self._fn("group_set_setting")(self._g, str(key).encode(), str(value).encode()))

    def render_async(self, camera, status=abi.RESET):
        pod = camera.pod() if hasattr(camera, "pod") else camera
        self._check(self._fn("group_render")(self._g, C.byref(pod), int(status)))

    def gather(self):
        self._check(self._fn("group_gather")(self._g))

    def wait(self):
        self._check(self._fn("group_wait")(self._g))

    def render_frame(self, camera, status=abi.RESET):
        self.render_async(camera, status)
        self.wait()

    def framebuffer(self):
        out = np.empty((self.height, self.width, 4), dtype=np.float32)
        self._check(self._fn("group_read_framebuffer")(self._g, out.ctypes.data))
        return out

    def present_async(self, slot):
        """Enqueue gather + device-to-host copy of the image into pinned host slot 0 / 1 (frames in flight)."""
        self._check(self._fn("group_present_async")(self._g, int(slot)))

    def present_wait(self, slot):
        """Block until slot's copy has landed; returns the image as a numpy view of the pinned buffer."""
        ptr = C.c_void_p()
        self._check(self._fn("group_present_wait")(self._g, int(slot), C.byref(ptr)))
        buf = (C.c_float * (self.width * self.height * 4)).from_address(ptr.value)
        return np.frombuffer(buf, dtype=np.float32).reshape(self.height, self.width, 4)

    def display(self, format="rgba8"):
        """gather + the display stage on the root + wait: H x W x 4 uint8 ("rgba8") or float32 ("rgba32f")."""
        code, dt = CoreBinding.display_format(format)
        out = np.empty((self.height, self.width, 4), dtype=dt)
        self._check(self._fn("group_read_display")(self._g, code, out.ctypes.data))
        return out

    def get_noise(self):
        """The noise of the whole image: every rank reduces its strips, the root adds the records (CoreBinding.get_noise)."""
        st = abi.NoiseStats()
        self._check(self._fn("group_get_noise")(self._g, C.byref(st)))
        return st.as_dict()

    def get_adaptive(self):
        """Adaptive sampling of the whole image: the ranks' records added up (CoreBinding.get_adaptive)."""
        st = abi.AdaptiveStats()
        self._check(self._fn("group_get_adaptive")(self._g, C.byref(st)))
        return st.as_dict()

    def meter(self):
        """The exposure meter of the group: the root's record (CoreBinding.meter)."""
        st = abi.MeterStats()
        self._check(self._fn("group_get_meter")(self._g, C.byref(st)))
        return st.as_dict()

    def present_display_async(self, slot, format="rgba8"):
        """present_async with the display stage behind the gather: the copy carries the display image."""
        self._check(self._fn("group_present_display_async")(self._g, int(slot), CoreBinding.display_format(format)[0]))

    def present_display_wait(self, slot):
        """Block until slot's display image has landed; a numpy view of the pinned buffer (uint8 or float32 by its format)."""
        ptr, fmt = C.c_void_p(), C.c_int()
        self._check(self._fn("group_present_display_wait")(self._g, int(slot), C.byref(ptr), C.byref(fmt)))
        n = self.width * self.height * 4
        if fmt.value == 0:
            return np.frombuffer((C.c_uint8 * n).from_address(ptr.value), dtype=np.uint8).reshape(self.height, self.width, 4)
        return np.frombuffer((C.c_float * n).from_address(ptr.value), dtype=np.float32).reshape(self.height, self.width, 4)

    def jpeg_bound(self):
        return self.contexts[0].jpeg_bound()

    def display_jpeg(self, cap=None):
        """gather + the display stage + the JPEG encoder on the root + wait: the stream as bytes (CoreBinding.display_jpeg)."""
        return self.contexts[0]._jpeg_call(lambda p, c, n: self._check_code(self._fn("group_read_display_jpeg")(self._g, p, c, n)), cap)

    def save_jpeg(self, path):
        data = self.display_jpeg()
        with open(path, "wb") as f:
            f.write(data)
        return len(data)

    def _check_code(self, code):
        self._check(code)
        return 0

    def present_jpeg_async(self, slot):
        """present_async with the display stage and the JPEG encoder behind the gather: only the record travels until the wait."""
        self._check(self._fn("group_present_jpeg_async")(self._g, int(slot)))

    def present_jpeg_wait(self, slot, cap=None):
        """Block until slot's stream is encoded; copies exactly its bytes -> bytes."""
        return self.contexts[0]._jpeg_call(lambda p, c, n: self._check_code(self._fn("group_present_jpeg_wait")(self._g, int(slot), p, c, n)), cap)

    def framebuffer_device(self):
        """(device pointer, device ordinal) of the root-side image of the last completed gather."""
        ptr, dev = C.c_void_p(), C.c_int()
        self._check(self._fn("group_framebuffer_device")(self._g, C.byref(ptr), C.byref(dev)))
        return ptr.value, dev.value

    def get_stats(self):
        return [c.get_stats() for c in self.contexts]

    def read_denoise_guides(self):
        """The denoiser's guides: the root's (rank 0 computes them for the whole image)."""
        return self.contexts[0].read_denoise_guides()

    def destroy(self):
        if self._g:
            for c in self.contexts:
                c.destroy()  # (borrowed: forgets the pointer)
            self._fn("group_destroy")(self._g)
            self._g = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass
