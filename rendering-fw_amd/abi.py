"""ctypes / numpy mirrors of include/rfwhip_abi.h (byte layouts of the reference's plugin-boundary PODs).

Reference layouts: RFW/system/context/rfw/context/structs.h:24-255, device_structs.h:95-103, context.h:50-72,
camera.h:27-37, RFW/system/bvh/include/bvh/bvh_node.h:23-28.  Sizes are asserted at import time.
"""
import ctypes as C

import numpy as np

# ---- numpy dtypes (bulk data) -----------------------------------------------------------------------------------
TRIANGLE_DTYPE = np.dtype(
    [
        ("u", "<f4", 3), ("lightTriIdx", "<i4"),
        ("v", "<f4", 3), ("material", "<u4"),
        ("vN0", "<f4", 3), ("Nx", "<f4"),
        ("vN1", "<f4", 3), ("Ny", "<f4"),
        ("vN2", "<f4", 3), ("Nz", "<f4"),
        ("T", "<f4", 3), ("area", "<f4"),
        ("B", "<f4", 3), ("LOD", "<f4"),
        ("vertex0", "<f4", 3), ("dummy1", "<f4"),
        ("vertex1", "<f4", 3), ("dummy2", "<f4"),
        ("vertex2", "<f4", 3), ("dummy3", "<f4"),
    ]
)
assert TRIANGLE_DTYPE.itemsize == 160

MAP_DESC_DTYPE = np.dtype(
    [("width", "<i2"), ("height", "<i2"), ("uscale", "<f2"), ("vscale", "<f2"), ("uoffs", "<f2"), ("voffs", "<f2"),
     ("addr", "<u4")]
)
assert MAP_DESC_DTYPE.itemsize == 16

MATERIAL_DTYPE = np.dtype(
    [("diffuse", "<f2", 3), ("transmittance", "<f2", 3), ("flags", "<u4"), ("parameters", "<u4", 4),
     ("map", MAP_DESC_DTYPE, 10)]
)
assert MATERIAL_DTYPE.itemsize == 192

MATERIAL_TEX_IDS_DTYPE = np.dtype([("texture", "<i4", 11)])
assert MATERIAL_TEX_IDS_DTYPE.itemsize == 44

AREA_LIGHT_DTYPE = np.dtype(
    [("position", "<f4", 3), ("energy", "<f4"), ("normal", "<f4", 3), ("area", "<f4"), ("radiance", "<f4", 3),
     ("dummy0", "<i4"), ("vertex0", "<f4", 3), ("triIdx", "<i4"), ("vertex1", "<f4", 3), ("instIdx", "<i4"),
     ("vertex2", "<f4", 3), ("dummy1", "<i4")]
)
assert AREA_LIGHT_DTYPE.itemsize == 96
POINT_LIGHT_DTYPE = np.dtype([("position", "<f4", 3), ("energy", "<f4"), ("radiance", "<f4", 3), ("dummy", "<i4")])
assert POINT_LIGHT_DTYPE.itemsize == 32
SPOT_LIGHT_DTYPE = np.dtype(
    [("position", "<f4", 3), ("cosInner", "<f4"), ("radiance", "<f4", 3), ("cosOuter", "<f4"),
     ("direction", "<f4", 3), ("energy", "<f4")]
)
assert SPOT_LIGHT_DTYPE.itemsize == 48
DIRECTIONAL_LIGHT_DTYPE = np.dtype(
    [("direction", "<f4", 3), ("energy", "<f4"), ("radiance", "<f4", 3), ("dummy", "<i4")]
)
assert DIRECTIONAL_LIGHT_DTYPE.itemsize == 32

BVH_NODE_DTYPE = np.dtype([("bmin", "<f4", 3), ("bmax", "<f4", 3), ("left_first", "<i4"), ("count", "<i4")])
assert BVH_NODE_DTYPE.itemsize == 32
# the light tree (rfwhip_get_light_tree; rfwhip_abi.h: rfwhip_light_tree_node / rfwhip_light_tree_path)
LIGHT_TREE_NODE_DTYPE = np.dtype([("lo", "<f4", 3), ("energy", "<f4"), ("hi", "<f4", 3), ("cos_o", "<f4"), ("axis", "<f4", 3),
                                  ("child", "<u4"), ("light", "<u4"), ("count", "<u4"), ("pad", "<u4", 2)])
assert LIGHT_TREE_NODE_DTYPE.itemsize == 64
LIGHT_TREE_PATH_DTYPE = np.dtype([("bits", "<u4"), ("depth", "<u4")])
assert LIGHT_TREE_PATH_DTYPE.itemsize == 8

# the traversed 4-wide nodes (rfwhip_get_bvh4): compressed (rt::Node4c, rt_types.h) and their float form (rt::Node4f).
# Compressed planes: byte k of qlo[a] / qhi[a] is child k's plane on axis a, decoded as fma(q, scale[a], org[a]).
NODE4C_DTYPE = np.dtype([("org", "<f4", 3), ("scale_x", "<f4"), ("entry", "<u4", 4), ("qlo", "<u4", 3), ("qhi", "<u4", 3),
                         ("scale_y", "<f4"), ("scale_z", "<f4")])
assert NODE4C_DTYPE.itemsize == 64
NODE4F_DTYPE = np.dtype([("lo", "<f4", (3, 4)), ("hi", "<f4", (3, 4)), ("entry", "<u4", 4), ("pad", "<u4", 4)])
assert NODE4F_DTYPE.itemsize == 128
ENTRY_LEAF = 0x80000000
ENTRY_TLAS = 0x40000000
ENTRY_EMPTY = 0xFFFFFFFC
ENTRY_FIRST_MASK = 0x07FFFFFF   # 27 bits: first triangle of a leaf; bits 27..29: count - 1
ENTRY_INDEX_MASK = 0x3FFFFFFF   # 30 bits: a 4-wide node

# MatPropFlags, structs.h:67-83
MAT_IS_DIELECTRIC = 0
MAT_DIFFUSE_MAP_IS_HDR = 1
MAT_HAS_DIFFUSE_MAP = 2
MAT_HAS_NORMAL_MAP = 3
MAT_HAS_SPECULARITY_MAP = 4
MAT_HAS_ROUGHNESS_MAP = 5
MAT_IS_ANISOTROPIC = 6
MAT_HAS_2ND_NORMAL_MAP = 7
MAT_HAS_3RD_NORMAL_MAP = 8
MAT_HAS_2ND_DIFFUSE_MAP = 9
MAT_HAS_3RD_DIFFUSE_MAP = 10
MAT_HAS_SMOOTH_NORMALS = 11
MAT_HAS_ALPHA = 12
MAT_HAS_ALPHA_MAP = 13

TEX_FLOAT4 = 0
TEX_UINT = 1

RESET = 0  # rfw::RenderStatus, context.h:19-23
CONVERGE = 1


# ---- ctypes structs (small, passed by pointer/value) --------------------------------------------------------------
class Mesh(C.Structure):
    _fields_ = [("vertices", C.c_void_p), ("normals", C.c_void_p), ("texCoords", C.c_void_p),
                ("triangles", C.c_void_p), ("indices", C.c_void_p), ("vertexCount", C.c_size_t),
                ("triangleCount", C.c_size_t)]


class Texture(C.Structure):
    _fields_ = [("type", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("texelCount", C.c_uint32),
                ("texAddr", C.c_uint32), ("_pad", C.c_uint32), ("data", C.c_void_p)]


# rfwhip_texture_source (include/rfwhip_abi.h): a texture as finished texels, an encoded JPEG file, or a file's RGBA8 pixels
TEXSRC_TEXELS, TEXSRC_JPEG, TEXSRC_RGBA8 = 0, 1, 2
TEXSRC_FLIP_ROWS, TEXSRC_LINEARIZE_REFERENCE, TEXSRC_LINEARIZE_SRGB = 1, 2, 4


class TextureSource(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("flags", C.c_uint32), ("data", C.c_void_p), ("bytes", C.c_size_t), ("width", C.c_uint32),
                ("height", C.c_uint32), ("type", C.c_uint32), ("texelCount", C.c_uint32)]


class TextureDecodeRecord(C.Structure):
    """rfwhip_texture_decode_record (include/rfwhip.h, rfwhip_get_texture_decode): the decoder's 32-byte record."""
    _fields_ = [(n, C.c_uint32) for n in ("width", "height", "blocks", "intervals", "errors", "alpha_zero", "path", "reserved")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "reserved"}


class ImageInfo(C.Structure):
    """rfwhip_image_info_t (include/rfwhip.h, rfwhip_image_info)."""
    _fields_ = [(n, C.c_uint32) for n in ("width", "height", "components", "h_sampling", "v_sampling", "restart_interval", "intervals",
                                          "supported")] + [("reason", C.c_char * 96)]


# the sky's loaders (include/rfwhip.h, rfwhip_set_sky_hdr / rfwhip_read_sky_table)
SKYSRC_FLIP_ROWS = 1
SKYTAB_VALID, SKYTAB_DEVICE = 1, 2
SKY_ALIAS_DTYPE = np.dtype([("keep", np.float32), ("alias", np.uint32)])  # rfwhip_sky_alias


class HdrInfo(C.Structure):
    """rfwhip_hdr_info_t (include/rfwhip.h, rfwhip_hdr_info)."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("exposure", C.c_float), ("rle", C.c_uint32), ("supported", C.c_uint32),
                ("reason", C.c_char * 96)]


class SkyTableRecord(C.Structure):
    """rfwhip_sky_table_record (include/rfwhip.h, rfwhip_read_sky_table): the 32-byte record of the alias table's chain."""
    _fields_ = [("S", C.c_double), ("heaviest", C.c_uint32), ("light", C.c_uint32), ("heavy", C.c_uint32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32 * 2)]

    def as_dict(self):
        return dict(S=float(self.S), heaviest=int(self.heaviest), light=int(self.light), heavy=int(self.heavy), flags=int(self.flags))


# animations (include/rfwhip_abi.h: rfwhip_rig and its records; rfwhip_set_rig / rfwhip_animate / rfwhip_read_rig)
RIG_PATHS = {"translation": 0, "rotation": 1, "scale": 2, "weights": 3}
RIG_METHODS = {"STEP": 0, "LINEAR": 1, "CUBICSPLINE": 2}
RIG_READ = {"trs": 0, "world": 1, "joints": 2, "weights": 3, "status": 4}
RIG_BASE_POSE = 0xFFFFFFFF
RIG_NODE_DTYPE = np.dtype([("parent", "<i4"), ("translation", "<f4", 3), ("rotation", "<f4", 4), ("scale", "<f4", 3), ("weight_offset", "<u4"),
                           ("matrix", "<f4", 16), ("weight_count", "<u4"), ("reserved", "<u4", 3)])
RIG_SKIN_DTYPE = np.dtype([("mesh_node", "<u4"), ("joint_offset", "<u4"), ("joint_count", "<u4"), ("reserved", "<u4")])
RIG_ANIMATION_DTYPE = np.dtype([("channel_offset", "<u4"), ("channel_count", "<u4")])
RIG_CHANNEL_DTYPE = np.dtype([("node", "<u4"), ("path", "<u4"), ("method", "<u4"), ("key_count", "<u4"), ("time_offset", "<u4"),
                              ("value_offset", "<u4"), ("value_count", "<u4"), ("reserved", "<u4")])
assert (RIG_NODE_DTYPE.itemsize, RIG_SKIN_DTYPE.itemsize, RIG_ANIMATION_DTYPE.itemsize, RIG_CHANNEL_DTYPE.itemsize) == (128, 16, 8, 32)
# the tables of a rig as numpy arrays, in the order of rfwhip_rig's (pointer, count) pairs; inverse_bind shares joints' count
RIG_TABLES = (("nodes", RIG_NODE_DTYPE), ("weights", np.float32), ("skins", RIG_SKIN_DTYPE), ("joints", np.uint32),
              ("inverse_bind", np.float32), ("animations", RIG_ANIMATION_DTYPE), ("channels", RIG_CHANNEL_DTYPE), ("times", np.float32),
              ("values", np.float32))


class Rig(C.Structure):
    """rfwhip_rig (include/rfwhip_abi.h)."""
    _fields_ = [("nodes", C.c_void_p), ("node_count", C.c_size_t), ("weights", C.c_void_p), ("weight_count", C.c_size_t),
                ("skins", C.c_void_p), ("skin_count", C.c_size_t), ("joints", C.c_void_p), ("inverse_bind", C.c_void_p),
                ("joint_count", C.c_size_t), ("animations", C.c_void_p), ("animation_count", C.c_size_t), ("channels", C.c_void_p),
                ("channel_count", C.c_size_t), ("times", C.c_void_p), ("time_count", C.c_size_t), ("values", C.c_void_p),
                ("value_count", C.c_size_t)]


assert C.sizeof(Rig) == 136


class LightCount(C.Structure):
    _fields_ = [("areaLightCount", C.c_uint32), ("pointLightCount", C.c_uint32), ("spotLightCount", C.c_uint32),
                ("directionalLightCount", C.c_uint32)]


class CameraPOD(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("direction", C.c_float * 3), ("focalDistance", C.c_float),
                ("aperture", C.c_float), ("brightness", C.c_float), ("contrast", C.c_float), ("FOV", C.c_float),
                ("aspectRatio", C.c_float), ("clampValue", C.c_float), ("pixelCount", C.c_int32 * 2)]


class CameraView(C.Structure):
    _fields_ = [("pos", C.c_float * 3), ("p1", C.c_float * 3), ("p2", C.c_float * 3), ("p3", C.c_float * 3),
                ("aperture", C.c_float), ("spreadAngle", C.c_float)]


# rfwhip_read_denoise_history's outputs, in argument order (include/rfwhip.h): I~ | lum, var, colour history | lum, (mu1, mu2), n
DENOISE_HISTORY_KEYS = ("pre", "var", "history", "moments", "length")


class Bvh4Info(C.Structure):
    _fields_ = [("n4_base", C.c_uint32), ("n4_count", C.c_uint32), ("tri_base", C.c_uint32), ("tri_count", C.c_uint32),
                ("node_base", C.c_uint32), ("node_count2", C.c_uint32), ("stack_need", C.c_int32),
                ("device_built", C.c_uint32)]


class RenderStats(C.Structure):
    _fields_ = [("primaryTime", C.c_float), ("primaryCount", C.c_uint32), ("secondaryTime", C.c_float),
                ("secondaryCount", C.c_uint32), ("deepTime", C.c_float), ("deepCount", C.c_uint32),
                ("shadowTime", C.c_float), ("shadowCount", C.c_uint32), ("shadeTime", C.c_float),
                ("finalizeTime", C.c_float), ("animationTime", C.c_float), ("renderTime", C.c_float)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class Counters(C.Structure):
    _fields_ = [("rays_extend", C.c_uint64), ("rays_shadow", C.c_uint64), ("inner_extend", C.c_uint64),
                ("tris_extend", C.c_uint64), ("inner_shadow", C.c_uint64), ("tris_shadow", C.c_uint64),
                ("shaded", C.c_uint64), ("samples", C.c_uint64),
                # rendercore only (the oracle fills the first eight): node visits served by the LDS top-of-tree cache
                ("lds_extend", C.c_uint64), ("lds_shadow", C.c_uint64),
                ("extend_ticks", C.c_uint64), ("extend_launches_timed", C.c_uint64)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class NoiseStats(C.Structure):
    """rfwhip_noise_stats (include/rfwhip.h, rfwhip_get_noise)."""
    _fields_ = [("samples", C.c_uint64), ("pixels", C.c_uint64), ("converged", C.c_uint64), ("mean_error", C.c_double),
                ("max_error", C.c_float), ("threshold", C.c_float)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class MeterStats(C.Structure):
    """rfwhip_meter_stats (include/rfwhip.h, rfwhip_get_meter): the exposure meter's 32-byte record."""
    _fields_ = [("exposure", C.c_float), ("log2_exposure", C.c_float), ("log2_target", C.c_float), ("log2_luminance", C.c_float),
                ("valid", C.c_uint32), ("excluded", C.c_uint32), ("steps", C.c_uint32), ("reserved", C.c_uint32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}


METER_BINS = 256


class JpegStats(C.Structure):
    """rfwhip_jpeg_stats (include/rfwhip.h, rfwhip_get_jpeg): the JPEG encoder's 32-byte record."""
    _fields_ = [(n, C.c_uint32) for n in ("bytes", "intervals", "mcus", "blocks", "stuffed_bytes", "overflow", "header_bytes", "reserved")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "reserved"}


class AdaptiveStats(C.Structure):
    """rfwhip_adaptive_stats (include/rfwhip.h, rfwhip_get_adaptive)."""
    _fields_ = [(n, C.c_uint64) for n in ("tiles", "active_tiles", "pixels", "active_pixels", "samples_taken", "samples_uniform")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


# rfwhip_noise_tile: one record per 32 x 8 noise tile
NOISE_TILE_DTYPE = np.dtype([("sum_e", np.float32), ("max_e", np.float32), ("pixels", np.uint32), ("converged", np.uint32)])
NOISE_TILE_X, NOISE_TILE_Y = 32, 8

assert C.sizeof(AdaptiveStats) == 48
assert C.sizeof(NoiseStats) == 40 and NOISE_TILE_DTYPE.itemsize == 16
assert C.sizeof(Mesh) == 56
assert C.sizeof(Texture) == 32
assert C.sizeof(CameraPOD) == 60
assert C.sizeof(CameraView) == 56
assert C.sizeof(RenderStats) == 48
