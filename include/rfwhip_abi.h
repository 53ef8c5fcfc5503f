/*
 * rfwhip_abi.h — plain-C restatement of the POD structs that cross the RenderContext plugin boundary of
 * MeirBon/rendering-fw.  No glm, no half.hpp: every field is a scalar or a fixed array, the byte layout is
 * identical to the reference's structs (sizes are static-asserted below), so a reference-side shim can pass
 * `reinterpret_cast`ed pointers straight through.
 *
 * Reference layouts restated here (file:line under /root/reference):
 *   rfw::Triangle / DeviceTriangle  RFW/system/context/rfw/context/structs.h:24-60, device_structs.h:22-33   160 B
 *   rfw::Material / DeviceMaterial  structs.h:85-127, device_structs.h:56-74                                 192 B
 *   rfw::MaterialTexIds             structs.h:163-167                                                        44 B
 *   rfw::Mesh                       structs.h:175-191                                                        56 B
 *   rfw::TextureData                structs.h:193-205                                                        32 B
 *   rfw::LightCount + 4 lights      structs.h:207-255                                            16/96/32/48/32 B
 *   rfw::CameraView                 device_structs.h:95-103                                                  56 B
 *   rfw::Camera (data members)      RFW/system/context/rfw/context/camera.h:27-37                            60 B
 *   rfw::RenderStats                RFW/system/context/rfw/context/context.h:50-72                           48 B
 *   rfw::bvh::BVHNode               RFW/system/bvh/include/bvh/bvh_node.h:23-28, src/bvh_node.cpp:10         32 B
 */
#ifndef RFWHIP_ABI_H
#define RFWHIP_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
#define RFWHIP_STATIC_ASSERT(c, m) static_assert(c, m)
extern "C" {
#else
#define RFWHIP_STATIC_ASSERT(c, m) _Static_assert(c, m)
#endif

/* structs.h:24-60 — per-face shading record, AoS as the host application hands it over. */
typedef struct rfwhip_triangle
{
	float u0, u1, u2;
	int32_t lightTriIdx; /* -1 = not a light; index into the area-light array otherwise (structs.h:37) */
	float v0, v1, v2;
	uint32_t material;
	float vN0[3];
	float Nx;
	float vN1[3];
	float Ny;
	float vN2[3];
	float Nz;
	float T[3];
	float area;
	float B[3];
	float LOD;
	float vertex0[3];
	float dummy1;
	float vertex1[3];
	float dummy2;
	float vertex2[3];
	float dummy3;
} rfwhip_triangle;
RFWHIP_STATIC_ASSERT(sizeof(rfwhip_triangle) == 160, "Triangle must be 160 B (structs.h:60)");

/* One 16-byte texture/normal-map descriptor inside Material (structs.h:99-127). */
typedef struct rfwhip_map_desc
{
	int16_t width, height;
	uint16_t uscale, vscale, uoffs, voffs; /* IEEE binary16 bit patterns */
	uint32_t addr;						   /* index into the TextureData array (EmbreeRT/src/Context.cpp:452) */
} rfwhip_map_desc;
RFWHIP_STATIC_ASSERT(sizeof(rfwhip_map_desc) == 16, "map descriptor must be 128 bit");

/* Material flag bits (structs.h:67-83). */
enum rfwhip_mat_flag
{
	RFWHIP_MAT_IS_DIELECTRIC = 0,
	RFWHIP_MAT_DIFFUSE_MAP_IS_HDR = 1,
	RFWHIP_MAT_HAS_DIFFUSE_MAP = 2,
	RFWHIP_MAT_HAS_NORMAL_MAP = 3,
	RFWHIP_MAT_HAS_SPECULARITY_MAP = 4,
	RFWHIP_MAT_HAS_ROUGHNESS_MAP = 5,
	RFWHIP_MAT_IS_ANISOTROPIC = 6,
	RFWHIP_MAT_HAS_2ND_NORMAL_MAP = 7,
	RFWHIP_MAT_HAS_3RD_NORMAL_MAP = 8,
	RFWHIP_MAT_HAS_2ND_DIFFUSE_MAP = 9,
	RFWHIP_MAT_HAS_3RD_DIFFUSE_MAP = 10,
	RFWHIP_MAT_HAS_SMOOTH_NORMALS = 11,
	RFWHIP_MAT_HAS_ALPHA = 12,
	RFWHIP_MAT_HAS_ALPHA_MAP = 13
};

/* structs.h:85-127.  parameters[] holds 16 8-bit Disney parameters in the order of bsdf/compat.h:57-72:
 * x: metallic, subsurface, specular, roughness | y: specTint, anisotropic, sheen, sheenTint |
 * z: clearcoat, clearcoatGloss, transmission, eta*0.5 | w: custom0..3  (material_list.cpp:337-340). */
typedef struct rfwhip_material
{
	uint16_t diffuse[3];	   /* binary16 */
	uint16_t transmittance[3]; /* binary16 */
	uint32_t flags;
	uint32_t parameters[4];
	rfwhip_map_desc map[10]; /* tex0-2, nmap0-2, smap, rmap, cmap, amap */
} rfwhip_material;
RFWHIP_STATIC_ASSERT(sizeof(rfwhip_material) == 192, "Material must be 192 B (device_structs.h:56-74)");

typedef struct rfwhip_material_tex_ids
{
	int32_t texture[11];
} rfwhip_material_tex_ids;
RFWHIP_STATIC_ASSERT(sizeof(rfwhip_material_tex_ids) == 44, "MaterialTexIds must be 44 B");

/* structs.h:175-191.  All pointers are BORROWED for the duration of the call only. */
typedef struct rfwhip_mesh
{
	const float *vertices;			   /* vec4[vertexCount] */
	const float *normals;			   /* vec3[vertexCount] or NULL */
	const float *texCoords;			   /* vec2[vertexCount] or NULL */
	const rfwhip_triangle *triangles; /* [triangleCount] */
	const uint32_t *indices;		   /* uvec3[triangleCount] or NULL (then triangle i = vertices 3i..3i+2) */
	size_t vertexCount;
	size_t triangleCount;
} rfwhip_mesh;
RFWHIP_STATIC_ASSERT(sizeof(rfwhip_mesh) == 56, "Mesh must be 56 B");

enum rfwhip_texture_type
{
	RFWHIP_TEX_FLOAT4 = 0,
	RFWHIP_TEX_UINT = 1
};

/* structs.h:193-205.  UINT texels are r | g<<8 | b<<16 | a<<24, decoded with 1/256 (Context.cpp:466-470). */
typedef struct rfwhip_texture
{
	uint32_t type;
	uint32_t width, height, texelCount;
	uint32_t texAddr;
	uint32_t _pad;
	const void *data;
} rfwhip_texture;
RFWHIP_STATIC_ASSERT(sizeof(rfwhip_texture) == 32, "TextureData must be 32 B");

/* A texture as a host has it before rfw::texture (texture.cpp of the reference's system layer, which a backend never sees) has
 * decoded it: finished texels, an encoded JPEG file, or a file's RGBA8 pixels (rfwhip_set_texture_sources, rfwhip.h). */
enum rfwhip_texture_source_kind
{
	RFWHIP_TEXSRC_TEXELS = 0, /* as rfwhip_texture: type, width, height, texelCount, data */
	RFWHIP_TEXSRC_JPEG = 1,	  /* data / bytes: a baseline JPEG stream; width, height, type, texelCount are ignored */
	RFWHIP_TEXSRC_RGBA8 = 2	  /* data: width x height pixels r, g, b, a in file order (top row first); bytes = 4 width height */
};
enum rfwhip_texture_source_flags
{
	RFWHIP_TEXSRC_FLIP_ROWS = 1,		   /* texel row 0 is the image's bottom row (texture.cpp:83-86, FLIPPED) */
	RFWHIP_TEXSRC_LINEARIZE_REFERENCE = 2, /* c c >> 8 per colour byte, before the mips (texture.cpp:6-14,90, LINEARIZED) */
	RFWHIP_TEXSRC_LINEARIZE_SRGB = 4	   /* the exact sRGB EOTF per colour byte, rounded to nearest, before the mips */
};
typedef struct rfwhip_texture_source
{
	uint32_t kind;
	uint32_t flags;
	const void *data;
	size_t bytes;
	uint32_t width, height;
	uint32_t type;
	uint32_t texelCount;
} rfwhip_texture_source;
RFWHIP_STATIC_ASSERT(sizeof(rfwhip_texture_source) == 40, "rfwhip_texture_source must be 40 B");

/* A sky as a host has it before rfw::skybox::load has decoded it: the bytes of a Radiance .hdr file (rfwhip_set_sky_hdr, rfwhip.h). */
enum rfwhip_sky_source_flags
{
	RFWHIP_SKYSRC_FLIP_ROWS = 1 /* sky row 0 is the file's last scanline */
};
/* One bucket of the sky's alias table (sky_sampling; rfwhip_read_sky_table, rfwhip.h): texel k is kept with probability keep, texel
 * alias is handed out otherwise.  The layout of rt::SkyAlias, which the shade kernel reads. */
typedef struct rfwhip_sky_alias
{
	float keep;
	uint32_t alias;
} rfwhip_sky_alias;
RFWHIP_STATIC_ASSERT(sizeof(rfwhip_sky_alias) == 8, "rfwhip_sky_alias must be 8 B");

/* A rig: the animation data of a glTF file as flat tables (rfwhip_set_rig, rfwhip.h).  Matrices are 16 floats, column-major, like
 * rfwhip_set_instance's. */
enum rfwhip_rig_path
{
	RFWHIP_RIG_PATH_TRANSLATION = 0, /* 3 floats per key */
	RFWHIP_RIG_PATH_ROTATION = 1,	 /* 4: xyzw */
	RFWHIP_RIG_PATH_SCALE = 2,		 /* 3 */
	RFWHIP_RIG_PATH_WEIGHTS = 3		 /* the node's weight_count */
};
enum rfwhip_rig_method
{
	RFWHIP_RIG_METHOD_STEP = 0,
	RFWHIP_RIG_METHOD_LINEAR = 1,
	RFWHIP_RIG_METHOD_CUBICSPLINE = 2 /* three times the floats per key: in-tangent, value, out-tangent (weights: per target) */
};
enum rfwhip_rig_read
{
	RFWHIP_RIG_READ_TRS = 0,
	RFWHIP_RIG_READ_WORLD = 1,
	RFWHIP_RIG_READ_JOINTS = 2,
	RFWHIP_RIG_READ_WEIGHTS = 3,
	RFWHIP_RIG_READ_STATUS = 4
};
#define RFWHIP_RIG_BASE_POSE 0xFFFFFFFFu /* rfwhip_animate: no animation, the base pose */
typedef struct rfwhip_rig_node
{
	int32_t parent; /* -1: a root; nodes may come in any order */
	float translation[3];
	float rotation[4]; /* xyzw */
	float scale[3];
	uint32_t weight_offset; /* the node's base morph weights: weights[weight_offset .. + weight_count) */
	float matrix[16];		/* the node's constant matrix: local = T R S matrix */
	uint32_t weight_count;
	uint32_t reserved[3];
} rfwhip_rig_node;
typedef struct rfwhip_rig_skin
{
	uint32_t mesh_node;					/* the node the skinned mesh hangs on */
	uint32_t joint_offset, joint_count; /* joints[joint_offset .. + joint_count) and the same range of inverse_bind */
	uint32_t reserved;
} rfwhip_rig_skin;
typedef struct rfwhip_rig_animation
{
	uint32_t channel_offset, channel_count;
} rfwhip_rig_animation;
typedef struct rfwhip_rig_channel
{
	uint32_t node, path, method;
	uint32_t key_count;
	uint32_t time_offset;				/* times[time_offset .. + key_count): finite, strictly increasing */
	uint32_t value_offset, value_count; /* values[value_offset .. + value_count), value_count = floats per key x key_count (x 3) */
	uint32_t reserved;
} rfwhip_rig_channel;
typedef struct rfwhip_rig
{
	const rfwhip_rig_node *nodes;
	size_t node_count;
	const float *weights;
	size_t weight_count;
	const rfwhip_rig_skin *skins;
	size_t skin_count;
	const uint32_t *joints;	   /* node indices */
	const float *inverse_bind; /* 16 floats per entry of joints */
	size_t joint_count;
	const rfwhip_rig_animation *animations;
	size_t animation_count;
	const rfwhip_rig_channel *channels;
	size_t channel_count;
	const float *times;
	size_t time_count;
	const float *values;
	size_t value_count;
} rfwhip_rig;
/* What an evaluation leaves beside its values (rfwhip_read_rig, RFWHIP_RIG_READ_STATUS). */
typedef struct rfwhip_rig_status
{
	float time;					 /* the given time after the wrap of the animation's first channel; as given for a base pose */
	uint32_t rotation_fallbacks; /* sampled rotations of zero or non-finite norm, replaced by the identity */
	uint32_t inverse_fallbacks;	 /* skins whose mesh node had a zero or non-finite determinant, its inverse replaced by the identity */
	uint32_t serial;			 /* the evaluations of this rig so far */
	uint32_t animation;			 /* the animation evaluated, RFWHIP_RIG_BASE_POSE for the base pose */
	uint32_t reserved[3];
} rfwhip_rig_status;
RFWHIP_STATIC_ASSERT(sizeof(rfwhip_rig_node) == 128, "rfwhip_rig_node must be 128 B");
RFWHIP_STATIC_ASSERT(sizeof(rfwhip_rig_skin) == 16, "rfwhip_rig_skin must be 16 B");
RFWHIP_STATIC_ASSERT(sizeof(rfwhip_rig_animation) == 8, "rfwhip_rig_animation must be 8 B");
RFWHIP_STATIC_ASSERT(sizeof(rfwhip_rig_channel) == 32, "rfwhip_rig_channel must be 32 B");
RFWHIP_STATIC_ASSERT(sizeof(rfwhip_rig) == 136, "rfwhip_rig must be 136 B");
RFWHIP_STATIC_ASSERT(sizeof(rfwhip_rig_status) == 32, "rfwhip_rig_status must be 32 B");

typedef struct rfwhip_light_count
{
	uint32_t areaLightCount, pointLightCount, spotLightCount, directionalLightCount;
} rfwhip_light_count;

typedef struct rfwhip_area_light
{
	float position[3];
	float energy;
	float normal[3];
	float area;
	float radiance[3];
	int32_t dummy0;
	float vertex0[3];
	int32_t triIdx;
	float vertex1[3];
	int32_t instIdx;
	float vertex2[3];
	int32_t dummy1;
} rfwhip_area_light;
RFWHIP_STATIC_ASSERT(sizeof(rfwhip_area_light) == 96, "AreaLight must be 96 B");

typedef struct rfwhip_point_light
{
	float position[3];
	float energy;
	float radiance[3];
	int32_t dummy;
} rfwhip_point_light;
RFWHIP_STATIC_ASSERT(sizeof(rfwhip_point_light) == 32, "PointLight must be 32 B");

typedef struct rfwhip_spot_light
{
	float position[3];
	float cosInner;
	float radiance[3];
	float cosOuter;
	float direction[3];
	float energy;
} rfwhip_spot_light;
RFWHIP_STATIC_ASSERT(sizeof(rfwhip_spot_light) == 48, "SpotLight must be 48 B");

typedef struct rfwhip_directional_light
{
	float direction[3];
	float energy;
	float radiance[3];
	int32_t dummy;
} rfwhip_directional_light;
RFWHIP_STATIC_ASSERT(sizeof(rfwhip_directional_light) == 32, "DirectionalLight must be 32 B");

/* camera.h:27-37 — the data members of rfw::Camera in declaration order. */
typedef struct rfwhip_camera
{
	float position[3];
	float direction[3]; /* assumed normalised (Camera.cpp:112) */
	float focalDistance;
	float aperture;
	float brightness;
	float contrast;
	float FOV; /* degrees */
	float aspectRatio;
	float clampValue;
	int32_t pixelCount[2];
} rfwhip_camera;
RFWHIP_STATIC_ASSERT(sizeof(rfwhip_camera) == 60, "Camera data members are 60 B");

/* device_structs.h:95-103 */
typedef struct rfwhip_camera_view
{
	float pos[3];
	float p1[3];
	float p2[3];
	float p3[3];
	float aperture;
	float spreadAngle;
} rfwhip_camera_view;
RFWHIP_STATIC_ASSERT(sizeof(rfwhip_camera_view) == 56, "CameraView must be 56 B");

/* context.h:50-72 — times in milliseconds. */
typedef struct rfwhip_render_stats
{
	float primaryTime;
	uint32_t primaryCount;
	float secondaryTime;
	uint32_t secondaryCount;
	float deepTime;
	uint32_t deepCount;
	float shadowTime;
	uint32_t shadowCount;
	float shadeTime;
	float finalizeTime;
	float animationTime;
	float renderTime;
} rfwhip_render_stats;
RFWHIP_STATIC_ASSERT(sizeof(rfwhip_render_stats) == 48, "RenderStats must be 48 B");

/* bvh_node.h:23-28 — BVH2 node: leaf iff count >= 0 (then left_first = first prim), otherwise the two children
 * live at left_first and left_first+1. */
typedef struct rfwhip_bvh_node
{
	float bmin[3];
	float bmax[3];
	int32_t left_first;
	int32_t count;
} rfwhip_bvh_node;
RFWHIP_STATIC_ASSERT(sizeof(rfwhip_bvh_node) == 32, "BVHNode must be 32 B (bvh_node.cpp:10)");

/* A node of the light tree (setting light_sampling=tree; rfwhip_get_light_tree; rfwhip.h has the formulas).  Node 0 is the root,
 * node 1 is unused, the children of a node are `child` and `child + 1` with `child` even; child == 0: a leaf holding `light`. */
typedef struct rfwhip_light_tree_node
{
	float lo[3], energy; /* box of the lights below; sum of their energies (a negative or NaN energy counts as 0) */
	float hi[3], cos_o;	 /* cosine of the half angle of the cone of their normals; -1: every direction */
	float axis[3];		 /* the cone's axis */
	uint32_t child, light, count; /* count: lights below */
	uint32_t pad[2];
} rfwhip_light_tree_node;
RFWHIP_STATIC_ASSERT(sizeof(rfwhip_light_tree_node) == 64, "light-tree node must be 64 B");
/* A light's way down the tree: bit i of `bits` set = the right child at level i; `depth` levels (0, 0 for a directional light). */
typedef struct rfwhip_light_tree_path
{
	uint32_t bits, depth;
} rfwhip_light_tree_path;
RFWHIP_STATIC_ASSERT(sizeof(rfwhip_light_tree_path) == 8, "light-tree path must be 8 B");

/* context.h:19-23 */
enum rfwhip_render_status
{
	RFWHIP_RESET = 0,
	RFWHIP_CONVERGE = 1
};

/* Known-answer records of rfwhip_kat(): every function reads one record of RFWHIP_KAT_IN floats and writes one of
 * RFWHIP_KAT_OUT floats (integers travel as their bit patterns).  BSDF record: [0..2] colour, [3..5] absorption,
 * [6..8] ShadingData parameters x,y,z (bsdf/compat.h:57-72), [9..11] N, [12..14] wo, [15..17] wi, [18] t,
 * [19] backfacing, [20] r3 (or r0), [21] r4.  Light record: [0..2] I, [3..5] N, [6] r0, [7] r1, [8] light index,
 * [9..11] O. */
enum
{
	RFWHIP_KAT_IN = 24,
	RFWHIP_KAT_OUT = 8
};
enum rfwhip_kat_function
{
	RFWHIP_KAT_BSDF_EVAL = 0,		   /* disney.h:104-185 BSDFEval            -> rgb */
	RFWHIP_KAT_BSDF_PDF = 1,		   /* disney.h:83-101  BSDFPdf             -> pdf */
	RFWHIP_KAT_BSDF_SAMPLE = 2,		   /* disney.h:188-262 BSDFSample, frame by createTangentSpace(N) -> wi, pdf */
	RFWHIP_KAT_TANGENT_SPACE = 3,	   /* tools.h:204-211                      -> T, B */
	RFWHIP_KAT_PACK_NORMAL = 4,		   /* tools.h:10-29                        -> packed bits, unpacked normal */
	RFWHIP_KAT_RANDOM_BARYCENTRICS = 5, /* lights.h:119-157, r0 = [20]          -> barycentrics */
	RFWHIP_KAT_POINT_ON_LIGHT = 6,	   /* lights.h:159-265 on the context's lights -> P, pickProb, lightPdf, colour */
	RFWHIP_KAT_LIGHT_PICK_PROB = 7,	   /* lights.h:83-116                      -> probability */
	RFWHIP_KAT_BLUE_NOISE = 8,		   /* tools.h:163-181, [0..3] = x, y, sample, dimension (ints) -> value */
	RFWHIP_KAT_HASH = 9,			   /* tools.h:218-235, [0] = seed -> WangHash bits, RandomFloat, state bits */
	RFWHIP_KAT_FASTDIV = 11,		   /* the slot -> pixel mapping's division by per-frame constants (rt_types.h: fast_div): [0..7] = four (n, d) pairs, n < 2^31, 0 < d < 2^31 (ints) -> four quotients (ints) */
	RFWHIP_KAT_TEX_WRAP = 12,		   /* the wrap of a texel coordinate (getShadingData.h:33-41: `% width`, `% height`; rt_core.h: tex_wrap): [0..7] = four (x, w) pairs, 0 <= x < 2^31, 1 <= w < 2^31 (ints) -> four remainders (ints) */
	RFWHIP_KAT_HALF_TO_FLOAT = 10,	   /* half -> float as the shade kernels read materials (structs.h:88-117): [0..7] = 8 half bit patterns (ints) -> 8 floats */
	/* sky sampling on the table of the last rfwhip_update() with sky_sampling=1 (rt_core.h: sky_sample / sky_eval).  Both answer
	 * [0..2] = the direction, [3] = the sampling density per steradian (lum / S), [4..6] = the radiance, [7] = the texel (int, -1: none) */
	RFWHIP_KAT_SKY_SAMPLE = 13,		   /* [0..4] = u0, u1 (the bucket's row, column), coin (texel or alias), a, b (position in phi, cos theta) -> the texel drawn and a direction in it */
	RFWHIP_KAT_SKY_PDF = 14,		   /* [0..2] = D -> what pt_sky reads for D and the density there */
	/* the texture sampler on the scene of the last rfwhip_update() (getShadingData.h:25-217; rt_core.h: fetch_texel, fetch_trilinear,
	 * pt_surface, pt_textures).  An index outside the scene's tables is an error. */
	RFWHIP_KAT_TEX_FETCH = 15,		   /* [0] = texture (int), [1] = form (int: 0 = the trilinear fetch of a colour layer, 1 = the bilinear fetch at level 0 of a normal-map layer), [2] = lambda, [3..4] = tu, tv, [5..6] = width, height as the material's map descriptor gives them (ints, 1..65536) -> rgba */
	RFWHIP_KAT_SURFACE_LAYERS = 16,   /* [0] = instance, [1] = triangle (ints), [2..3] = barycentrics u, v (weights of vertex 1, 2), [4..6] = D, [7] = t, [8] = the camera's spread angle -> [0..2] = colour after the texture layers, [3..5] = shading normal after the normal maps, [6] = flags (int): bit 0 alpha pass-through, bit 1 the material is textured */
	/* what setting material_maps makes of the same hit, whatever the setting is (rt_core.h: pt_maps_alpha, pt_maps_params; rfwhip.h has the rule) */
	RFWHIP_KAT_SURFACE_MAPS = 20,	   /* the input record of SURFACE_LAYERS -> [0] = the roughness byte, [1] = the metallic byte after their maps (ints; the material's own for a hit the mask passes through), [2] = a (1 without a mask), [3] = flags (int): bit 0 alpha pass-through by the mask, bit 1 slot 6 (metallic) present, bit 2 slot 7 (roughness) present, bit 3 slot 9 (alpha mask) present */
	/* the light tree of light_sampling=tree (rt_core.h: lt_sample / lt_pick_prob); RFWHIP_ERR_STATE in any other mode */
	RFWHIP_KAT_LT_SAMPLE = 17,		   /* [0..2] = I, [3..5] = N, [6] = r0, [7] = r1 -> [0..2] = P, [3] = q, [4] = lightPdf (area: dist^2 / (area LNdotL)), [5] = the light (int, -1: none), [6] = its rank in the order r1 walks through (int) */
	RFWHIP_KAT_LT_PICK_PROB = 18, 	   /* [0..2] = I, [3..5] = N, [8] = light (int) -> q, bit for bit what LT_SAMPLE gives when it draws that light */
	/* the exposure meter's bin of a luminance (csrc/metering.h: mt_bin; rfwhip.h, rfwhip_get_meter, has the formula) */
	RFWHIP_KAT_METER_BIN = 19		   /* [0..7] = eight Y values -> eight bins (ints, 0..255); -1 where Y is not valid (not 0 < Y < +inf) */
};

#ifdef __cplusplus
}
#endif
#endif /* RFWHIP_ABI_H */
