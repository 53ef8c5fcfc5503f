/*
 * rfwhip.h — C ABI of the MI355X-native (gfx950, HIP) wavefront rendercore for MeirBon/rendering-fw.
 *
 * This is the drop-in boundary: a `rfw::RenderContext` plugin (RFW/system/context/rfw/context/context.h:74-111)
 * forwards each virtual call to the entry point listed beside it below; `rendering-fw_amd/csrc/plugin/HipRT.cpp`
 * is that plugin, and INTEGRATION.md shows the binding.  Only PODs from rfwhip_abi.h, plain pointers and sizes
 * cross this boundary; errors are int codes + rfwhip_last_error() (the reference throws std::runtime_error across
 * the .so boundary, context.h:84-91 — the plugin shim re-throws).  Every pointer argument is borrowed for the call
 * only: the core uploads into HBM inside the call and never dereferences host memory later (contrast
 * EmbreeRT/src/Mesh.cpp:29,46 which keeps shared buffers).
 *
 * All calls for one context must come from one thread at a time (RFW/system/src/rfw/app.cpp:15-16).
 */
#ifndef RFWHIP_H
#define RFWHIP_H

#include "rfwhip_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RFWHIP_API __attribute__((visibility("default")))

typedef struct rfwhip_context rfwhip_context;

enum rfwhip_status
{
	RFWHIP_OK = 0,
	RFWHIP_ERR_INVALID_ARGUMENT = 1,
	RFWHIP_ERR_NO_DEVICE = 2, /* no HIP device / kernel image not loadable: the core never falls back to a CPU path */
	RFWHIP_ERR_HIP = 3,
	RFWHIP_ERR_STATE = 4,
	RFWHIP_ERR_UNSUPPORTED = 5
};

/* Thread-local description of the last failure of any rfwhip_* call on this thread. */
RFWHIP_API const char *rfwhip_last_error(void);
RFWHIP_API const char *rfwhip_version(void);

/* ---- lifetime ------------------------------------------------------------------------------------------------
 * createRenderContext / destroyRenderContext   (RFW/system/context/rfw/context/export.h:8-15)
 * rank/world: this context renders the 8-row strips it owns.  Strips are dealt to the ranks in periods of
 * `world`, forwards in even periods and backwards in odd ones (0 1 .. w-1 | w-1 .. 1 0 | ...): strip s belongs to rank
 * (s / world) odd ? world - 1 - s % world : s % world — NOT plain s % world (rows get dearer down an image of terrain
 * under sky, and the serpentine cancels that gradient).  A host that gathers local framebuffers itself de-interleaves
 * with rfwhip_deinterleave_*; rfwhip_group_* / rfwhip_comm_* below do the whole gather.  world = 1 renders everything. */
#define RFWHIP_STRIP_ROWS 8
/* the rank (of `world`) that owns image row y: the rule above, for hosts that route per-pixel queries (the probe) themselves */
static inline int rfwhip_row_owner(int y, int world)
{
	const int strip = y / RFWHIP_STRIP_ROWS, k = strip / world, pos = strip % world;
	return (k & 1) ? world - 1 - pos : pos;
}
RFWHIP_API int rfwhip_create(int device_ordinal, int rank, int world, rfwhip_context **out);
/* RenderContext::cleanup() (context.h:93).  Idempotent: the reference calls it twice on unload
 * (system.cpp:160-178 + EmbreeRT/src/Context.cpp:30). */
RFWHIP_API int rfwhip_cleanup(rfwhip_context *ctx);
RFWHIP_API void rfwhip_destroy(rfwhip_context *ctx);

/* RenderContext::init(GLuint*, uint width, uint height) (context.h:88) with the headless BUFFER target
 * (RenderTarget::BUFFER, context.h:27-34); may be called again on resize (app.cpp:44-59). */
RFWHIP_API int rfwhip_init(rfwhip_context *ctx, uint32_t width, uint32_t height);

/* ---- scene synchronisation, in the order rfw::system::synchronize issues them (system.cpp:247-433) ----------- */
/* set_sky(const std::vector<glm::vec3>&, size_t w, size_t h)                               context.h:100 */
RFWHIP_API int rfwhip_set_sky(rfwhip_context *ctx, const float *rgb, size_t width, size_t height);
/* set_textures(const std::vector<TextureData>&)                                            context.h:97 */
RFWHIP_API int rfwhip_set_textures(rfwhip_context *ctx, const rfwhip_texture *textures, size_t count);
/* set_materials(const std::vector<DeviceMaterial>&, const std::vector<MaterialTexIds>&)    context.h:95-96 */
RFWHIP_API int rfwhip_set_materials(rfwhip_context *ctx, const rfwhip_material *materials,
									const rfwhip_material_tex_ids *tex_ids, size_t count);
/* set_mesh(size_t index, const Mesh&): same vertexCount as before => refit, else rebuild    context.h:98,
 * EmbreeRT/src/Mesh.cpp:33-35, bvh/src/top_level_bvh.cpp:26 */
RFWHIP_API int rfwhip_set_mesh(rfwhip_context *ctx, size_t index, const rfwhip_mesh *mesh);
/* set_instance(size_t i, size_t meshIdx, const mat4& transform, const mat3& inverse_transform)
 * transform: column-major 4x4 object->world; normal_matrix: column-major 3x3 inverse-transpose
 * (system.cpp:347).                                                                          context.h:99 */
RFWHIP_API int rfwhip_set_instance(rfwhip_context *ctx, size_t index, size_t mesh_index, const float *transform16,
								   const float *normal_matrix9);
/* set_lights(LightCount, area*, point*, spot*, directional*)                                context.h:101-103 */
RFWHIP_API int rfwhip_set_lights(rfwhip_context *ctx, rfwhip_light_count count, const rfwhip_area_light *area,
								 const rfwhip_point_light *point, const rfwhip_spot_light *spot,
								 const rfwhip_directional_light *directional);
/* The 5 x 65536-word table of the reference's blue-noise sampler (createBlueNoiseBuffer(), blue_noise.h:8204, uploaded
 * by CUDART/src/Context.cpp:43-46).  The table is data of the reference tree and is NOT part of this library: the
 * plugin shim hands it over when it is built there.  With a table and sampler=bluenoise the pt integrator draws the
 * primary-ray jitter / lens sample from blueNoiseSampler (Kernels.cu:391-394) instead of the hash RNG. */
RFWHIP_API int rfwhip_set_blue_noise(rfwhip_context *ctx, const uint32_t *table, size_t words);
/* ---- device skinning (extension: rfw::system skins on the host, geometry/gltf/mesh.cpp:18-125, and re-sends the mesh
 * through set_mesh; these two calls keep the bind pose on the device and take the CPU out of the animation loop) ----
 * set_mesh_skin: per vertex of mesh `index` (as last set with rfwhip_set_mesh = bind pose) four joint indices, four
 * weights and the bind-pose vertex normal (xyz, w ignored).
 * pose_mesh: joint_count column-major 4x4 joint matrices -> vertex = sum_k w_k M[j_k] * base, normal =
 * normalize(base_normal * inverse(that matrix)) (mesh.cpp:35-44), triangles' vertex/face normals (update_triangles,
 * mesh.cpp:428-485), then the same device refit as a same-count rfwhip_set_mesh.  rfwhip_update() afterwards. */
RFWHIP_API int rfwhip_set_mesh_skin(rfwhip_context *ctx, size_t mesh_index, const uint32_t *joints4, const float *weights4,
									const float *base_normals4, size_t vertex_count);
RFWHIP_API int rfwhip_pose_mesh(rfwhip_context *ctx, size_t mesh_index, const float *joint_matrices16, size_t joint_count);
/* ---- device morph targets (extension, same idea: SceneMesh::set_pose(weights), geometry/gltf/mesh.cpp:127-147, runs on the
 * host in the reference).  set_mesh_morph: for mesh `index` (last rfwhip_set_mesh = base pose) the base vertex normals and
 * target_count displacement sets, each vertex_count float4 positions and float4 normals (w ignored), target-major.
 * morph_mesh: vertex = base + sum_j weights[j] * target_j for positions and normals (normals NOT renormalised, as there),
 * then update_triangles (mesh.cpp:428-485) and the device refit.  rfwhip_update() afterwards. */
RFWHIP_API int rfwhip_set_mesh_morph(rfwhip_context *ctx, size_t mesh_index, const float *base_normals4,
									 const float *target_positions4, const float *target_normals4, size_t target_count,
									 size_t vertex_count);
RFWHIP_API int rfwhip_morph_mesh(rfwhip_context *ctx, size_t mesh_index, const float *weights, size_t weight_count);
/* ---- animations on the device (extension: SceneAnimation::setTime, geometry/gltf/animation.cpp:231-322, 374-422, and the node
 * hierarchy, node.cpp:54-116, run on the host in the reference).  The two pairs of calls above took the vertices out of the host's
 * animation loop; these take the pose out of it: a host hands over a TIME, the device samples the keyframes, multiplies the
 * hierarchy, and writes the joint matrices and morph weights that the skinning and morph kernels read (csrc/animation.h, kernel
 * family 18).
 * set_rig: the flat tables of rfwhip_rig (rfwhip_abi.h) become rig `rig_index`.  Everything is validated on the host before a byte
 *   goes to the device; a refused rig leaves a message that names the node, skin or channel, and the previous rig of that index
 *   stays in place with its bindings.  Refused: an index or offset out of range, a parent cycle, key_count 0, a key time that is not
 *   finite or not greater than its predecessor, a value range whose length is not path x method x key_count, a weights channel on a
 *   node without weights, a skin without joints, two channels of one animation on the same node and path.  An accepted rig replaces
 *   the previous one of its index and drops that one's bindings.
 * bind_rig: mesh `mesh_index` follows the rig: a mesh with rfwhip_set_mesh_skin takes the joint matrices of skin `skin_index`
 *   (refused when the mesh refers to a joint the skin does not have), a mesh with rfwhip_set_mesh_morph the weights of node
 *   `node_index` (refused unless the node has as many weights as the mesh has targets).  Several meshes may follow one rig; a mesh
 *   follows at most one, binding it again replaces the binding.
 * animate: every listed rig is evaluated at its own time in ONE launch (a workgroup per rig), then every mesh bound to a listed rig
 *   is posed or morphed and refitted as by rfwhip_pose_mesh / rfwhip_morph_mesh — the same kernels, reading the rig's buffers — with
 *   the same ordering and the same bookkeeping: lights_follow_geometry and denoise_motion see an animated mesh as they see a posed
 *   one.  animations[i] == RFWHIP_RIG_BASE_POSE, or a rig without animations: the base pose.  A rig listed twice, a time that is not
 *   finite and a bound mesh that is not resident are refused before anything runs.  Per rig, 12 bytes travel to the device and none
 *   come back.  rfwhip_update() afterwards.
 *   The rule (all float32, every product and sum of a fixed shape, csrc/animation.h): per channel time = fmodf(time, last key) when
 *   time > last key > 0; the segment k = #{j in [1, n-2]: time > t_j}; f = (time - t_k) / (t_k+1 - t_k); one key or f <= 0: the first
 *   key's value; STEP key k, LINEAR (1 - f) a + f b, CUBICSPLINE the Hermite form with tangents scaled by t_k+1 - t_k; rotations per
 *   component, then normalised (no slerp); local = T R S M, world = world[parent] local, joint = inverse(world[mesh node])
 *   world[joint] inverseBind with the affine closed-form inverse.  A sampled rotation of zero norm and a mesh node of zero
 *   determinant give the identity and are counted in the status record.
 * read_rig: values of the last evaluation of the rig into out[0 .. cap) floats: RFWHIP_RIG_READ_TRS 10 per node (translation,
 *   rotation xyzw, scale), _WORLD 16 per node (column-major), _JOINTS the joint matrices of skin `index` (16 per joint, column-major),
 *   _WEIGHTS the weights of node `index`, _STATUS the 8 words of rfwhip_rig_status.  For tests, and for hosts that move INSTANCES by
 *   node animation: the top-level tree is built on the host, so such a host reads the node's world matrix and calls
 *   rfwhip_set_instance as before. */
RFWHIP_API int rfwhip_set_rig(rfwhip_context *ctx, size_t rig_index, const rfwhip_rig *rig);
RFWHIP_API int rfwhip_bind_rig(rfwhip_context *ctx, size_t rig_index, size_t skin_index, size_t node_index, size_t mesh_index);
RFWHIP_API int rfwhip_animate(rfwhip_context *ctx, const uint32_t *rigs, const uint32_t *animations, const float *times, size_t count);
RFWHIP_API int rfwhip_read_rig(rfwhip_context *ctx, size_t rig_index, int what, size_t index, float *out, size_t cap);
/* update(): once after a batch of set_* — builds the TLAS, uploads descriptors              context.h:108 */
RFWHIP_API int rfwhip_update(rfwhip_context *ctx);

/* ---- per-frame ---------------------------------------------------------------------------------------------- */
/* Camera::get_view() (Camera.cpp:74-88) as a free function; pure host arithmetic. */
RFWHIP_API void rfwhip_camera_get_view(const rfwhip_camera *camera, rfwhip_camera_view *view);
/* render_frame(const Camera&, RenderStatus) (context.h:94).  Enqueues `spp` samples per pixel on the context's
 * HIP stream and returns without a host sync; RESET clears the accumulator and the sample index, CONVERGE
 * accumulates (context.h:19-23, CUDART/src/Context.cpp:75-80). */
RFWHIP_API int rfwhip_render(rfwhip_context *ctx, const rfwhip_camera *camera, int status);
/* Block until every enqueued render has finished (the reference's render_frame ends with glFinish /
 * cudaDeviceSynchronize: the plugin shim calls rfwhip_render + rfwhip_wait). Resolves stage timings. */
RFWHIP_API int rfwhip_wait(rfwhip_context *ctx);

/* Present: accumulator / samples -> float4 RGBA rows, row 0 = top image row.
 * Full image on this rank (world == 1), host or device destination of width*height*4 floats. */
RFWHIP_API int rfwhip_read_framebuffer(rfwhip_context *ctx, float *rgba_host);
RFWHIP_API int rfwhip_read_framebuffer_device(rfwhip_context *ctx, void *rgba_device);
/* Multi-GPU: this rank's strips, compacted, padded to rfwhip_local_rows() rows (same on every rank). */
RFWHIP_API uint32_t rfwhip_local_rows(const rfwhip_context *ctx);
RFWHIP_API int rfwhip_read_local_framebuffer_device(rfwhip_context *ctx, void *rgba_device);
/* Root-side inverse of the strip interleave: gathered = [world][local_rows][width] float4 -> [height][width]. */
RFWHIP_API int rfwhip_deinterleave_device(rfwhip_context *ctx, const void *gathered_device, void *rgba_device);

/* Stream-ordered forms of the two calls above: enqueue only, no host synchronisation.  hip_stream is a hipStream_t of the
 * caller (e.g. torch's current stream); the present is ordered behind everything this context has enqueued and the
 * context's next rfwhip_render waits on the device until the present has read the accumulator. */
RFWHIP_API int rfwhip_read_local_framebuffer_stream(rfwhip_context *ctx, void *rgba_device, void *hip_stream);
RFWHIP_API int rfwhip_deinterleave_stream(rfwhip_context *ctx, const void *gathered_device, void *rgba_device,
										  void *hip_stream);

/* ---- display stage (no GL needed: the reference does these steps in its GL shaders) -------------------------------------
 * The presented linear float4 image -> something a host can show or save: the reference's ACES tone map with the camera's
 * brightness and contrast (rfw::system::render_frame(camera, status, toneMap), assets/shaders/tone-map.frag, system.cpp:682-711),
 * the FXAA of its window blit (assets/shaders/draw-tex-fxaa.vert:15-22, .frag:17-57), an optional sRGB encoding, and 8-bit
 * quantisation, in ONE kernel on the device (csrc/display.h has the formulas).  The stage always runs on the
 * FULL image — after the gather and after the denoiser, on the root — never on a rank's strips (FXAA needs a pixel's neighbours).
 * Every entry point above still returns linear float4; with the display settings at their defaults and none of the calls below
 * made, nothing changes.
 *   Settings (not listed by rfwhip_get_settings):
 *     display_tonemap = "aces" (default) | "none" (clamp to [0, 1] only)
 *     display_fxaa    = "0" | "1" (default)
 *     display_srgb    = "0" (default: the reference's bytes) | "1" (the sRGB OETF on the colour channels)
 *   Per colour channel x of a pixel: v = min(max(x - 0.5 contrast + 0.5 + brightness, 0), 65504); a NaN channel becomes 0; the upper
 *   clamp (our one deviation from the reference, for non-finite input only) keeps +inf finite.  alpha = clamp(in.w, 0, 1), untouched
 *   by FXAA and the encoding.  Brightness and contrast: the camera of the last rfwhip_render; before the first render the
 *   reference's defaults (0.05, 1; Camera.cpp:8-9) applied to the empty image.
 *   Formats: RGBA8 = 4 bytes per pixel, R in the lowest byte, each (int)rintf(c * 255); RGBA32F = the same values as 4 floats. */
enum rfwhip_display_format
{
	RFWHIP_DISPLAY_RGBA8 = 0,
	RFWHIP_DISPLAY_RGBA32F = 1
};
/* World-1 contexts: present -> denoise when on -> display, into host or device memory of width * height * (4 | 16) bytes.  The host
 * variant copies only the format's bytes. */
RFWHIP_API int rfwhip_read_display(rfwhip_context *ctx, int format, void *out_host);
RFWHIP_API int rfwhip_read_display_device(rfwhip_context *ctx, int format, void *out_device);
/* Stream-ordered: the stage on a full float4 image in device memory, enqueued on the caller's hipStream_t; nothing waits on the host.
 * A rfwhip_comm_* host calls it on the root behind rfwhip_comm_gather (ordered by the caller: rfwhip_comm_wait or an event).  The input
 * is read-only and in place is not allowed: rgba_device == out_device is RFWHIP_ERR_INVALID_ARGUMENT. */
RFWHIP_API int rfwhip_display_stream(rfwhip_context *ctx, const void *rgba_device, void *out_device, int format, void *hip_stream);
/* Known-answer hook, the counterpart of rfwhip_denoise_image: the stage on a host image of the context's target size with the
 * context's display settings and the given brightness and contrast. */
RFWHIP_API int rfwhip_display_image(rfwhip_context *ctx, const float *rgba_in, float brightness, float contrast, int format,
									void *out_host);

/* ---- exposure meter: the display stage measures the image it shows ------------------------------------------------------------
 * A luminance histogram of the image in front of the display kernel, a robust average of it, and a multiplicative exposure with
 * temporal adaptation: two small kernels on the device, stream-ordered, nothing read back (csrc/metering.h has the formulas;
 * DESIGN.md section 17).  Off by default: with display_exposure = "manual" and display_exposure_ev = 0 every entry point above
 * launches the kernels and returns the bits it did without the meter.
 *   Settings (not listed by rfwhip_get_settings):
 *     display_exposure        = "manual" (default) | "auto"
 *     display_exposure_ev     = stops, finite, in [-32, 32] (default 0); manual: E = 2^ev; auto: a compensation added to the target
 *     display_exposure_key    = the target key, a finite number > 0 (default 0.18)
 *     display_exposure_low / _high = the percentile window, 0 <= low < high <= 1 (defaults 0.1 / 0.9); a set that breaks the order is
 *                               refused and leaves both values unchanged
 *     display_exposure_speed  = the fraction of the way to the target per STEP, in (0, 1] (default 1 = immediate).  Per step, not
 *                               per second: the same calls give the same images
 *     display_exposure_min_ev / _max_ev = the clamp of the target, finite, in [-64, 64], min <= max (defaults -16 / 16)
 *   Per pixel: c = max(rgb, 0) (a NaN channel is 0), Y = 0.2126 r + 0.7152 g + 0.0722 b; valid iff 0 < Y < +inf, every other pixel
 *   counts as `excluded`.  bin = clamp((bits(Y) >> 20) - 888, 0, 255): 256 bins, 8 per octave over [2^-16, 2^16), linear inside an
 *   octave; bin b stands for lambda_b = (b >> 3) - 16 + log2(1 + ((b & 7) + 0.5) / 8) in log2 units.
 *   A STEP: N = valid pixels; the histogram's mass between low N and high N (a bin cut by an end counts with the part inside) gives
 *   lambda = the mean of lambda_b over it, in double.  No mass (no valid pixel): no step, the state stays.  Else, in float32:
 *     l_target = clamp(log2(key) - lambda + ev, min_ev, max_ev);  l = first step ? l_target : l + speed (l_target - l);  E = 2^l
 *   and the display's tone step sees x E per colour channel in place of x (alpha untouched).
 *   WHEN a step is taken (auto): rfwhip_read_display / _device meter the presented image behind the denoiser, in front of the display
 *   kernel, on the context's stream — ONE step per rfwhip_render call: a second read of the same frame returns the same bytes and
 *   leaves `steps` alone; a change of a display_exposure* setting meters the frame again.  rfwhip_display_stream and
 *   rfwhip_display_image show a caller's image: every call is one step on that image, on the given stream.
 *   rfwhip_group_read_display and rfwhip_group_present_display_async go through rfwhip_display_stream on the root: a group read or
 *   present is one step, nothing is read back to the host on that path, and frames in flight stay in flight.  RFWHIP_RESET does not
 *   reset the exposure (a camera move must not flash), neither does rfwhip_init; rfwhip_meter_reset does. */
#define RFWHIP_METER_BINS 256
typedef struct rfwhip_meter_stats /* 32 bytes: the record as it lies on the device */
{
	float exposure;		  /* E = 2^log2_exposure: 1 before any step; manual mode with ev != 0 writes 2^ev here when it displays */
	float log2_exposure;  /* l, after adaptation */
	float log2_target;	  /* l_target of the last step */
	float log2_luminance; /* lambda of the last step */
	uint32_t valid;		  /* pixels in the histogram of the last metered image */
	uint32_t excluded;	  /* ... and left out of it */
	uint32_t steps;		  /* steps taken since rfwhip_meter_reset (or the context's creation) */
	uint32_t reserved;
} rfwhip_meter_stats;
/* The record / the summed histogram of the last step (excluded may be null), after everything enqueued on the context's streams and
 * after a step enqueued on a caller's stream.  RFWHIP_ERR_STATE before rfwhip_init. */
RFWHIP_API int rfwhip_get_meter(rfwhip_context *ctx, rfwhip_meter_stats *stats);
RFWHIP_API int rfwhip_read_meter_histogram(rfwhip_context *ctx, uint32_t bins[RFWHIP_METER_BINS], uint32_t *excluded);
/* E = 1, steps = 0: the next step is a first step. */
RFWHIP_API int rfwhip_meter_reset(rfwhip_context *ctx);
/* Known-answer hooks, the counterparts of rfwhip_display_image, under the current settings.
 * rfwhip_meter_image: one step on a host image of the context's target size; bins (RFWHIP_METER_BINS words) may be null.
 * rfwhip_meter_histogram: the reduce alone (k_meter_reduce) on a caller's histogram, whose counts add up to at most 2^32 - 1. */
RFWHIP_API int rfwhip_meter_image(rfwhip_context *ctx, const float *rgba_in, rfwhip_meter_stats *stats, uint32_t *bins);
RFWHIP_API int rfwhip_meter_histogram(rfwhip_context *ctx, const uint32_t bins[RFWHIP_METER_BINS], uint32_t excluded,
									  rfwhip_meter_stats *stats);

/* ---- bloom: an HDR glow pyramid in front of the tone map -----------------------------------------------------------------------
 * With display_bloom = 1 every entry point of the display stage above (rfwhip_read_display*, rfwhip_display_stream,
 * rfwhip_display_image, the group's reads and presents) runs a chain of small kernels on the image it is about to show — behind the
 * meter's step, which sees the unbloomed image — and the display kernel reads the chain's image instead: highlights far above display
 * white bleed into their surroundings and stay readable as bright after the tone map clips them.  csrc/bloom.h has the formulas line
 * by line; DESIGN.md section 19.  Off by default: nothing is allocated, no bloom kernel runs, every byte is what it was.
 *   Settings (not listed by rfwhip_get_settings):
 *     display_bloom           = "0" (default) | "1"
 *     display_bloom_intensity = in [0, 16] (default 0.2): the weight of the glow added to the image
 *     display_bloom_threshold = a finite number >= 0 (default 1): in EXPOSED units, 1 = display white under any exposure
 *     display_bloom_knee      = in [0, 1] (default 0.5): the soft knee's half width as a fraction of the threshold
 *     display_bloom_scatter   = in [0, 1] (default 0.7): how much of the next coarser level a level takes on the way up
 *     display_bloom_levels    = a whole number in [1, 8] (default 6): levels of the pyramid; fewer when the image reaches 1 x 1 first
 *     display_bloom_time      (read-only, stage_timing = 1) kernel family 12 by kernel since its last reset: the milliseconds of
 *                               k_bloom_down0, k_bloom_down, k_bloom_up and k_bloom_apply, then their launches — eight numbers
 *   With E the exposure the display kernel applies (the meter record's, else 1), per colour channel c = min(max(x, 0), 65504) (a NaN
 *   channel is 0), T = threshold, K = knee T:
 *     br = E max(c.r, c.g, c.b); soft = clamp(br - T + K, 0, 2 K); g = max(soft^2 / (4 K + 1e-4), br - T) / max(br, 1e-4); p = c g
 *   Level k is W_k x H_k, W_0 = W, W_k = (W_{k-1} + 1) >> 1.  Level 1: texel (i, j) = the source texels (2i - 1 .. 2i + 2) x
 *   (2j - 1 .. 2j + 2), edge-clamped, weights h (x) h with h = (1, 3, 3, 1) / 8 times the tap's 1 / (1 + luminance(p)), normalised (one
 *   firefly does not flash a blob).  Level k + 1 from level k: the same taps, plain weights.  On the way up, k = levels - 1 .. 1:
 *   U_k = D_k + scatter (up(U_{k+1}) - D_k), up = two taps per axis with weights (1/4, 3/4) or (3/4, 1/4).  Then
 *   out.rgb = c + intensity up(U_1), out.a = in.a bit for bit.  The chain runs on the stream of the call; a call on another stream
 *   than the previous one waits for that chain and its display kernel first (the pyramid and the bloomed image belong to the context).
 * Known-answer hooks.  rfwhip_bloom_image: the chain alone (whatever display_bloom says) on a host image of the target's size under the
 * exposure E = `exposure` (finite, >= 0) and the current display_bloom_* settings -> the linear float4 image the display kernel would read.
 * rfwhip_read_bloom_level: U_level of the last chain, level in 1 .. the levels it ran; *w, *h = its size (either may be null); `out`
 * holds `cap` floats and needs 4 w h (null: the size alone).  RFWHIP_ERR_STATE when no chain has run since rfwhip_init. */
RFWHIP_API int rfwhip_bloom_image(rfwhip_context *ctx, const float *rgba_in, float exposure, float *rgba_out);
RFWHIP_API int rfwhip_read_bloom_level(rfwhip_context *ctx, int level, float *out, size_t cap, uint32_t *w, uint32_t *h);

/* ---- colour grading and dither: white balance, CDL, a 3D LUT, ordered dither ------------------------------------------------------
 * With display_grade = 1 every entry point of the display stage above launches ONE kernel, k_display_graded, in place of the display
 * kernel — behind the meter's step and the bloom chain, which see the ungraded image; nothing is read back.  csrc/display_grade.h has
 * the work items; DESIGN.md section 20.  Off by default: nothing is allocated, no new kernel runs, every byte is what it was.
 *   Settings (not listed by rfwhip_get_settings):
 *     display_grade            = "0" (default) | "1"
 *     display_wb_temperature   = T in kelvin in [1667, 25000] (default 6500): the light the image was lit by; below 6500 = a warmer
 *                                light, the image moves towards blue
 *     display_grade_slope / display_grade_offset / display_grade_power = one number for the three channels or three "r g b"
 *                                (defaults 1 / 0 / 1); slope finite and >= 0, offset finite, power finite and > 0; read back as three
 *     display_grade_saturation = in [0, 4] (default 1)
 *     display_dither           = "0" (default) | "1": ordered dither of the RGBA8 output; RGBA32F ignores it
 *     display_lut              (read-only) the size n of the LUT set with rfwhip_set_display_lut, 0 without one
 *     display_grade_time       (read-only, stage_timing = 1) kernel family 13 since its last reset: the milliseconds of
 *                                k_display_graded, then its launches
 *   A value that does not parse or lies outside its range is refused and the setting keeps its value.
 *   Per texel, with E the exposure the display kernel would apply (the meter record's; without one nothing is multiplied):
 *     x    <- x E
 *     LINEAR, when the white balance, a CDL channel or the saturation is not at its identity (else x goes to the tone step as it is):
 *       c    = min(max(x, 0), 65504) per colour channel (max = fmaxf: a NaN channel is 0); alpha is untouched throughout
 *       WB   c <- M_wb c, row i: fmaf(M_i2, c_b, fmaf(M_i1, c_g, M_i0 c_r)); M_wb is built in double and stored as float32
 *       CDL  c_i <- powf(max(fmaf(c_i, slope_i, offset_i), 0), power_i), for every channel whose three parameters are not (1, 0, 1);
 *            power_i = 1: the clamped value itself, without a powf
 *       SAT  Y = fmaf(0.0722, c_b, fmaf(0.7152, c_g, 0.2126 c_r));  c_i <- fmaf(sat, c_i - Y, Y)
 *     TONE v = the tone step of rfwhip_read_display above on the result (brightness / contrast, aces | none, clamp to [0, 1])
 *     LUT  v <- clamp(tetra(L, v), 0, 1), when a LUT is set (entries outside [0, 1], a look's overshoot, are accepted; what the
 *          step hands on is clamped, so FXAA, the encoding and the bytes see values in [0, 1] as without a LUT)
 *     FXAA, ENCODE as above, on the graded values
 *     DITHER (RGBA8, display_dither = 1): byte = clamp(rint(255 v + d(x, y) - 0.5), 0, 255) for r, g, b, ties to even, decided without a
 *          rounding of 255 v + d; alpha as without.  d(x, y) = (B + 0.5) / 256, B = the 16 x 16 Bayer index of (x & 15, y & 15): with
 *          q = x ^ y, bit b (0 .. 3) of q is bit 2 (3 - b) + 1 of B and bit b of y is bit 2 (3 - b); the 2 x 2 case is [[0, 2], [3, 1]].
 *          The same pattern for the three channels, a pure function of the pixel: two reads of a frame are equal.
 *   A step at its identity (T = 6500; slope 1, offset 0, power 1 of a channel; saturation 1; no LUT; dither 0; no E) is skipped, not
 *   multiplied through: display_grade = 1 with everything at its default is bit for bit display_grade = 0, for every input.
 *   WHITE BALANCE.  The white point (x_T, y_T) of T on the Planckian locus (Kim et al.'s cubic splines):
 *     x = -0.2661239e9 / T^3 - 0.2343589e6 / T^2 + 0.8776956e3 / T + 0.179910      T <= 4000
 *         -3.0258469e9 / T^3 + 2.1070379e6 / T^2 + 0.2226347e3 / T + 0.240390      T >  4000
 *     y = -1.1063814 x^3 - 1.34811020 x^2 + 2.18555832 x - 0.20219683              T <= 2222
 *         -0.9549476 x^3 - 1.37418593 x^2 + 2.09137015 x - 0.16748867              2222 < T <= 4000
 *          3.0817580 x^3 - 5.87338670 x^2 + 3.75112997 x - 0.37001483              T >  4000
 *     XYZ_T = (x / y, 1, (1 - x - y) / y);  rho = B XYZ;  M_wb = M_xyz->rgb B^-1 diag(rho_6500 / rho_T) B M_rgb->xyz
 *     B = the Bradford matrix (0.8951, 0.2664, -0.1614; -0.7502, 1.7135, 0.0367; 0.0389, -0.0685, 1.0296), M_rgb->xyz = linear Rec.709 / D65
 *     (0.4124564, 0.3575761, 0.1804375; 0.2126729, 0.7151522, 0.0721750; 0.0193339, 0.1191920, 0.9503041), M_xyz->rgb its inverse.
 *     The reference white is the locus point of 6500 K itself: the default is exactly the identity (the step is skipped).  One
 *     parameter: tint, a white point off the locus, is not supported.
 *   LUT.  L = n^3 RGB float triples, 2 <= n <= 65, red fastest (the order of a .cube file), uploaded once as float4.  tetra, per colour:
 *     p = v (n - 1) per channel; i = min((int)p, n - 2); f = p - i; the three fractions in descending order f_a >= f_b >= f_c, ties in
 *     channel order r, g, b; V0 = L[i], V1 = the lattice point one step along axis a, V2 = one further step along b,
 *     V3 = L[i + (1, 1, 1)]; w = (1 - f_a, f_a - f_b, f_b - f_c, f_c); out = fmaf(w3, V3, fmaf(w2, V2, fmaf(w1, V1, w0 V0))).
 *     A lattice colour, 1.0 included, returns its entry bit for bit whenever n - 1 is a power of two.
 * rfwhip_set_display_lut: rgb = n^3 triples; null or n = 0 removes the LUT.  A non-finite entry or n outside [2, 65]:
 * RFWHIP_ERR_INVALID_ARGUMENT, the old LUT stays.  In a group the LUT belongs to the root's context (rfwhip_group_set_display_lut;
 * in a process that does not hold the root the call does nothing and returns RFWHIP_OK).
 * rfwhip_set_display_lut_cube: the same from the text of a .cube file — LUT_3D_SIZE n (required, once), optional TITLE and "#"
 * comments, DOMAIN_MIN 0 0 0 / DOMAIN_MAX 1 1 1 the only domains accepted, then exactly n^3 lines of three numbers; a 1D LUT, any
 * other keyword or another count is refused and the old LUT stays.
 * rfwhip_get_display_lut: *n = the size (0: none; may be null); `rgb` holds `cap` floats and needs 3 n^3 (null: the size alone).
 * Known-answer hook rfwhip_grade_colors: `count` RGB triples through k_kat_grade under the current settings (whatever display_grade
 * says) — which = 0: the LINEAR block on linear colours; 1: tetra on display colours, clamped to [0, 1] first, its result NOT clamped (without a LUT:
 * the colours themselves).  RFWHIP_ERR_STATE before rfwhip_init. */
RFWHIP_API int rfwhip_set_display_lut(rfwhip_context *ctx, const float *rgb, uint32_t n);
RFWHIP_API int rfwhip_set_display_lut_cube(rfwhip_context *ctx, const char *text, size_t len);
RFWHIP_API int rfwhip_get_display_lut(rfwhip_context *ctx, float *rgb, size_t cap, uint32_t *n);
RFWHIP_API int rfwhip_grade_colors(rfwhip_context *ctx, int which, size_t count, const float *rgb_in, float *rgb_out);

/* ---- baseline JPEG: the presented 8-bit frame, encoded on the device (csrc/display_jpeg.h) ------------------
 * The display stage ends at an RGBA8 image in device memory; these calls encode that image as a baseline JPEG (T.81, JFIF) on the
 * device, so that a host copies the few hundred kilobytes a browser, an MJPEG stream or a file takes as they are instead of 4
 * bytes per pixel.  Four kernels behind the display kernel on the same stream (kernel family 14), nothing read back by the chain;
 * off unless one of these calls is made: nothing is allocated before, and no other kernel changes.  Unlisted settings (a value out of
 * range or not a whole number is RFWHIP_ERR_INVALID_ARGUMENT and the setting keeps its value):
 *     display_jpeg_quality      1 .. 100, default 90 (the IJG scale)
 *     display_jpeg_subsampling  "444" | "420", default 420
 *     display_jpeg_restart      Ri, the MCUs per restart interval, 1 .. 65535, default 8
 *     display_jpeg_bytes        (read-only) the length of the last stream this library read back to the host, 0 before
 *     display_jpeg_time         (read-only, stage_timing = 1) kernel family 14 by kernel since its last reset: the milliseconds of
 *                               k_jpeg_blocks, k_jpeg_entropy, k_jpeg_offsets, k_jpeg_pack, then their launches
 * THE STREAM is defined in integers; an implementation of this text agrees with the device byte for byte.
 *   Input: W x H RGBA8, row 0 first, R in the lowest byte; alpha is ignored.  W, H <= 65535.
 *   MCU = 8 x 8 pixels ("444") or 16 x 16 ("420"); the image is extended to whole MCUs by clamping the pixel coordinates.
 *   Colour (JFIF, full range):  Y = (19595 R + 38470 G + 7471 B + 32768) >> 16,  Cb = (-11059 R - 21709 G + 32768 B + 8421375) >> 16,
 *     Cr = (32768 R - 27439 G - 5329 B + 8421375) >> 16;  "420": Cb and Cr are 2 x 2 box means (a + b + c + d + 2) >> 2.
 *     Blocks of an MCU: Y ("420": top-left, top-right, bottom-left, bottom-right), Cb, Cr.
 *   DCT: K[u][x] = round(8192 a(u) cos((2 x + 1) u pi / 16)), a(0) = sqrt(1 / 8), a(u > 0) = 1 / 2;  X = block - 128;
 *     T = (K X + 512) >> 10 (arithmetic shift);  S = T K^T = 2^16 x T.81's FDCT; everything fits int32.
 *   Quantisation: q = sgn(S) ((|S| + (Q << 15)) / (Q << 16)), integer division; Q = the entry of T.81 Annex K.1 (luminance for Y,
 *     chrominance for Cb, Cr) scaled by the quality: s = 5000 / quality below 50, else 200 - 2 quality; Q = clamp((base s + 50) / 100, 1, 255).
 *   Entropy coding: baseline Huffman with the Annex K.3 tables; DC differences per component with the predictor 0 at the start of
 *     every restart interval; AC run / size with ZRL and EOB (no EOB when coefficient 63 is non-zero); a negative value v is coded
 *     as v - 1 in `size` bits; a 0x00 behind every 0xFF byte of entropy data.
 *   Restart intervals: Ri MCUs each in raster order; every interval is padded to a byte with 1-bits; interval i is followed by
 *     FF D0 + (i mod 8), the last one by EOI.
 *   Header (613 bytes, built by the host): SOI; APP0 "JFIF" 1.01, units 0, density 1 : 1, no thumbnail; one DQT with tables 0 and 1
 *     in zigzag order; SOF0 (precision 8, H, W, components 1 / 2 / 3 with sampling 0x11 or 0x22 for Y and 0x11 for the others,
 *     tables 0 / 1 / 1); one DHT (DC0, AC0, DC1, AC1); DRI; SOS (1:00 2:11 3:11, 0, 63, 0).
 * rfwhip_display_jpeg_bound: the capacity that always suffices for the target size under the current settings: 613 + 416 per block
 *   (a block's code is at most 1658 bits, every byte of it may be stuffed) + 2 per interval.
 * rfwhip_read_display_jpeg (world 1): present -> denoise when on -> display (RGBA8, as rfwhip_read_display) -> encode; the host waits
 *   for the 32-byte record, then copies exactly *bytes.  *bytes (may be null) is the stream's length also when it did not fit: a `cap`
 *   below it is RFWHIP_ERR_INVALID_ARGUMENT with the needed size in the message, and nothing is written to out_host.
 * rfwhip_display_jpeg_stream: the four kernels, stream-ordered on `hip_stream`, on a W x H RGBA8 image in device memory (the output
 *   of rfwhip_display_stream) -> the stream in out_device (cap >= 613 bytes) and the record in record_device (32 bytes); when the
 *   stream exceeds cap nothing is written behind the header and the record's overflow is 1.  The kernels share one scratch per
 *   context: an encode enqueued on another stream first waits, on the host, for the previous one.
 * rfwhip_get_jpeg: the record of the last stream this library read back.
 * Hooks: rfwhip_jpeg_image encodes a host RGBA8 image of the target's size; rfwhip_read_jpeg_coefficients copies the quantised
 *   blocks of the last encode — *blocks of them (may be null), 64 int16 each in zigzag order, in stream order (MCU by MCU); out null:
 *   the count alone; cap_blocks too small: RFWHIP_ERR_INVALID_ARGUMENT. */
typedef struct rfwhip_jpeg_stats /* 32 bytes: the record as it lies on the device */
{
	uint32_t bytes;			/* the whole stream: header, entropy data, markers, EOI */
	uint32_t intervals;		/* restart intervals */
	uint32_t mcus, blocks;	/* MCUs and 8 x 8 blocks coded */
	uint32_t stuffed_bytes; /* 0x00 bytes behind an 0xFF */
	uint32_t overflow;		/* 1: bytes > cap, nothing was written behind the header */
	uint32_t header_bytes;	/* 613 */
	uint32_t reserved;
} rfwhip_jpeg_stats;
RFWHIP_API int rfwhip_display_jpeg_bound(rfwhip_context *ctx, size_t *bytes);
RFWHIP_API int rfwhip_read_display_jpeg(rfwhip_context *ctx, void *out_host, size_t cap, size_t *bytes);
RFWHIP_API int rfwhip_display_jpeg_stream(rfwhip_context *ctx, const void *rgba8_device, void *out_device, size_t cap, void *record_device,
										   void *hip_stream);
RFWHIP_API int rfwhip_get_jpeg(rfwhip_context *ctx, rfwhip_jpeg_stats *stats);
RFWHIP_API int rfwhip_jpeg_image(rfwhip_context *ctx, const void *rgba8_in, void *out_host, size_t cap, size_t *bytes);
RFWHIP_API int rfwhip_read_jpeg_coefficients(rfwhip_context *ctx, int16_t *out, size_t cap_blocks, uint32_t *blocks);

/* ---- image textures: JPEG decode and the mip chain on the device (csrc/texture_decode.h) ---------------------
 * In the reference a texture file is decoded, flipped, linearised and given its mip chain by rfw::texture (texture.cpp of the system
 * layer, FreeImage); a backend sees texels only (rfwhip_set_textures).  These calls take the file instead: the bytes of a baseline
 * JPEG, or a PNG's RGBA8 pixels, and build the texture's slot of the one texel table on the device (kernel family 15).  Level 0 of a
 * JPEG never crosses the bus as texels.
 * ACCEPTED STREAMS  SOF0, or SOF1 with 8-bit samples and Huffman coding; 1 component, or 3 in one interleaved scan with luma sampling
 *   1x1, 2x1 or 2x2 over chroma 1x1; 8-bit quantisation tables; up to four DC and four AC Huffman tables in any number of DHT segments;
 *   DRI or none; APPn, COM and fill bytes are skipped.  Everything else (progressive, arithmetic, 12-bit, 4 components, several scans,
 *   other sampling, an APP14 that declares RGB or CMYK) is RFWHIP_ERR_UNSUPPORTED with a message naming the form; a malformed stream
 *   is RFWHIP_ERR_INVALID_ARGUMENT.
 * THE DECODE is defined in integers (an implementation of this text agrees with the device, and with the common decoders' defaults,
 *   byte for byte):
 *   Coefficients: blocks of 64 int16 in zigzag order, MCU by MCU: the luma blocks row by row, then Cb, Cr.  The entropy data of a
 *     stream with restart intervals is decoded on the device, a lane per interval; of a stream without on the host (one interval is
 *     serial), its coefficients uploaded.  Setting texture_entropy = auto | host | device forces either; both give the same words.
 *   Inverse DCT: dequantise; the 13-bit-constant "slow integer" transform (even part from 4433, 6270, 15137; odd part from 2446, 3196,
 *     7373, 9633, 12299, 16069, 16819, 20995, 25172), columns first with a descale by 11 bits, rows with 18, each rounding half up;
 *     + 128; clamp.  All in wrapping 32-bit arithmetic.
 *   Chroma: the component at its own size ceil(w / 2) x ceil(h / 2), edges replicated.  2x2: v = 3 near + far vertically, then
 *     (3 this + left + 8) >> 4 for even and (3 this + right + 7) >> 4 for odd columns.  2x1: (3 this + left + 1) >> 2 and
 *     (3 this + right + 2) >> 2.  A component at most 2 columns wide is replicated instead.
 *   Colour, with FIX(x) = int(x 65536 + 0.5), Cb and Cr centred on 0:  R = Y + ((FIX(1.402) Cr + 32768) >> 16),
 *     B = Y + ((FIX(1.772) Cb + 32768) >> 16),  G = Y + ((-FIX(0.34414) Cb + 32768 - FIX(0.71414) Cr) >> 16), clamped; grey: R = G = B = Y;
 *     alpha 255.  Then the flags (rfwhip_abi.h): flip, linearise.  Texel = r | g << 8 | b << 16 | a << 24.
 *   Mips: five levels (MIPLEVELCOUNT), level i is (w >> i) x (h >> i), back to back behind level 0; a colour channel is the truncated
 *     quarter of the aligned 2 x 2 quad's sum, alpha the minimum of the four (construct_mipmaps, texture.cpp:163-209).
 * rfwhip_set_texture_sources: rfwhip_set_textures for mixed sources (replaces rfw::texture's constructors, texture.cpp:16-138): parses
 *   every header, lays out the one table, uploads TEXELS entries as they are, decodes and mips the others on the context's stream.
 *   All or nothing: on any error the previous textures stay in place and the message names the texture's index.
 * rfwhip_image_info (host only; replaces FreeImage's header queries, texture.cpp:34-49): RFWHIP_OK with supported = 1, or with
 *   supported = 0 and the reason for a well-formed stream of a form not decoded here; RFWHIP_ERR_INVALID_ARGUMENT for a malformed one.
 * rfwhip_get_texture_decode: the record of texture `index` of the current table (zeros for a TEXELS entry); alpha_zero is what the
 *   reference derives HAS_ALPHA from (texture.cpp:52-58).  index = (size_t)-1: the record of the last rfwhip_decode_image.
 * rfwhip_read_texture: all levels of one texture, *texels of them (may be null; 4 bytes each, 16 for a FLOAT4 texture); out null: the
 *   count alone; cap_texels too small: RFWHIP_ERR_INVALID_ARGUMENT.
 * rfwhip_png_unfilter (host only; replaces FreeImage's PNG reader, texture.cpp:41): undoes PNG's row filters — `rows` scanlines of a
 *   filter byte and row_bytes bytes each -> the rows alone; bpp = bytes per whole pixel.
 * Hooks: rfwhip_decode_image decodes level 0 alone into host memory (cap_texels too small or out null: *w, *h alone) and needs no
 *   scene; rfwhip_read_texture_coefficients copies the coefficients of the last decode, as rfwhip_read_jpeg_coefficients does.
 * Unlisted settings: texture_entropy; texture_decode_time (read-only, stage_timing = 1): family 15 by kernel — the milliseconds of
 *   k_texdec_zero, k_texdec_entropy, k_texdec_idct, k_texdec_color, k_tex_mips, k_texdec_finish, then their launches. */
enum rfwhip_texture_decode_error
{
	RFWHIP_TEXDEC_ERR_TRUNCATED = 1, /* an interval's data ended inside a code */
	RFWHIP_TEXDEC_ERR_RUN = 2,		 /* a zero run past coefficient 63 */
	RFWHIP_TEXDEC_ERR_NOCODE = 4,	 /* 16 bits that are no code of the table */
	RFWHIP_TEXDEC_ERR_MARKER = 8	 /* an 0xFF inside an interval that is not followed by 0x00 */
};
typedef struct rfwhip_texture_decode_record /* 32 bytes: the record as it lies on the device */
{
	uint32_t width, height;
	uint32_t blocks, intervals; /* 8 x 8 blocks and restart intervals decoded (0 for RGBA8 and TEXELS) */
	uint32_t errors;			/* rfwhip_texture_decode_error bits, ORed over the intervals */
	uint32_t alpha_zero;		/* level-0 texels with alpha 0 */
	uint32_t path;				/* 0: nothing to decode, 1: entropy decoding on the host, 2: on the device */
	uint32_t reserved;
} rfwhip_texture_decode_record;
typedef struct rfwhip_image_info_t
{
	uint32_t width, height, components;
	uint32_t h_sampling, v_sampling; /* of the luma component: 1 1, 2 1 or 2 2 */
	uint32_t restart_interval;		 /* Ri in MCUs, 0 without DRI */
	uint32_t intervals;
	uint32_t supported;
	char reason[96]; /* empty when supported */
} rfwhip_image_info_t;
RFWHIP_API int rfwhip_set_texture_sources(rfwhip_context *ctx, const rfwhip_texture_source *sources, size_t count);
RFWHIP_API int rfwhip_image_info(const void *data, size_t bytes, rfwhip_image_info_t *info);
RFWHIP_API int rfwhip_get_texture_decode(rfwhip_context *ctx, size_t index, rfwhip_texture_decode_record *record);
RFWHIP_API int rfwhip_read_texture(rfwhip_context *ctx, size_t index, void *out, size_t cap_texels, size_t *texels);
RFWHIP_API int rfwhip_png_unfilter(const uint8_t *in, size_t rows, size_t row_bytes, size_t bpp, uint8_t *out);
RFWHIP_API int rfwhip_decode_image(rfwhip_context *ctx, const void *data, size_t bytes, uint32_t flags, void *out_rgba8_host, size_t cap_texels,
								   uint32_t *w, uint32_t *h);
RFWHIP_API int rfwhip_read_texture_coefficients(rfwhip_context *ctx, int16_t *out, size_t cap_blocks, uint32_t *blocks);

/* ---- the sky's loaders: Radiance HDR files, and the alias table of sky_sampling on the device ----------------------------------
 * (csrc/sky_load.h, kernel family 17)  rfw::skybox::load reads a .hdr file through FreeImage; a host of this
 * library hands over the file's bytes and the device decodes them into the sky.
 * rfwhip_set_sky_hdr(ctx, data, bytes, flags): the file `data` becomes the sky, as rfwhip_set_sky does for finished texels.
 *   Accepted: the magic "#?RADIANCE" or "#?RGBE", header lines up to a blank one, among them FORMAT=32-bit_rle_rgbe (EXPOSURE= is
 *   reported by rfwhip_hdr_info and not applied, the rest is skipped), the resolution line "-Y H +X W", and per scanline either
 *   new-style RLE (2 2 hi lo with hi lo = W, for 8 <= W <= 32767: four component planes of count bytes, above 128 a run of
 *   count - 128, otherwise `count` literal bytes, none across a plane's end) or W flat RGBE quadruples; the two may mix in a file.
 *   A texel is rgb = mantissa * 2^(e - 136), all three 0 when e = 0 (FreeImage's rgbe_RGBEToFloat), w = 0: exact in float.  Row 0
 *   of the sky is the file's first scanline (what the reference's loader has after flipping FreeImage's bottom-up bitmap);
 *   RFWHIP_SKYSRC_FLIP_ROWS turns the rows over.
 *   Not decoded — RFWHIP_ERR_UNSUPPORTED, the message names the form: other orientations (+Y, X-major), 32-bit_rle_xyze, old-style
 *   run pixels (1 1 1 n).  Malformed — RFWHIP_ERR_INVALID_ARGUMENT, the message names the scanline: a count byte of 0, a run or
 *   literal that overruns its plane, a scanline header whose width is not W, a buffer that ends early, a header without a blank
 *   line.  The call is all or nothing: whatever it answers but RFWHIP_OK, the previous sky is in place.
 * rfwhip_hdr_info (host only): width, height, the product of the EXPOSURE lines, whether any scanline is RLE, supported and the
 *   reason; RFWHIP_OK with supported = 0 for a form that is not decoded, RFWHIP_ERR_INVALID_ARGUMENT for a malformed file.
 * rfwhip_read_sky: the sky's texels back to the host, 4 floats each (r, g, b, 0); out null: *width, *height alone.
 *
 * sky_table = "host" (default) | "device" (unlisted): who builds the alias table of sky_sampling = 1.  "host": the sky is read
 *   back, one core runs Walker / Vose, the table goes up — every byte and every image as before.  "device": seven kernels on the
 *   context's stream and a 32-byte record back.  With n = W H, w_k = lum_k omega_row(k) (double; lum = 0.2126 r + 0.7152 g +
 *   0.0722 b, 0 when negative or NaN; omega the row's solid angle from the host), S = sum w, mu = S / n, texel k heavy when w_k > mu,
 *   d_k = max(mu - w_k, 0), e_k = max(w_k - mu, 0) and D, E their inclusive prefix sums:
 *     light k: a = the first index with E_a > D_k - d_k: keep = (float)(w_k / mu), alias = a; no such a (rounding): keep = 1,
 *              alias = k — or, for w_k = 0, keep = 0, alias = the heaviest texel;
 *     heavy k: nxt = the first index with E_nxt > E_k, i = the first index with D_i >= E_k: keep = (float)clamp(1 - (D_i - E_k) / mu,
 *              0, 1), alias = nxt; either missing: keep = 1, alias = k.
 *   Every alias is a heavy texel; a texel of weight 0 has keep = 0 and is nobody's alias: it is never drawn.  Sums and prefix sums
 *   have a fixed shape (no atomics; csrc/sky_load.h), the prefix sums are non-decreasing by construction.  The table describes the
 *   same distribution as the host's, not the same bytes.  S = 0 or not finite: no table and p = 0, as with "host".
 * rfwhip_read_sky_table: the current table (sky_sampling = 1; built now if a setting or the sky changed since the last update) and
 *   its record; out null or cap too small: *entries and the record alone.  A host-built table reports S and RFWHIP_SKYTAB_VALID only.
 * rfwhip_sky_alias_from_weights (hook): the total, scan and assign stages over n given weights (negative or NaN: 0), n < 2^31.
 * sky_load_time (read-only, stage_timing = 1): family 17 by kernel — the milliseconds of k_skyhdr_planes, k_skyhdr_texels,
 *   k_skytab_weights, k_skytab_total, k_skytab_scan_block, k_skytab_scan_super, k_skytab_scan_top, k_skytab_scan_apply,
 *   k_skytab_assign, then their launches. */
enum rfwhip_sky_hdr_error /* what k_skyhdr_planes flags (the host's walk refuses the same streams before any launch) */
{
	RFWHIP_SKYHDR_ERR_ZERO = 1,	   /* a count byte of 0 */
	RFWHIP_SKYHDR_ERR_OVERRUN = 2, /* a run or literal past the plane's W bytes */
	RFWHIP_SKYHDR_ERR_TRUNCATED = 4 /* the plane's bytes ended early */
};
enum rfwhip_sky_table_flags
{
	RFWHIP_SKYTAB_VALID = 1, /* S is positive and finite: there is a table */
	RFWHIP_SKYTAB_DEVICE = 2 /* built by the kernels: heaviest, light and heavy are filled */
};
typedef struct rfwhip_hdr_info_t
{
	uint32_t width, height;
	float exposure; /* the product of the header's EXPOSURE lines (1 without one); not applied */
	uint32_t rle;	/* some scanline is run-length encoded */
	uint32_t supported;
	char reason[96]; /* empty when supported */
} rfwhip_hdr_info_t;
typedef struct rfwhip_sky_table_record /* 32 bytes: the record as it lies on the device */
{
	double S;			/* the sum of the weights */
	uint32_t heaviest;	/* the first texel of the largest weight */
	uint32_t light;		/* texels with w <= mu */
	uint32_t heavy;		/* texels with w > mu */
	uint32_t flags;		/* rfwhip_sky_table_flags */
	uint32_t reserved[2];
} rfwhip_sky_table_record;
RFWHIP_API int rfwhip_set_sky_hdr(rfwhip_context *ctx, const void *data, size_t bytes, uint32_t flags);
RFWHIP_API int rfwhip_hdr_info(const void *data, size_t bytes, rfwhip_hdr_info_t *info);
RFWHIP_API int rfwhip_read_sky(rfwhip_context *ctx, float *out_rgba, size_t cap_texels, uint32_t *width, uint32_t *height);
RFWHIP_API int rfwhip_read_sky_table(rfwhip_context *ctx, rfwhip_sky_alias *out, size_t cap_entries, size_t *entries, rfwhip_sky_table_record *record);
RFWHIP_API int rfwhip_sky_alias_from_weights(rfwhip_context *ctx, const double *weights, size_t n, rfwhip_sky_alias *table_out,
											 rfwhip_sky_table_record *record_out);

/* ---- noise estimate: when has a progressive render converged? ---------------------------------------------------------------
 * With noise_estimate = 1 the resolve of every rfwhip_render (its variant k_resolve_noise) keeps two floats per pixel beside the
 * accumulator — sumY, the sum of the luminance Y = 0.2126 r + 0.7152 g + 0.0722 b of the pixel's samples (a sample's value is what
 * the resolve adds to the accumulator for it), and M2 = sum (Y - mean)^2, updated per call in the shifted, mergeable form
 * (csrc/noise.h has the formulas).  The framebuffer is bit-identical with the setting on and off; the moments
 * are cleared wherever the accumulator is (RFWHIP_RESET, rfwhip_init) and begin with the first RESET or rfwhip_init after the
 * setting came on.  With it off nothing is allocated and no other kernel runs.
 *   Settings (not listed by rfwhip_get_settings):
 *     noise_estimate  = "0" (default) | "1"
 *     noise_floor     = a finite number > 0 (default 0.01): added to the mean, so that a black pixel has a finite error
 *     noise_threshold = a finite number > 0 (default 0.05): a pixel has converged when its error is at most this
 *   Per pixel, n >= 2 samples (n is the context's sample count since the last RESET, one number for all pixels):
 *     mean = sumY / n,  var = M2 / (n - 1),  e = sqrt(var / n) / (mean + noise_floor)
 *   the standard error of the mean relative to the mean; e = FLT_MAX where a moment is not finite (a NaN or infinite sample): such a
 *   pixel never converges.
 *   Tiles: 32 x 8 pixels, aligned to the ownership strips, so a tile belongs to one rank; a partial tile counts its real pixels. */
typedef struct rfwhip_noise_stats
{
	uint64_t samples;	/* n: the context's sample count since the RESET (with adaptive_sampling too, where a tile's own count is n_tile) */
	uint64_t pixels;	/* pixels judged (a rank: the pixels of its strips) */
	uint64_t converged; /* ... of which e <= threshold */
	double mean_error;	/* sum of e / pixels */
	float max_error;
	float threshold;	/* noise_threshold as it was applied */
} rfwhip_noise_stats;
typedef struct rfwhip_noise_tile
{
	float sum_e; /* over the tile's pixels, at most FLT_MAX */
	float max_e;
	uint32_t pixels;
	uint32_t converged;
} rfwhip_noise_tile;
/* Two kernels on the context's stream behind the last render — per-pixel error and per-tile records, then ONE workgroup that folds
 * the tile records in index order (no float atomics: the same state gives the same bytes) — and a wait for the 32 bytes of the
 * result; the map stays on the device.  RFWHIP_ERR_STATE when noise_estimate is off (or came on after the accumulation began) or
 * n < 2.  A rank of a strip split answers for its own strips: rfwhip_group_get_noise adds the ranks' answers; a rfwhip_comm_* host
 * (one process per device) adds its ranks' records itself — pixels, converged and mean_error * pixels are sums, max_error a maximum. */
RFWHIP_API int rfwhip_get_noise(rfwhip_context *ctx, rfwhip_noise_stats *stats);
/* World-1 contexts: e of every pixel, width * height floats, row 0 first. */
RFWHIP_API int rfwhip_read_noise_map(rfwhip_context *ctx, float *e);
/* The tile records of this rank, row-major: tiles_x = ceil(width / 32), tiles_y = this rank's padded rows / 8 (world 1:
 * ceil(height / 8)).  cap = records the array holds; too few: RFWHIP_ERR_INVALID_ARGUMENT. */
RFWHIP_API int rfwhip_read_noise_tiles(rfwhip_context *ctx, rfwhip_noise_tile *records, size_t cap, uint32_t *tiles_x, uint32_t *tiles_y);
/* Test hook, world-1 contexts: the two moments of every pixel, width * height floats each. */
RFWHIP_API int rfwhip_read_noise_moments(rfwhip_context *ctx, float *sumY, float *m2);
/* Known-answer hooks, the counterparts of rfwhip_display_image: the product's kernels on the caller's data, whatever the context
 * renders and whether or not noise_estimate is on.
 * rfwhip_noise_merge: one call's update of `pixels` pixels that hold n_a samples with the moments sumY_a / m2_a, on S given sample
 * values per pixel (samples_rgb: pixels x S x 3 floats, a pixel's samples in order).
 * rfwhip_noise_image: the metric on given moments of a width x height image of its own size, with n samples per pixel and the
 * context's noise_floor / noise_threshold; e_map (width * height floats) and tiles (ceil(width / 32) * ceil(height / 8) records)
 * may be null. */
RFWHIP_API int rfwhip_noise_merge(rfwhip_context *ctx, size_t pixels, uint32_t n_a, const float *sumY_a, const float *m2_a, uint32_t S,
								  const float *samples_rgb, float *sumY_out, float *m2_out);
RFWHIP_API int rfwhip_noise_image(rfwhip_context *ctx, uint32_t width, uint32_t height, uint32_t n, const float *sumY, const float *m2,
								  rfwhip_noise_stats *stats, float *e_map, rfwhip_noise_tile *tiles);

/* ---- adaptive sampling: samples only where the noise estimate asks for them ---------------------------------------------------
 * With adaptive_sampling = 1 (beside noise_estimate = 1, pt integrator) every 32 x 8 noise tile of a rank carries a sample count n_tile
 * and an active flag; RFWHIP_RESET and rfwhip_init set n_tile = 0 and active = 1.  A render call of S = spp samples traces primary
 * paths only for the pixels of active tiles and adds S to their n_tile; the sample indices are what they are without the setting
 * (a retired pixel does not draw the indices of the calls it sits out), so an active pixel's accumulator, moments and error are, bit
 * for bit, those of the same calls with the setting off.  Calls since the RESET are numbered 1, 2, ..; after call k with
 * k % adaptive_every == 0 a DECISION is taken on the device: an active tile retires when n_tile >= adaptive_min_samples and every
 * real pixel of it has e <= noise_threshold (its record has converged == pixels).  A RETIRED TILE STAYS RETIRED until the next RESET
 * or rfwhip_init, whatever noise_threshold, noise_floor or adaptive_min_samples do later: its accumulator, moments and error are
 * frozen.  The mask a call uses is a function of the state after the call before it and of nothing else — no scheduling setting
 * (ring, streams, overlap, sub_batch_paths, fuse, refill, group_flags, sample_group) and no pipelining of rfwhip_render calls changes
 * a bit of any image.  Stopping a tile by an estimate made of the very samples it is judged by biases its mean slightly (DESIGN.md
 * section 15); adaptive_min_samples is the guard.
 *   Settings (not listed by rfwhip_get_settings):
 *     adaptive_sampling    = "0" (default) | "1"; like the moments it takes effect — on AND off — with the next RESET or
 *                            rfwhip_init.  "1" without noise_estimate = 1 is RFWHIP_ERR_STATE, and so is noise_estimate = 0 while
 *                            this is on or while the accumulation in progress is an adaptive one
 *     adaptive_min_samples = integer >= 2 (default 16); read at every decision: a new value holds from the next decision on
 *     adaptive_every       = integer in [1, 64] (default 4): render calls between two decisions; read after every call (a
 *                            decision follows call k when k % adaptive_every == 0 with the value as it stands then)
 *   rfwhip_render with integrator = parity returns RFWHIP_ERR_STATE while the setting is on.
 *   Every presented image (rfwhip_read_framebuffer*, the local / stream forms, the group's and a comm host's gathers, and with them
 *   the denoiser and the display stage) scales a pixel by 1 / n_tile, the float32 quotient 1.0f / (float)n_tile (0 for 0).
 *   rfwhip_get_noise and the noise reads use n_tile per tile; rfwhip_noise_stats::samples stays the context's count since the RESET.
 *   rfwhip_read_primary_hits reports prim -2 ("not sampled in the last call") and t 1e34 for the pixels of retired tiles;
 *   rfwhip_get_probe_results keeps its last valid answer when the probe pixel was not sampled.
 *   The queries below return RFWHIP_ERR_STATE unless the accumulation in progress is an adaptive one (the setting was on at the last
 *   RESET / rfwhip_init). */
typedef struct rfwhip_adaptive_stats
{
	uint64_t tiles;			  /* tiles of this rank with at least one real pixel */
	uint64_t active_tiles;
	uint64_t pixels;		  /* real pixels of those tiles */
	uint64_t active_pixels;
	uint64_t samples_taken;	  /* sum over tiles of n_tile x real pixels */
	uint64_t samples_uniform; /* samples since the RESET x pixels: what the same calls take without the setting */
} rfwhip_adaptive_stats;
/* Waits for the calls enqueued so far and reads the tiles' 5 bytes each. */
RFWHIP_API int rfwhip_get_adaptive(rfwhip_context *ctx, rfwhip_adaptive_stats *stats);
/* n_tile and the active flag of every tile of this rank, row-major, tiles_x x tiles_y as rfwhip_read_noise_tiles (the tiles of the
 * padded rows below the image included).  cap = tiles the arrays hold; too few: RFWHIP_ERR_INVALID_ARGUMENT. */
RFWHIP_API int rfwhip_read_adaptive_tiles(rfwhip_context *ctx, uint32_t *n, uint8_t *active, size_t cap, uint32_t *tiles_x, uint32_t *tiles_y);
/* Known-answer hook: forces the mask.  active = one byte per tile in the order of rfwhip_read_adaptive_tiles, count = their number;
 * a 0 retires the tile now, a non-zero byte leaves it as it is — flags only clear, a retired tile stays retired.  Waits for the
 * calls enqueued so far. */
RFWHIP_API int rfwhip_adaptive_set_tiles(rfwhip_context *ctx, const uint8_t *active, size_t count);

/* Where a context runs and what it renders into (for hosts that move its strips themselves). */
RFWHIP_API int rfwhip_get_placement(rfwhip_context *ctx, int *device_ordinal, int *rank, int *world);
RFWHIP_API int rfwhip_get_target_size(rfwhip_context *ctx, uint32_t *width, uint32_t *height);

/* ---- multi-GPU below this ABI (no counterpart in the reference, which renders on one device) ------------
 * The frame is split into interleaved 8-row strips over `world` devices of one node, each device holds the whole scene,
 * and per presented frame the rank-local strips are gathered ONCE into the root's (rank 0's) HBM and de-interleaved
 * there.  Transport: RCCL point-to-point over xGMI (ncclSend on every rank, world - 1 ncclRecv on the root, one
 * ncclGroup), or peer copies (hipMemcpyPeerAsync).  Everything below is enqueue-only unless it says it waits.
 *
 * rfwhip_group_*: ONE process, ONE thread drives n devices — the reference's host model (RFW/system/src/rfw/app.cpp:3-26).
 *   create   n contexts, context i = rank i of world n on devices[i]; a device may be listed more than once only with the
 *            peer transport (tests on one GPU).  AUTO = RCCL when the devices are distinct and librccl.so opens.
 *   context  the i-th context, for the scene calls: the host repeats every rfwhip_set_* per context (each device keeps
 *            its own copy of the scene), then calls rfwhip_group_update.
 *   init / update / set_setting / render / wait   the context call of the same name on every rank.
 *   gather   present on every rank -> transfer -> de-interleave into the group's full image on the root's device.
 *   read_framebuffer   gather + wait + copy to the host: width * height float4.
 *   framebuffer_device the root-side image (valid after a gather has completed) and the device it lives on. */
enum rfwhip_transport
{
	RFWHIP_TRANSPORT_AUTO = 0,
	RFWHIP_TRANSPORT_RCCL = 1,
	RFWHIP_TRANSPORT_PEER = 2
};
typedef struct rfwhip_group rfwhip_group;
RFWHIP_API int rfwhip_group_create(const int *devices, int n, int transport, rfwhip_group **out);
RFWHIP_API void rfwhip_group_destroy(rfwhip_group *group);
RFWHIP_API int rfwhip_group_size(const rfwhip_group *group);
RFWHIP_API int rfwhip_group_transport(const rfwhip_group *group);
RFWHIP_API rfwhip_context *rfwhip_group_context(rfwhip_group *group, int rank);
RFWHIP_API int rfwhip_group_init(rfwhip_group *group, uint32_t width, uint32_t height);
RFWHIP_API int rfwhip_group_update(rfwhip_group *group);
RFWHIP_API int rfwhip_group_set_setting(rfwhip_group *group, const char *key, const char *value);
RFWHIP_API int rfwhip_group_render(rfwhip_group *group, const rfwhip_camera *camera, int status);
RFWHIP_API int rfwhip_group_gather(rfwhip_group *group);
RFWHIP_API int rfwhip_group_wait(rfwhip_group *group);
RFWHIP_API int rfwhip_group_read_framebuffer(rfwhip_group *group, float *rgba_host);
RFWHIP_API int rfwhip_group_framebuffer_device(rfwhip_group *group, void **rgba_device, int *device_ordinal);
/* Pipelined presentation (frames in flight): present_async = gather + asynchronous copy of the image into one of
 * RFWHIP_PRESENT_SLOTS pinned host buffers, enqueue only; present_wait blocks until that slot's copy has landed and hands out
 * the buffer (valid until the slot is presented into again).  A host that keeps n <= RFWHIP_PRESENT_SLOTS frames in flight —
 * render(k), present_async(k % n), present_wait((k + 1) % n) from frame n - 1 on — shows frame k - n + 1 while frames up to
 * k render: a frame's launch chain is ten dependent kernels of tails, and it takes about four chains in flight to fill the
 * device (1080p, 1 spp, image on the host every frame: 2.76 ms per frame with render + wait + read-back, 2.14 ms with two
 * frames in flight, 1.70 ms with four). */
#define RFWHIP_PRESENT_SLOTS 4
RFWHIP_API int rfwhip_group_present_async(rfwhip_group *group, int slot);
RFWHIP_API int rfwhip_group_present_wait(rfwhip_group *group, int slot, const float **rgba_host);
/* The display stage for a group (see rfwhip_read_display): read_display = gather + display on the root + wait + copy of the format's
 * bytes.  present_display_async / _wait are present_async / _wait with the display stage behind the gather: the same slots, streams
 * and events, and the copy carries the display image (a quarter of the float image's bytes for RGBA8).  A slot remembers what was
 * last presented into it: rfwhip_group_present_wait on a slot that holds a display image, and rfwhip_group_present_display_wait on
 * one that holds a float image, return RFWHIP_ERR_STATE. */
/* The noise estimate of the whole image (see rfwhip_get_noise): every rank reduces its own strips on its device, the root adds the
 * ranks' records in rank order on the host — counts exactly, the sum of errors in double, the maximum of the maxima. */
RFWHIP_API int rfwhip_group_get_noise(rfwhip_group *group, rfwhip_noise_stats *stats);
/* Adaptive sampling of the whole image (see rfwhip_get_adaptive): tiles and their decisions are per rank; the ranks' records are
 * added in rank order. */
RFWHIP_API int rfwhip_group_get_adaptive(rfwhip_group *group, rfwhip_adaptive_stats *stats);
/* The exposure meter of a group (see rfwhip_get_meter): the root's record — the root shows the gathered image, so its meter is the
 * group's.  Waits for the steps of the reads and presents enqueued so far. */
RFWHIP_API int rfwhip_group_get_meter(rfwhip_group *group, rfwhip_meter_stats *stats);
/* The LUT of the display stage (rfwhip_set_display_lut above), for the root's context: the display kernel runs there. */
RFWHIP_API int rfwhip_group_set_display_lut(rfwhip_group *group, const float *rgb, uint32_t n);
/* rfwhip_set_texture_sources on every member: each decodes its own replica of the table on its own device.  The sources are parsed by
 * every member alike, so a refused table is refused by all of them and every member keeps its previous one. */
RFWHIP_API int rfwhip_group_set_texture_sources(rfwhip_group *group, const rfwhip_texture_source *sources, size_t count);
/* rfwhip_set_sky_hdr on every member: each decodes its own replica of the sky on its own device; a refused file is refused by all. */
RFWHIP_API int rfwhip_group_set_sky_hdr(rfwhip_group *group, const void *data, size_t bytes, uint32_t flags);
/* rfwhip_set_rig / rfwhip_bind_rig / rfwhip_animate on every member: each evaluates its own copy of the rig on its own device, as
 * rfwhip_group_update does for the scene; nothing crosses the gather.  A refused rig or call is refused by all. */
RFWHIP_API int rfwhip_group_set_rig(rfwhip_group *group, size_t rig_index, const rfwhip_rig *rig);
RFWHIP_API int rfwhip_group_bind_rig(rfwhip_group *group, size_t rig_index, size_t skin_index, size_t node_index, size_t mesh_index);
RFWHIP_API int rfwhip_group_animate(rfwhip_group *group, const uint32_t *rigs, const uint32_t *animations, const float *times, size_t count);
RFWHIP_API int rfwhip_group_set_display_lut_cube(rfwhip_group *group, const char *text, size_t len);
RFWHIP_API int rfwhip_group_read_display(rfwhip_group *group, int format, void *out_host);
RFWHIP_API int rfwhip_group_present_display_async(rfwhip_group *group, int slot, int format);
RFWHIP_API int rfwhip_group_present_display_wait(rfwhip_group *group, int slot, const void **out_host, int *format);
/* Baseline JPEG for a group (see rfwhip_read_display_jpeg): read_display_jpeg = gather + display (RGBA8) + encode on the root + wait
 * + copy of the record, then of exactly *bytes.  present_jpeg_async / _wait use the slots of present_async: the async call enqueues
 * gather, display, encode and the copy of the 32-byte record and of as many bytes as the last stream had plus an eighth (one byte
 * per pixel the first time); the wait blocks for the record, then hands exactly *bytes of the slot's stream to out_host — from
 * the pinned copy, or with a second copy when the stream is longer than the guess (cap bytes; a smaller cap: RFWHIP_ERR_INVALID_ARGUMENT with the needed size, the slot stays
 * presented).  A slot remembers which of the three kinds was presented into it; waiting for another kind is RFWHIP_ERR_STATE. */
RFWHIP_API int rfwhip_group_read_display_jpeg(rfwhip_group *group, void *out_host, size_t cap, size_t *bytes);
RFWHIP_API int rfwhip_group_present_jpeg_async(rfwhip_group *group, int slot);
RFWHIP_API int rfwhip_group_present_jpeg_wait(rfwhip_group *group, int slot, void *out_host, size_t cap, size_t *bytes);

/* rfwhip_comm_*: one process per device (e.g. under torch.distributed.run).  Rank 0 calls rfwhip_comm_unique_id and
 * hands the RFWHIP_COMM_ID_BYTES bytes to the other ranks by any means (a file, MPI, a torch broadcast); then EVERY rank
 * calls rfwhip_comm_create with its context (rank / world as given to rfwhip_create) — a collective call, like
 * ncclCommInitRank.  rfwhip_comm_gather is collective too: every rank presents and sends, the root receives and
 * de-interleaves into rgba_device (width * height float4 on its device; ignored on the other ranks; NULL = an internal
 * buffer).  The transport is RCCL; nothing but the id travels outside this library.  A world of ONE needs no id (the gather is a
 * copy); given one all the same, rfwhip_comm_create builds a real one-rank RCCL communicator and the gather sends the strips to
 * itself through it (ncclSend + ncclRecv on rank 0): the library's RCCL calls exercised on a box with a single device. */
#define RFWHIP_COMM_ID_BYTES 128
typedef struct rfwhip_comm rfwhip_comm;
RFWHIP_API int rfwhip_comm_unique_id(void *id, size_t cap);
RFWHIP_API int rfwhip_comm_create(rfwhip_context *ctx, const void *id, rfwhip_comm **out);
RFWHIP_API void rfwhip_comm_destroy(rfwhip_comm *comm);
RFWHIP_API int rfwhip_comm_gather(rfwhip_comm *comm, void *rgba_device);
RFWHIP_API int rfwhip_comm_wait(rfwhip_comm *comm);

/* get_probe_results / set_probe_index                                                       context.h:104,109 */
RFWHIP_API int rfwhip_set_probe_index(rfwhip_context *ctx, uint32_t x, uint32_t y);
RFWHIP_API int rfwhip_get_probe_results(rfwhip_context *ctx, uint32_t *instance_index, uint32_t *primitive_index,
										float *distance);
/* get_stats()                                                                               context.h:110 */
RFWHIP_API int rfwhip_get_stats(rfwhip_context *ctx, rfwhip_render_stats *stats);

/* get_settings / set_setting (context.h:106-107). Keys:
 *   integrator   = "parity" (restates EmbreeRT/src/Context.cpp:104-300) | "pt" (CUDART/src/Kernels.cu:571-794)
 *   spp          = samples per pixel enqueued by one rfwhip_render call (default 1)
 *   max_depth    = MAX_PATH_LENGTH of the pt integrator (settings.h:5, default 2)
 *   jitter       = "xor128" (EmbreeRT: rfw::utils::xor128 stream) | "center" (r0=r1=0.5) — parity integrator only
 *   builder      = "host" (parallel binned SAH on the CPU, the default) | "device" (on the GPU, lbvh.hip: 63-bit Morton
 *                  order, parallel locally-ordered clustering (PLOC), device collapse to 4-wide nodes; applies to the next
 *                  rfwhip_set_mesh that (re)builds)
 *   sampler      = "hash" (WangHash + xorshift32, tools.h:218-235; default) | "bluenoise" (needs rfwhip_set_blue_noise)
 *                  — pt integrator: primary rays (dimensions 0-3, Kernels.cu:391-394) and, for the first 256 samples, the
 *                  light sample of next-event estimation (dimensions 4-5, Kernels.cu:712-719)
 *   stage_timing = "0"|"1": bracket every stage with hipEvents (fills RenderStats like the reference's timers)
 *   count_traversal = "0"|"1": instrumented traversal (popped inner nodes / triangle tests), for the roofline
 *   lds_nodes    = top-of-tree 4-wide nodes of the largest mesh BVH that every traversal workgroup keeps in LDS
 *                  (-1 = as many as the kernels were built for, the default; 0 disables)
 *   streams      = sub-batches of one render call that run concurrently on their own HIP streams (1..8, default 4)
 *   overlap      = "1": the connection (shadow) wave of depth d runs on a second stream beside extend / shade of depth d + 1
 *                  (hides kernel tails when launches are small); "0": in order on the sub-batch's stream; "-1" (default):
 *                  chosen by the size of the render call
 *   sub_batch_paths = a render call's spp are cut into concurrent sub-batches only if each gets at least this many path
 *                  slots and there are four of them (default 50000000: 1080p from 128 spp per call).  A call below the
 *                  threshold stays ONE sub-batch and rotates through the ring (below) — whose depth in turn depends on the
 *                  device's FREE memory (232 B of path state + 32 B of radiance per slot and ring entry: 1080p at 64 spp =
 *                  35 GB per entry; the ring falls back 3 -> 2 -> 1 before the call fails), so what this setting does to
 *                  throughput depends on how much HBM the rest of the process holds
 *   sample_group = slot layout: up to this many samples of a pixel sit side by side in one wave (power of two <= 64,
 *                  default 64 = a wave is one pixel; the largest such group that divides every sub-batch of a call is
 *                  used: 32 for a 128-spp call cut into four sub-batches; 1 = a wave is one 8x8 tile of one sample).
 *                  Changes which path sits where, never the image
 *   flat_instances = "1" (default): an instance with the identity transform whose mesh no other instance uses is linked
 *                  into the top-level tree directly (rays reach its triangles without an instance switch; hit records,
 *                  images and counters are unchanged), and static instances that are transformed or share their mesh are
 *                  written out in world space under one tree (the WORLD TREE, flatten_bytes); "0": every instance behind
 *                  a top-level leaf, the reference's two-level walk.  Takes effect with the next rfwhip_update()
 *   flatten_bytes = default 268435456 (2.4 M triangles): the world tree is built as long as the world-space copy of its members'
 *                  triangles (every instance of a host-built mesh that is not animated) stays below this many bytes; "0":
 *                  never.  The tree is built on the host INSIDE rfwhip_update() whenever its members change (~0.2 s per million
 *                  member triangles on 16 cores): raise the budget for large static scenes, lower it where updates must stay
 *                  short.  The hit is the same triangle of the same instance at the same t as the two-level walk's up to
 *                  rounding (M p is tested instead of M^-1 o; the triangle test's determinant threshold is scaled by |det M|,
 *                  so a triangle is rejected as degenerate exactly when the reference's object-space test rejects it).
 *                  Animated meshes always keep the two-level walk; an instance whose matrix changes leaves the tree and
 *                  rejoins after 8 updates without a change — 16, 32 ... after every further episode
 *   arm          = retired (round 4's self-arming primary kernels): accepted and ignored
 *   ring         = render calls that are ONE sub-batch rotate through this many sets of wave buffers / streams / counters,
 *                  so that up to `ring` consecutive calls are in flight (1..4, default 3: three chains + the main stream
 *                  are the HIP runtime's four hardware queues; a host that keeps four frames in flight with
 *                  rfwhip_group_present_async sets 4)
 *   refill       = bit mask, default 15: bit 0 the extension (bounce) waves, bit 1 the shadow waves keep persistent lanes (a
 *                  lane that finishes its ray pulls the next one from the wave's run of the launch's queue; off: the
 *                  one-ray-per-lane kernels, kept as a cross-check); bit 3: the pt primary wave in PACKET form — a wave walks
 *                  the tree once for the rays of its 64 slots (scalar node fetches, one stack per wave; used when the samples
 *                  of a pixel sit side by side, sample_group >= 2, or the launch is large, and only for scenes whose trees fit
 *                  its 61-entry stack; hit records are those of the per-lane kernels; off: one ray per lane).  Bit 2 selected
 *                  a persistent-lane primary kernel until round 5 and is ignored
 *   fuse         = "1" (default): the extension rays of depth d + 1 and the shadow rays of depth d share ONE launch (both
 *                  queues are complete when the shade stage of depth d has finished; one kernel tail per depth instead of
 *                  two: 1-spp frames 1.34 -> 1.21 ms); "0": a launch each.  Never changes the image
 *   shadow_packets = "-1" (default) | "1" | "0": the connection wave of the PRIMARY vertices in packet form — their shadow rays
 *                  carry the chosen light's bin in the top bits of their slot word, a wave sorts runs of 256 rays by it and walks
 *                  the tree once per 64 rays (wave-uniform occlusion traversal) instead of once per lane; applies where the pt
 *                  primary wave can run in packet form and the samples of a pixel sit side by side (sample_group >= 8); 16 bins up
 *                  to 2^27 path slots per sub-batch, 8 / 4 / 2 for larger ones.  "-1": while the sorted runs of the last waited frame hold at most
 *                  8 light bins on average (read-only key "shadow_bins_per_run"; "shadow_packets_on" says what the next call
 *                  will do; measured: 3.6 bins per run + 8 %, 5.5 bins + 0.6 %).  Never changes the image
 *   group_flags  = "1" (default): the packet form of the pt primary wave flags the 64-slot groups it has finished itself (no hit:
 *                  sky terms written) in a byte each, and the shade kernel's scan passes them by without reading their records
 *                  (a quarter of the terrain's groups).  "0": every record is read.  Never changes the image
 *   shadow_side  = "1" (default): that wave runs on the sub-batch's connection stream, beside the extension wave of depth 1;
 *                  "0": on the sub-batch's own stream, in front of it (per-stage timings)
 *   denoise      = "0" (default) | "1": the presented FULL image is denoised (the reference's OptiX 6 DENOISE setting,
 *                  OptiX6Context/src/OptiXContext.cpp:812-822, as a native filter) — rfwhip_read_framebuffer / _device of a world-1
 *                  context, the group's image after every gather (rfwhip_group_gather / read_framebuffer / framebuffer_device /
 *                  present_async: on the root's device and stream), the root's image after rfwhip_comm_gather (the ROOT's setting
 *                  decides).  Strip-local reads (rfwhip_read_local_framebuffer_*, rfwhip_deinterleave_*) are never denoised.  Only
 *                  output is filtered: the accumulator keeps the raw samples (CONVERGE goes on accumulating them) and "0" gives the
 *                  raw image back bit for bit.  Buffers of the full image, allocated when the setting is first turned on and freed
 *                  by rfwhip_cleanup / rfwhip_init: guides 2 x 16 B, irradiance 2 x 16 B, variance 2 x 4 B per pixel (1080p: 149 MB).
 *                  The algorithm, term by term (csrc/denoise.h, DESIGN.md "Denoiser"):
 *                  GUIDES: one ray per pixel from the pixel centre and the lens centre, the path tracer's closest-hit traversal; at
 *                  the hit the shade kernel's surface, material colour and texture layers: albedo = material colour after textures,
 *                  normal = shading normal after normal maps, flipped to face the camera (octahedral, 2 x snorm16), z = distance
 *                  along the ray, grad z = central differences of z in x and y (one-sided at borders / next to invalid pixels).
 *                  A pixel is INVALID when its ray misses, meets an emitter (a colour component > 1) or passes more than 8
 *                  alpha-tested layers (pass-through as in the path tracer: on from I + 1e-5 D).  The guides are recomputed only
 *                  when the camera of the last render (by value), the scene (any rfwhip_update) or the target size changed.
 *                  Reads with "1": before the first rfwhip_render (since init) the empty image is returned unfiltered; when the
 *                  guides are stale AND the scene has changed since the last rfwhip_update (set_* calls not yet committed), the
 *                  read fails with RFWHIP_ERR_STATE, as a render would — current guides are used while such calls are pending.  A
 *                  traversal-stack overflow of the guide pass fails rfwhip_read_framebuffer* / rfwhip_read_denoise_guides (its own
 *                  counter: the render's statistics are not touched).
 *                  FILTER (SVGF's spatial filter, Schied et al. HPG 2017; its temporal stage: "denoise_temporal"), valid pixels p:
 *                    a_p = max(albedo_p, 1e-3) per channel, I_p = c_p / a_p, l = 0.2126 r + 0.7152 g + 0.0722 b of I;
 *                    var_p = sum_q w_q (l_q - m)^2 / sum_q w_q, m = sum_q w_q l_q / sum_q w_q over the valid q of the 3 x 3
 *                      neighbourhood, w_q = w_z(s = 1) w_n;
 *                    pass i = 0 .. iterations - 1, s = 2^i, taps q = p + s (dx, dy), dx, dy in -2..2, valid and inside the image:
 *                      w = h(dx) h(dy) w_z w_n w_l, h = (1, 4, 6, 4, 1) / 16,
 *                      w_z = exp(-|z_p - z_q| / (sigma_depth |s (dx grad_x z_p + dy grad_y z_p)| + 1e-4)),
 *                      w_n = max(0, n_p . n_q)^sigma_normal,
 *                      w_l = exp(-|l_p - l_q| / (sigma_luminance sqrt(g_p) + 1e-10)), g_p = sum k(dx) k(dy) var_q / sum k(dx) k(dy)
 *                        over the valid q of the 3 x 3 neighbourhood (step 1), k = (1, 2, 1) / 4;
 *                      I'_p = sum w I_q / sum w, var'_p = sum w^2 var_q / (sum w)^2, l'_p = lum(I'_p);
 *                    last pass: out_p = I'_p a_p, out_p.w = c_p.w.  Invalid pixels: out = c bit for bit, never a neighbour.
 *                  Fixed tap order, no atomics, no communication between workgroups: the output depends on the image and the guides
 *                  only — the same whichever rank, group or context produced the image
 *   denoise_iterations = a-trous passes, 1..8 (default 5)
 *   denoise_sigma_luminance / denoise_sigma_normal / denoise_sigma_depth = the filter's edge-stopping parameters (SVGF's defaults:
 *                  4 / 128 / 1)
 *   denoise_temporal = "0" (default) | "1": SVGF's temporal stage, a reprojected history of the presented frames.
 *                  SAMPLE ORIGIN: with "1" a RESET render sets o = S mod 256, S = samples per pixel this context has rendered since
 *                  rfwhip_init; the pt integrator's sample indices run o + samples_done + ... (with "0", o = 0: reset frames of one
 *                  camera are identical).  Every rank renders the same counts: o, and so the image, is independent of the world size.
 *                  The stage runs once per PRESENTED frame F: the first denoised world-1 read after a render, each group gather
 *                  (frames in flight included), each rfwhip_comm_gather on the root.  Further reads of the same frame return the
 *                  same bits (two history sets; a read runs the stage again from P's set into F's) while the scene is unchanged:
 *                  an rfwhip_update after F was presented traces F's guides again against the new scene, and a further read of F
 *                  (or rfwhip_read_denoise_history) then filters with those.  P = the previous presented
 *                  frame.  The HISTORY IS USABLE when a frame P has been presented since the history was cleared, the size is
 *                  P's, and a RESET render came after P (a CONVERGE accumulator holds P's samples).  Cleared by rfwhip_init,
 *                  rfwhip_cleanup and by turning "denoise" or "denoise_temporal" on.  It follows the demodulation above:
 *                    I_p = c_p / a_p, l_p = lum(I_p).  REPROJECTION: X = pos_F + z_p D_p (D_p the guide's centre ray); the ray
 *                    pos_P -> X meets P's image plane (p1, right, up) at p1 + u right + v up, s > 0 (X in front of P);
 *                    (x', y') = (u W - 0.5, v H - 0.5); the 4 bilinear taps q of (x', y'), each CONSISTENT when: its weight > 0,
 *                    inside the image, P's guide at q valid, P's guide saw the same instance as p, that instance (transform,
 *                    mesh, its rebuild / refit / pose / morph) unchanged by every rfwhip_update since P's guides,
 *                    |z_P(q) - |X - pos_P|| <= 2 (|dz/dx_P(q)| + |dz/dy_P(q)|) + 0.01 |X - pos_P|, n_p . n_P(q) >= 0.9.  The
 *                    consistent weights are renormalised; their sum < 0.01 (or no usable history): p is FRESH.
 *                    BLEND, fresh: n = 1, I~ = I, mu1 = l, mu2 = l^2 (no history is read); else with the renormalised weights
 *                    H, (m1, m2), n_P = sum w (history colour, moments, length) at q, n = min(n_P + 1, 64), a = max(alpha, 1 / n),
 *                    I~ = (1 - a) H + a I, mu1 = (1 - a) m1 + a l, mu2 = (1 - a) m2 + a l^2.
 *                    VARIANCE: n >= 3.99 (4, with a margin for the rounding of the weighted n_P): var = max(0, mu2 - mu1^2);
 *                    else the 3 x 3 estimate above (from I).
 *                    The passes above then run on (I~, lum(I~), var) unchanged.  HISTORY written: the demodulated output of
 *                    pass 0 (the colour), (mu1, mu2), n, F's guides and instance ids, F's camera; invalid pixels store n = 0
 *                    (and their output is c bit for bit, as above).  A fresh frame (the first, after a cut, any CONVERGE frame)
 *                    is the spatial filter's output bit for bit.  Moving or deforming instances are not reprojected: they restart,
 *                    unless "denoise_motion".
 *                  Root-only buffers, allocated when the setting is turned on: 16 B (P's guides) + 2 x 4 B (instance ids) +
 *                  2 x 28 B (history) per pixel.  rfwhip_denoise_image stays spatial-only.
 *   denoise_alpha = SVGF's alpha in (0, 1] for colour and moments (default 0.2)
 *   denoise_motion = "0" (default) | "1", meaningful with denoise = 1 and denoise_temporal = 1 (inert otherwise): a pixel whose
 *                  instance moved or deformed since P is reprojected through the previous position of its own surface point
 *                  instead of restarting.  "0": every image, every history value and the kernels launched are those of
 *                  denoise_temporal alone.  Turning it on clears the history (as "denoise" and "denoise_temporal" do).
 *                  For the stage of a new presented frame F the host puts every instance into one of three STATES:
 *                    STILL: unchanged by every rfwhip_update since P's guides (the test above).  Its pixels take the path above,
 *                      X = pos_F + z_p D_p: a frame in which nothing moved has the bits of "0".
 *                    MOVED: changed, and all of: used at P's guides and at F's; the same mesh index; the mesh's build is the one
 *                      P's guides saw (no rebuild since: refits, poses and morphs keep it.  As rfwhip_set_mesh's refit path does,
 *                      equal vertex and triangle counts are taken to mean the same triangles: vertex j of triangle k now is
 *                      vertex j of triangle k then, and the indices are read as they are now); the history is usable; P's
 *                      transform is known (P's guide pass ran with the setting on); the current vertices are the ones F's guide
 *                      pass traced; P's vertex positions are available: either the mesh was not edited between the two guide
 *                      passes (they are the current ones), or the context's ONE snapshot of the mesh is P's.  The snapshot
 *                      (16 B per vertex, root only, only for meshes edited in place) is copied on the context's stream in front
 *                      of the first rfwhip_pose_mesh / rfwhip_morph_mesh / same-topology rfwhip_set_mesh that follows a
 *                      presented frame, when the vertices are still the ones that frame's guide pass traced, and is tagged with
 *                      that frame; nothing is copied or allocated while the setting is off.
 *                    RESTART: anything else (a rebuilt mesh, another mesh, a new instance, a snapshot that is not P's).  Its
 *                      pixels are fresh, as above.
 *                  A pixel p of a MOVED instance, with the primitive k and barycentrics (u, v) of the hit the guide pass kept
 *                  (after its alpha pass-through layers; w = 1 - u - v on vertex 0, u on vertex 1, v on vertex 2), a_j the current
 *                  object-space vertices of triangle k, b_j the ones at P's guides, M_F / M_P the instance's transform at F's / P's
 *                  guides:
 *                    X_P = M_P (w b_0 + u b_1 + v b_2) replaces X in the REPROJECTION above (the intersection with P's image
 *                      plane, the 4 taps, |X_P - pos_P| in the depth test); inside / valid / same-instance / depth tests unchanged;
 *                    the normal test is n'_p . n_P(q) >= 0.9 with p's normal carried back by the triangle's own deformation:
 *                      A_j = M_F a_j, B_j = M_P b_j, e_1 = A_1 - A_0, e_2 = A_2 - A_0, N_a = normalize(e_1 x e_2), f_1, f_2, N_b
 *                      likewise from B, d = |f_1 x f_2|, c = (e_1 . n_p, e_2 . n_p, N_a . n_p),
 *                      n'_p = normalize((c_1 (f_2 x N_b) + c_2 (N_b x f_1)) / d + c_3 N_b)  (= F^-T n_p for the linear map F
 *                      taking (e_1, e_2, N_a) to (f_1, f_2, N_b); for a rigid motion, the rotation);
 *                    a degenerate current or previous triangle (d = 0, |e_1 x e_2| = 0, anything not finite): p is fresh.
 *                  Blend, variance, history writes and the passes are unchanged.  Lighting that moves with the object (shadows,
 *                  reflections) is left to alpha and the luminance moments, as in SVGF.
 *                  A FURTHER READ of F uses F's table again while neither an rfwhip_update nor a mesh edit (set_mesh, pose,
 *                  morph) followed F's presentation; after one, every instance that is not STILL restarts in such a read (the
 *                  current vertices and the snapshot may belong to another frame; they are never read then).
 *                  Root-only buffers: 16 B per pixel (primitive, u, v of the guide pass; allocated when the setting is turned on
 *                  with denoise_temporal, freed with the other denoiser buffers), 144 B per instance (the stage's table).
 *   sky_sampling = "0" (default: the sky is found only by BSDF-sampled rays that miss) | "1": the pt integrator's next-event
 *                  estimation importance-samples the sky.  The table is built by rfwhip_update, or by the next render after the
 *                  setting changed, from the sky of the last update, when the sky or the setting changed; it is allocated only
 *                  while the setting is on (8 B per texel).  The parity integrator ignores it and sky_pick.
 *                  TEXELS, as the pt integrator reads the sky: column i of W covers phi in [-pi + 2 pi i / W, -pi + 2 pi (i + 1) / W),
 *                    phi = atan2(D.x, -D.z); row j of H covers theta in [pi j / H, pi (j + 1) / H), theta = acos(D.y);
 *                    Omega_ij = (2 pi / W) (cos theta_j - cos theta_{j+1}); lum_ij = max(0, 0.2126 r + 0.7152 g + 0.0722 b)
 *                    (NaN and negative texels weigh 0); S = sum lum_ij Omega_ij (in double); P_ij = lum_ij Omega_ij / S.
 *                  DENSITY per steradian: pdf_sky(D) = lum(texel(D)) / S — 0 for a black texel and for a direction the
 *                    integrator reads as black.
 *                  SAMPLE: a texel (i, j) with probability P_ij (Walker / Vose alias table), then a, b uniform:
 *                    phi = -pi + 2 pi (i + a) / W, cos theta = cos theta_j - b (cos theta_j - cos theta_{j+1}),
 *                    D = (sin theta sin phi, cos theta, -sin theta cos phi).
 *                  ESTIMATOR, p = the sky's share (sky_pick), at a non-specular vertex with throughput T and survival factor
 *                    s = min(1, max(T)) (the one its BSDF continuation divides by): q1 < p samples the sky with (q0, q1 / p)
 *                    (the bucket's row and column; the alias coin and a, b come from the path's hash state), else a light with
 *                    (q0, (q1 - p) / (1 - p)) and pick probability (1 - p) pick;
 *                    sky term = T f(L) Lsky(L) (N.L) / ((bsdf_pdf(L) + p pdf_sky(L)) s), shadow ray to t = 1e34;
 *                    a BSDF-sampled miss after a non-specular vertex (depth >= 1) adds T Lsky(D) / (bsdfPdf + p pdf_sky(D));
 *                    an emitter hit's light pdf takes the factor 1 - p.  After a specular vertex and at depth 0 nothing changes.
 *                  p = 0 (sky_pick "0", no sky, or a sky whose S is 0) runs the default kernels: bit-identical to "0".
 *   sky_pick = "-1" (default: auto, p = 1 when the scene has no lights, 0.5 otherwise) | a probability p in [0, 1]
 *   rfwhip_get_setting also answers read-only keys: "textured" (the textured shade kernel variant is in use), "packet" (the
 *   pt primary wave can run in packet form), "world_tree" (triangles in the world tree of the last update; 0: none),
 *   "shadow_bins_per_run", "shadow_packets_on", "sky" (the last update left p > 0: the shade waves run the sky variant),
 *   "light_tree" (nodes of the light tree the next render would use; 0: none, or light_sampling is not "tree"),
 *   "lights_bound" (area lights the last refresh of lights_follow_geometry found bound; 0 while that setting is off),
 *   "light_tree_refits" (refits of the light tree on the device since it was last built), "primary_entry_on" (the primary wave of
 *   the last render call started from its entry snapshot: see primary_entry), "material_maps_on" (the next render's pt shade waves
 *   run the map kernels: material_maps is "1" and some material has a present alpha, roughness or metallic map).
 *   Not listed by rfwhip_get_settings, but settable:
 *   primary_entry = "-1" (default) | "0" | "1": the entry snapshot of the pt primary wave in packet form.  Where the camera-ordered
 *                  node table is used (kernel family 11 below), the camera has no lens (aperture 0) and count_traversal is 0, a pass
 *                  walks the top of the tree once per 64-slot group of path slots — with sample groups of 64: once per pixel — and
 *                  every wave of that group, in every sample group and sub-batch and in every later call with the same view, starts
 *                  its walk from the record the pass left instead of at the root.  "1": records for every view; "-1": for calls of
 *                  at least 720 paths per record, and for smaller calls from the second call with the same view on (a camera at rest);
 *                  "0": never.  No pixel depends on it.  The passes are kernel family 16 of rfwhip_get_kernel_time.
 *   light_sampling = "reference" (default: the reference's estimator, the default kernels) | "linear" (its potentials, consistent
 *                  weights) | "tree" (the light tree, O(log lights) per next-event vertex, the same weights): rfwhip_get_light_tree
 *                  below has the formulas.  The parity integrator ignores it.
 *   display_tonemap / display_fxaa / display_srgb = the display stage, see rfwhip_read_display above.
 *   display_exposure / display_exposure_ev / _key / _low / _high / _speed / _min_ev / _max_ev = the exposure meter, see
 *                  rfwhip_get_meter above.
 *   display_bloom / display_bloom_intensity / _threshold / _knee / _scatter / _levels = bloom, see rfwhip_bloom_image above.
 *   display_grade / display_wb_temperature / display_grade_slope / _offset / _power / _saturation / display_dither = colour grading
 *                  and dither, see rfwhip_set_display_lut above.
 *   noise_estimate / noise_floor / noise_threshold = the noise estimate, see rfwhip_get_noise above.
 *   adaptive_sampling / adaptive_min_samples / adaptive_every = adaptive sampling, see rfwhip_get_adaptive above.
 *   material_maps = "0" (default: map slots 6 - 9 of a material are ignored, as in the reference) | "1": the pt integrator reads the
 *                  alpha mask of slot 9 and the roughness / metallic maps of slots 7 / 6.  The parity integrator ignores it.
 *                  At a hit with interpolated (tu, tv) and the level of detail lambda of the colour layers, slot K's texel is the
 *                  trilinear fetch of its own descriptor, as a colour layer's:
 *                    texel_K = fetch(textures[map[K].addr], lambda, uscale_K (uoffs_K + tu), vscale_K (voffs_K + tv), width_K, height_K).
 *                  A slot is PRESENT when its flag is set and map[K].addr < the textures of the last rfwhip_set_textures — with or
 *                  without a diffuse map.
 *                    alpha mask (HasAlphaMap, slot 9): a = min(texel_9.r, texel_9.a) — a grey mask with alpha 255 gives its grey, a
 *                      white one with an alpha channel its alpha.  a < 0.5 is HasAlpha's pass-through, unchanged: the path goes on from
 *                      I + 1e-5 D, its state untouched, one depth deeper, and nothing else of the surface is evaluated.  With
 *                      HasAlpha as well, either test passes the ray through.
 *                    roughness (HasRoughnessMap, slot 7): r = roughness * texel_7.g;  metallic (HasSpecularityMap, slot 6):
 *                      m = metallic * texel_6.b, roughness and metallic the bytes of parameters[0] over 255 — glTF's packing, so a
 *                      host points both slots at one metallic-roughness texture (with the same descriptor in both, one fetch serves
 *                      both); a grey map scales the same two parameters.  Both go back into the 8 bits the BSDF reads,
 *                      byte(v) = (uint32)(min(max(v, 0), 1) * 255 + 0.5), a NaN gives 0; the specular test (roughness < 0.01) and the
 *                      BSDF then read the mapped bytes.  Emitters (a colour component > 1) and hits passed through read neither.
 *                    slot 8 (colour mask) stays ignored.
 *                  The map kernels (k_shade_pt_maps) run only while some material of the last rfwhip_set_materials has a present slot
 *                  6, 7 or 9 ("material_maps_on"); otherwise the setting changes no byte of any image.  The denoiser's guide pass
 *                  looks through the mask under the same condition, and a change of the setting makes the guides stale.
 *                  RFWHIP_KAT_SURFACE_MAPS evaluates the rule on given hits whatever the setting is.
 *   lights_follow_geometry = "0" (default) | "1": rfwhip_update derives the area lights of emissive geometry on the device and
 *                  refits the light tree, see rfwhip_read_area_lights below.
 * Returns the number of keys; fills up to cap pointers with static strings. */
RFWHIP_API int rfwhip_set_setting(rfwhip_context *ctx, const char *key, const char *value);
RFWHIP_API int rfwhip_get_setting(rfwhip_context *ctx, const char *key, char *value, size_t cap);
RFWHIP_API int rfwhip_get_settings(rfwhip_context *ctx, const char **keys, size_t cap);

/* ---- measurement hooks (bench / tests; not part of the reference interface) ---------------------------------- */
typedef struct rfwhip_counters
{
	uint64_t rays_extend;	 /* closest-hit rays traced since the last reset (primary + extension) */
	uint64_t rays_shadow;	 /* any-hit rays traced */
	uint64_t inner_extend;	 /* popped 4-wide inner nodes (64 bytes = 4 rows of 16 B each), closest-hit rays */
	uint64_t tris_extend;	 /* triangle tests, closest-hit rays */
	uint64_t inner_shadow;
	uint64_t tris_shadow;
	uint64_t shaded;		 /* shade-kernel invocations with a hit */
	uint64_t samples;		 /* pixel samples started */
	uint64_t lds_extend;	 /* of inner_extend: visits served by the LDS top-of-tree cache (no vector-L1 lane-loads) */
	uint64_t lds_shadow;	 /* of inner_shadow: the same */
	uint64_t extend_ticks;	 /* extend-stage kernels, first workgroup in to last workgroup out, summed: ticks of the 100 MHz device clock */
	uint64_t extend_launches_timed; /* launches in extend_ticks */
} rfwhip_counters;
RFWHIP_API int rfwhip_get_counters(rfwhip_context *ctx, rfwhip_counters *out, int reset);

/* Accumulated hipEvent time (ms) and launch count per kernel family since the last reset; requires
 * stage_timing=1.  which: 0 generate, 1 extend, 2 shade, 3 connect, 4 finalize, 5 refit, 6 denoise (a guide pass is two launches,
 * guide rays + depth gradient; a filter is 1 + denoise_iterations launches: demodulation / variance, then the a-trous passes),
 * 7 display (one launch per displayed image), 8 noise (the metric: two launches per query; the moments are part of the resolve,
 * family 4), 9 the exposure meter's histogram pass k_meter_hist and 10 its reduce k_meter_reduce (one launch each per step; the
 * exposed display kernels count as family 7), 11 the primary wave's ordering pass k_order4f: a pt render call whose primary wave
 * runs in packet form and is large enough (or RFWHIP_PRIMARY_ORDER=1 in the environment when the context was created; =0: never)
 * reads a second float node table whose nodes hold their children near to far as seen from the camera, rewritten in front of the
 * call when the camera position or a tree has changed since — `launches` counts those passes, one per rewrite, with or without
 * stage_timing; the image does not depend on it.  12 bloom: one count per launch of a chain, 2 x the levels it ran (the down
 * passes, the up passes and the apply pass).  13 grade: k_display_graded, one launch per displayed image with display_grade = 1 (in
 * place of family 7's).  14 jpeg: the four kernels of a JPEG encode, one count each.  15 the image-texture decoder.  16 the
 * primary wave's entry snapshot pass k_primary_entry (setting primary_entry): one count per pass, with or without stage_timing.  17 the
 * sky's loaders (rfwhip_set_sky_hdr, sky_table = device): one count per launch; by kernel: the setting sky_load_time.  18 the rig
 * kernel k_rig_evaluate (rfwhip_animate): one launch per call, however many rigs it lists; the vertex kernels and the refit behind
 * it count as family 5, as they do for rfwhip_pose_mesh. */
RFWHIP_API int rfwhip_get_kernel_time(rfwhip_context *ctx, int which, float *ms, uint32_t *launches, int reset);

/* The denoiser's guides of the full image (see "denoise"), for the camera of the last render — the guide pass runs first if they are
 * stale.  albedo: W x H x 4 floats (rgb, w = 1 valid / 0 invalid); normal_depth: W x H x 4 floats (the unpacked normal, z; z = -1 for
 * an invalid pixel).  Either pointer may be NULL.  World-1 contexts and the root of a group. */
RFWHIP_API int rfwhip_read_denoise_guides(rfwhip_context *ctx, float *albedo, float *normal_depth);
/* The motion part of the temporal stage of the last presented frame (see "denoise_motion"; world-1 contexts whose last render has
 * been presented with denoise, denoise_temporal and denoise_motion on).  Runs the stage of the frame again, as
 * rfwhip_read_denoise_history does.  state: W x H int32, 0 invalid pixel, 1 its instance is STILL, 2 MOVED, 3 RESTART (every valid
 * pixel while the history is not usable); prev_position: W x H x 3, X_P for state 2, X for state 1, 0 otherwise; prev_normal:
 * W x H x 3, n'_p for state 2, n_p for state 1, 0 otherwise (a pixel on a degenerate triangle reports X and n_p and is fresh).
 * Any pointer may be NULL. */
RFWHIP_API int rfwhip_read_denoise_motion(rfwhip_context *ctx, int32_t *state, float *prev_position, float *prev_normal);
/* Filter a given W x H float4 image (host memory) with the current guides and the context's denoise_* knobs, whatever "denoise"
 * says (the guide pass runs first if they are stale).  rgba_out may equal rgba_in. */
RFWHIP_API int rfwhip_denoise_image(rfwhip_context *ctx, const float *rgba_in, float *rgba_out);
/* The temporal stage of the last presented frame (see "denoise_temporal"; world-1 contexts whose last render has been presented
 * with denoise and denoise_temporal on): pre_rgbl = I~ and lum(I~), var = the variance the passes start from (W x H x 4 / W x H
 * floats; 0 at invalid pixels), hist_rgbl = the stored colour history (pass 0's demodulated output, lum), moments = (mu1, mu2)
 * (W x H x 2), length = n (W x H; 0 at invalid pixels).  Any pointer may be NULL.  It runs the stage of the frame again with the
 * current guides and instance table: the presented frame's values while the scene is unchanged (no rfwhip_update since). */
RFWHIP_API int rfwhip_read_denoise_history(rfwhip_context *ctx, float *pre_rgbl, float *var, float *hist_rgbl, float *moments,
										   float *length);

/* Raw closest-hit records of the most recent primary wave (parity tests): per pixel of this rank's local image
 * t (1e34 = miss), primID, instID, u, v. Any pointer may be NULL. */
RFWHIP_API int rfwhip_read_primary_hits(rfwhip_context *ctx, float *t, int32_t *prim, int32_t *inst, float *u,
										float *v);

/* Trace n arbitrary world-space rays (org/dir: n x 3 floats, closest hit in (t_min, t_max)) through the resident
 * scene with the extend kernel; any output pointer may be NULL.  t = t_max on a miss. */
RFWHIP_API int rfwhip_trace_rays(rfwhip_context *ctx, size_t n, const float *org, const float *dir, float t_min,
								 float t_max, float *t, int32_t *prim, int32_t *inst, float *u, float *v);

/* Test entry: the caller's rays through ONE chosen form of the traversal — the product's own launchers (kernels.h), not copies.
 * rfwhip_trace_rays reaches only the one-ray-per-lane closest-hit kernel; a render's incoherent waves run the other forms.
 *
 *   form                          launcher                                   rays read from                   result
 *   RFWHIP_FORM_LANE_CLOSEST  0   launch_extend(GEN_RANGED), depth 1         org[1] / dir[1], w = (1e-5, 1e34)  hit records
 *   RFWHIP_FORM_STREAM_CLOSEST 1  launch_extend(GEN_BUFFER), refill bit 0    org[1] / dir[1], org.w = tag       hit records
 *   RFWHIP_FORM_LANE_ANY      2   launch_connect, refill bit 1 clear, depth 1  sh_org / sh_dir, sh_org.w = tag,   visibility
 *   RFWHIP_FORM_STREAM_ANY    3   launch_connect, refill bit 1 set, depth 1      sh_dir.w = t_max
 *   RFWHIP_FORM_FUSED         4   launch_trace_fused: the closest-hit set at depth 3 and the occlusion set at depth 2 in one
 *                                 launch (either may be empty)                                                both
 *   RFWHIP_FORM_PACKET_ANY    5   launch_shadow_packets, depth 0, FrameView::shadow_bins = bins, rad_nee present    visibility
 *
 * The closest-hit set: n rays (org / dir: n x 3 floats), interval (1e-5, 1e34) — the kernels' own.  tag: n words or NULL.  A tag
 * is the word the queue entry carries in org.w: any value below 2^31, or 0xFFFFFFFF (RAY_VOID) for a void entry, whose record
 * comes back with prim = -2 (HIT_VOID).  NULL: tag = ray index.  LANE_CLOSEST reads no tag and accepts no void entry.  Outputs
 * t / u / v / prim / inst (n each, any may be NULL; prim = -1 and inst = -1 on a miss).
 * The occlusion set: n_any rays, t_max_any per ray (interval (1e-5, t_max); t_max <= 1e-5 or negative: traced, hits nothing),
 * tag_any: n_any words or NULL (= ray index).  A tag is the path slot the result is folded into, below n_any and UNIQUE within the
 * call (connect_finish is a read-modify-write), or 0xFFFFFFFF for a void entry.  PACKET_ANY: tag = bin << (31 - bins) | slot with
 * 1 <= bins <= 4 (the bin is every bit from 31 - bins to 30).  visible (n_any floats, indexed by SLOT): 1 = nothing inside the interval, 0 = occluded,
 * RFWHIP_FORM_UNTOUCHED (-777) = a slot no entry of the queue named.  (LANE / STREAM / FUSED: sh_rad = (1, 0, 0) is added to a
 * zeroed rad[slot] for a visible ray; PACKET: rad_nee[slot] starts at 1 and an occluded ray zeroes it.)
 * grid_items is handed to the launcher as max_items: only the grid is derived from it, the queue lengths come from the counters,
 * so a small ray count can reach every run length of the persistent-lane kernels (0: the ray count).
 * Before the launch the hit records hold a sentinel (prim = RFWHIP_FORM_SENTINEL_PRIM, t = NaN): a record no kernel wrote is
 * returned as such.  launch_counters (or NULL): 4 x uint64 of this launch, counted whatever count_traversal says — rays_extend,
 * rays_shadow, sp_runs, stack_overflow.  A stack overflow is RFWHIP_ERR_STATE, as in rfwhip_trace_rays.
 * In the host-emulation build the forms collapse to the per-item loops (kernels_emu.inc): LANE_* = STREAM_* = FUSED = PACKET. */
#define RFWHIP_FORM_LANE_CLOSEST 0
#define RFWHIP_FORM_STREAM_CLOSEST 1
#define RFWHIP_FORM_LANE_ANY 2
#define RFWHIP_FORM_STREAM_ANY 3
#define RFWHIP_FORM_FUSED 4
#define RFWHIP_FORM_PACKET_ANY 5
#define RFWHIP_FORM_UNTOUCHED (-777.0f)
#define RFWHIP_FORM_SENTINEL_PRIM 0x5E5E5E5E
RFWHIP_API int rfwhip_trace_rays_form(rfwhip_context *ctx, int form, uint32_t grid_items, uint32_t bins, size_t n, const float *org,
									  const float *dir, const uint32_t *tag, float *t, int32_t *prim, int32_t *inst, float *u, float *v,
									  size_t n_any, const float *org_any, const float *dir_any, const float *t_max_any,
									  const uint32_t *tag_any, float *visible, uint64_t *launch_counters);

/* Known-answer hook: one of the path tracer's DEVICE functions (rt_core.h: BSDF, light sampling, packing, samplers — the
 * very functions the shade kernel calls) evaluated by a kernel on n records; functions and record layout: RFWHIP_KAT_* in
 * rfwhip_abi.h.  in: n x RFWHIP_KAT_IN floats, out: n x RFWHIP_KAT_OUT floats (host pointers).  The light functions use
 * the lights of the last rfwhip_update(), BLUE_NOISE the table of rfwhip_set_blue_noise, TEX_FETCH and SURFACE_LAYERS the
 * textures, materials, meshes and instances of the last rfwhip_update(): a record that names a texture, instance or triangle
 * the scene does not have is RFWHIP_ERR_INVALID_ARGUMENT. */
RFWHIP_API int rfwhip_kat(rfwhip_context *ctx, int function, size_t n, const float *in, float *out);

/* BVH of mesh `index` as built on the device side (bvh_node.h layout) + its primitive order. */
RFWHIP_API int rfwhip_get_bvh(rfwhip_context *ctx, size_t mesh_index, rfwhip_bvh_node *nodes, size_t node_cap,
							  uint32_t *prim_indices, size_t prim_cap, size_t *node_count, size_t *prim_count);

/* What rfwhip_get_bvh4 reports about a resident mesh's slice of the traversal tables (32 B). */
typedef struct rfwhip_bvh4_info
{
	uint32_t n4_base, n4_count;	 /* its 4-wide nodes in the scene-wide table: [n4_base, n4_base + n4_count) */
	uint32_t tri_base, tri_count; /* its leaf-ordered triangles: [tri_base, tri_base + tri_count) */
	uint32_t node_base, node_count2; /* its BVH2 nodes (what src4 refers to, mesh-relative) */
	int32_t stack_need;			  /* traversal-stack entries the mesh was admitted with (bvh::stack_need4) */
	uint32_t device_built;		  /* 1: built by the device builder (builder=device), 0: by the host builder */
} rfwhip_bvh4_info;
RFWHIP_STATIC_ASSERT(sizeof(rfwhip_bvh4_info) == 32, "rfwhip_bvh4_info is 32 B");

/* The TRAVERSED tree of mesh `index` as it sits on the device (a test hook like rfwhip_get_bvh, not part of the build path).
 * Entries stay absolute.  nodes4c: n4_count compressed 4-wide nodes (64 B each, rt::Node4c), nodes4f: their float form
 * (128 B each, rt::Node4f), src4: 4 x n4_count BVH2 node indices (mesh-relative, 0xFFFFFFFF = unused slot), tri_verts:
 * 3 x tri_count float4 in leaf order (v0.w = primitive id bits, v1.w = 1, v2.w = determinant threshold).  At most node_cap
 * nodes and tri_cap triangles are copied; any pointer may be NULL.  A mesh that is not resident (set again since the last
 * rfwhip_update) fails with RFWHIP_ERR_STATE. */
RFWHIP_API int rfwhip_get_bvh4(rfwhip_context *ctx, size_t mesh_index, void *nodes4c, void *nodes4f, uint32_t *src4,
							   size_t node_cap, float *tri_verts, size_t tri_cap, rfwhip_bvh4_info *info);

/* The light tree of setting light_sampling=tree as the next render would use it (a test hook like rfwhip_get_bvh; built on the
 * host at the setting, at rfwhip_set_lights and at rfwhip_update, downloaded here on demand).  Returns the node count — 0 when
 * the mode is not `tree` or no area, point or spot light exists, 1 for one such light, 2 n for n >= 2 — or a negative error
 * code.  At most node_cap nodes and light_cap paths (one per light of all four kinds, in the order area, point, spot,
 * directional) are copied; either pointer may be NULL.
 *
 * light_sampling = reference (default) | linear | tree.  `reference` is the reference's estimator, untouched.  `linear` picks a
 * light by the reference's potentials, `tree` by descending the tree; both weight consistently, so that they converge to the
 * same image whatever the picking rule (q = the probability of the picked light, times 1 - p under sky sampling):
 *   area light, next event:  T bs radiance NdotL / (shadowPdf + q p_w),   p_w = dist^2 / (area LNdotL)   (no 1 / |radiance|)
 *   point, spot, directional: T bs radiance NdotL / (q lightPdf)        (lightPdf as the reference has it; no BSDF pdf)
 *   emitter found by a BSDF ray: T colour / (bsdfPdf + p_w q),          q by the rule that picks.
 * The tree: binary, over the area, point and spot lights; split at the median of the centroids along the longest axis of the
 * centroid box, ties by light index; a leaf holds one light.  Directional lights form a flat list beside the root.  The
 * importance of a node for a point I with normal N — c = (lo + hi) / 2, r = |hi - lo| / 2, v = I - c, d = |v| —
 *   d <= r:  E / max(r^2, 1e-12)
 *   else:    E cos(max(0, theta - theta_o - theta_u)) cos(max(0, theta_i - theta_u)) / d^2,
 *            theta_u = asin(r / d), theta = angle(axis, v), theta_i = angle(N, -v),
 * where a cosine c of a positive angle counts as max(0, c + 1e-5) (a margin for the rounding of the sine and cosine identities
 * the kernel uses: a light with a positive potential must never lose a node on its path).  Selection: r1 chooses
 * among [root by importance, directional 0 .. k - 1 by potential]; each level below picks a child in proportion to importance,
 * left first, and rescales r1 into the child's interval; q is the product of the probabilities. */
RFWHIP_API int rfwhip_get_light_tree(rfwhip_context *ctx, rfwhip_light_tree_node *nodes, size_t node_cap,
									 rfwhip_light_tree_path *paths, size_t light_cap);

/* ---- moving emitters: setting lights_follow_geometry = "0" (default) | "1" --------------------------------------------------
 * Poses, morphs, same-count rfwhip_set_mesh and rfwhip_set_instance move geometry on the device; an area light is a record the
 * host derived from host triangles (system::update_area_lights, system.cpp:967-1032) and stays where it was.  With "1",
 * rfwhip_update() brings the lights of the last rfwhip_set_lights up to date on the device, before anything reads them.
 *
 * BOUND.  An area light is bound when instIdx names an instance in use, triIdx is below the triangle count of that instance's
 * mesh, and that triangle is a light triangle (its lightTriIdx >= 0: the back-pointer of system.cpp:1021).  Every other area
 * light — the (-1, -1) of a free-standing light, an index out of range, a triangle that does not emit — is unbound and keeps
 * the host's bytes, always.  Binding is evaluated anew at every refresh.  Point, spot and directional lights are never touched.
 *
 * REFRESH (system.cpp:1003-1024).  Runs in rfwhip_update when the setting is on, an area light exists, and since the last
 * refresh an instance was set, a mesh was set, posed or morphed (or placed again), the lights were set, or the setting came on.
 * Per bound light, with v_j the current object-space vertices of triangle triIdx (after pose and morph), M the instance's
 * transform and Nm the normal matrix given to rfwhip_set_instance, all in float32:
 *   vertex_j = M v_j                      per coordinate fma(m2, z, fma(m1, y, m0 x)) + m3
 *   position = ((vertex0 + vertex1) + vertex2) * (1/3)
 *   normal   = Nm N                       N: the face normal of the triangle's shading record as the device's update_triangles
 *                                         (rfwhip_pose_mesh / rfwhip_morph_mesh) or the last rfwhip_set_mesh left it; not renormalised
 *   area     = |(v1 - v0) x (v2 - v0)| / 2   in OBJECT space, as the reference's updateArea has it (its quirk under a scaling
 *                                         transform, kept for parity); the same float is written to the triangle's shading
 *                                         record, which the emitter-hit density reads: both sides of MIS see one area
 *   radiance, energy, triIdx, instIdx and the two padding words stay bit for bit.
 *
 * REFIT.  With light_sampling=tree and a tree that stands (not stale), the refresh is followed by a refit over the EXISTING
 * topology, bottom-up: lo / hi / axis / cos_o of every leaf that holds a bound area light and of every ancestor of such a leaf.
 * A leaf: the min / max of its light's three vertices, the normalised normal, cos_o = 1 (a zero or non-finite normal: cos_o = -1).
 * An inner node: the min / max of its two children's boxes (exact), and the union of its two children's cones (Conty Estevez
 * and Kulla 2018, Alg. 1) in float32, widened by a derived margin (light_follow.h) so that it is conservative: every light
 * below lies in the cone.  The host build unites a node's lights one after another in double, the refit unites the two children:
 * two different bounds, both valid.  energy, child, light, count and the lights' paths stay bit for bit; leaves of point and
 * spot lights and of unbound area lights, and inner nodes without a bound leaf below, are not rewritten.  No atomics, a fixed
 * order: the same lights give the same bytes.  The topology is rebuilt where it always was — rfwhip_set_lights, or setting
 * light_sampling — and that is the way to force a rebuild after emitters have moved far; a stale tree is built from the
 * refreshed lights.  With the setting on, rfwhip_set_lights does not make the topology of the geometry fields it is handed (they
 * are about to be overwritten and may be zeros): it leaves the tree stale, and the rfwhip_update that must follow builds it from
 * what its refresh derives.  (A rfwhip_get_light_tree in between sees a tree of the host's fields; the update builds it anew.)
 *
 * ORDER.  Refresh and refit overwrite tables that render calls in flight read.  They are ordered as the device refit of
 * rfwhip_pose_mesh is: rfwhip_update first waits for every stream of the ring, for a present on a caller's stream and for a
 * denoise on a gather stream, enqueues the work on the context's stream, and synchronises that stream before it returns.  No
 * scheduling setting (ring, streams, overlap, fuse, shadow_packets, shadow_side) changes a bit of any image.
 * Every rank of a group refreshes and refits its own copy inside rfwhip_group_update; nothing crosses the gather.
 *
 * rfwhip_read_area_lights: the area lights as the next render would read them, setting on or off; waits for the context's
 * stream; copies at most cap records; returns the count of the last rfwhip_set_lights, or a negative error code. */
RFWHIP_API int rfwhip_read_area_lights(rfwhip_context *ctx, rfwhip_area_light *out, size_t cap);
/* Known-answer hook (like rfwhip_noise_image): the product's refit kernels on the caller's tree and lights, whatever the context
 * renders.  nodes: node_count nodes as rfwhip_get_light_tree returned them for the same light counts, refitted in place;
 * area: the n_area area lights (lights 0 .. n_area - 1 of the tree); bound: n_area bytes, 1 = treat as bound (NULL: all).
 * Nodes that are not laid out as the build lays them out are RFWHIP_ERR_INVALID_ARGUMENT. */
RFWHIP_API int rfwhip_light_tree_refit(rfwhip_context *ctx, rfwhip_light_tree_node *nodes, size_t node_count,
									   const rfwhip_area_light *area, size_t n_area, const uint8_t *bound);

#ifdef __cplusplus
}
#endif
#endif /* RFWHIP_H */
