// rfwhip_api.cpp — the C ABI of include/rfwhip.h: scene residency in HBM, BVH construction, wave scheduling.
//
// Host-side responsibilities (the kernels are in kernels.hip):
//   * copy every borrowed host buffer into device memory inside the call (context.h ownership rules),
//   * build one BVH2 per mesh (bvh_build.cpp), concatenate all meshes into the flat arrays of rt::SceneView,
//     build the top-level BVH over instances in update(), refit instead of rebuild when a mesh keeps its counts,
//   * enqueue the wavefront stages of a frame on the context's HIP stream without any host read-back between
//     bounces (contrast CUDART/src/Context.cpp:98,145), gather stage timings with hipEvents.
#include "rfwhip.h"

#include "bvh_build.h"
#include "device_layer.h"
#include "internal.h"
#include "kernels.h"
#include "rt_types.h"
#include "sky_sampling.h"
#include "light_tree.h"

#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using rt::f4;

// =================================================================================================================
// error reporting
// =================================================================================================================
static thread_local char g_error[1024] = "";
int rfwhip_internal_set_error(int code, const char *fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_error, sizeof(g_error), fmt, ap);
	va_end(ap);
	return code;
}
#define set_error rfwhip_internal_set_error // (this file's short name for it)
extern "C" const char *rfwhip_last_error(void) { return g_error; }
extern "C" const char *rfwhip_version(void)
{
#if defined(RFWHIP_HOST_EMULATION)
	return "rfwhip 0.1 (HOST EMULATION BUILD — tests only)";
#else
	return "rfwhip 0.1 (gfx950 HIP)";
#endif
}

#define RF_TRY(x)            \
	do                       \
	{                        \
		const int rc_ = (x); \
		if (rc_)             \
			return rc_;      \
	} while (0)

struct DevBuf
{
	void *p = nullptr;
	size_t cap = 0;
	int ensure(size_t bytes)
	{
		if (bytes <= cap && p)
			return 0;
		dm::release(p);
		p = nullptr, cap = 0;
		// grow with headroom so animation / resize do not reallocate every call
		const size_t want = bytes + bytes / 8 + 256;
		RF_TRY(dm::alloc(&p, want));
		cap = want;
		return 0;
	}
	// exactly `bytes` (the path-state buffers: tens of GB, no headroom); an existing larger allocation is kept
	int ensure_exact(size_t bytes)
	{
		if (bytes <= cap && p)
			return 0;
		dm::release(p);
		p = nullptr, cap = 0;
		if (dm::alloc(&p, bytes + 256))
		{
			p = nullptr;
			return RFWHIP_ERR_HIP;
		}
		cap = bytes + 256;
		return 0;
	}
	void free_()
	{
		dm::release(p);
		p = nullptr, cap = 0;
	}
	template <typename T> T *as() const { return (T *)p; }
};

// "Work I enqueued on a stream that is not mine may still be running": the record behind that work.  The context keeps every one of
// them in rfwhip_context::marks, which sync_all (before anything frees or rewrites device memory) and free_all walk: a mark outside
// that array does not exist.  `pending` is the host's view (nobody has waited for the record on the host); a stream that must run
// behind the record waits for it on the device (wait_on), which leaves `pending` alone.
struct StreamMark
{
	dm::event_t ev;
	bool timed = false;		// how the event is created (set once, in rfwhip_create)
	bool ready = false;		// ev exists: it is created by the first record, so it has held one ever since
	bool pending = false;	// the last record has not been waited for on the host
	void *stream = nullptr; // the stream of the last record
	int record(void *s, bool host_wait)
	{
		if (!ready)
		{
			RF_TRY(dm::event_create(&ev, timed));
			ready = true;
		}
		RF_TRY(dm::event_record(ev, s));
		stream = s, pending = host_wait;
		return 0;
	}
	int wait_on(void *s) { return ready ? dm::stream_wait_event(s, ev) : 0; } // device side: s runs behind the last record
	int sync()																   // host side
	{
		if (pending)
			RF_TRY(dm::event_sync(ev));
		pending = false;
		return 0;
	}
	void destroy()
	{
		if (ready)
			dm::event_destroy(ev);
		ready = false, pending = false, stream = nullptr;
	}

private:
	StreamMark() {} // (only rfwhip_context::marks can hold one: a mark elsewhere does not compile)
	friend struct rfwhip_context;
};
enum MarkId
{
	MK_PRESENT = 0, // a present on a caller's stream (rfwhip_read_local_framebuffer_stream) still reads the accumulator
	MK_DENOISE,		// a denoise on a gather stream reads the scene and the guides
	MK_METER,		// a meter step on a caller's stream writes the record and the histogram
	MK_BLOOM,		// the last bloom chain and the display kernel that read its image, on any stream: they write / read the pyramid
	MK_GRADE,		// a graded display kernel on a caller's stream reads the LUT
	MK_JPEG,		// the last encode, on any stream: it writes the JPEG scratch
	MK_COUNT
};

// A table that is rewritten on the main stream and read by primary waves on the sub-batch streams.  Behind a rewrite the main stream
// records ev and the serial goes up (publish); a sub-batch stream that has not waited for that record yet does so before its next
// primary wave (acquire); a stream whose wave reads the table says so (read_by), and the next rewrite waits for that sub-batch's
// end first (before_rewrite).  ev is created and destroyed with the render loop's own events.
constexpr int MAX_SUB_BATCHES = 8;
struct rfwhip_context;
struct Published
{
	dm::event_t ev;
	uint64_t serial = 0, seen[MAX_SUB_BATCHES] = {};
	bool reader[MAX_SUB_BATCHES] = {}; // a primary wave of this sub-batch slot has read the table since its last rewrite
	int publish(void *main_stream)
	{
		RF_TRY(dm::event_record(ev, main_stream));
		serial++;
		return 0;
	}
	int acquire(int i, void *s)
	{
		if (seen[i] != serial)
		{
			RF_TRY(dm::stream_wait_event(s, ev));
			seen[i] = serial;
		}
		return 0;
	}
	void read_by(int i) { reader[i] = true; }
	int before_rewrite(rfwhip_context *c); // (below the context)
};

// The milliseconds and launches of one kernel family by kernel (stage_timing = 1), and the read-only setting that prints them
struct KindTimes
{
	static constexpr int MAX_KINDS = 9;
	int count = 0;
	float ms[MAX_KINDS] = {};
	uint32_t launches[MAX_KINDS] = {};
	void add(int kind, float t) { ms[kind] += t, launches[kind]++; }
	void reset()
	{
		for (int k = 0; k < MAX_KINDS; k++)
			ms[k] = 0.0f, launches[k] = 0;
	}
};

// =================================================================================================================
// context
// =================================================================================================================
struct MeshRec
{
	bool used = false;
	size_t vertexCount = 0, triCount = 0;
	bool indexed = false;
	bvh::Result bvh;				   // host copy of the topology as built
	std::vector<rt::Node4> n4;		   // 4-wide traversal nodes collapsed from it (relative entries)
	uint32_t n4_base = 0;
	std::vector<f4> leaf_verts;		   // 3 per leaf slot (host staging for (re)upload)
	std::vector<rt::TriShade> shade;   // mesh order
	std::vector<rt::TriUV> uv;		   // mesh order (texture coordinates: rt_types.h)
	float bounds_min[3] = {0, 0, 0}, bounds_max[3] = {0, 0, 0};
	DevBuf d_verts, d_indices;		   // raw vertices / indices (kept for refit)
	DevBuf d_parents, d_flags;		   // refit helpers
	uint32_t node_base = 0, tri_base = 0, shade_base = 0;
	// built on the device (builder=device): no host copy of the tree; the mesh-local device arrays below are what
	// rfwhip_update() places (device-to-device copies + an entry rebase)
	bool device_built = false;
	bool built = false; // the last (re)build of this mesh succeeded: the counts below describe its tree
	DevBuf d_b_nodes, d_b_nodes4, d_b_src, d_b_tri_verts;
	uint32_t node_count2 = 0, n4_count = 0; // BVH2 nodes / 4-wide nodes of the mesh, whoever built them
	int stack_need = 0;		   // worst-case traversal-stack entries of the 4-wide tree (bvh::stack_need4)
	uint32_t max_material = 0; // largest material id any triangle refers to
	bool resident = false; // placed in the global arrays by the last update()
	bool dirty = true;	   // host staging newer than the global arrays
	bool refit_pending = false;
	uint32_t generation = 0; // counts the (re)builds of this mesh (the world tree's cache key)
	uint32_t refits = 0;	 // same-topology rfwhip_set_mesh calls since the last build: an animated mesh (never written into the world tree)
	uint32_t edits = 0;		 // rebuilds, refits, poses and morphs (the denoiser's temporal stage: instance_versions)
	// "denoise_motion": `edits` as the last guide pass traced the mesh and as the last presented frame's guide pass did; ONE snapshot
	// of d_verts, taken in front of the first in-place edit after a presented frame and tagged with that frame (dn_snapshot_mesh)
	uint32_t dn_g_edits = 0, dn_p_edits = 0;
	DevBuf d_dn_snap;
	unsigned long long dn_snap_pres = 0; // rfwhip_context::dn_pres_id of the frame whose vertices it holds (0: none)
	// device skinning (rfwhip_set_mesh_skin / rfwhip_pose_mesh)
	bool skinned = false, posed = false;
	DevBuf d_base_verts, d_base_normals, d_joints, d_weights, d_vnormals, d_joint_mats;
	uint32_t joint_count = 0;
	// device morph targets (rfwhip_set_mesh_morph / rfwhip_morph_mesh); shares d_base_verts / d_base_normals / d_vnormals
	bool morphed = false;
	DevBuf d_tgt_pos, d_tgt_nrm, d_morph_weights;
	uint32_t target_count = 0;
	// animations (rfwhip_bind_rig): the rig the mesh follows (-1: none) and the skin (a skinned mesh) or node (a morphed one) of it
	int rig = -1;
	uint32_t rig_item = 0;
	uint32_t skin_max_joint = 0; // the largest joint index of the last rfwhip_set_mesh_skin
};

// A rig (rfwhip_set_rig; animation.h): the tables and the validator's plan in one device allocation, what an evaluation writes in
// another, and what the host keeps to bind meshes and to size read-backs
struct RigRec
{
	bool used = false, evaluated = false;
	DevBuf d_tables, d_state;
	rtk::RigView view{};
	std::vector<uint32_t> node_weight_offset, node_weight_count, skin_joint_count, skin_first_item;
	std::vector<size_t> meshes; // bound to it
};

// "denoise_motion": an instance as a guide pass traced it
struct DnInstSnap
{
	bool used = false;
	size_t mesh = 0;
	uint32_t generation = 0, edits = 0;
	float transform[16];
};

struct InstRec
{
	bool used = false;
	size_t mesh = 0;
	float transform[16];
	float normal[9];
	// world-tree membership (prepare_world): an instance whose matrix changed in one of the last few updates is being animated
	// through its matrix and keeps the two-level walk — writing it out in world space would rebuild the world tree per frame
	float prev_transform[16];
	size_t prev_mesh = 0;
	uint32_t prev_generation = 0;
	bool has_prev = false;
	uint32_t moving = 0; // updates left before it may (re)join the world tree
	uint32_t moves = 0;	 // times it has started to move out of stillness: the waiting time doubles with each (an object that moves now
						 // and then would otherwise cost two rebuilds of the world tree — seconds for millions of triangles — per episode)
	// the denoiser's temporal stage: what the instance was at the last rfwhip_update, and the scene version of the update that last
	// changed it (instance_versions)
	bool dn_used = false;
	size_t dn_mesh = 0;
	uint32_t dn_edits = 0;
	float dn_transform[16];
	unsigned long long dn_version = 0;
};

// The WORLD TREE (rfwhip_update): the triangles of the static instances written out in world space under ONE tree.
struct WorldRec
{
	bool valid = false;
	std::vector<uint32_t> key;		   // what it was built from: (instance, mesh, mesh generation, transform) per member
	std::vector<uint8_t> member;	   // per instance: its triangles are in the tree
	std::vector<uint8_t> mesh_all;	   // per mesh: EVERY live instance of it is a member (no ray walks the mesh's own tree)
	std::vector<uint8_t> mesh_member;  // per mesh: at least one of its instances is (an instance that moves keeps the two-level walk of
									   // the same mesh: see fill_params for what that means for the LDS top-of-tree choice)
	std::vector<rt::Node4> n4;		   // relative entries, like MeshRec::n4
	std::vector<f4> leaf_verts;		   // 3 per leaf slot: v0.w = primitive id (mesh order), v1.w = instance index
	uint32_t root_first = 0, root_count = 0; // the root when it is a leaf (n4 empty)
	size_t tris = 0;
	int stack_need = 0;
	float bmin[3] = {0, 0, 0}, bmax[3] = {0, 0, 0};
	uint32_t n4_base = 0, tri_base = 0;
	bool resident = false; // placed in the scene-wide arrays by the last layout
};

enum KernelFamily
{
	KF_GENERATE = 0,
	KF_EXTEND = 1,
	KF_SHADE = 2,
	KF_CONNECT = 3,
	KF_FINALIZE = 4,
	KF_REFIT = 5,
	KF_DENOISE = 6, // the denoiser of the presented image: guide pass + filter (denoise.h)
	KF_DISPLAY = 7, // the display stage: tone map + FXAA + encoding (display.h), one launch per displayed image
	KF_NOISE = 8,	// the noise metric: k_noise_tiles + k_noise_final (noise.h), two launches per query
	KF_METER_HIST = 9,	 // the exposure meter's histogram pass k_meter_hist (metering.h), one launch per step
	KF_METER_REDUCE = 10, // ... and its one-workgroup reduce k_meter_reduce, one launch per step
	KF_PRIMARY_ORDER = 11, // the primary wave's ordering pass k_order4f (primary_order.h): ONE count per pass over the table, with or
						   // without stage_timing (the milliseconds only with it)
	KF_BLOOM = 12, // bloom (bloom.h): the down, up and apply passes of a chain, one count per launch
	KF_GRADE = 13, // colour grading (display_grade.h): k_display_graded in place of family 7's kernel, one count per displayed image
	KF_JPEG = 14,  // baseline JPEG of the display image (display_jpeg.h): four launches per stream, one count each
	KF_TEXDEC = 15, // image textures (texture_decode.h): the kernels of a decode and of a mip chain, one count per launch
	KF_PRIMARY_ENTRY = 16, // the primary wave's entry snapshot pass k_primary_entry (primary_entry.h): one count per pass, with or without
						   // stage_timing (the milliseconds only with it)
	KF_SKYLOAD = 17, // the sky's loaders (sky_load.h): the kernels of an HDR decode and of the alias table's chain, one count per launch
	KF_RIG = 18, // animations (animation.h): k_rig_evaluate, one launch per rfwhip_animate
	KF_COUNT = 19
};

// A run of the float node table the ordering pass handles alike (primary_order.h): the nodes of one tree
struct OrderRange
{
	uint32_t first = 0, count = 0;
	bool object_space = false; // the camera position goes through inv first (the mesh tree of exactly one instance)
	float inv[12];			   // rt::Instance::inv of that instance
};

struct TimedSpan
{
	dm::event_t a, b;
	bool fused = false; // a k_trace_fused launch: extension rays of `depth` + shadow rays of depth - 1 (split by the device's tick sums)
	int family;
	int depth; // wave depth for extend spans, -1 otherwise
};

struct rfwhip_context
{
	int device = 0, rank = 0, world = 1, cus = 256;
	void *stream = nullptr; // main stream: scene uploads, refits, prologue, resolve, presents
	static constexpr int MAX_SUB = MAX_SUB_BATCHES;
	static constexpr int MAX_RING = 4;
	// every sub-batch of a render call runs on its own stream, its connection (shadow) waves on a second one beside it
	void *sub_stream[MAX_SUB] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
	void *conn_stream[MAX_SUB] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
	DevBuf d_counters_sub[MAX_SUB]; // [0] is d_counters' alias slot (unused), 1.. are the extra sub-batches' counters
	dm::event_t ev_prologue, ev_sub_done[MAX_SUB];
	dm::event_t ev_resolve[MAX_RING];								// resolve of the last call that used radiance buffer set 0 / 1
	dm::event_t ev_shade[MAX_SUB][rt::MAX_DEPTH_SLOTS];		// shade stage of depth d enqueued (its connections may start)
	dm::event_t ev_conn[MAX_SUB][rt::MAX_DEPTH_SLOTS];		// connection wave of depth d enqueued
	dm::event_t ev_conn_last[MAX_SUB];						// everything of the call on the connection stream
	bool conn_used[MAX_SUB] = {false, false, false, false, false, false, false, false};
	bool resolve_recorded[MAX_RING] = {false, false, false, false};
	uint32_t call_slot = 0;	  // which set of the ring the next render call uses
	int ring = 3;			  // single-sub-batch calls rotate through this many sets of wave buffers / streams / counters
							  // (3: with the main stream that is four streams = the HIP runtime's four hardware queues; a
							  // fourth set shares a queue with another chain: 1-spp frames 1.43 vs 1.67 ms)
	int ring_active = 0;	  // ring size of the calls in flight (2 for calls cut into sub-batches: radiance double-buffered)
	size_t paths_active = 0;  // path slots per call of the calls in flight
	int subs_active = 0;	  // ... and their sub-batch count
	dm::event_t ev_present_in; // hand-off to a caller's stream (rfwhip_*_stream); the way back is marks[MK_PRESENT]
	// work enqueued on streams that are not this context's (StreamMark): every one of them, by MarkId.  When each records and who
	// waits for it besides sync_all stands at its *_mark function or its recording site
	StreamMark marks[MK_COUNT];
	bool events_ready = false;
	size_t last_wave_off = 0; // where the most recent call's first sub-batch keeps its per-path records
	int subs_last = 1, subs_first = 0; // sub-batch slots of the most recent render call: subs_first .. subs_first + subs_last - 1
	bool cleaned = false;
	uint32_t W = 0, H = 0;

	// settings
	int integrator = 0; // 0 parity, 1 pt
	int spp = 1;
	int max_depth = 2;
	int jitter = 0; // 0 xor128, 1 center
	int stage_timing = 0;
	int count_traversal = 0;
	int builder = 0;	// 0 host (binned SAH), 1 device (Morton / Karras, lbvh.hip)
	DevBuf d_lbvh_scratch;
	int sampler = 0;	// 0 hash RNG, 1 blue noise
	DevBuf d_blue_noise;
	bool have_blue_noise = false;
	int lds_nodes = -1; // -1: as many as the kernels hold (rtk::max_lds_nodes())
	int refill = 15; // persistent lanes on — bit 0: extension waves, bit 1: shadow waves (off: the one-ray-per-lane kernels, kept as
					// a cross-check of the persistent-lane ones), bit 3: the pt primary wave in packet form (wave-uniform traversal,
					// kernels.hip: trace_packet; off: one ray per lane); bit 2 selected round 2's persistent-lane primary kernel, which
					// round 5 removed — accepted and ignored
	bool packet_ok = false; // the scene's trees fit the packet kernel's stack and its 32-bit node offsets
	int streams = 4; // sub-batches of one render call that run concurrently on their own HIP streams
	long long sub_batch_paths = 50000000; // a render call is cut into sub-batches only if each gets at least this many path slots
	int flat_instances = 1; // identity-transform instances of singly used meshes are linked into the top-level tree directly, and
							// static instances that are used several times or transformed are written out in world space (world tree)
	bool depth_stats_valid = false; // c->stats counts paths of the CURRENT scene (depth_items)
	int shadow_packets = -1;		// the connection wave of the primary vertices in packet form (kernels.hip: k_shadow_packet) where it applies:
									// 1 always, 0 never, -1 (default) while the runs it sorts hold few light bins (shadow_bins_per_run)
	int group_flags = 1;				// the packet form of the pt primary wave flags the 64-slot groups it finishes; the shade scan passes them by
	int shadow_side = 1;				// ... on the sub-batch's connection stream, beside the extension wave of depth 1 (0: on the sub-batch's own
									// stream, in front of it — what a per-stage timing wants)
	bool shadow_packets_auto_on = true; // -1: what the last waited frame's bins per run said (reset to true by rfwhip_update)
	double shadow_bins_per_run = 0.0;
	unsigned long long sp_at_wait[MAX_SUB][2] = {};
	unsigned long long fused_ticks_at_wait[MAX_SUB][rt::MAX_DEPTH_SLOTS][2] = {}; // WaveCounters::fused_ticks at the last rfwhip_wait, per counter set
	long long flatten_bytes = 1ll << 28; // ... as long as the world-space copy stays below this many bytes (256 MiB = 2.4 M triangles:
										 // the tree is built on the host inside rfwhip_update, ~0.2 s per million triangles on 16 cores)
	WorldRec wtree;
	int sample_group = 64; // slot layout: up to this many samples of a pixel share a wave (rt_core.h; the largest power of two
						   // <= this that divides every sub-batch of the call is used; 1 = a wave is one 8x8 tile of one sample;
						   // 64 = a wave is ONE pixel: primary wave 3.67 instead of 4.01 ms per 32 spp, depth-0 shadow wave -7 %)
	uint32_t sgroup_last = 0; // log2 of the group the most recent render call used
	int fuse = 1;	  // extension rays of depth d + 1 and shadow rays of depth d in one launch (kernels.hip: k_trace_fused)
	int overlap = -1; // connection waves beside the next depth's stages on a second stream: 0 off, 1 on, -1 by launch size
	// denoiser of the presented image (denoise.h): knobs, buffers of the full image, the guides' cache key
	int denoise = 0;
	int dn_iterations = 5;
	float dn_sigma_l = 4.0f, dn_sigma_n = 128.0f, dn_sigma_z = 1.0f;
	DevBuf d_dn_guides, d_dn_img, d_dn_var; // 2 x 16 B, 2 x 16 B, 2 x 4 B per pixel
	bool guides_valid = false;				 // the guides were computed for guide_cam / guide_scene / guide_W x guide_H
	rfwhip_camera guide_cam, last_cam;		 // ... and the camera of the most recent rfwhip_render
	bool have_last_cam = false;
	unsigned long long scene_version = 0, guide_scene = 0; // scene_version: rfwhip_update calls
	uint32_t guide_W = 0, guide_H = 0;
	// ... its temporal stage (setting "denoise_temporal"): P = the last presented frame, F = the frame being presented
	int dn_temporal = 0;
	float dn_alpha = 0.2f;
	DevBuf d_dn_prev, d_dn_ids, d_dn_hist, d_dn_inst_ver; // P's guides (16 B), ids of F | P (2 x 4 B), 2 history sets (2 x 28 B) per pixel
	unsigned long long frame_serial = 0;	// rfwhip_render calls
	unsigned long long samples_total = 0; // samples per pixel rendered since rfwhip_init (the sample origin of a RESET)
	uint32_t sample_origin = 0;			// the pt integrator's sample indices start here (0 unless denoise_temporal)
	bool dn_have_pres = false;				// a frame P has been presented since the history was last cleared
	unsigned long long dn_pres_serial = 0;	// ... its render serial
	rt::CamView dn_pres_cam{};				// ... its camera, the scene version and size of its guides
	uint32_t dn_pres_scene = 0, dn_pres_W = 0, dn_pres_H = 0;
	bool dn_guides_pres = false;			// d_dn_guides / ids still hold P's guides
	bool dn_prev_ok = false;				// d_dn_prev / P's ids hold the guides of frame dn_saved_serial
	unsigned long long dn_saved_serial = 0;
	bool dn_reset_since = false;			// a RESET render since P was presented
	int dn_hist_cur = 0;					// the history set P's stage wrote
	bool dn_t_usable = false;				// the stage of the last presented frame: history usable, P's camera and scene version
	rt::CamView dn_t_pcam{};
	uint32_t dn_t_pscene = 0;
	std::vector<uint32_t> dn_inst_ver;		// per instance: InstRec::dn_version (uploaded into d_dn_inst_ver)
	bool dn_inst_ver_stale = true;			// d_dn_inst_ver is missing or older than dn_inst_ver: uploaded before the next stage
	// ... and its motion part (setting "denoise_motion"): the surface record of the current guides (16 B per pixel), the instances as
	// the current guides (g) and P's guides (p) traced them, and the stage's per-instance table (host copy + device copy)
	int dn_motion = 0;
	DevBuf d_dn_surf, d_dn_minst;
	std::vector<DnInstSnap> dn_g_rec, dn_p_rec;
	bool dn_g_rec_ok = false, dn_p_rec_ok = false; // (recorded by a guide pass that ran with the setting on)
	unsigned long long dn_pres_id = 1;		// counts presented frames: the tag of the meshes' vertex snapshots
	unsigned long long dn_edit_count = 0;	// counts rfwhip_set_mesh / pose / morph calls
	std::vector<rtk::DnMotionInst> dn_mtab; // the table of the last presented frame's stage ...
	uint32_t dn_mtab_scene = 0;				// ... valid for a further read of that frame while no update and no mesh edit followed
	unsigned long long dn_mtab_edits = 0;
	bool dn_mtab_stale = true;

	// scene (host side)
	std::vector<MeshRec> meshes;
	std::vector<InstRec> instances;
	rfwhip_light_count lc = {0, 0, 0, 0};
	bool scene_dirty = true;

	// scene (device side)
	DevBuf d_nodes4f; // float form of d_nodes4 (rt::Node4f), refreshed at the end of every rfwhip_update that may need it
	bool nodes4f_current = false; // ... which is when the packet form of the primary wave can run (packet_ok, refill bit 3)
	size_t nodes4_live = 0;		  // 4-wide nodes in use: all mesh trees + the top-level tree
	// the primary wave's camera-ordered copy of d_nodes4f (primary_order.h): same size, same indexing.  It holds
	// the order for camera position ord_cam (bits) of table version ord_version; a render call whose primary wave wants it and finds it
	// stale rewrites it on the main stream in front of its sub-batches, which wait for that (order_pub)
	int primary_order = -1; // RFWHIP_PRIMARY_ORDER as the context was created: 0 never, 1 wherever the packet form runs, else by call size
	DevBuf d_nodes4f_ord;
	std::vector<OrderRange> ord_ranges; // the trees that have ONE origin, as the last rfwhip_update laid them out (the rest is copied)
	unsigned long long nodes4f_version = 0, ord_version = 0; // nodes4f_version: rewrites of d_nodes4f
	bool ord_valid = false;
	uint32_t ord_cam[3] = {0, 0, 0};
	Published order_pub;
	// the primary wave's entry snapshot (primary_entry.h): one record per 64-slot group of one sample group, for the
	// view, frame layout and ordered table of ent_key; rewritten like the ordered table, on the main stream behind the ordering pass
	int primary_entry = -1; // setting: 0 never, 1 wherever the ordered table is used without a lens, -1 where the pass also pays (ensure_primary_entry)
	uint32_t ent_last_key[32] = {}; // the key of the previous call that could have used records: the same again = the view is at rest
	bool primary_entry_last = false; // did the last render call's primary wave start from the snapshot?
	DevBuf d_primary_entry;
	bool ent_valid = false;
	uint32_t ent_key[32] = {};
	Published entry_pub;
	DevBuf d_nodes, d_nodes4, d_nodes4_src, d_tri_verts, d_tri_shade, d_tri_uv, d_tlas_prims, d_instances;
	size_t blas_nodes4 = 0, node4_capacity = 0; // d_nodes4 = [all BLAS 4-wide nodes | TLAS 4-wide nodes | spare]
	DevBuf d_materials, d_textures, d_tex_u32, d_tex_f4, d_sky, d_area, d_point, d_spot, d_dir;
	uint32_t material_count = 0, texture_count = 0, sky_w = 0, sky_h = 0;
	bool textured = false; // some material carries a map
	// setting material_maps: the setting, and whether some material of the last rfwhip_set_materials has a
	// present alpha, roughness or metallic map (present: the flag and a texture of the last rfwhip_set_textures) / a present mask
	int material_maps = 0;
	bool maps_present = false, mask_present = false;
	struct MapSlots { uint32_t flags, addr6, addr7, addr9; };
	std::vector<MapSlots> map_slots; // of the last rfwhip_set_materials, as resolved
	// sky sampling (sky_sampling.h): the settings, and what the last rfwhip_update made of them
	int sky_sampling = 0;
	float sky_pick = -1.0f;		 // -1: auto (1 without lights, 0.5 with)
	uint64_t sky_version = 0;	 // rfwhip_set_sky calls
	uint64_t sky_table_of = ~0ull; // the sky_version d_sky_alias was built from (~0: none)
	double sky_total = 0.0;		 // S of that table (0: no texel with a positive weight)
	DevBuf d_sky_alias;			 // allocated only while sky_sampling is on
	// the sky's loaders (sky_load.h): sky_table = 0 host | 1 device: who builds d_sky_alias; the record of the current table
	int sky_table = 0;
	int sky_table_by = -1; // the sky_table value d_sky_alias was built with (-1: none)
	rtk::SkyTabRecord sky_record = {0.0, 0, 0, 0, 0, {0, 0}};
	KindTimes skyload_times{9};	 // family KF_SKYLOAD by kernel: planes, texels, weights, total, scan_block, scan_super, scan_top,
								 // scan_apply, assign (the read-only setting sky_load_time)
	rt::SkyView sky_view{};		 // pick == 0: the default kernels run
	bool sky_stale = false;		 // a sky setting changed since: the next render (or update) refreshes the view
	// light sampling (light_tree.h): 0 reference, 1 linear, 2 tree; the tree of the lights of the last rfwhip_set_lights
	int light_sampling = 0;
	// the display stage (display.h): tone map 0 aces | 1 none, FXAA, sRGB encoding; d_display: where the host reads land
	int display_tonemap = 0, display_fxaa = 1, display_srgb = 0;
	DevBuf d_display;
	// the exposure meter (metering.h): the display_exposure* settings; d_meter_rec = the 32-byte record (allocated, with steps = 0 and
	// E = 1, by the first call that needs it), d_meter_hist = the summed histogram, d_meter_part = the partial records of one pass
	int exposure_auto = 0; // display_exposure: 0 manual, 1 auto
	float exposure_ev = 0.0f, exposure_key = 0.18f, exposure_low = 0.1f, exposure_high = 0.9f, exposure_speed = 1.0f;
	float exposure_min_ev = -16.0f, exposure_max_ev = 16.0f;
	DevBuf d_meter_rec, d_meter_hist, d_meter_part;
	bool meter_have = false;			   // rfwhip_read_display* has metered frame meter_serial under the settings as they stand
	unsigned long long meter_serial = 0;
	bool meter_manual_stale = true;		   // manual mode: the record's E is not (yet) exp2(display_exposure_ev)
	float meter_manual_E = 1.0f;		   // ... the value the next exposed display uploads (kept here: the copy's source)
	// bloom (bloom.h): the display_bloom* settings; d_bloom_pyr = the levels 1 .. 8 of the target's pyramid, one behind the other,
	// d_bloom_out = the image the display kernel reads, d_bloom_one = a float 1 (the E of an unexposed display) — allocated when the
	// setting is first on with a render target.  bloom_ran: the levels of the last chain (0: none since rfwhip_init)
	int bloom_on = 0, bloom_levels = 6;
	float bloom_intensity = 0.2f, bloom_threshold = 1.0f, bloom_knee = 0.5f, bloom_scatter = 0.7f;
	DevBuf d_bloom_pyr, d_bloom_out, d_bloom_one;
	uint32_t bloom_ran = 0;
	KindTimes bloom_times{4}; // family KF_BLOOM by kernel: k_bloom_down0, k_bloom_down, k_bloom_up, k_bloom_apply (display_bloom_time)
	// colour grading and dither (display_grade.h): the display_grade* settings; grade_wb = M_wb of the temperature, built in double;
	// lut_host = the LUT as it was set (n^3 triples), d_grade_lut = its float4 copy, uploaded when it is set
	int grade_on = 0, grade_dither = 0;
	float grade_temperature = 6500.0f, grade_wb[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
	float grade_slope[3] = {1, 1, 1}, grade_offset[3] = {0, 0, 0}, grade_power[3] = {1, 1, 1}, grade_sat = 1.0f;
	std::vector<float> lut_host;
	uint32_t lut_n = 0;
	DevBuf d_grade_lut;
	// baseline JPEG (display_jpeg.h): the display_jpeg_* settings; every buffer is allocated by the first encode: d_jpeg_tab = the
	// constant tables, d_jpeg_coef = the quantised blocks, d_jpeg_slots = the intervals' stuffed bytes, d_jpeg_counts / _offsets = the
	// interval tables, d_jpeg_rec / d_jpeg_out = the record and the stream of the calls that read back themselves
	int jpeg_quality = 90, jpeg_sub = 1, jpeg_restart = 8;
	DevBuf d_jpeg_tab, d_jpeg_coef, d_jpeg_slots, d_jpeg_counts, d_jpeg_offsets, d_jpeg_rec, d_jpeg_out;
	rtk::JpegRecord jpeg_rec_host = {0, 0, 0, 0, 0, 0, 0, 0}; // the last record this library read back
	uint32_t jpeg_coef_blocks = 0;						   // blocks of the last encode (rfwhip_read_jpeg_coefficients)
	KindTimes jpeg_times{4}; // family KF_JPEG by kernel: k_jpeg_blocks, k_jpeg_entropy, k_jpeg_offsets, k_jpeg_pack (display_jpeg_time)
	// image textures (texture_decode.h): texture_entropy = 0 auto | 1 host | 2 device; the scratch of a decode, allocated by the first
	// one (the stream, the intervals' ranges, the tables, the coefficients, the intervals' flags, the components' planes, the mip
	// tiles' alpha counts, an RGBA8 source, the sRGB table, the image of rfwhip_decode_image); d_td_rec: a record per texture
	int td_entropy = 0;
	DevBuf d_td_stream, d_td_ranges, d_td_tab, d_td_coef, d_td_flags, d_td_planes, d_td_alpha, d_td_src, d_td_lin, d_td_out, d_td_rec;
	std::vector<rtk::TexRecord> td_records; // of the current table's textures (zeros for textures that came as texels)
	std::vector<rt::TexDesc> tex_desc_host; // the current table's descriptors (rfwhip_read_texture)
	uint32_t td_coef_blocks = 0;			// blocks of the last decode (rfwhip_read_texture_coefficients)
	rtk::TexRecord td_hook_record = {0, 0, 0, 0, 0, 0, 0, 0}; // of the last rfwhip_decode_image (rfwhip_get_texture_decode, index -1)
	bool td_hook_ran = false;
	KindTimes texdec_times{6}; // family KF_TEXDEC by kernel: zero, entropy, idct, color, mips, finish (texture_decode_time)
	// the noise estimate (noise.h): d_noise = two moments per local pixel, allocated while noise_estimate is on.  noise_live: the
	// moments cover every sample of the accumulator (the setting was on at the last RESET / rfwhip_init and ever since)
	int noise_estimate = 0;
	float noise_floor = 0.01f, noise_threshold = 0.05f;
	bool noise_live = false;
	DevBuf d_noise, d_noise_map, d_noise_tiles, d_noise_total, d_noise_in;
	// adaptive sampling (adaptive.h): per noise tile a sample count and an active flag, per slot tile a mask byte; the buffers live and
	// die with d_noise.  adaptive_live: the state covers the accumulation (the setting was on, beside noise_estimate, at the last RESET /
	// rfwhip_init).  The setting takes effect, on AND off, with the next RESET or rfwhip_init: a tile's accumulator holds n_tile samples
	// and only the adaptive present scales it right
	int adaptive_sampling = 0, adaptive_min_samples = 16, adaptive_every = 4;
	bool adaptive_live = false;
	uint32_t adaptive_calls = 0; // render calls since the RESET
	DevBuf d_ad_n, d_ad_active, d_ad_mask;
	// the mask changed on the main stream (RESET, a decision call): it is published behind that, and a sub-batch stream acquires it
	// before its next primary wave.  No reader is noted: a decision call rewrites it behind its own epilogue on the main stream
	Published adaptive_pub;
	bool adaptive_mask_moved = false;
	DevBuf d_lt_nodes, d_lt_paths; // allocated only while light_sampling is tree
	rt::LightTreeView lt_view{};   // nodes == nullptr: linear (or no light with a position)
	bool lt_stale = false;		   // the setting changed since: the next render (or update) builds the tree
	// moving emitters (light_follow.h): the setting, "something a bound light depends on changed since the last refresh", what the
	// last refresh found, the level ranges of the tree as built and the refits it has had since
	int lights_follow = 0;
	bool lf_dirty = false;
	bool lt_rebuild_after_refresh = false; // rfwhip_set_lights under the setting: the next refresh is followed by a build, not a refit
	uint32_t lights_bound = 0, lt_refits = 0;
	rtk::LightTreeLevels lt_levels{};
	DevBuf d_lf_inst, d_lf_bound, d_lf_count, d_lt_touched;
	// animations (animation.h): the rigs by index, their views as the kernel reads them, the triples of the current call
	std::vector<RigRec> rigs;
	DevBuf d_rig_table, d_rig_calls;
	uint32_t tlas_root_entry = 0, instance_count = 0;
	rt::SceneView sv;

	// wave state
	// shadow-ray buffers: two sets (by depth parity) so that shade(d + 1) can write while connect(d) still reads;
	// radiance: two sets (by call parity) x {shade, connections}, so that a call can start while the previous one resolves
	DevBuf d_org[2], d_dir2[2], d_thr[2], d_hit, d_hit_inst, d_hit0, d_hit0_inst, d_hit0_done, d_sh_org[2], d_sh_dir[2], d_sh_rad[2],
		d_rad[2], d_rad_nee[2], d_acc, d_counters, d_packet_rng, d_jump_table, d_present;
	uint32_t samples_done = 0;
	size_t wave_capacity = 0; // path slots the wave buffers can hold
	size_t rad_capacity[2] = {0, 0}; // ... and the two radiance sets
	rt::FrameView fr;
	bool jump_table_uploaded = false;

	// xor128 stream position (EmbreeRT's m_Rng persists across frames, Context.h:78)
	uint32_t rng_state[4] = {123456789u, 362436069u, 521288629u, 88675123u};
	std::vector<uint32_t> jump_table; // 64 x 128 x 4

	uint32_t probe_x = 0, probe_y = 0;
	uint32_t probe_inst = 0, probe_prim = 0;
	float probe_dist = 0;

	// timing
	std::vector<TimedSpan> spans;
	std::vector<dm::event_t> event_pool;
	size_t events_used = 0;
	float kernel_ms[KF_COUNT] = {};
	uint32_t kernel_launches[KF_COUNT] = {};
	rfwhip_render_stats stats;
	std::chrono::steady_clock::time_point render_t0;
	bool render_in_flight = false; // rfwhip_render since the last rfwhip_wait
	rfwhip_counters totals;
	KindTimes *kind_times(int family) // the families that are timed by kernel
	{
		switch (family)
		{
		case KF_BLOOM: return &bloom_times;
		case KF_JPEG: return &jpeg_times;
		case KF_TEXDEC: return &texdec_times;
		case KF_SKYLOAD: return &skyload_times;
		default: return nullptr;
		}
	}
};

int Published::before_rewrite(rfwhip_context *c)
{
	for (int i = 0; i < rfwhip_context::MAX_SUB; i++)
		if (reader[i])
		{
			RF_TRY(dm::stream_wait_event(c->stream, c->ev_sub_done[i]));
			reader[i] = false;
		}
	return 0;
}

// =================================================================================================================
// small math
// =================================================================================================================
static void mat4_inverse(const float *m, float *inv)
{
	float t[16];
	t[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] + m[13] * m[6] * m[11] - m[13] * m[7] * m[10];
	t[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] - m[12] * m[6] * m[11] + m[12] * m[7] * m[10];
	t[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] + m[12] * m[5] * m[11] - m[12] * m[7] * m[9];
	t[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] - m[12] * m[5] * m[10] + m[12] * m[6] * m[9];
	t[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] - m[13] * m[2] * m[11] + m[13] * m[3] * m[10];
	t[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] + m[12] * m[2] * m[11] - m[12] * m[3] * m[10];
	t[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] - m[12] * m[1] * m[11] + m[12] * m[3] * m[9];
	t[13] = m[0] * m[9] * m[14] - m[0] * m[10] * m[13] - m[8] * m[1] * m[14] + m[8] * m[2] * m[13] + m[12] * m[1] * m[10] - m[12] * m[2] * m[9];
	t[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] + m[13] * m[2] * m[7] - m[13] * m[3] * m[6];
	t[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] - m[12] * m[2] * m[7] + m[12] * m[3] * m[6];
	t[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] + m[12] * m[1] * m[7] - m[12] * m[3] * m[5];
	t[14] = -m[0] * m[5] * m[14] + m[0] * m[6] * m[13] + m[4] * m[1] * m[14] - m[4] * m[2] * m[13] - m[12] * m[1] * m[6] + m[12] * m[2] * m[5];
	t[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] - m[5] * m[3] * m[10] - m[9] * m[2] * m[7] + m[9] * m[3] * m[6];
	t[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] + m[4] * m[3] * m[10] + m[8] * m[2] * m[7] - m[8] * m[3] * m[6];
	t[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] - m[4] * m[3] * m[9] - m[8] * m[1] * m[7] + m[8] * m[3] * m[5];
	t[15] = m[0] * m[5] * m[10] - m[0] * m[6] * m[9] - m[4] * m[1] * m[10] + m[4] * m[2] * m[9] + m[8] * m[1] * m[6] - m[8] * m[2] * m[5];
	float det = m[0] * t[0] + m[1] * t[4] + m[2] * t[8] + m[3] * t[12];
	det = 1.0f / det;
	for (int i = 0; i < 16; i++)
		inv[i] = t[i] * det;
}

// xor128 is GF(2)-linear: jump_table[k] = M^(2^k), 128 columns of 4 words each.
static uint32_t xor128_step(uint32_t s[4])
{
	const uint32_t t = s[0] ^ (s[0] << 11);
	s[0] = s[1], s[1] = s[2], s[2] = s[3];
	s[3] = s[3] ^ (s[3] >> 19) ^ (t ^ (t >> 8));
	return s[3];
}
static void gf2_apply(const uint32_t *m, uint32_t s[4])
{
	uint32_t r[4] = {0, 0, 0, 0};
	for (int w = 0; w < 4; w++)
		for (int b = 0; b < 32; b++)
			if ((s[w] >> b) & 1u)
			{
				const uint32_t *c = m + 4 * (w * 32 + b);
				r[0] ^= c[0], r[1] ^= c[1], r[2] ^= c[2], r[3] ^= c[3];
			}
	memcpy(s, r, 16);
}
static void build_jump_table(std::vector<uint32_t> &tab)
{
	tab.assign(64 * 512, 0u);
	for (int i = 0; i < 128; i++)
	{
		uint32_t e[4] = {0, 0, 0, 0};
		e[i / 32] = 1u << (i % 32);
		xor128_step(e);
		memcpy(&tab[4 * i], e, 16);
	}
	for (int k = 1; k < 64; k++)
		for (int i = 0; i < 128; i++)
		{
			uint32_t c[4];
			memcpy(c, &tab[512 * (k - 1) + 4 * i], 16);
			gf2_apply(&tab[512 * (k - 1)], c);
			memcpy(&tab[512 * k + 4 * i], c, 16);
		}
}
static void xor128_jump(const std::vector<uint32_t> &tab, uint32_t s[4], unsigned long long draws)
{
	for (int k = 0; k < 64; k++)
		if ((draws >> k) & 1ull)
			gf2_apply(&tab[512 * k], s);
}

static uint32_t total_light_count(const rfwhip_context *c)
{
	return c->lc.areaLightCount + c->lc.pointLightCount + c->lc.spotLightCount + c->lc.directionalLightCount;
}

static void set_sample_group(rt::FrameView &fr, uint32_t sgroup_log2)
{
	fr.sgroup_log2 = sgroup_log2;
	fr.div_group = rt::make_fastdiv((uint32_t)std::min<unsigned long long>((unsigned long long)fr.slots << sgroup_log2, 0x7FFFFFFFull));
}
static uint32_t local_rows_of(const rfwhip_context *c)
{
	const uint32_t strips = (c->H + rt::STRIP_ROWS - 1) / rt::STRIP_ROWS;
	return ((strips + c->world - 1) / c->world) * rt::STRIP_ROWS;
}

static int update_light_tree(rfwhip_context *c, const rt::AreaLight *h_area = nullptr, const rt::PointLight *h_point = nullptr,
							 const rt::SpotLight *h_spot = nullptr);
static int sync_all(rfwhip_context *c);

// =================================================================================================================
// lifetime
// =================================================================================================================
extern "C" int rfwhip_create(int device_ordinal, int rank, int world, rfwhip_context **out)
{
	if (!out || world < 1 || rank < 0 || rank >= world)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_create: bad arguments (rank %d, world %d)", rank, world);
	int cus = 0;
	RF_TRY(dm::init(device_ordinal, &cus));
	rfwhip_context *c = new rfwhip_context();
	c->device = device_ordinal, c->rank = rank, c->world = world, c->cus = cus;
	c->marks[MK_PRESENT].timed = c->marks[MK_DENOISE].timed = true;
	if (const char *e = getenv("RFWHIP_PRIMARY_ORDER")) // (an environment variable, read once per context: not a setting)
		c->primary_order = e[0] == '0' && !e[1] ? 0 : (e[0] == '1' && !e[1] ? 1 : -1);
	rtk::set_device_cus(cus);
	memset(&c->stats, 0, sizeof(c->stats));
	memset(&c->totals, 0, sizeof(c->totals));
	memset(&c->sv, 0, sizeof(c->sv));
	memset(&c->fr, 0, sizeof(c->fr));
	if (dm::stream_create(&c->stream))
	{
		delete c;
		return RFWHIP_ERR_HIP;
	}
	build_jump_table(c->jump_table);
	if (c->d_counters.ensure(sizeof(rt::WaveCounters)) || dm::zero(c->d_counters.p, sizeof(rt::WaveCounters), c->stream))
	{
		delete c;
		return RFWHIP_ERR_HIP;
	}
	*out = c;
	return RFWHIP_OK;
}

// the denoiser's temporal stage forgets every presented frame: the next one starts fresh
static void dn_clear_history(rfwhip_context *c)
{
	c->dn_have_pres = false, c->dn_guides_pres = false, c->dn_prev_ok = false, c->dn_reset_since = false;
	c->dn_p_rec_ok = false, c->dn_mtab_stale = true;
}

// "denoise_motion": keep the vertices the last presented frame's guide pass traced, in front of the first in-place edit of the mesh
// that follows it (called after sync_all, before the edit is enqueued on the context's stream).  No copy when the mesh has been
// edited since that guide pass (the vertices are no longer P's: its instances restart) or the snapshot is P's already.
static int dn_snapshot_mesh(rfwhip_context *c, MeshRec &m)
{
	c->dn_edit_count++;
	if (!c->dn_motion || !c->dn_temporal || !c->denoise || c->rank != 0 || !c->dn_have_pres || !c->dn_p_rec_ok)
		return 0;
	if (m.dn_snap_pres == c->dn_pres_id || m.edits != m.dn_p_edits || !m.d_verts.p)
		return 0;
	RF_TRY(m.d_dn_snap.ensure(m.vertexCount * sizeof(f4)));
	RF_TRY(dm::d2d(m.d_dn_snap.p, m.d_verts.p, m.vertexCount * sizeof(f4), c->stream));
	m.dn_snap_pres = c->dn_pres_id;
	return 0;
}

static void free_all(rfwhip_context *c)
{
	for (auto &m : c->meshes)
	{
		DevBuf *mb[] = {&m.d_verts, &m.d_indices, &m.d_parents, &m.d_flags, &m.d_base_verts, &m.d_base_normals, &m.d_joints,
						&m.d_weights, &m.d_vnormals, &m.d_joint_mats, &m.d_tgt_pos, &m.d_tgt_nrm, &m.d_morph_weights,
						&m.d_b_nodes, &m.d_b_nodes4, &m.d_b_src, &m.d_b_tri_verts, &m.d_dn_snap};
		for (DevBuf *b : mb)
			b->free_();
	}
	for (auto &r : c->rigs)
		r.d_tables.free_(), r.d_state.free_();
	c->rigs.clear(), c->d_rig_table.free_(), c->d_rig_calls.free_();
	c->d_lbvh_scratch.free_(), c->d_blue_noise.free_();
	c->have_blue_noise = false;
	DevBuf *bufs[] = {&c->d_nodes4, &c->d_nodes4f, &c->d_nodes4f_ord, &c->d_primary_entry, &c->d_nodes4_src, &c->d_nodes, &c->d_tri_verts, &c->d_tri_shade, &c->d_tri_uv, &c->d_tlas_prims, &c->d_instances,
					  &c->d_materials, &c->d_textures, &c->d_tex_u32, &c->d_tex_f4, &c->d_sky, &c->d_area, &c->d_point,
					  &c->d_spot, &c->d_dir, &c->d_org[0], &c->d_org[1], &c->d_dir2[0], &c->d_dir2[1], &c->d_thr[0],
					  &c->d_thr[1], &c->d_hit, &c->d_hit_inst, &c->d_hit0, &c->d_hit0_inst, &c->d_hit0_done, &c->d_sh_org[0], &c->d_sh_org[1],
					  &c->d_sh_dir[0], &c->d_sh_dir[1], &c->d_sh_rad[0], &c->d_sh_rad[1], &c->d_rad[0], &c->d_rad[1],
					  &c->d_rad_nee[0], &c->d_rad_nee[1], &c->d_acc, &c->d_counters, &c->d_packet_rng, &c->d_jump_table,
					  &c->d_present, &c->d_dn_guides, &c->d_dn_img, &c->d_dn_var, &c->d_dn_prev, &c->d_dn_ids, &c->d_dn_hist,
					  &c->d_dn_inst_ver, &c->d_dn_surf, &c->d_dn_minst, &c->d_sky_alias, &c->d_lt_nodes, &c->d_lt_paths, &c->d_display,
					  &c->d_meter_rec, &c->d_meter_hist, &c->d_meter_part, &c->d_bloom_pyr, &c->d_bloom_out, &c->d_bloom_one, &c->d_grade_lut,
					  &c->d_jpeg_tab, &c->d_jpeg_coef, &c->d_jpeg_slots, &c->d_jpeg_counts, &c->d_jpeg_offsets, &c->d_jpeg_rec, &c->d_jpeg_out,
					  &c->d_td_stream, &c->d_td_ranges, &c->d_td_tab, &c->d_td_coef, &c->d_td_flags, &c->d_td_planes, &c->d_td_alpha, &c->d_td_src,
					  &c->d_td_lin, &c->d_td_out, &c->d_td_rec,
					  &c->d_noise, &c->d_noise_map, &c->d_noise_tiles, &c->d_noise_total, &c->d_noise_in,
					  &c->d_ad_n, &c->d_ad_active, &c->d_ad_mask, &c->d_lf_inst, &c->d_lf_bound, &c->d_lf_count, &c->d_lt_touched};
	for (DevBuf *b : bufs)
		b->free_();
	c->noise_live = false, c->adaptive_live = false;
	c->ord_valid = false, c->ent_valid = false;
	for (StreamMark &m : c->marks)
		m.destroy();
	c->meter_have = false, c->meter_manual_stale = true;
	c->bloom_ran = 0;
	c->lut_host.clear(), c->lut_n = 0;
	c->td_records.clear(), c->tex_desc_host.clear(), c->td_coef_blocks = 0;
	c->jpeg_coef_blocks = 0;
	c->guides_valid = false;
	dn_clear_history(c);
	c->dn_inst_ver_stale = true;
	for (auto &e : c->event_pool)
		dm::event_destroy(e);
	c->event_pool.clear();
	for (int i = 0; i < rfwhip_context::MAX_SUB; i++)
		c->d_counters_sub[i].free_();
	if (c->events_ready)
	{
		dm::event_destroy(c->ev_prologue);
		for (int r = 0; r < rfwhip_context::MAX_RING; r++)
			dm::event_destroy(c->ev_resolve[r]);
		dm::event_destroy(c->ev_present_in);
		dm::event_destroy(c->adaptive_pub.ev), dm::event_destroy(c->order_pub.ev), dm::event_destroy(c->entry_pub.ev);
		for (int i = 0; i < rfwhip_context::MAX_SUB; i++)
		{
			dm::event_destroy(c->ev_sub_done[i]), dm::event_destroy(c->ev_conn_last[i]);
			for (int d = 0; d < rt::MAX_DEPTH_SLOTS; d++)
				dm::event_destroy(c->ev_shade[i][d]), dm::event_destroy(c->ev_conn[i][d]);
		}
		c->events_ready = false;
	}
	for (int i = 0; i < rfwhip_context::MAX_SUB; i++)
	{
		dm::stream_destroy(c->sub_stream[i]), dm::stream_destroy(c->conn_stream[i]);
		c->sub_stream[i] = nullptr, c->conn_stream[i] = nullptr;
		c->conn_used[i] = false;
	}
	for (int r = 0; r < rfwhip_context::MAX_RING; r++)
		c->resolve_recorded[r] = false;
	c->ring_active = 0, c->call_slot = 0;
	c->wave_capacity = 0, c->rad_capacity[0] = c->rad_capacity[1] = 0;
	c->blas_nodes4 = 0, c->node4_capacity = 0;
}

extern "C" int rfwhip_cleanup(rfwhip_context *c)
{
	if (!c)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "null context");
	if (c->cleaned)
		return RFWHIP_OK; // the reference calls cleanup() twice on unload
	dm::use(c->device);
	if (c->stream)
		(void)sync_all(c); // every stream of the context and a present still pending on a caller's stream
	free_all(c);
	c->meshes.clear(), c->instances.clear(), c->wtree = WorldRec();
	c->cleaned = true;
	return RFWHIP_OK;
}

extern "C" void rfwhip_destroy(rfwhip_context *c)
{
	if (!c)
		return;
	rfwhip_cleanup(c);
	dm::stream_destroy(c->stream);
	delete c;
}

static int dn_ensure(rfwhip_context *c);
// the moments of the noise estimate start over with the accumulator (RESET, rfwhip_init); off: no buffer
// the metric's view of `moments` (local layout of `rows` x W) with n samples per pixel; the outputs are the context's buffers
static rtk::NoiseView noise_view(rfwhip_context *c, const float *moments, uint32_t W, uint32_t H, uint32_t rows, uint32_t rank, uint32_t world, uint32_t n)
{
	rtk::NoiseView v;
	v.W = W, v.H = H, v.local_rows = rows, v.rank = rank, v.world = world, v.n = n;
	v.moments = moments, v.e_map = c->d_noise_map.as<float>(), v.tiles = c->d_noise_tiles.as<rtk::NoiseTile>();
	v.total = c->d_noise_total.as<rtk::NoiseTotal>();
	v.floor_ = c->noise_floor, v.threshold = c->noise_threshold;
	return v;
}
static rtk::AdaptiveView adaptive_view(rfwhip_context *c, uint32_t local_rows, uint32_t width)
{
	rtk::AdaptiveView a;
	a.ntx = rtk::noise_tiles_x(width), a.count = a.ntx * (local_rows / rtk::NZ_TILE_Y);
	a.tiles_x = (width + rt::TILE - 1) / rt::TILE, a.min_samples = (uint32_t)c->adaptive_min_samples;
	a.n_tile = c->d_ad_n.as<uint32_t>(), a.active = c->d_ad_active.as<unsigned char>(), a.mask = c->d_ad_mask.as<unsigned char>();
	a.tiles = c->d_noise_tiles.as<rtk::NoiseTile>();
	return a;
}
static rtk::AdaptiveView adaptive_view(rfwhip_context *c) { return adaptive_view(c, c->fr.local_rows, c->W); }
static int noise_clear(rfwhip_context *c, uint32_t local_rows, uint32_t width, void *stream)
{
	const bool was_adaptive = c->adaptive_live;
	c->noise_live = c->noise_estimate != 0;
	c->adaptive_live = c->noise_live && c->adaptive_sampling != 0;
	c->adaptive_calls = 0;
	if (was_adaptive && !c->adaptive_live)
	{
		RF_TRY(sync_all(c)); // (a primary wave or a present in flight may still read them)
		c->d_ad_n.free_(), c->d_ad_active.free_(), c->d_ad_mask.free_();
	}
	if (!c->noise_live)
		return RFWHIP_OK;
	const size_t bytes = (size_t)local_rows * width * 2u * sizeof(float);
	const uint32_t tiles = rtk::noise_tiles_x(width) * (local_rows / rtk::NZ_TILE_Y);
	const size_t mask_bytes = ((size_t)((width + rt::TILE - 1) / rt::TILE) * (local_rows / rt::TILE) + 7u) & ~(size_t)3u; // (whole words: a scalar load per wave)
	if (bytes > c->d_noise.cap || (c->adaptive_live && ((size_t)tiles * 4u > c->d_ad_n.cap || mask_bytes > c->d_ad_mask.cap)))
		RF_TRY(sync_all(c));
	RF_TRY(c->d_noise.ensure(bytes));
	RF_TRY(dm::zero(c->d_noise.p, bytes, stream));
	if (c->adaptive_live)
	{
		// (the decision calls run the metric: its buffers are the queries')
		RF_TRY(c->d_noise_map.ensure((size_t)local_rows * width * sizeof(float)));
		RF_TRY(c->d_noise_tiles.ensure((size_t)tiles * sizeof(rtk::NoiseTile)));
		RF_TRY(c->d_noise_total.ensure(sizeof(rtk::NoiseTotal)));
		RF_TRY(c->d_ad_n.ensure((size_t)tiles * 4u));
		RF_TRY(c->d_ad_active.ensure(tiles));
		RF_TRY(c->d_ad_mask.ensure(mask_bytes));
		RF_TRY(dm::zero(c->d_ad_mask.p, mask_bytes, stream));
		rtk::launch_adaptive_reset(adaptive_view(c, local_rows, width), stream);
		RF_TRY(dm::last_launch_error());
		c->adaptive_mask_moved = true;
	}
	return RFWHIP_OK;
}

#define CTX_ENTER(c)                                                                      \
	if (!(c))                                                                             \
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "null context");                    \
	if ((c)->cleaned)                                                                     \
		return set_error(RFWHIP_ERR_STATE, "context already cleaned up");                 \
	RF_TRY(dm::use((c)->device))

extern "C" int rfwhip_init(rfwhip_context *c, uint32_t width, uint32_t height)
{
	CTX_ENTER(c);
	if (!width || !height || width > 65536 || height > 65536)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_init: bad target size %ux%u", width, height);
	RF_TRY(sync_all(c));
	c->W = width, c->H = height;
	c->d_dn_guides.free_(), c->d_dn_img.free_(), c->d_dn_var.free_(); // (re-allocated at the new size while denoise is on)
	c->d_dn_prev.free_(), c->d_dn_ids.free_(), c->d_dn_hist.free_(), c->d_dn_surf.free_();
	c->guides_valid = false;
	dn_clear_history(c);
	c->d_bloom_pyr.free_(), c->d_bloom_out.free_(), c->bloom_ran = 0; // (the pyramid's layout is the target's; back with the next chain)
	c->samples_total = 0, c->sample_origin = 0;
	if (c->denoise && c->rank == 0)
		RF_TRY(dn_ensure(c));
	const uint32_t lr = local_rows_of(c);
	RF_TRY(c->d_acc.ensure((size_t)lr * width * sizeof(f4)));
	RF_TRY(dm::zero(c->d_acc.p, (size_t)lr * width * sizeof(f4), c->stream));
	c->samples_done = 0;
	RF_TRY(noise_clear(c, lr, width, c->stream));
	c->fr.W = width, c->fr.H = height, c->fr.local_rows = lr;
	c->fr.inv_w = 1.0f / (float)width, c->fr.inv_h = 1.0f / (float)height;
	c->fr.tiles_x = (width + rt::TILE - 1) / rt::TILE;
	c->fr.div_tiles_x = rt::make_fastdiv(c->fr.tiles_x);
	c->fr.slots = c->fr.tiles_x * rt::TILE * lr;
	set_sample_group(c->fr, 0);
	c->fr.rank = (uint32_t)c->rank, c->fr.world = (uint32_t)c->world;
	return RFWHIP_OK;
}

// =================================================================================================================
// scene
// =================================================================================================================
extern "C" int rfwhip_set_sky(rfwhip_context *c, const float *rgb, size_t width, size_t height)
{
	CTX_ENTER(c);
	if (!rgb || !width || !height)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_set_sky: empty sky");
	std::vector<f4> px(width * height);
	for (size_t i = 0; i < width * height; i++)
		px[i] = f4{rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], 0.0f};
	RF_TRY(sync_all(c));
	RF_TRY(c->d_sky.ensure(px.size() * sizeof(f4)));
	RF_TRY(dm::h2d(c->d_sky.p, px.data(), px.size() * sizeof(f4), c->stream));
	RF_TRY(dm::sync(c->stream));
	c->sky_w = (uint32_t)width, c->sky_h = (uint32_t)height;
	c->sky_version++;
	c->scene_dirty = true;
	return RFWHIP_OK;
}

extern "C" int rfwhip_set_blue_noise(rfwhip_context *c, const uint32_t *table, size_t words)
{
	CTX_ENTER(c);
	if (!table || words < rt::BLUE_NOISE_WORDS)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_set_blue_noise: the table has 5 x 65536 words");
	RF_TRY(sync_all(c));
	RF_TRY(c->d_blue_noise.ensure(rt::BLUE_NOISE_WORDS * sizeof(uint32_t)));
	RF_TRY(dm::h2d(c->d_blue_noise.p, table, rt::BLUE_NOISE_WORDS * sizeof(uint32_t), c->stream));
	RF_TRY(dm::sync(c->stream));
	c->have_blue_noise = true;
	return RFWHIP_OK;
}

// material_maps: is a slot 6, 7 or 9 of some material present (its flag bit 4, 5 or 13, and a texture behind its address)?
static void update_maps_present(rfwhip_context *c)
{
	c->maps_present = false, c->mask_present = false;
	for (const auto &m : c->map_slots)
	{
		const bool mask = (m.flags >> 13 & 1u) && m.addr9 < c->texture_count;
		c->mask_present = c->mask_present || mask;
		c->maps_present = c->maps_present || mask || ((m.flags >> 4 & 1u) && m.addr6 < c->texture_count) || ((m.flags >> 5 & 1u) && m.addr7 < c->texture_count);
	}
}
// which kernels the next render runs: the MAPS variants (pt shade waves) / the guide pass's variant
static bool material_maps_on(const rfwhip_context *c) { return c->material_maps && c->maps_present; }

extern "C" int rfwhip_set_textures(rfwhip_context *c, const rfwhip_texture *tex, size_t count)
{
	CTX_ENTER(c);
	if (count && !tex)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_set_textures: null array");
	std::vector<rt::TexDesc> desc(count);
	std::vector<uint32_t> u32;
	std::vector<f4> f4s;
	for (size_t i = 0; i < count; i++)
	{
		rt::TexDesc &d = desc[i];
		memset(&d, 0, sizeof(d));
		d.type = tex[i].type, d.width = tex[i].width, d.height = tex[i].height, d.texelCount = tex[i].texelCount;
		if (!tex[i].data || !tex[i].texelCount)
			return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_set_textures: texture %zu has no data", i);
		if (tex[i].type == RFWHIP_TEX_UINT)
		{
			d.offset = (uint32_t)u32.size();
			const uint32_t *src = (const uint32_t *)tex[i].data;
			u32.insert(u32.end(), src, src + tex[i].texelCount);
		}
		else if (tex[i].type == RFWHIP_TEX_FLOAT4)
		{
			d.offset = (uint32_t)f4s.size();
			const f4 *src = (const f4 *)tex[i].data;
			f4s.insert(f4s.end(), src, src + tex[i].texelCount);
		}
		else
			return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_set_textures: texture %zu has unknown type %u", i, tex[i].type);
	}
	RF_TRY(sync_all(c));
	RF_TRY(c->d_textures.ensure(desc.size() * sizeof(rt::TexDesc)));
	RF_TRY(c->d_tex_u32.ensure(u32.size() * 4));
	RF_TRY(c->d_tex_f4.ensure(f4s.size() * sizeof(f4)));
	RF_TRY(dm::h2d(c->d_textures.p, desc.data(), desc.size() * sizeof(rt::TexDesc), c->stream));
	RF_TRY(dm::h2d(c->d_tex_u32.p, u32.data(), u32.size() * 4, c->stream));
	RF_TRY(dm::h2d(c->d_tex_f4.p, f4s.data(), f4s.size() * sizeof(f4), c->stream));
	RF_TRY(dm::sync(c->stream));
	c->texture_count = (uint32_t)count;
	update_maps_present(c);
	c->tex_desc_host = desc, c->td_records.assign(count, rtk::TexRecord{0, 0, 0, 0, 0, 0, 0, 0}); // (rfwhip_read_texture, rfwhip_get_texture_decode)
	c->scene_dirty = true;
	return RFWHIP_OK;
}

extern "C" int rfwhip_set_materials(rfwhip_context *c, const rfwhip_material *materials,
									const rfwhip_material_tex_ids *tex_ids, size_t count)
{
	CTX_ENTER(c);
	if (count && !materials)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_set_materials: null array");
	// Every map descriptor's address becomes the index of its texture in the set_textures array.  rfw::system leaves
	// only texaddr0 filled — with the id of the LAST map it packed (material_list.cpp:385-455 write texaddr0 for every
	// slot) — and hands the per-slot texture ids over in MaterialTexIds; a backend resolves them per slot
	// (CUDART/src/Context.cpp:171-190: texture[0..2] diffuse layers, [3..5] normal maps, [6] specularity,
	// [7] roughness, [9] colour mask, [10] alpha mask).  Without ids the descriptors are taken as they are.
	std::vector<rfwhip_material> mats(materials, materials + count);
	if (tex_ids)
	{
		static const int slot_of_id[11] = {0, 1, 2, 3, 4, 5, 6, 7, -1, 8, 9};
		for (size_t i = 0; i < count; i++)
			for (int k = 0; k < 11; k++)
				if (slot_of_id[k] >= 0 && tex_ids[i].texture[k] != -1)
					mats[i].map[slot_of_id[k]].addr = (uint32_t)tex_ids[i].texture[k];
	}
	RF_TRY(sync_all(c));
	RF_TRY(c->d_materials.ensure(count * sizeof(rfwhip_material)));
	RF_TRY(dm::h2d(c->d_materials.p, mats.data(), count * sizeof(rfwhip_material), c->stream));
	RF_TRY(dm::sync(c->stream));
	c->material_count = (uint32_t)count;
	// does any material use a map?  (bits 2..5, 7..10: diffuse / normal / specularity / roughness maps and their extra layers)
	c->textured = false;
	for (size_t i = 0; i < count; i++)
		c->textured = c->textured || (mats[i].flags & 0x7BCu) != 0;
	c->map_slots.resize(count);
	for (size_t i = 0; i < count; i++)
		c->map_slots[i] = {mats[i].flags, mats[i].map[6].addr, mats[i].map[7].addr, mats[i].map[9].addr};
	update_maps_present(c);
	c->scene_dirty = true;
	return RFWHIP_OK;
}

static void fill_shade_records(MeshRec &m, const rfwhip_triangle *tris)
{
	m.shade.resize(m.triCount);
	m.uv.resize(m.triCount);
	m.max_material = 0;
	for (size_t i = 0; i < m.triCount; i++)
	{
		const rfwhip_triangle &t = tris[i];
		rt::TriShade &s = m.shade[i];
		s.n0 = f4{t.vN0[0], t.vN0[1], t.vN0[2], t.Nx};
		s.n1 = f4{t.vN1[0], t.vN1[1], t.vN1[2], t.Ny};
		s.n2 = f4{t.vN2[0], t.vN2[1], t.vN2[2], t.Nz};
		float lt, mt;
		memcpy(&lt, &t.lightTriIdx, 4), memcpy(&mt, &t.material, 4);
		s.ex = f4{t.area, t.LOD, lt, mt};
		m.uv[i].tu = f4{t.u0, t.u1, t.u2, 0.0f};
		m.uv[i].tv = f4{t.v0, t.v1, t.v2, 0.0f};
		m.max_material = std::max(m.max_material, t.material);
	}
}

static inline void tri_indices(const rfwhip_mesh *mesh, size_t i, uint32_t &a, uint32_t &b, uint32_t &cidx)
{
	if (mesh->indices)
		a = mesh->indices[3 * i], b = mesh->indices[3 * i + 1], cidx = mesh->indices[3 * i + 2];
	else
		a = (uint32_t)(3 * i), b = a + 1, cidx = a + 2;
}

#ifndef RT_MAX_LEAF
#define RT_MAX_LEAF 4
#endif
constexpr int BLAS_MAX_LEAF = RT_MAX_LEAF; // triangles per leaf (<= rt::MAX_LEAF_PRIMS = 8)
// Traversal-stack budget (rt::STACK_CAPACITY entries per ray in every traversal kernel): a 4-wide node pushes at most 3
// entries and spans at least 2 BVH2 levels when it does, so a root-to-leaf path needs <= 1.5 entries per BVH2 level.
// The depth limits make the budgets hold by construction for the host builder (32 levels -> <= 48 entries, as deep as the
// reference's MAX_DEPTH, bvh_node.h:56-81; 14 levels -> <= 21 entries for the TLAS), and the exact need of every tree
// (bvh::stack_need4) is checked against them: BLAS + TLAS + 1 sentinel <= STACK_CAPACITY.
constexpr int BLAS_DEPTH_LIMIT = 32;
constexpr int TLAS_DEPTH_LIMIT = 14;
constexpr int BLAS_STACK_BUDGET = 48;
constexpr int TLAS_STACK_BUDGET = rt::STACK_CAPACITY - 1 - BLAS_STACK_BUDGET;
static_assert(TLAS_STACK_BUDGET >= (3 * TLAS_DEPTH_LIMIT) / 2 && BLAS_STACK_BUDGET >= (3 * BLAS_DEPTH_LIMIT) / 2, "traversal stack too small for the builders' depth limits");

// ---- refit of a resident mesh from its device vertices -------------------------------------------------------------------
// The chain on c->stream: the shading records of a posed mesh (skin_shade), the 2-wide tree bottom-up (refit), the compressed
// 4-wide nodes from it (refresh4).  skin_shade goes first wherever it runs: it writes d_tri_shade from d_verts / d_vnormals,
// which the other two only read, and nothing else of theirs — on one stream its place in the chain changes no result.
static int launch_refit_chain(rfwhip_context *c, MeshRec &m, bool shade)
{
	const uint32_t *indices = m.indexed ? m.d_indices.as<uint32_t>() : nullptr;
	if (shade)
		rtk::launch_skin_shade(c->d_tri_shade.as<rt::TriShade>() + m.shade_base, m.d_verts.as<f4>(), m.d_vnormals.as<f4>(), indices,
							   (uint32_t)m.triCount, c->stream);
	rtk::launch_refit(c->d_nodes.as<rt::Node>(), m.node_base, m.d_parents.as<int>(), m.node_count2, c->d_tri_verts.as<f4>(), m.tri_base,
					  m.d_verts.as<f4>(), indices, (uint32_t)m.triCount, m.d_flags.as<uint32_t>(), c->stream);
	rtk::launch_refresh4(c->d_nodes4.as<rt::Node4c>() + m.n4_base, c->d_nodes4_src.as<uint32_t>() + 4ull * m.n4_base, m.n4_count,
						 c->d_nodes.as<rt::Node>() + m.node_base, c->stream);
	return dm::last_launch_error();
}

// "stage_timing" of a refit: the events exist only when the setting is on, bracket what is enqueued on c->stream between the
// constructor and stop(), and are destroyed on every path out of the scope.  add() after the stream has been synchronised.
struct RefitTimer
{
	rfwhip_context *c;
	const bool timed;
	dm::event_t ea{}, eb{};
	explicit RefitTimer(rfwhip_context *c) : c(c), timed(c->stage_timing != 0)
	{
		if (timed)
		{
			dm::event_create(&ea), dm::event_create(&eb);
			dm::event_record(ea, c->stream);
		}
	}
	RefitTimer(const RefitTimer &) = delete;
	~RefitTimer()
	{
		if (timed)
			dm::event_destroy(ea), dm::event_destroy(eb);
	}
	void stop()
	{
		if (timed)
			dm::event_record(eb, c->stream);
	}
	void add(uint32_t launches)
	{
		if (!timed)
			return;
		c->kernel_ms[KF_REFIT] += dm::event_ms(ea, eb);
		c->kernel_launches[KF_REFIT] += launches;
		c->stats.animationTime = dm::event_ms(ea, eb);
	}
};

// rfwhip_pose_mesh / rfwhip_morph_mesh behind their vertex launch: the chain, the new mesh bounds, the bookkeeping
static int refit_deformed(rfwhip_context *c, MeshRec &m, RefitTimer &timer)
{
	RF_TRY(launch_refit_chain(c, m, true));
	timer.stop();
	// the instance boxes of the TLAS come from the mesh bounds = the refitted root (its two children's union)
	rt::Node root;
	RF_TRY(dm::d2h(&root, c->d_nodes.as<rt::Node>() + m.node_base, sizeof(rt::Node), c->stream)); // (synchronises the stream)
	for (int a = 0; a < 3; a++)
		m.bounds_min[a] = root.bmin[a] - 2e-5f, m.bounds_max[a] = root.bmax[a] + 2e-5f;
	timer.add(5);
	m.posed = true, m.edits++;
	c->scene_dirty = true, c->lf_dirty = true; // instance boxes change: the TLAS is rebuilt in update()
	return RFWHIP_OK;
}

extern "C" int rfwhip_set_mesh(rfwhip_context *c, size_t index, const rfwhip_mesh *mesh)
{
	CTX_ENTER(c);
	if (!mesh || !mesh->vertices || !mesh->triangles || !mesh->vertexCount || !mesh->triangleCount)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_set_mesh: empty mesh %zu", index);
	if (!mesh->indices && mesh->vertexCount < 3 * mesh->triangleCount)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_set_mesh: non-indexed mesh %zu needs 3 vertices per triangle", index);
	if (mesh->triangleCount > rt::ENTRY_FIRST_MASK)
		return set_error(RFWHIP_ERR_UNSUPPORTED, "rfwhip_set_mesh: more than 2^27 triangles in one mesh");
	if (mesh->indices)
		for (size_t i = 0; i < 3 * mesh->triangleCount; i++)
			if (mesh->indices[i] >= mesh->vertexCount)
				return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_set_mesh: index %u out of range in mesh %zu", mesh->indices[i], index);
	if (index >= c->meshes.size())
		c->meshes.resize(index + 1);
	MeshRec &m = c->meshes[index];
	const bool same_topology = m.used && m.resident && !m.dirty && m.vertexCount == mesh->vertexCount &&
							   m.triCount == mesh->triangleCount && m.indexed == (mesh->indices != nullptr);
	RF_TRY(sync_all(c));
	c->lf_dirty = true;
	if (same_topology)
		RF_TRY(dn_snapshot_mesh(c, m));
	else
		c->dn_edit_count++;
	// vertices / indices always go to the device (the refit kernels read them there)
	RF_TRY(m.d_verts.ensure(mesh->vertexCount * sizeof(f4)));
	RF_TRY(dm::h2d(m.d_verts.p, mesh->vertices, mesh->vertexCount * sizeof(f4), c->stream));
	if (mesh->indices)
	{
		RF_TRY(m.d_indices.ensure(mesh->triangleCount * 12));
		RF_TRY(dm::h2d(m.d_indices.p, mesh->indices, mesh->triangleCount * 12, c->stream));
	}
	m.vertexCount = mesh->vertexCount, m.triCount = mesh->triangleCount, m.indexed = mesh->indices != nullptr;
	m.used = true;
	m.posed = false; // host vertices again; skinning data (if any) stays valid while the counts stay
	if (m.skinned && !same_topology)
		m.skinned = false;
	if (m.morphed && !same_topology)
		m.morphed = false;
	fill_shade_records(m, mesh->triangles);
	// mesh bounds (for the instance boxes of the TLAS)
	for (int a = 0; a < 3; a++)
		m.bounds_min[a] = 1e34f, m.bounds_max[a] = -1e34f;
	const f4 *V = (const f4 *)mesh->vertices;
	if (same_topology)
	{
		m.refits++, m.edits++;
		// animated mesh: same counts => refit on the device (EmbreeRT/src/Mesh.cpp:33-35, top_level_bvh.cpp:26)
		for (size_t i = 0; i < mesh->triangleCount; i++)
		{
			uint32_t ia, ib, ic;
			tri_indices(mesh, i, ia, ib, ic);
			const uint32_t id[3] = {ia, ib, ic};
			for (int k = 0; k < 3; k++)
			{
				const f4 &p = V[id[k]];
				m.bounds_min[0] = std::min(m.bounds_min[0], p.x), m.bounds_max[0] = std::max(m.bounds_max[0], p.x);
				m.bounds_min[1] = std::min(m.bounds_min[1], p.y), m.bounds_max[1] = std::max(m.bounds_max[1], p.y);
				m.bounds_min[2] = std::min(m.bounds_min[2], p.z), m.bounds_max[2] = std::max(m.bounds_max[2], p.z);
			}
		}
		for (int a = 0; a < 3; a++)
			m.bounds_min[a] -= 2e-5f, m.bounds_max[a] += 2e-5f;
		RF_TRY(dm::h2d(c->d_tri_shade.as<rt::TriShade>() + m.shade_base, m.shade.data(), m.shade.size() * sizeof(rt::TriShade), c->stream));
		RF_TRY(dm::h2d(c->d_tri_uv.as<rt::TriUV>() + m.shade_base, m.uv.data(), m.uv.size() * sizeof(rt::TriUV), c->stream));
		RefitTimer timer(c);
		RF_TRY(launch_refit_chain(c, m, false));
		timer.stop();
		RF_TRY(dm::sync(c->stream));
		timer.add(3);
		c->scene_dirty = true; // instance boxes change: the TLAS is rebuilt in update()
		return RFWHIP_OK;
	}
	// (re)build.  From here on the record no longer describes what sits in the scene-wide arrays: whatever fails below, the
	// next set_mesh must not take the refit path and the next update must place the mesh again.
	m.dirty = true, m.resident = false;
	c->scene_dirty = true;
	// ... and until the build below has succeeded it describes NO tree (an error return leaves a mesh rfwhip_update() refuses,
	// not the counts of the previous build beside freed or half-written arrays)
	m.built = false, m.device_built = false, m.node_count2 = m.n4_count = 0, m.stack_need = 0;
	m.generation++, m.refits = 0, m.edits++;
	const size_t n = mesh->triangleCount;
	bool device_built = false;
	if (c->builder == 1 && n > (size_t)BLAS_MAX_LEAF)
	{
		// Construction on the device, end to end (lbvh.hip): Morton order, locally-ordered clustering, 4-wide collapse with
		// quantisation, depth-first triangle order — all into this mesh's own device arrays.  Only the counts, the stack
		// need and the root box come back; rfwhip_update() places the mesh with device-to-device copies.
		const size_t n2 = 2 * n;
		RF_TRY(c->d_lbvh_scratch.ensure(rtk::device_build_scratch_bytes((uint32_t)n)));
		RF_TRY(m.d_b_nodes.ensure(n2 * sizeof(rt::Node)));
		RF_TRY(m.d_parents.ensure(n2 * sizeof(int)));
		RF_TRY(m.d_flags.ensure(n2 * sizeof(uint32_t)));
		RF_TRY(m.d_b_nodes4.ensure(n * sizeof(rt::Node4c)));
		RF_TRY(m.d_b_src.ensure(4 * n * sizeof(uint32_t)));
		RF_TRY(m.d_b_tri_verts.ensure(3 * n * sizeof(f4)));
		const auto t0 = std::chrono::steady_clock::now();
		rtk::DeviceBuildResult res;
		const int rc = rtk::launch_device_build(m.d_verts.as<f4>(), m.indexed ? m.d_indices.as<uint32_t>() : nullptr, (uint32_t)n,
												c->d_lbvh_scratch.p, c->d_lbvh_scratch.cap, m.d_b_nodes.as<rt::Node>(),
												m.d_parents.as<int>(), m.d_flags.as<uint32_t>(), m.d_b_nodes4.as<rt::Node4c>(),
												m.d_b_src.as<uint32_t>(), m.d_b_tri_verts.as<f4>(), &res, c->stream);
		if (rc > 1 && rc != 5) // (5: the clustering did not converge within its pass budget — the host builder takes the mesh)
			return set_error(RFWHIP_ERR_HIP, "rfwhip_set_mesh: device BVH build failed (%d)", rc);
		RF_TRY(dm::last_launch_error());
		if (c->stage_timing)
		{
			c->kernel_ms[KF_REFIT] += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
			c->kernel_launches[KF_REFIT] += 1;
		}
		// a tree too deep for the traversal stack falls back to the host builder
		device_built = rc == 0 && (int)res.stack_need <= BLAS_STACK_BUDGET;
		if (device_built)
		{
			m.node_count2 = res.node_count, m.n4_count = res.node4_count, m.stack_need = (int)res.stack_need;
			for (int a = 0; a < 3; a++)
				m.bounds_min[a] = res.bmin[a], m.bounds_max[a] = res.bmax[a];
			m.bvh = bvh::Result(), m.n4.clear(), m.leaf_verts.clear();
		}
	}
	if (device_built)
	{
		RF_TRY(dm::sync(c->stream));
		m.device_built = true, m.built = true;
		return RFWHIP_OK;
	}
	if (!device_built)
	{
		std::vector<float> bmin(3 * n), bmax(3 * n);
		for (size_t i = 0; i < n; i++)
		{
			uint32_t ia, ib, ic;
			tri_indices(mesh, i, ia, ib, ic);
			const f4 &p0 = V[ia], &p1 = V[ib], &p2 = V[ic];
			// per-triangle box grown by 1e-5 (bvh_tree.cpp:407-412)
			bmin[3 * i + 0] = std::min(p0.x, std::min(p1.x, p2.x)) - 1e-5f, bmax[3 * i + 0] = std::max(p0.x, std::max(p1.x, p2.x)) + 1e-5f;
			bmin[3 * i + 1] = std::min(p0.y, std::min(p1.y, p2.y)) - 1e-5f, bmax[3 * i + 1] = std::max(p0.y, std::max(p1.y, p2.y)) + 1e-5f;
			bmin[3 * i + 2] = std::min(p0.z, std::min(p1.z, p2.z)) - 1e-5f, bmax[3 * i + 2] = std::max(p0.z, std::max(p1.z, p2.z)) + 1e-5f;
		}
		bvh::build(bmin.data(), bmax.data(), n, BLAS_MAX_LEAF, BLAS_DEPTH_LIMIT, m.bvh);
	}
	for (int a = 0; a < 3; a++)
		m.bounds_min[a] = m.bvh.nodes[0].bmin[a], m.bounds_max[a] = m.bvh.nodes[0].bmax[a];
	bvh::collapse4(m.bvh, false, m.n4);
	m.node_count2 = (uint32_t)m.bvh.nodes.size(), m.n4_count = (uint32_t)m.n4.size();
	m.stack_need = bvh::stack_need4(m.n4);
	if (m.stack_need > BLAS_STACK_BUDGET)
		return set_error(RFWHIP_ERR_UNSUPPORTED, "rfwhip_set_mesh: the BVH of mesh %zu needs %d traversal-stack entries (budget %d)",
						 index, m.stack_need, BLAS_STACK_BUDGET);
	m.leaf_verts.resize(3 * n);
	for (size_t s = 0; s < n; s++)
	{
		const uint32_t prim = m.bvh.order[s];
		uint32_t ia, ib, ic;
		tri_indices(mesh, prim, ia, ib, ic);
		float pw;
		memcpy(&pw, &prim, 4);
		m.leaf_verts[3 * s + 0] = f4{V[ia].x, V[ia].y, V[ia].z, pw};
		m.leaf_verts[3 * s + 1] = f4{V[ib].x, V[ib].y, V[ib].z, 1.0f};
		m.leaf_verts[3 * s + 2] = f4{V[ic].x, V[ic].y, V[ic].z, rt::TRI_EPS}; // (w: the triangle's determinant threshold, rt::tri_test)
	}
	RF_TRY(m.d_parents.ensure(m.bvh.parents.size() * sizeof(int)));
	RF_TRY(dm::h2d(m.d_parents.p, m.bvh.parents.data(), m.bvh.parents.size() * sizeof(int), c->stream));
	RF_TRY(m.d_flags.ensure(m.bvh.nodes.size() * sizeof(uint32_t)));
	RF_TRY(dm::sync(c->stream));
	m.built = true;
	return RFWHIP_OK;
}

extern "C" int rfwhip_set_instance(rfwhip_context *c, size_t index, size_t mesh_index, const float *transform16,
								   const float *normal_matrix9)
{
	CTX_ENTER(c);
	if (!transform16 || !normal_matrix9)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_set_instance: null matrix");
	if (mesh_index >= c->meshes.size() || !c->meshes[mesh_index].used)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_set_instance: instance %zu refers to unknown mesh %zu", index, mesh_index);
	if (index >= c->instances.size())
		c->instances.resize(index + 1);
	InstRec &in = c->instances[index];
	in.used = true, in.mesh = mesh_index;
	memcpy(in.transform, transform16, 64), memcpy(in.normal, normal_matrix9, 36);
	c->scene_dirty = true, c->lf_dirty = true;
	return RFWHIP_OK;
}

extern "C" int rfwhip_set_lights(rfwhip_context *c, rfwhip_light_count n, const rfwhip_area_light *area,
								 const rfwhip_point_light *point, const rfwhip_spot_light *spot,
								 const rfwhip_directional_light *directional)
{
	CTX_ENTER(c);
	if ((n.areaLightCount && !area) || (n.pointLightCount && !point) || (n.spotLightCount && !spot) ||
		(n.directionalLightCount && !directional))
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_set_lights: count > 0 with a null array");
	RF_TRY(sync_all(c));
	RF_TRY(c->d_area.ensure(n.areaLightCount * sizeof(rfwhip_area_light)));
	RF_TRY(c->d_point.ensure(n.pointLightCount * sizeof(rfwhip_point_light)));
	RF_TRY(c->d_spot.ensure(n.spotLightCount * sizeof(rfwhip_spot_light)));
	RF_TRY(c->d_dir.ensure(n.directionalLightCount * sizeof(rfwhip_directional_light)));
	RF_TRY(dm::h2d(c->d_area.p, area, n.areaLightCount * sizeof(rfwhip_area_light), c->stream));
	RF_TRY(dm::h2d(c->d_point.p, point, n.pointLightCount * sizeof(rfwhip_point_light), c->stream));
	RF_TRY(dm::h2d(c->d_spot.p, spot, n.spotLightCount * sizeof(rfwhip_spot_light), c->stream));
	RF_TRY(dm::h2d(c->d_dir.p, directional, n.directionalLightCount * sizeof(rfwhip_directional_light), c->stream));
	RF_TRY(dm::sync(c->stream));
	c->lc = n;
	c->scene_dirty = true, c->lf_dirty = true;
	c->lt_stale = true;
	// lights_follow_geometry=1: the host's geometry fields are about to be overwritten (and may be zeros), so the topology is not
	// made of them: the tree stays stale and rfwhip_update builds it from the lights its refresh derives
	c->lt_rebuild_after_refresh = c->lights_follow != 0;
	if (c->light_sampling == 2 && !c->lights_follow) // (static_asserts below: the ABI's light records are the kernels')
		RF_TRY(update_light_tree(c, reinterpret_cast<const rt::AreaLight *>(area), reinterpret_cast<const rt::PointLight *>(point),
								 reinterpret_cast<const rt::SpotLight *>(spot)));
	return RFWHIP_OK;
}

// ---- device skinning (not part of the RenderContext interface: rfw::system skins on the host,
// geometry/gltf/mesh.cpp:18-125, and hands the result to set_mesh) ---------------------------------------------------
extern "C" int rfwhip_set_mesh_skin(rfwhip_context *c, size_t index, const uint32_t *joints4, const float *weights4,
									const float *base_normals4, size_t vertex_count)
{
	CTX_ENTER(c);
	if (index >= c->meshes.size() || !c->meshes[index].used)
		return set_error(RFWHIP_ERR_STATE, "rfwhip_set_mesh_skin: mesh %zu has not been set", index);
	MeshRec &m = c->meshes[index];
	if (!joints4 || !weights4 || !base_normals4 || vertex_count != m.vertexCount)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_set_mesh_skin: need joints, weights and normals for the mesh's %zu vertices", m.vertexCount);
	if (m.posed)
		return set_error(RFWHIP_ERR_STATE, "rfwhip_set_mesh_skin: mesh %zu is posed; set_mesh the bind pose first", index);
	RF_TRY(sync_all(c));
	const size_t n = vertex_count;
	RF_TRY(m.d_base_verts.ensure(n * sizeof(f4)));
	RF_TRY(m.d_base_normals.ensure(n * sizeof(f4)));
	RF_TRY(m.d_vnormals.ensure(n * sizeof(f4)));
	RF_TRY(m.d_joints.ensure(n * 16));
	RF_TRY(m.d_weights.ensure(n * sizeof(f4)));
	RF_TRY(dm::d2d(m.d_base_verts.p, m.d_verts.p, n * sizeof(f4), c->stream)); // the vertices of the last set_mesh = bind pose
	RF_TRY(dm::h2d(m.d_base_normals.p, base_normals4, n * sizeof(f4), c->stream));
	RF_TRY(dm::h2d(m.d_joints.p, joints4, n * 16, c->stream));
	RF_TRY(dm::h2d(m.d_weights.p, weights4, n * sizeof(f4), c->stream));
	RF_TRY(dm::sync(c->stream));
	m.skinned = true;
	m.skin_max_joint = 0; // (for rfwhip_bind_rig: the skin it binds to must have this joint)
	for (size_t i = 0; i < 4 * n; i++)
		m.skin_max_joint = std::max(m.skin_max_joint, joints4[i]);
	return RFWHIP_OK;
}

extern "C" int rfwhip_pose_mesh(rfwhip_context *c, size_t index, const float *joint_matrices16, size_t joint_count)
{
	CTX_ENTER(c);
	if (index >= c->meshes.size() || !c->meshes[index].used || !c->meshes[index].skinned)
		return set_error(RFWHIP_ERR_STATE, "rfwhip_pose_mesh: mesh %zu has no skin (rfwhip_set_mesh_skin)", index);
	MeshRec &m = c->meshes[index];
	if (!joint_matrices16 || !joint_count)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_pose_mesh: no joint matrices");
	if (!m.resident || m.dirty)
		return set_error(RFWHIP_ERR_STATE, "rfwhip_pose_mesh: mesh %zu is not resident yet (rfwhip_update first)", index);
	RF_TRY(sync_all(c));
	RF_TRY(dn_snapshot_mesh(c, m));
	RF_TRY(m.d_joint_mats.ensure(joint_count * 64));
	RF_TRY(dm::h2d(m.d_joint_mats.p, joint_matrices16, joint_count * 64, c->stream));
	m.joint_count = (uint32_t)joint_count;
	RefitTimer timer(c);
	rtk::launch_skin_vertices(m.d_verts.as<f4>(), m.d_vnormals.as<f4>(), m.d_base_verts.as<f4>(), m.d_base_normals.as<f4>(),
							  m.d_joints.as<uint32_t>(), m.d_weights.as<f4>(), m.d_joint_mats.as<float>(), m.joint_count,
							  (uint32_t)m.vertexCount, c->stream);
	return refit_deformed(c, m, timer);
}

// float 4-wide node of the collapse -> the compressed node the rays fetch (entries as they are)
static rt::Node4c compress4(const rt::Node4 &nd)
{
	rt::Node4c out;
	bool valid[4];
	for (int k = 0; k < 4; k++)
		valid[k] = nd.entry[k] != rt::ENTRY_EMPTY, out.entry[k] = nd.entry[k];
	rt::pack_boxes4c(out, nd.lo, nd.hi, valid);
	return out;
}

// ---- device morph targets (geometry/gltf/mesh.cpp:127-147 on the device) ---------------------------------------
extern "C" int rfwhip_set_mesh_morph(rfwhip_context *c, size_t index, const float *base_normals4, const float *target_positions4,
									 const float *target_normals4, size_t target_count, size_t vertex_count)
{
	CTX_ENTER(c);
	if (index >= c->meshes.size() || !c->meshes[index].used)
		return set_error(RFWHIP_ERR_STATE, "rfwhip_set_mesh_morph: mesh %zu has not been set", index);
	MeshRec &m = c->meshes[index];
	if (!base_normals4 || !target_positions4 || !target_normals4 || !target_count || vertex_count != m.vertexCount)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_set_mesh_morph: need base normals and >= 1 target for the mesh's %zu vertices", m.vertexCount);
	if (m.posed)
		return set_error(RFWHIP_ERR_STATE, "rfwhip_set_mesh_morph: mesh %zu is posed; set_mesh the base pose first", index);
	RF_TRY(sync_all(c));
	const size_t n = vertex_count;
	RF_TRY(m.d_base_verts.ensure(n * sizeof(f4)));
	RF_TRY(m.d_base_normals.ensure(n * sizeof(f4)));
	RF_TRY(m.d_vnormals.ensure(n * sizeof(f4)));
	RF_TRY(m.d_tgt_pos.ensure(target_count * n * sizeof(f4)));
	RF_TRY(m.d_tgt_nrm.ensure(target_count * n * sizeof(f4)));
	RF_TRY(m.d_morph_weights.ensure(target_count * sizeof(float)));
	RF_TRY(dm::d2d(m.d_base_verts.p, m.d_verts.p, n * sizeof(f4), c->stream)); // the vertices of the last set_mesh = base pose
	RF_TRY(dm::h2d(m.d_base_normals.p, base_normals4, n * sizeof(f4), c->stream));
	RF_TRY(dm::h2d(m.d_tgt_pos.p, target_positions4, target_count * n * sizeof(f4), c->stream));
	RF_TRY(dm::h2d(m.d_tgt_nrm.p, target_normals4, target_count * n * sizeof(f4), c->stream));
	RF_TRY(dm::sync(c->stream));
	m.morphed = true, m.skinned = false;
	m.target_count = (uint32_t)target_count;
	return RFWHIP_OK;
}

extern "C" int rfwhip_morph_mesh(rfwhip_context *c, size_t index, const float *weights, size_t weight_count)
{
	CTX_ENTER(c);
	if (index >= c->meshes.size() || !c->meshes[index].used || !c->meshes[index].morphed)
		return set_error(RFWHIP_ERR_STATE, "rfwhip_morph_mesh: mesh %zu has no morph targets (rfwhip_set_mesh_morph)", index);
	MeshRec &m = c->meshes[index];
	if (!weights || weight_count != m.target_count)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_morph_mesh: mesh %zu has %u targets, got %zu weights", index, m.target_count, weight_count);
	if (!m.resident || m.dirty)
		return set_error(RFWHIP_ERR_STATE, "rfwhip_morph_mesh: mesh %zu is not resident yet (rfwhip_update first)", index);
	RF_TRY(sync_all(c));
	RF_TRY(dn_snapshot_mesh(c, m));
	RF_TRY(dm::h2d(m.d_morph_weights.p, weights, weight_count * sizeof(float), c->stream));
	RefitTimer timer(c);
	rtk::launch_morph_vertices(m.d_verts.as<f4>(), m.d_vnormals.as<f4>(), m.d_base_verts.as<f4>(), m.d_base_normals.as<f4>(),
							   m.d_tgt_pos.as<f4>(), m.d_tgt_nrm.as<f4>(), m.d_morph_weights.as<float>(), m.target_count,
							   (uint32_t)m.vertexCount, c->stream);
	return refit_deformed(c, m, timer);
}

// ---- animations on the device (work items and kernel: animation.h) ---------------------------------------
static_assert(sizeof(rfwhip_rig_node) == sizeof(rtk::RigNode) && sizeof(rfwhip_rig_skin) == sizeof(rtk::RigSkin) &&
				  sizeof(rfwhip_rig_animation) == sizeof(rtk::RigAnim) && sizeof(rfwhip_rig_channel) == sizeof(rtk::RigChannel) &&
				  sizeof(rfwhip_rig) == sizeof(rtk::RigSource) && sizeof(rfwhip_rig_status) == sizeof(rtk::RigStatus) &&
				  offsetof(rfwhip_rig_node, matrix) == offsetof(rtk::RigNode, matrix) && offsetof(rfwhip_rig, values) == offsetof(rtk::RigSource, values),
			  "rfwhip_abi.h: the rig's records are the kernel's (animation.h)");
static_assert(rtk::RIG_INVALID == RFWHIP_ERR_INVALID_ARGUMENT && rtk::RIG_WEIGHTS == RFWHIP_RIG_PATH_WEIGHTS && rtk::RIG_ROTATION == RFWHIP_RIG_PATH_ROTATION &&
				  rtk::RIG_CUBICSPLINE == RFWHIP_RIG_METHOD_CUBICSPLINE && rtk::RIG_LINEAR == RFWHIP_RIG_METHOD_LINEAR &&
				  rtk::RIG_READ_STATUS == RFWHIP_RIG_READ_STATUS && rtk::RIG_READ_JOINTS == RFWHIP_RIG_READ_JOINTS && rtk::RIG_BASE_POSE == RFWHIP_RIG_BASE_POSE,
			  "animation.h restates rfwhip_abi.h's codes");

static void rig_unbind_all(rfwhip_context *c, size_t rig_index)
{
	for (size_t mi : c->rigs[rig_index].meshes)
		if (mi < c->meshes.size() && c->meshes[mi].rig == (int)rig_index)
			c->meshes[mi].rig = -1;
	c->rigs[rig_index].meshes.clear();
}

extern "C" int rfwhip_set_rig(rfwhip_context *c, size_t rig_index, const rfwhip_rig *rig)
{
	CTX_ENTER(c);
	const char *const who = "rfwhip_set_rig";
	if (!rig)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s: null rig", who);
	if (rig_index >= (1u << 20))
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s: rig index %zu out of range", who, rig_index);
	rtk::RigSource src;
	memcpy(&src, rig, sizeof(src));
	rtk::RigPlan plan;
	if (rtk::rig_validate(src, plan))
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s: rig %zu: %s", who, rig_index, plan.msg);
	// the tables and the plan, one after the other at 16-byte offsets, in one allocation; the evaluation's values in another
	std::vector<uint8_t> blob;
	const auto put = [&](const void *p, size_t bytes) {
		const size_t at = (blob.size() + 15u) & ~(size_t)15u;
		blob.resize(at + bytes);
		if (bytes)
			memcpy(blob.data() + at, p, bytes);
		return at;
	};
	const size_t n = src.node_count, items = plan.item_skin.size();
	const size_t o_nodes = put(src.nodes, n * sizeof(rtk::RigNode)), o_bw = put(src.weights, src.weight_count * 4u);
	const size_t o_skins = put(src.skins, src.skin_count * sizeof(rtk::RigSkin)), o_joints = put(src.joints, src.joint_count * 4u);
	const size_t o_ibm = put(src.inverse_bind, src.joint_count * 64u), o_anims = put(src.animations, src.animation_count * sizeof(rtk::RigAnim));
	const size_t o_chan = put(src.channels, src.channel_count * sizeof(rtk::RigChannel)), o_times = put(src.times, src.time_count * 4u);
	const size_t o_values = put(src.values, src.value_count * 4u), o_order = put(plan.order.data(), n * 4u);
	const size_t o_level = put(plan.level_first.data(), plan.level_first.size() * 4u), o_iskin = put(plan.item_skin.data(), items * 4u);
	const size_t o_ijoint = put(plan.item_joint.data(), items * 4u);
	size_t state = 0;
	const auto room = [&](size_t bytes) {
		const size_t at = state;
		state = (state + bytes + 15u) & ~(size_t)15u;
		return at;
	};
	const size_t s_trs = room(n * rtk::RIG_TRS * 4u), s_w = room(src.weight_count * 4u), s_world = room(n * 64u), s_local = room(n * 64u);
	const size_t s_inv = room(src.skin_count * 64u), s_joint = room(items * 64u), s_flags = room((src.channel_count + src.skin_count) * 4u);
	const size_t s_status = room(sizeof(rtk::RigStatus));
	// a new rig beside the current one: the current one stays whatever happens below
	RF_TRY(sync_all(c));
	RigRec fresh;
	const auto drop = [&](int rc) {
		(void)dm::sync(c->stream);
		fresh.d_tables.free_(), fresh.d_state.free_();
		return rc;
	};
	int rc = fresh.d_tables.ensure(blob.size());
	rc = rc ? rc : fresh.d_state.ensure(state);
	rc = rc ? rc : dm::h2d(fresh.d_tables.p, blob.data(), blob.size(), c->stream);
	rc = rc ? rc : dm::zero(fresh.d_state.p, state, c->stream);
	if (rc)
		return drop(rc);
	const char *const T = (const char *)fresh.d_tables.p;
	char *const S = (char *)fresh.d_state.p;
	rtk::RigView &v = fresh.view;
	memset(&v, 0, sizeof(v));
	v.nodes = (const rtk::RigNode *)(T + o_nodes), v.base_weights = (const float *)(T + o_bw), v.skins = (const rtk::RigSkin *)(T + o_skins);
	v.joints = (const uint32_t *)(T + o_joints), v.ibm = (const float *)(T + o_ibm), v.anims = (const rtk::RigAnim *)(T + o_anims);
	v.channels = (const rtk::RigChannel *)(T + o_chan), v.times = (const float *)(T + o_times), v.values = (const float *)(T + o_values);
	v.order = (const uint32_t *)(T + o_order), v.level_first = (const uint32_t *)(T + o_level);
	v.item_skin = (const uint32_t *)(T + o_iskin), v.item_joint = (const uint32_t *)(T + o_ijoint);
	v.trs = (float *)(S + s_trs), v.weights = (float *)(S + s_w), v.world = (float *)(S + s_world), v.local = (float *)(S + s_local);
	v.inv = (float *)(S + s_inv), v.joint_mats = (float *)(S + s_joint), v.flags = (uint32_t *)(S + s_flags), v.status = (rtk::RigStatus *)(S + s_status);
	v.node_count = (uint32_t)n, v.weight_count = (uint32_t)src.weight_count, v.skin_count = (uint32_t)src.skin_count, v.item_count = (uint32_t)items;
	v.anim_count = (uint32_t)src.animation_count, v.channel_count = (uint32_t)src.channel_count, v.levels = plan.levels;
	fresh.used = true;
	for (size_t i = 0; i < n; i++)
		fresh.node_weight_offset.push_back(src.nodes[i].weight_offset), fresh.node_weight_count.push_back(src.nodes[i].weight_count);
	for (size_t s = 0; s < src.skin_count; s++)
		fresh.skin_joint_count.push_back(src.skins[s].joint_count), fresh.skin_first_item.push_back(plan.out_offset[s]);
	// the table of views the kernel indexes: every rig's, with this one's new view in its place
	const size_t count = std::max(c->rigs.size(), rig_index + 1);
	std::vector<rtk::RigView> table(count);
	for (size_t i = 0; i < count; i++)
		if (i == rig_index)
			table[i] = v;
		else if (i < c->rigs.size())
			table[i] = c->rigs[i].view;
		else
			memset(&table[i], 0, sizeof(rtk::RigView));
	DevBuf n_table;
	rc = n_table.ensure(count * sizeof(rtk::RigView));
	rc = rc ? rc : dm::h2d(n_table.p, table.data(), count * sizeof(rtk::RigView), c->stream);
	rc = rc ? rc : dm::sync(c->stream);
	if (rc)
	{
		n_table.free_();
		return drop(rc);
	}
	if (c->rigs.size() < count)
		c->rigs.resize(count);
	rig_unbind_all(c, rig_index);
	std::swap(c->rigs[rig_index], fresh);
	std::swap(c->d_rig_table, n_table);
	n_table.free_();
	drop(0);
	return RFWHIP_OK;
}

extern "C" int rfwhip_bind_rig(rfwhip_context *c, size_t rig_index, size_t skin_index, size_t node_index, size_t mesh_index)
{
	CTX_ENTER(c);
	const char *const who = "rfwhip_bind_rig";
	if (rig_index >= c->rigs.size() || !c->rigs[rig_index].used)
		return set_error(RFWHIP_ERR_STATE, "%s: rig %zu has not been set (rfwhip_set_rig)", who, rig_index);
	if (mesh_index >= c->meshes.size() || !c->meshes[mesh_index].used)
		return set_error(RFWHIP_ERR_STATE, "%s: mesh %zu has not been set", who, mesh_index);
	RigRec &r = c->rigs[rig_index];
	MeshRec &m = c->meshes[mesh_index];
	uint32_t item = 0;
	if (m.skinned)
	{
		if (skin_index >= r.skin_joint_count.size())
			return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s: rig %zu has %zu skins, no skin %zu", who, rig_index, r.skin_joint_count.size(), skin_index);
		if (m.skin_max_joint >= r.skin_joint_count[skin_index])
			return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s: mesh %zu refers to joint %u, skin %zu of rig %zu has %u joints", who, mesh_index,
							 m.skin_max_joint, skin_index, rig_index, r.skin_joint_count[skin_index]);
		item = (uint32_t)skin_index;
	}
	else if (m.morphed)
	{
		if (node_index >= r.node_weight_count.size())
			return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s: rig %zu has %zu nodes, no node %zu", who, rig_index, r.node_weight_count.size(), node_index);
		if (r.node_weight_count[node_index] != m.target_count)
			return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s: mesh %zu has %u targets, node %zu of rig %zu has %u weights", who, mesh_index,
							 m.target_count, node_index, rig_index, r.node_weight_count[node_index]);
		item = (uint32_t)node_index;
	}
	else
		return set_error(RFWHIP_ERR_STATE, "%s: mesh %zu has neither a skin nor morph targets (rfwhip_set_mesh_skin / rfwhip_set_mesh_morph)", who, mesh_index);
	if (m.rig >= 0 && (size_t)m.rig < c->rigs.size()) // binding it again replaces the binding
	{
		std::vector<size_t> &old = c->rigs[(size_t)m.rig].meshes;
		old.erase(std::remove(old.begin(), old.end(), mesh_index), old.end());
	}
	m.rig = (int)rig_index, m.rig_item = item;
	r.meshes.push_back(mesh_index);
	return RFWHIP_OK;
}

extern "C" int rfwhip_animate(rfwhip_context *c, const uint32_t *rigs, const uint32_t *animations, const float *times, size_t count)
{
	CTX_ENTER(c);
	const char *const who = "rfwhip_animate";
	if (!rigs || !animations || !times || !count)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s: null argument or no rigs", who);
	std::vector<rtk::RigCall> calls(count);
	std::vector<uint8_t> listed(c->rigs.size(), 0);
	for (size_t i = 0; i < count; i++)
	{
		if (rigs[i] >= c->rigs.size() || !c->rigs[rigs[i]].used)
			return set_error(RFWHIP_ERR_STATE, "%s: rig %u has not been set (rfwhip_set_rig)", who, rigs[i]);
		const RigRec &r = c->rigs[rigs[i]];
		if (listed[rigs[i]])
			return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s: rig %u is listed twice", who, rigs[i]);
		listed[rigs[i]] = 1;
		if (animations[i] != RFWHIP_RIG_BASE_POSE && r.view.anim_count && animations[i] >= r.view.anim_count)
			return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s: rig %u has %u animations, no animation %u", who, rigs[i], r.view.anim_count, animations[i]);
		if (!(times[i] - times[i] == 0.0f))
			return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s: the time of rig %u is not finite", who, rigs[i]);
		for (size_t mi : r.meshes)
		{
			const MeshRec &m = c->meshes[mi];
			if (!m.used || !(m.skinned || m.morphed))
				return set_error(RFWHIP_ERR_STATE, "%s: mesh %zu, bound to rig %u, has lost its skin or morph targets", who, mi, rigs[i]);
			if (!m.resident || m.dirty)
				return set_error(RFWHIP_ERR_STATE, "%s: mesh %zu, bound to rig %u, is not resident yet (rfwhip_update first)", who, mi, rigs[i]);
		}
		calls[i].rig = rigs[i], calls[i].animation = r.view.anim_count ? animations[i] : RFWHIP_RIG_BASE_POSE, calls[i].time = times[i];
	}
	RF_TRY(sync_all(c));
	for (size_t i = 0; i < count; i++)
		for (size_t mi : c->rigs[rigs[i]].meshes)
			RF_TRY(dn_snapshot_mesh(c, c->meshes[mi]));
	RF_TRY(c->d_rig_calls.ensure(count * sizeof(rtk::RigCall)));
	RF_TRY(dm::h2d(c->d_rig_calls.p, calls.data(), count * sizeof(rtk::RigCall), c->stream));
	{
		// (the rig kernel's own events, read behind the synchronisation of the first refit below — or, without a bound mesh, one of
		// their own; only with stage_timing)
		const bool timed = c->stage_timing != 0;
		dm::event_t ea{}, eb{};
		if (timed)
			dm::event_create(&ea), dm::event_create(&eb), dm::event_record(ea, c->stream);
		rtk::launch_rig_evaluate(c->d_rig_table.as<rtk::RigView>(), c->d_rig_calls.as<rtk::RigCall>(), (uint32_t)count, c->stream);
		int rc = dm::last_launch_error();
		if (timed)
		{
			dm::event_record(eb, c->stream);
			rc = rc ? rc : dm::sync(c->stream);
			if (!rc)
				c->kernel_ms[KF_RIG] += dm::event_ms(ea, eb), c->kernel_launches[KF_RIG] += 1;
			dm::event_destroy(ea), dm::event_destroy(eb);
		}
		RF_TRY(rc);
	}
	for (size_t i = 0; i < count; i++)
	{
		RigRec &r = c->rigs[rigs[i]];
		r.evaluated = true;
		for (size_t mi : r.meshes)
		{
			MeshRec &m = c->meshes[mi];
			RefitTimer timer(c);
			if (m.skinned)
			{
				m.joint_count = r.skin_joint_count[m.rig_item];
				rtk::launch_skin_vertices(m.d_verts.as<f4>(), m.d_vnormals.as<f4>(), m.d_base_verts.as<f4>(), m.d_base_normals.as<f4>(),
										  m.d_joints.as<uint32_t>(), m.d_weights.as<f4>(), r.view.joint_mats + 16u * (size_t)r.skin_first_item[m.rig_item],
										  m.joint_count, (uint32_t)m.vertexCount, c->stream);
			}
			else
				rtk::launch_morph_vertices(m.d_verts.as<f4>(), m.d_vnormals.as<f4>(), m.d_base_verts.as<f4>(), m.d_base_normals.as<f4>(),
										   m.d_tgt_pos.as<f4>(), m.d_tgt_nrm.as<f4>(), r.view.weights + r.node_weight_offset[m.rig_item], m.target_count,
										   (uint32_t)m.vertexCount, c->stream);
			RF_TRY(refit_deformed(c, m, timer));
		}
	}
	return RFWHIP_OK;
}

extern "C" int rfwhip_read_rig(rfwhip_context *c, size_t rig_index, int what, size_t index, float *out, size_t cap)
{
	CTX_ENTER(c);
	const char *const who = "rfwhip_read_rig";
	if (rig_index >= c->rigs.size() || !c->rigs[rig_index].used)
		return set_error(RFWHIP_ERR_STATE, "%s: rig %zu has not been set (rfwhip_set_rig)", who, rig_index);
	const RigRec &r = c->rigs[rig_index];
	if (!r.evaluated)
		return set_error(RFWHIP_ERR_STATE, "%s: rig %zu has not been evaluated (rfwhip_animate)", who, rig_index);
	const void *from = nullptr;
	size_t floats = 0;
	switch (what)
	{
	case RFWHIP_RIG_READ_TRS:
		from = r.view.trs, floats = (size_t)r.view.node_count * rtk::RIG_TRS;
		break;
	case RFWHIP_RIG_READ_WORLD:
		from = r.view.world, floats = (size_t)r.view.node_count * 16u;
		break;
	case RFWHIP_RIG_READ_JOINTS:
		if (index >= r.skin_joint_count.size())
			return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s: rig %zu has %zu skins, no skin %zu", who, rig_index, r.skin_joint_count.size(), index);
		from = r.view.joint_mats + 16u * (size_t)r.skin_first_item[index], floats = (size_t)r.skin_joint_count[index] * 16u;
		break;
	case RFWHIP_RIG_READ_WEIGHTS:
		if (index >= r.node_weight_count.size())
			return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s: rig %zu has %zu nodes, no node %zu", who, rig_index, r.node_weight_count.size(), index);
		from = r.view.weights + r.node_weight_offset[index], floats = r.node_weight_count[index];
		break;
	case RFWHIP_RIG_READ_STATUS:
		from = r.view.status, floats = sizeof(rtk::RigStatus) / 4u;
		break;
	default:
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s: unknown selector %d", who, what);
	}
	if (!out || cap < floats)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s: %zu floats, room for %zu", who, floats, out ? cap : (size_t)0);
	RF_TRY(sync_all(c));
	if (!floats)
		return RFWHIP_OK;
	return dm::d2h(out, from, floats * 4u, c->stream);
}

// The float copy of the traversal nodes (rt::Node4f) — written only when its one reader, the packet form of the pt primary wave,
// can run: at the end of an update, or by the first render call after `refill` bit 3 was switched on.
static int ensure_nodes4f(rfwhip_context *c)
{
	if (c->nodes4f_current || !c->packet_ok || !(c->refill & 8) || !c->nodes4_live)
		return 0;
	RF_TRY(c->d_nodes4f.ensure(c->node4_capacity * sizeof(rt::Node4f)));
	rtk::launch_expand4(c->d_nodes4.as<rt::Node4c>(), c->d_nodes4f.as<rt::Node4f>(), (uint32_t)c->nodes4_live, c->stream);
	RF_TRY(dm::last_launch_error());
	c->sv.nodes4f = c->d_nodes4f.as<rt::Node4f>();
	c->nodes4f_current = true;
	c->nodes4f_version++; // (the ordered copy is stale: ensure_primary_order)
	return 0;
}

// ---- the WORLD TREE -------------------------------------------------------------------------------------------------------------
// The reference walks two levels for every ray: top-level leaf -> instance -> the ray in object space -> mesh tree -> back
// (top_level_bvh.cpp:104-168).  A static instance needs none of that at run time: its triangles can be written out in WORLD space
// once, per update, and then ALL static geometry hangs under ONE tree built over all of it — no instance switch (ray transform,
// three reciprocals, a leaf phase in and one out per instance a ray's box test passes), no top-level tree over boxes that contain
// each other (a room around its columns), one top-of-tree cache in LDS instead of several trees' tops.  Semantics kept: the hit
// is the same triangle of the same instance at the same t (directions are not renormalised in the two-level walk, so t is shared;
// here the triangle simply moved instead of the ray); primitive ids stay mesh-relative (v0.w) and the instance index travels in
// v1.w, so shading still goes through the instance's record (normal matrix, shading records in object space).  For an instance
// whose matrix is the identity the world-space vertices ARE the object-space ones and nothing a ray computes changes; for a
// transformed one the triangle test sees M p instead of M^-1 o: the same numbers up to rounding.
// Members: every instance of a mesh that was built on the host and is not animated (skinned, morphed, posed, or re-set with the same
// topology since its build) whose own matrix has not changed in the last eight updates, as long as the copy stays below `flatten_bytes`.  A single member that is an identity instance of a
// singly used mesh has its mesh tree linked into the top-level tree instead (flat instances, below): same effect, no copy.
// Animated meshes and meshes built on the device keep the two-level walk.  The tree is rebuilt only when its key — members, their
// meshes' build generations, their matrices — changes (an animated scene's per-frame update leaves it alone).
constexpr uint32_t WORLD_ID = 0xFFFFFFFFu;
static int prepare_world(rfwhip_context *c, bool &changed)
{
	WorldRec &w = c->wtree;
	changed = false;
	std::vector<uint8_t> member(c->instances.size(), 0), mesh_member(c->meshes.size(), 0);
	std::vector<uint32_t> key;
	size_t tris = 0;
	bool worth = false;
	if (c->flat_instances != 0)
	{
		std::vector<uint32_t> uses(c->meshes.size(), 0u);
		for (const InstRec &in : c->instances)
			if (in.used && in.mesh < c->meshes.size() && c->meshes[in.mesh].used)
				uses[in.mesh]++;
		static const float ident[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
		for (size_t i = 0; i < c->instances.size(); i++)
		{
			InstRec &in = c->instances[i];
			if (!in.used || in.mesh >= c->meshes.size() || !c->meshes[in.mesh].used)
				continue;
			// (another mesh, or the same one rebuilt: a new object in this slot, not a moving one)
			const bool same_object = in.has_prev && in.prev_mesh == in.mesh && in.prev_generation == c->meshes[in.mesh].generation;
			if (!same_object)
				in.moving = 0u, in.moves = 0u;
			else if (memcmp(in.prev_transform, in.transform, sizeof(in.transform)) != 0)
			{
				// stable for eight updates before it rejoins: one rebuild when an animation starts, one after it ends — and twice as
				// long after every further episode (8, 16, 32 ... 8192 updates): an instance that keeps starting and stopping ends up
				// outside the tree for good instead of paying two synchronous host rebuilds per episode (round 5's advisor)
				if (!in.moving)
					in.moves = std::min(in.moves + 1u, 11u);
				in.moving = 8u << (in.moves - 1u);
			}
			else if (in.moving)
				in.moving--;
			memcpy(in.prev_transform, in.transform, sizeof(in.transform));
			in.prev_mesh = in.mesh, in.prev_generation = c->meshes[in.mesh].generation, in.has_prev = true;
			if (in.moving)
				continue;
			const MeshRec &m = c->meshes[in.mesh];
			if (!m.built || m.device_built || m.skinned || m.morphed || m.posed || m.refits != 0u || m.leaf_verts.size() != 3 * m.triCount || !m.triCount)
				continue;
			member[i] = 1, mesh_member[in.mesh] = 1, tris += m.triCount;
			if (memcmp(in.transform, ident, sizeof(ident)) != 0 || uses[in.mesh] > 1u)
				worth = true;
			key.push_back((uint32_t)i), key.push_back((uint32_t)in.mesh), key.push_back(m.generation);
			for (int k = 0; k < 16; k++)
			{
				uint32_t b;
				memcpy(&b, &in.transform[k], 4);
				key.push_back(b);
			}
		}
	}
	if (key.size() > 19) // (two members or more: one tree over all of them beats a top-level tree over theirs even when every one of
		worth = true;	 // them is an identity instance — terrain + light quads of the bench scene: +0.9 %)
	const unsigned long long bytes = (unsigned long long)tris * (3 * sizeof(f4) + sizeof(rt::Node4c)); // (at most one 4-wide node per triangle)
	if (!worth || !tris || bytes > (unsigned long long)c->flatten_bytes)
	{
		std::fill(member.begin(), member.end(), 0), std::fill(mesh_member.begin(), mesh_member.end(), 0);
		key.clear(), tris = 0;
	}
	if (key == w.key && w.member.size() == member.size())
		return 0; // as built (or, if that build was refused, as refused)
	changed = true;
	w = WorldRec();
	w.key = key;
	w.member.assign(member.size(), 0), w.mesh_member.assign(mesh_member.size(), 0);
	if (key.empty())
		return 0;
	// the members' triangles in world space (leaf order of their meshes: any order does), with what a hit record needs
	std::vector<f4> verts(3 * tris);
	std::vector<float> bmin(3 * tris), bmax(3 * tris);
	size_t t = 0;
	for (size_t i = 0; i < c->instances.size(); i++)
	{
		if (!member[i])
			continue;
		const InstRec &in = c->instances[i];
		const MeshRec &m = c->meshes[in.mesh];
		const float *M = in.transform; // column-major 4x4, like the instance boxes below
		const uint32_t ii = (uint32_t)i;
		float iw;
		memcpy(&iw, &ii, 4);
		// the determinant threshold of the reference's triangle test, stated in object space (rt::tri_test): a = e1 . (d x e2) of the
		// world-space triangle is det(M) times the object-space one
		const double det3 = (double)M[0] * ((double)M[5] * M[10] - (double)M[9] * M[6]) - (double)M[4] * ((double)M[1] * M[10] - (double)M[9] * M[2]) +
							(double)M[8] * ((double)M[1] * M[6] - (double)M[5] * M[2]);
		const float tri_eps = std::max((float)((double)rt::TRI_EPS * fabs(det3)), 1e-37f); // (a singular matrix: every triangle is rejected)
		for (size_t s = 0; s < m.triCount; s++, t++)
		{
			for (int k = 0; k < 3; k++)
			{
				const f4 &p = m.leaf_verts[3 * s + k];
				f4 q;
				q.x = M[0] * p.x + M[4] * p.y + M[8] * p.z + M[12];
				q.y = M[1] * p.x + M[5] * p.y + M[9] * p.z + M[13];
				q.z = M[2] * p.x + M[6] * p.y + M[10] * p.z + M[14];
				q.w = k == 0 ? p.w : (k == 1 ? iw : tri_eps); // v0.w: primitive id (mesh order), v1.w: instance, v2.w: determinant threshold
				verts[3 * t + k] = q;
			}
			const f4 &a = verts[3 * t], &b = verts[3 * t + 1], &d = verts[3 * t + 2];
			// per-triangle box grown by 1e-5 (bvh_tree.cpp:407-412), as rfwhip_set_mesh does
			bmin[3 * t + 0] = std::min(a.x, std::min(b.x, d.x)) - 1e-5f, bmax[3 * t + 0] = std::max(a.x, std::max(b.x, d.x)) + 1e-5f;
			bmin[3 * t + 1] = std::min(a.y, std::min(b.y, d.y)) - 1e-5f, bmax[3 * t + 1] = std::max(a.y, std::max(b.y, d.y)) + 1e-5f;
			bmin[3 * t + 2] = std::min(a.z, std::min(b.z, d.z)) - 1e-5f, bmax[3 * t + 2] = std::max(a.z, std::max(b.z, d.z)) + 1e-5f;
		}
	}
	bvh::Result tree;
	bvh::build(bmin.data(), bmax.data(), tris, BLAS_MAX_LEAF, BLAS_DEPTH_LIMIT, tree);
	const bool inner = bvh::collapse4(tree, false, w.n4);
	w.stack_need = bvh::stack_need4(w.n4);
	if (w.stack_need > BLAS_STACK_BUDGET)
	{
		// (a tree this deep is refused like a mesh's would be; the instances keep the two-level walk.  The key stays: no retry per update)
		w.n4.clear(), w.stack_need = 0;
		return 0;
	}
	if (!inner)
		w.root_first = (uint32_t)tree.nodes[0].left_first, w.root_count = (uint32_t)tree.nodes[0].count;
	w.leaf_verts.resize(3 * tris);
	for (size_t s = 0; s < tris; s++)
		for (int k = 0; k < 3; k++)
			w.leaf_verts[3 * s + k] = verts[3 * (size_t)tree.order[s] + k];
	for (int a = 0; a < 3; a++)
		w.bmin[a] = tree.nodes[0].bmin[a], w.bmax[a] = tree.nodes[0].bmax[a];
	w.tris = tris, w.member = member, w.mesh_member = mesh_member, w.valid = true;
	w.mesh_all = mesh_member;
	for (size_t i = 0; i < c->instances.size(); i++)
		if (c->instances[i].used && c->instances[i].mesh < w.mesh_all.size() && !member[i])
			w.mesh_all[c->instances[i].mesh] = 0;
	return 0;
}

// sky_sampling: the alias table (rebuilt when the sky or the setting changed) and p (the lights may have changed).  Called by
// rfwhip_update, and by a render or rfwhip_kat after a sky setting changed (they run on the scene of the last update).
// sky_table = device (sky_load.h; defined with the sky's loaders below): the table of the sky's n texels — or of n given weights —
// built by the kernels on the context's stream into `table`; the record comes back, the scratch is freed
static int sky_table_on_device(rfwhip_context *c, const double *weights, uint32_t n, DevBuf &table, rtk::SkyTabRecord *record);
static int update_sky_sampling(rfwhip_context *c)
{
	c->sky_stale = false;
	if (!c->sky_sampling)
	{
		if (c->d_sky_alias.p)
			RF_TRY(sync_all(c)); // (frames in flight may still read the table)
		c->d_sky_alias.free_(), c->sky_table_of = ~0ull, c->sky_total = 0.0;
		c->sky_table_by = -1, c->sky_record = rtk::SkyTabRecord{0.0, 0, 0, 0, 0, {0, 0}};
		c->sky_view = rt::SkyView{};
		return RFWHIP_OK;
	}
	const size_t n = (size_t)c->sky_w * c->sky_h;
	if (n >= (1ull << 31))
		return set_error(RFWHIP_ERR_UNSUPPORTED, "sky_sampling: a sky of %u x %u texels is too large", c->sky_w, c->sky_h);
	if (c->sky_table_of != c->sky_version || c->sky_table_by != c->sky_table)
	{
		RF_TRY(sync_all(c)); // (frames in flight may still read the table)
		c->sky_total = 0.0;
		c->sky_record = rtk::SkyTabRecord{0.0, 0, 0, 0, 0, {0, 0}};
		if (n && c->sky_table == 1) // the kernels build it in place: nothing but the record comes back
		{
			RF_TRY(sky_table_on_device(c, nullptr, (uint32_t)n, c->d_sky_alias, &c->sky_record));
			if (c->sky_record.flags & rtk::SKYTAB_VALID)
				c->sky_total = c->sky_record.S;
			else
				c->d_sky_alias.free_();
		}
		else // the host builds it: the sky comes down, the table goes up
		{
			std::vector<rt::SkyAlias> table;
			if (n)
			{
				std::vector<f4> px(n);
				RF_TRY(dm::d2h(px.data(), c->d_sky.p, n * sizeof(f4), c->stream));
				RF_TRY(dm::sync(c->stream));
				c->sky_total = skysamp::build_alias(px.data(), c->sky_w, c->sky_h, table);
			}
			if (table.empty())
				c->d_sky_alias.free_();
			else
			{
				RF_TRY(c->d_sky_alias.ensure(table.size() * sizeof(rt::SkyAlias)));
				RF_TRY(dm::h2d(c->d_sky_alias.p, table.data(), table.size() * sizeof(rt::SkyAlias), c->stream));
				RF_TRY(dm::sync(c->stream));
				c->sky_record.S = c->sky_total, c->sky_record.flags = rtk::SKYTAB_VALID;
			}
		}
		c->sky_table_of = c->sky_version, c->sky_table_by = c->sky_table;
	}
	// p: forced to 0 without a usable sky (the default kernels run: bit-identical to sky_sampling=0)
	float pick = c->sky_pick >= 0.0f ? c->sky_pick : (total_light_count(c) ? 0.5f : 1.0f);
	if (!(c->sky_total > 0.0))
		pick = 0.0f;
	c->sky_view = skysamp::view(c->sky_total > 0.0 ? c->d_sky_alias.as<rt::SkyAlias>() : nullptr, c->sky_total, pick, c->sky_w, c->sky_h);
	return RFWHIP_OK;
}

// light_sampling=tree: the tree over the lights of the last rfwhip_set_lights.  rfwhip_set_lights hands the host arrays it was
// given (h_*); rfwhip_update, a render, rfwhip_kat and rfwhip_get_light_tree after the setting changed read the lights back from
// the device, where rfwhip_set_lights has put them (no host copy is kept).  Every rank of a group builds the same tree from the
// same lights.  lt_stale is cleared only when the view is complete: after a failure the next render tries again (and fails
// again) instead of running the linear branch under the name of the tree.
static int update_light_tree(rfwhip_context *c, const rt::AreaLight *h_area, const rt::PointLight *h_point, const rt::SpotLight *h_spot)
{
	c->lt_stale = true;
	c->lt_view = rt::LightTreeView{};
	c->lt_levels.levels = 0, c->lt_refits = 0;
	if (c->light_sampling != 2)
	{
		if (c->d_lt_nodes.p || c->d_lt_paths.p)
			RF_TRY(sync_all(c)); // (a frame in flight may still read them)
		c->d_lt_nodes.free_(), c->d_lt_paths.free_();
		c->lt_stale = false;
		return RFWHIP_OK;
	}
	const uint32_t na = c->lc.areaLightCount, np = c->lc.pointLightCount, ns = c->lc.spotLightCount, nd = c->lc.directionalLightCount;
	if ((uint64_t)na + np + ns + nd >= (1ull << 30))
		return set_error(RFWHIP_ERR_UNSUPPORTED, "light_sampling=tree: too many lights");
	RF_TRY(sync_all(c));
	std::vector<rt::AreaLight> area;
	std::vector<rt::PointLight> point;
	std::vector<rt::SpotLight> spot;
	if (na && !h_area)
	{
		area.resize(na);
		RF_TRY(dm::d2h(area.data(), c->d_area.p, na * sizeof(rt::AreaLight), c->stream));
		h_area = area.data();
	}
	if (np && !h_point)
	{
		point.resize(np);
		RF_TRY(dm::d2h(point.data(), c->d_point.p, np * sizeof(rt::PointLight), c->stream));
		h_point = point.data();
	}
	if (ns && !h_spot)
	{
		spot.resize(ns);
		RF_TRY(dm::d2h(spot.data(), c->d_spot.p, ns * sizeof(rt::SpotLight), c->stream));
		h_spot = spot.data();
	}
	std::vector<rt::LightTreeNode> nodes;
	std::vector<rt::LightTreePath> paths;
	lighttree::build(h_area, na, h_point, np, h_spot, ns, nd, nodes, paths);
	rt::LightTreeView view{};
	view.n_spatial = na + np + ns;
	view.node_count = (uint32_t)nodes.size();
	if (!nodes.empty())
	{
		// (a sibling pair is one 128-byte line: the table starts on one)
		RF_TRY(c->d_lt_nodes.ensure(nodes.size() * sizeof(rt::LightTreeNode) + 128));
		rt::LightTreeNode *base = reinterpret_cast<rt::LightTreeNode *>(((uintptr_t)c->d_lt_nodes.p + 127u) & ~(uintptr_t)127u);
		RF_TRY(dm::h2d(base, nodes.data(), nodes.size() * sizeof(rt::LightTreeNode), c->stream));
		view.nodes = base;
	}
	else
		c->d_lt_nodes.free_();
	if (!paths.empty())
	{
		RF_TRY(c->d_lt_paths.ensure(paths.size() * sizeof(rt::LightTreePath)));
		RF_TRY(dm::h2d(c->d_lt_paths.p, paths.data(), paths.size() * sizeof(rt::LightTreePath), c->stream));
		view.paths = c->d_lt_paths.as<rt::LightTreePath>();
	}
	else
		c->d_lt_paths.free_();
	RF_TRY(dm::sync(c->stream));
	// the level ranges of the new topology, for the refits that follow it (light_follow.h).  No new way for a build to fail: a tree
	// whose levels cannot be read (build() lays out none such) has no ranges, and refresh_lights rebuilds it instead of refitting
	if (!lighttree::levels(nodes.data(), nodes.size(), view.n_spatial, c->lt_levels.first, c->lt_levels.count, rtk::LT_MAX_LEVELS, c->lt_levels.levels))
		c->lt_levels.levels = 0;
	c->lt_refits = 0;
	c->lt_view = view;
	c->lt_stale = false;
	return RFWHIP_OK;
}

// lights_follow_geometry=1: the bound area lights from the current triangles and transforms, and — where a tree stands — its refit
// (light_follow.h).  Called by rfwhip_update behind its sync_all and behind everything it writes of meshes and instances, in front
// of everything that reads the lights: the rule of rfwhip_pose_mesh's device refit — every stream of the ring drained first, the
// work enqueued on the context's stream, the stream synchronised before the call returns.
static int refresh_lights_enqueue(rfwhip_context *c, std::vector<rtk::LightInst> &tab, uint32_t &bound)
{
	const uint32_t na = c->lc.areaLightCount;
	for (size_t i = 0; i < c->instances.size(); i++)
	{
		const InstRec &in = c->instances[i];
		if (!in.used || in.mesh >= c->meshes.size() || !c->meshes[in.mesh].used || !c->meshes[in.mesh].resident)
			continue;
		const MeshRec &m = c->meshes[in.mesh];
		rtk::LightInst &e = tab[i];
		for (int r = 0; r < 3; r++)
		{
			for (int col = 0; col < 4; col++)
				e.m[4 * r + col] = in.transform[4 * col + r];
			for (int col = 0; col < 3; col++)
				e.nrm[4 * r + col] = in.normal[3 * col + r];
		}
		e.verts = m.d_verts.as<f4>(), e.indices = m.indexed ? m.d_indices.as<uint32_t>() : nullptr;
		e.tri_count = (uint32_t)m.triCount, e.shade_base = m.shade_base;
	}
	RF_TRY(c->d_lf_inst.ensure(tab.size() * sizeof(rtk::LightInst)));
	RF_TRY(c->d_lf_bound.ensure(na));
	RF_TRY(c->d_lf_count.ensure(sizeof(uint32_t)));
	RF_TRY(dm::h2d(c->d_lf_inst.p, tab.data(), tab.size() * sizeof(rtk::LightInst), c->stream));
	RF_TRY(dm::zero(c->d_lf_count.p, sizeof(uint32_t), c->stream));
	rtk::LightFollowView v{};
	v.area = c->d_area.as<rt::AreaLight>(), v.inst = c->d_lf_inst.as<rtk::LightInst>(), v.tri_shade = c->d_tri_shade.as<rt::TriShade>();
	v.bound = c->d_lf_bound.as<unsigned char>(), v.bound_count = c->d_lf_count.as<uint32_t>();
	v.n_area = na, v.n_inst = (uint32_t)c->instances.size();
	rtk::launch_light_refresh(v, c->stream);
	RF_TRY(dm::last_launch_error());
	// (a stale tree is built from the refreshed lights by update_light_tree, which follows in rfwhip_update)
	if (c->light_sampling == 2 && !c->lt_stale && c->lt_view.nodes)
	{
		if (!c->lt_levels.levels)
			c->lt_stale = true; // (no level ranges: built again instead)
		else
		{
			RF_TRY(c->d_lt_touched.ensure(c->lt_view.node_count));
			rtk::launch_light_tree_refit(const_cast<rt::LightTreeNode *>(c->lt_view.nodes), c->lt_levels, c->d_area.as<rt::AreaLight>(), na,
										 c->d_lf_bound.as<unsigned char>(), c->d_lt_touched.as<unsigned char>(), c->stream);
			RF_TRY(dm::last_launch_error());
			c->lt_refits++;
		}
	}
	return dm::d2h(&bound, c->d_lf_count.p, sizeof(bound), c->stream);
}
static int refresh_lights(rfwhip_context *c)
{
	if (!c->lights_follow)
	{
		c->lights_bound = 0, c->lt_rebuild_after_refresh = false;
		return RFWHIP_OK;
	}
	// the lights of a rfwhip_set_lights under the setting: whatever tree was made of the host's geometry fields since (a
	// rfwhip_get_light_tree in between) is built again from what this refresh derives
	if (c->lt_rebuild_after_refresh)
		c->lt_stale = true, c->lt_rebuild_after_refresh = false;
	if (!c->lf_dirty)
		return RFWHIP_OK;
	c->lights_bound = 0;
	if (c->lc.areaLightCount)
	{
		std::vector<rtk::LightInst> tab(std::max<size_t>(1, c->instances.size()));
		memset(tab.data(), 0, tab.size() * sizeof(rtk::LightInst));
		uint32_t bound = 0;
		const int rc = refresh_lights_enqueue(c, tab, bound);
		const int rs = dm::sync(c->stream); // (on every path: nothing enqueued may outlive `tab`)
		RF_TRY(rc);
		RF_TRY(rs);
		c->lights_bound = bound;
	}
	c->lf_dirty = false; // (only now: after a failure the next rfwhip_update tries again)
	return RFWHIP_OK;
}

extern "C" int rfwhip_update(rfwhip_context *c)
{
	CTX_ENTER(c);
	RF_TRY(sync_all(c));
	// the shade kernels index the material table with the triangles' ids unchecked
	for (size_t i = 0; i < c->meshes.size(); i++)
		if (c->meshes[i].used && c->meshes[i].max_material >= c->material_count)
			return set_error(RFWHIP_ERR_STATE, "rfwhip_update: mesh %zu refers to material %u, but %u materials are set",
							 i, c->meshes[i].max_material, c->material_count);
	for (size_t i = 0; i < c->meshes.size(); i++)
		if (c->meshes[i].used && !c->meshes[i].built)
			return set_error(RFWHIP_ERR_STATE, "rfwhip_update: the last rfwhip_set_mesh of mesh %zu failed; set it again", i);
	// ---- place meshes in the global arrays (only when some mesh was rebuilt) ----
	bool relayout = false;
	size_t live_instances = 0;
	for (auto &in : c->instances)
		if (in.used)
			live_instances++;
	const size_t tlas_reserve = live_instances + 3; // a 4-wide tree over n single-instance leaves (+ the world tree's) has < n inner nodes
	for (auto &m : c->meshes)
		if (m.used && m.dirty)
			relayout = true;
	bool world_changed = false;
	RF_TRY(prepare_world(c, world_changed));
	if (world_changed)
		relayout = true;
	WorldRec &world = c->wtree;
	if (c->blas_nodes4 + tlas_reserve > c->node4_capacity)
		relayout = true; // the TLAS lives behind the BLAS nodes in the same array: grow it together
	if (relayout)
	{
		c->lf_dirty = true; // (the shading records are uploaded again: a bound triangle's area is the host's once more)
		size_t nodes = 0, tris = 0, nodes4 = 0;
		for (auto &m : c->meshes)
			if (m.used)
			{
				m.node_base = (uint32_t)nodes, m.tri_base = (uint32_t)tris, m.shade_base = (uint32_t)tris;
				m.n4_base = (uint32_t)nodes4;
				nodes += m.node_count2, tris += m.triCount, nodes4 += m.n4_count;
			}
		// the world tree's nodes and world-space triangles follow the meshes' (shading records stay per mesh, in object space)
		const size_t mesh_tris = tris, mesh_nodes4 = nodes4;
		world.resident = false;
		if (world.valid)
		{
			world.n4_base = (uint32_t)nodes4, world.tri_base = (uint32_t)tris;
			nodes4 += world.n4.size(), tris += world.tris;
		}
		if (tris > rt::ENTRY_FIRST_MASK)
			return set_error(RFWHIP_ERR_UNSUPPORTED, "more than 2^27 triangles in the scene");
		c->blas_nodes4 = nodes4;
		c->node4_capacity = nodes4 + 2 * tlas_reserve + 64;
		if (c->node4_capacity >= (size_t(1) << 26))
			return set_error(RFWHIP_ERR_UNSUPPORTED, "more than 2^26 4-wide nodes (the traversal addresses them by 32-bit byte offsets)");
		RF_TRY(c->d_nodes.ensure(nodes * sizeof(rt::Node)));
		RF_TRY(c->d_nodes4.ensure(c->node4_capacity * sizeof(rt::Node4c)));
		RF_TRY(c->d_nodes4_src.ensure(4 * mesh_nodes4 * sizeof(uint32_t)));
		RF_TRY(c->d_tri_verts.ensure(3 * tris * sizeof(f4)));
		RF_TRY(c->d_tri_shade.ensure(mesh_tris * sizeof(rt::TriShade)));
		RF_TRY(c->d_tri_uv.ensure(mesh_tris * sizeof(rt::TriUV)));
		// One mesh at a time.  Device form everywhere: left_first / entries carry ready-made stack entries (rt::make_entry)
		// with ABSOLUTE indices — node index into the scene-wide arrays, leaf-ordered triangle index into tri_verts.
		std::vector<rt::Node> nodes2;
		std::vector<rt::Node4c> nodes4c;
		std::vector<uint32_t> src;
		for (auto &m : c->meshes)
		{
			if (!m.used)
				continue;
			rt::Node *dn = c->d_nodes.as<rt::Node>() + m.node_base;
			rt::Node4c *dn4 = c->d_nodes4.as<rt::Node4c>() + m.n4_base;
			uint32_t *dsrc = c->d_nodes4_src.as<uint32_t>() + 4ull * m.n4_base;
			f4 *dtv = c->d_tri_verts.as<f4>() + 3ull * m.tri_base;
			if (m.device_built)
			{
				// built on the device in mesh-local arrays: copy and rebase there, nothing touches the host
				RF_TRY(dm::d2d(dn, m.d_b_nodes.p, (size_t)m.node_count2 * sizeof(rt::Node), c->stream));
				RF_TRY(dm::d2d(dn4, m.d_b_nodes4.p, (size_t)m.n4_count * sizeof(rt::Node4c), c->stream));
				RF_TRY(dm::d2d(dsrc, m.d_b_src.p, 4ull * m.n4_count * sizeof(uint32_t), c->stream));
				RF_TRY(dm::d2d(dtv, m.d_b_tri_verts.p, 3ull * m.triCount * sizeof(f4), c->stream));
				rtk::launch_rebase(dn, m.node_count2, m.node_base, dn4, m.n4_count, m.n4_base, m.tri_base, c->stream);
				RF_TRY(dm::last_launch_error());
			}
			else
			{
				nodes2 = m.bvh.nodes;
				for (rt::Node &nd : nodes2)
				{
					if (nd.count > 0)
						nd.left_first = (int)rt::make_entry(nd.left_first + (int)m.tri_base, nd.count, false);
					else if (nd.count < 0)
						nd.left_first = (int)rt::make_entry(nd.left_first + (int)m.node_base, nd.count, false);
				}
				nodes4c.resize(m.n4.size()), src.resize(4 * m.n4.size());
				for (size_t k = 0; k < m.n4.size(); k++)
				{
					rt::Node4 nd = m.n4[k];
					for (int j = 0; j < 4; j++)
					{
						const uint32_t e = nd.entry[j];
						if (e == rt::ENTRY_EMPTY)
							continue;
						if (e & rt::ENTRY_LEAF)
							nd.entry[j] = (e & ~rt::ENTRY_FIRST_MASK) | (((e & rt::ENTRY_FIRST_MASK) + m.tri_base) & rt::ENTRY_FIRST_MASK);
						else
							nd.entry[j] = e + m.n4_base;
					}
					nodes4c[k] = compress4(nd); // what the rays fetch: compressed (rt::pack_boxes4c)
					memcpy(&src[4 * k], nd.src, 16); // BVH2 node (BLAS-relative) behind each child box, for the refit
				}
				RF_TRY(dm::h2d(dn, nodes2.data(), nodes2.size() * sizeof(rt::Node), c->stream));
				RF_TRY(dm::h2d(dn4, nodes4c.data(), nodes4c.size() * sizeof(rt::Node4c), c->stream));
				RF_TRY(dm::h2d(dsrc, src.data(), src.size() * sizeof(uint32_t), c->stream));
				RF_TRY(dm::h2d(dtv, m.leaf_verts.data(), m.leaf_verts.size() * sizeof(f4), c->stream));
				RF_TRY(dm::sync(c->stream)); // the staging vectors are reused by the next mesh
			}
			RF_TRY(dm::h2d(c->d_tri_shade.as<rt::TriShade>() + m.shade_base, m.shade.data(), m.shade.size() * sizeof(rt::TriShade), c->stream));
		RF_TRY(dm::h2d(c->d_tri_uv.as<rt::TriUV>() + m.shade_base, m.uv.data(), m.uv.size() * sizeof(rt::TriUV), c->stream));
		}
		if (world.valid)
		{
			nodes4c.resize(world.n4.size());
			for (size_t k = 0; k < world.n4.size(); k++)
			{
				rt::Node4 nd = world.n4[k];
				for (int j = 0; j < 4; j++)
				{
					const uint32_t e = nd.entry[j];
					if (e == rt::ENTRY_EMPTY)
						continue;
					if (e & rt::ENTRY_LEAF)
						nd.entry[j] = (e & ~rt::ENTRY_FIRST_MASK) | (((e & rt::ENTRY_FIRST_MASK) + world.tri_base) & rt::ENTRY_FIRST_MASK);
					else
						nd.entry[j] = e + world.n4_base;
				}
				nodes4c[k] = compress4(nd);
			}
			RF_TRY(dm::h2d(c->d_nodes4.as<rt::Node4c>() + world.n4_base, nodes4c.data(), nodes4c.size() * sizeof(rt::Node4c), c->stream));
			RF_TRY(dm::h2d(c->d_tri_verts.as<f4>() + 3ull * world.tri_base, world.leaf_verts.data(), world.leaf_verts.size() * sizeof(f4), c->stream));
			world.resident = true;
		}
		RF_TRY(dm::sync(c->stream));
		// meshes that had been refit since their build are re-refit from their device vertices after the move
		for (auto &m : c->meshes)
		{
			if (!m.used)
				continue;
			if (m.resident && !m.dirty)
				RF_TRY(launch_refit_chain(c, m, m.posed)); // (posed: the host copy of the shading records is the bind pose)
			m.resident = true, m.dirty = false;
		}
		RF_TRY(dm::sync(c->stream));
	}
	// ---- instances + TLAS ----
	std::vector<rt::Instance> inst(c->instances.size());
	std::vector<float> bmin, bmax;
	std::vector<uint32_t> live;
	for (size_t i = 0; i < c->instances.size(); i++)
	{
		rt::Instance &d = inst[i];
		memset(&d, 0, sizeof(d));
		const InstRec &in = c->instances[i];
		if (!in.used || in.mesh >= c->meshes.size() || !c->meshes[in.mesh].used)
			continue;
		const MeshRec &m = c->meshes[in.mesh];
		float inv[16];
		mat4_inverse(in.transform, inv);
		for (int r = 0; r < 3; r++)
			for (int col = 0; col < 4; col++)
				d.inv[4 * r + col] = inv[4 * col + r];
		for (int col = 0; col < 3; col++)
			for (int r = 0; r < 3; r++)
				d.nrm[4 * col + r] = in.normal[3 * col + r];
		d.node_base = m.node_base, d.tri_base = m.tri_base, d.shade_base = m.shade_base;
		d.root_entry = (m.device_built || m.bvh.nodes[0].count < 0)
						   ? rt::make_entry((int)m.n4_base, -1, false)
						   : rt::make_entry(m.bvh.nodes[0].left_first + (int)m.tri_base, m.bvh.nodes[0].count, false);
		float lo[3] = {1e34f, 1e34f, 1e34f}, hi[3] = {-1e34f, -1e34f, -1e34f};
		for (int k = 0; k < 8; k++)
		{
			const float p[3] = {k & 1 ? m.bounds_max[0] : m.bounds_min[0], k & 2 ? m.bounds_max[1] : m.bounds_min[1],
								k & 4 ? m.bounds_max[2] : m.bounds_min[2]};
			for (int r = 0; r < 3; r++)
			{
				const float w = in.transform[r] * p[0] + in.transform[4 + r] * p[1] + in.transform[8 + r] * p[2] + in.transform[12 + r];
				lo[r] = std::min(lo[r], w), hi[r] = std::max(hi[r], w);
			}
		}
		if (world.valid && world.member[i])
			continue; // its triangles hang in the world tree: no top-level leaf of its own
		for (int r = 0; r < 3; r++)
		{
			const float pad = 1e-4f + 1e-5f * std::max(std::fabs(lo[r]), std::fabs(hi[r]));
			bmin.push_back(lo[r] - pad), bmax.push_back(hi[r] + pad);
		}
		live.push_back((uint32_t)i);
	}
	if (world.valid)
	{
		for (int r = 0; r < 3; r++)
			bmin.push_back(world.bmin[r]), bmax.push_back(world.bmax[r]);
		live.push_back(WORLD_ID); // ONE top-level leaf for all of it, replaced by the entry of the world tree's root below
	}
	const uint32_t world_root_entry = !world.valid		 ? 0u
									  : !world.n4.empty() ? rt::make_entry((int)world.n4_base, -1, false)
														  : rt::make_entry((int)(world.root_first + world.tri_base), (int)world.root_count, false);
	bvh::Result tl;
	bvh::build(bmin.data(), bmax.data(), live.size(), 1, TLAS_DEPTH_LIMIT, tl);
	std::vector<uint32_t> tprims(std::max<size_t>(1, live.size()), 0u);
	for (size_t k = 0; k < live.size(); k++)
		tprims[k] = live[tl.order[k]];
	std::vector<rt::Node4> tl4;
	const bool tl_inner = bvh::collapse4(tl, true, tl4);
	{
		const int tlas_need = bvh::stack_need4(tl4);
		int blas_need = world.valid ? world.stack_need : 0;
		for (uint32_t i : live)
			if (i != WORLD_ID)
				blas_need = std::max(blas_need, c->meshes[c->instances[i].mesh].stack_need);
		// the packet form of the primary wave keeps ONE stack of PACKET_STACK entries per wave (kernels.hip: PacketStack)
		c->packet_ok = tlas_need + 1 + blas_need <= (int)rtk::PACKET_STACK;
		if (tlas_need + 1 + blas_need > rt::STACK_CAPACITY)
			return set_error(RFWHIP_ERR_UNSUPPORTED, "rfwhip_update: top-level tree over %zu instances needs %d traversal-stack "
							 "entries + 1 + %d for the deepest mesh (capacity %d)", live.size(), tlas_need, blas_need, rt::STACK_CAPACITY);
	}
	if (c->blas_nodes4 + tl4.size() > c->node4_capacity)
		return set_error(RFWHIP_ERR_STATE, "internal: TLAS does not fit behind the BLAS nodes");
	const uint32_t tlas_base = (uint32_t)c->blas_nodes4;
	// FLAT instances: an instance with the identity transform whose mesh no other instance uses is linked into the top-level
	// tree directly — its top-level leaf becomes the entry of its mesh's root, so a ray walks from the top-level nodes into the
	// mesh's nodes without the instance switch (ray transform and three divisions on the way in, the sentinel and the same on
	// the way out — and, in the wave kernels, a wait for the wave's next leaf phase each time).  The world-space ray IS the
	// object-space ray there (1 * x + 0 * y + 0 * z + 0 is exact), so nothing a ray computes changes; the triangles carry the
	// instance index the hit record needs (rtk::launch_stamp_instance).  Static world geometry is typically instanced this way.
	std::vector<uint8_t> flat(c->instances.size(), 0);
	{
		std::vector<uint32_t> uses(c->meshes.size(), 0u);
		for (uint32_t i : live)
			if (i != WORLD_ID)
				uses[c->instances[i].mesh]++;
		static const float ident[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
		for (uint32_t i : live)
		{
			if (i == WORLD_ID)
				continue;
			bool id = uses[c->instances[i].mesh] == 1u && c->flat_instances != 0;
			for (int k = 0; k < 12 && id; k++)
				id = inst[i].inv[k] == ident[k];
			flat[i] = id ? 1 : 0;
		}
	}
	auto flat_entry = [&](uint32_t e) -> uint32_t { // a top-level leaf entry -> the mesh root's entry when its instance is flat
		if (e == rt::ENTRY_EMPTY || !(e & rt::ENTRY_LEAF))
			return e;
		const uint32_t ii = tprims[e & rt::ENTRY_FIRST_MASK];
		if (ii == WORLD_ID)
			return world_root_entry;
		return flat[ii] ? inst[ii].root_entry : e;
	};
	for (rt::Node4 &nd : tl4)
		for (int j = 0; j < 4; j++)
		{
			if (nd.entry[j] != rt::ENTRY_EMPTY && !(nd.entry[j] & rt::ENTRY_LEAF))
				nd.entry[j] += tlas_base; // inner: absolute node index; leaves index tlas_prims
			else
				nd.entry[j] = flat_entry(nd.entry[j]);
		}
	for (uint32_t i : live)
		if (i != WORLD_ID && flat[i])
		{
			const MeshRec &m = c->meshes[c->instances[i].mesh];
			rtk::launch_stamp_instance(c->d_tri_verts.as<f4>() + 3ull * m.tri_base, (uint32_t)m.triCount, i, c->stream);
		}
	RF_TRY(dm::last_launch_error());
	RF_TRY(c->d_instances.ensure(std::max<size_t>(1, inst.size()) * sizeof(rt::Instance)));
	RF_TRY(c->d_tlas_prims.ensure(tprims.size() * 4));
	RF_TRY(dm::h2d(c->d_instances.p, inst.data(), inst.size() * sizeof(rt::Instance), c->stream));
	std::vector<rt::Node4c> tl4c(tl4.size());
	for (size_t k = 0; k < tl4.size(); k++)
		tl4c[k] = compress4(tl4[k]);
	RF_TRY(dm::h2d(c->d_nodes4.as<rt::Node4c>() + tlas_base, tl4c.data(), tl4c.size() * sizeof(rt::Node4c), c->stream));
	std::vector<uint32_t> tprims_dev = tprims; // (the world tree's top-level slot is never looked up: its leaf entry was replaced above)
	for (uint32_t &tp : tprims_dev)
		if (tp == WORLD_ID)
			tp = 0u;
	RF_TRY(dm::h2d(c->d_tlas_prims.p, tprims_dev.data(), tprims_dev.size() * 4, c->stream));
	// the float form of every traversal node (mesh trees as rebuilt / refitted above + the top-level tree): one streaming pass
	// (only when the packet form of the primary wave — its one reader — can run: the table is twice the compressed one's size)
	c->packet_ok = c->packet_ok && (tlas_base + tl4c.size()) * sizeof(rt::Node4f) < (1ull << 32);
	c->nodes4_live = tlas_base + tl4c.size(), c->nodes4f_current = false;
	RF_TRY(ensure_nodes4f(c));
	// the trees the primary wave's ordering pass can order (primary_order.h): a mesh tree exactly one instance walks (in that
	// instance's object space; a flat instance's is the world), the world tree and the top-level tree
	{
		c->ord_ranges.clear(), c->ord_valid = false, c->ent_valid = false;
		std::vector<uint32_t> uses(c->meshes.size(), 0u), who(c->meshes.size(), 0u);
		for (uint32_t i : live)
			if (i != WORLD_ID)
				uses[c->instances[i].mesh]++, who[c->instances[i].mesh] = i;
		for (size_t mi = 0; mi < c->meshes.size(); mi++)
		{
			const MeshRec &m = c->meshes[mi];
			if (!m.used || !m.resident || !m.n4_count || uses[mi] != 1u || (size_t)m.n4_base + m.n4_count > tlas_base)
				continue;
			OrderRange r;
			r.first = m.n4_base, r.count = m.n4_count, r.object_space = true;
			memcpy(r.inv, inst[who[mi]].inv, sizeof(r.inv));
			c->ord_ranges.push_back(r);
		}
		if (world.valid && world.resident && !world.n4.empty() && (size_t)world.n4_base + world.n4.size() <= tlas_base)
		{
			OrderRange r;
			r.first = world.n4_base, r.count = (uint32_t)world.n4.size();
			c->ord_ranges.push_back(r);
		}
		if (!tl4c.empty())
		{
			OrderRange r;
			r.first = tlas_base, r.count = (uint32_t)tl4c.size();
			c->ord_ranges.push_back(r);
		}
		std::sort(c->ord_ranges.begin(), c->ord_ranges.end(), [](const OrderRange &a, const OrderRange &b) { return a.first < b.first; });
	}
	RF_TRY(dm::last_launch_error());
	RF_TRY(dm::sync(c->stream));
	c->instance_count = (uint32_t)live.size();
	c->tlas_root_entry = live.empty() ? 0u
						 : tl_inner	   ? rt::make_entry((int)tlas_base, -1, true)
									   : flat_entry(rt::make_entry(tl.nodes[0].left_first, tl.nodes[0].count, true));

	rt::SceneView &sv = c->sv;
	sv.nodes4 = c->d_nodes4.as<rt::Node4c>(), sv.nodes4f = c->d_nodes4f.as<rt::Node4f>();
	sv.nodes = c->d_nodes.as<rt::Node>(), sv.tri_verts = c->d_tri_verts.as<f4>();
	sv.tri_shade = c->d_tri_shade.as<rt::TriShade>();
	sv.tri_uv = c->d_tri_uv.as<rt::TriUV>();
	sv.tlas_prims = c->d_tlas_prims.as<uint32_t>();
	sv.instances = c->d_instances.as<rt::Instance>();
	sv.tlas_root_entry = c->tlas_root_entry, sv.instance_count = c->instance_count;
	sv.materials = c->d_materials.as<rt::MaterialRec>(), sv.material_count = c->material_count;
	sv.textures = c->d_textures.as<rt::TexDesc>(), sv.texture_count = c->texture_count;
	sv.tex_u32 = c->d_tex_u32.as<uint32_t>(), sv.tex_f4 = c->d_tex_f4.as<f4>();
	sv.sky = c->d_sky.as<f4>(), sv.sky_w = c->sky_w, sv.sky_h = c->sky_h;
	sv.area = c->d_area.as<rt::AreaLight>(), sv.point = c->d_point.as<rt::PointLight>();
	sv.spot = c->d_spot.as<rt::SpotLight>(), sv.dir = c->d_dir.as<rt::DirectionalLight>();
	sv.n_area = c->lc.areaLightCount, sv.n_point = c->lc.pointLightCount, sv.n_spot = c->lc.spotLightCount;
	sv.n_dir = c->lc.directionalLightCount;
	RF_TRY(refresh_lights(c));
	RF_TRY(update_sky_sampling(c));
	if (c->lt_stale)
		RF_TRY(update_light_tree(c));
	c->scene_dirty = false;
	c->scene_version++; // (the denoiser's guides are recomputed)
	// which instances this update changed (transform, mesh, or the mesh's vertices): the temporal stage does not reproject them
	c->dn_inst_ver.assign(c->instances.size(), 0u);
	for (size_t i = 0; i < c->instances.size(); i++)
	{
		InstRec &in = c->instances[i];
		const uint32_t edits = in.used && in.mesh < c->meshes.size() ? c->meshes[in.mesh].edits : 0u;
		if (in.used != in.dn_used || (in.used && (in.mesh != in.dn_mesh || edits != in.dn_edits ||
												  memcmp(in.transform, in.dn_transform, sizeof(in.transform)) != 0)))
		{
			in.dn_version = c->scene_version;
			in.dn_used = in.used, in.dn_mesh = in.mesh, in.dn_edits = edits;
			memcpy(in.dn_transform, in.transform, sizeof(in.transform));
		}
		c->dn_inst_ver[i] = (uint32_t)in.dn_version;
	}
	c->dn_inst_ver_stale = true; // (uploaded by the next temporal stage: whatever the order of update, init and the setting)
	c->depth_stats_valid = false;
	c->shadow_packets_auto_on = true; // (another scene: the packet form of the depth-0 connection wave gets its chance again)
	return RFWHIP_OK;
}

// =================================================================================================================
// camera
// =================================================================================================================
extern "C" void rfwhip_camera_get_view(const rfwhip_camera *cam, rfwhip_camera_view *view)
{
	// Camera::get_view, Camera.cpp:74-88 + calculate_matrix :109-115
	const float dx = cam->direction[0], dy = cam->direction[1], dz = cam->direction[2];
	// x = normalize(cross(z, (0,1,0)))
	float rx = dy * 0.0f - 1.0f * dz, ry = dz * 0.0f - 0.0f * dx, rz = dx * 1.0f - 0.0f * dy;
	const float rl = 1.0f / sqrtf(rx * rx + ry * ry + rz * rz);
	rx *= rl, ry *= rl, rz *= rl;
	// y = cross(x, z)
	const float ux = ry * dz - dy * rz, uy = rz * dx - dz * rx, uz = rx * dy - dx * ry;
	const float pi = 3.14159265358979323846f;
	view->spreadAngle = (cam->FOV * pi / 180) / (float)cam->pixelCount[1];
	const float screenSize = tanf(cam->FOV / 2.0f / (180.0f / pi));
	const float cx = cam->position[0] + cam->focalDistance * dx, cy = cam->position[1] + cam->focalDistance * dy,
				cz = cam->position[2] + cam->focalDistance * dz;
	const float hx = ((screenSize * rx) * cam->focalDistance) * cam->aspectRatio,
				hy = ((screenSize * ry) * cam->focalDistance) * cam->aspectRatio,
				hz = ((screenSize * rz) * cam->focalDistance) * cam->aspectRatio;
	const float sv = screenSize * cam->focalDistance;
	const float vx = sv * ux, vy = sv * uy, vz = sv * uz;
	view->pos[0] = cam->position[0], view->pos[1] = cam->position[1], view->pos[2] = cam->position[2];
	view->p1[0] = (cx - hx) + vx, view->p1[1] = (cy - hy) + vy, view->p1[2] = (cz - hz) + vz;
	view->p2[0] = (cx + hx) + vx, view->p2[1] = (cy + hy) + vy, view->p2[2] = (cz + hz) + vz;
	view->p3[0] = (cx - hx) - vx, view->p3[1] = (cy - hy) - vy, view->p3[2] = (cz - hz) - vz;
	view->aperture = cam->aperture;
}

// =================================================================================================================
// render
// =================================================================================================================
static int sync_all(rfwhip_context *c);
// Path state per slot of the per-ray buffers: origin / direction / throughput x 2 depth parities, hit + instance x 2 (primary
// wave kept apart), shadow origin / direction / contribution x 2 depth parities = 232 B; radiance: shade + connections = 32 B
// per radiance slot.  rad_slots[k]: slots of radiance set k (a ring call uses set 0 only, as `ring` slices; a call cut into
// sub-batches double-buffers sets 0 / 1).
constexpr size_t WAVE_SLOT_BYTES = 2 * 3 * sizeof(f4) + 2 * (sizeof(f4) + 4) + 2 * 3 * sizeof(f4);
constexpr size_t RAD_SLOT_BYTES = 2 * sizeof(f4);
constexpr size_t HIT0_DONE_PAD = 512; // bytes beyond one per 64 slots in WaveView::hit0_done: every slice in flight begins on a byte of its own
constexpr double SHADOW_PACKET_MAX_BINS_PER_RUN = 8.0; // (shadow_packets = -1; measured: DESIGN.md §4 "Round 6")
static size_t wave_bytes_held(const rfwhip_context *c);
static int ensure_wave_buffers(rfwhip_context *c, size_t paths, size_t rad_slots0, size_t rad_slots1)
{
	const size_t rad_slots[2] = {rad_slots0, rad_slots1};
	if (paths <= c->wave_capacity && rad_slots0 <= c->rad_capacity[0] && rad_slots1 <= c->rad_capacity[1])
		return 0;
	RF_TRY(sync_all(c));
	for (int r = 0; r < rfwhip_context::MAX_RING; r++) // (everything was synchronised above)
		c->resolve_recorded[r] = false;
	// (a failed allocation leaves the capacities at 0: the next call lays everything out again)
	c->wave_capacity = 0, c->rad_capacity[0] = c->rad_capacity[1] = 0;
	const size_t b16 = paths * sizeof(f4);
	int rc = 0;
	for (int k = 0; k < 2 && !rc; k++)
		rc = c->d_org[k].ensure_exact(b16) || c->d_dir2[k].ensure_exact(b16) || c->d_thr[k].ensure_exact(b16) ||
			 c->d_sh_org[k].ensure_exact(b16) || c->d_sh_dir[k].ensure_exact(b16) || c->d_sh_rad[k].ensure_exact(b16) ||
			 c->d_rad[k].ensure_exact(rad_slots[k] * sizeof(f4)) || c->d_rad_nee[k].ensure_exact(rad_slots[k] * sizeof(f4));
	rc = rc || c->d_hit.ensure_exact(b16) || c->d_hit_inst.ensure_exact(paths * 4) || c->d_hit0.ensure_exact(b16) ||
		 c->d_hit0_inst.ensure_exact(paths * 4) || c->d_hit0_done.ensure_exact((paths >> 6) + HIT0_DONE_PAD);
	if (rc)
		return set_error(RFWHIP_ERR_HIP, "out of device memory for the path state: %zu slots x %zu B + %zu radiance slots x %zu B "
										 "(%.1f GB; lower spp, or ring / streams)", paths, WAVE_SLOT_BYTES, rad_slots0 + rad_slots1,
						 RAD_SLOT_BYTES, (paths * WAVE_SLOT_BYTES + (rad_slots0 + rad_slots1) * RAD_SLOT_BYTES) * 1e-9);
	c->wave_capacity = paths, c->rad_capacity[0] = rad_slots0, c->rad_capacity[1] = rad_slots1;
	return 0;
}
static size_t wave_bytes_held(const rfwhip_context *c)
{
	size_t n = c->d_hit.cap + c->d_hit_inst.cap + c->d_hit0.cap + c->d_hit0_inst.cap + c->d_hit0_done.cap;
	for (int k = 0; k < 2; k++)
		n += c->d_org[k].cap + c->d_dir2[k].cap + c->d_thr[k].cap + c->d_sh_org[k].cap + c->d_sh_dir[k].cap + c->d_sh_rad[k].cap +
			 c->d_rad[k].cap + c->d_rad_nee[k].cap;
	return n;
}

static dm::event_t *next_event(rfwhip_context *c)
{
	if (c->events_used == c->event_pool.size())
	{
		dm::event_t e;
		dm::event_create(&e);
		c->event_pool.push_back(e);
	}
	return &c->event_pool[c->events_used++];
}

struct StageTimer
{
	rfwhip_context *c;
	size_t ia = 0, ib = 0;
	bool on;
	void *stream;
	StageTimer(rfwhip_context *ctx, int family, int depth, void *st = nullptr)
		: c(ctx), on(ctx->stage_timing != 0), stream(st ? st : ctx->stream)
	{
		if (!on)
			return;
		next_event(c), ia = c->events_used - 1;
		next_event(c), ib = c->events_used - 1;
		dm::event_record(c->event_pool[ia], stream);
		fam = family, dep = depth;
	}
	int fam = 0, dep = 0;
	bool fused = false;
	void stop(int launches = 1)
	{
		if (!on)
			return;
		dm::event_record(c->event_pool[ib], stream);
		TimedSpan s;
		s.a = c->event_pool[ia], s.b = c->event_pool[ib], s.family = fam, s.depth = dep, s.fused = fused;
		c->spans.push_back(s);
		c->kernel_launches[fam] += (uint32_t)launches;
	}
};

static void fill_params(rfwhip_context *c, const rfwhip_camera *cam, rtk::Params &p)
{
	memset(&p, 0, sizeof(p));
	p.sc = c->sv;
	rt::WaveView &wv = p.wv;
	for (int k = 0; k < 2; k++)
		wv.org[k] = c->d_org[k].as<f4>(), wv.dir[k] = c->d_dir2[k].as<f4>(), wv.thr[k] = c->d_thr[k].as<f4>();
	wv.hit = c->d_hit.as<f4>(), wv.hit_inst = c->d_hit_inst.as<int>();
	wv.hit0 = c->d_hit0.as<f4>(), wv.hit0_inst = c->d_hit0_inst.as<int>(), wv.hit0_done = nullptr;
	wv.sh_org = c->d_sh_org[0].as<f4>(), wv.sh_dir = c->d_sh_dir[0].as<f4>(), wv.sh_rad = c->d_sh_rad[0].as<f4>();
	wv.rad = c->d_rad[0].as<f4>(), wv.rad_nee = nullptr, wv.acc = c->d_acc.as<f4>();
	wv.packet_rng = c->d_packet_rng.as<uint32_t>();
	wv.counters = c->d_counters.as<rt::WaveCounters>();
	p.cam.blue_noise = nullptr;
	if (cam)
	{
		rfwhip_camera_view v;
		rfwhip_camera_get_view(cam, &v);
		p.cam.pos = rt::f3{v.pos[0], v.pos[1], v.pos[2]};
		p.cam.p1 = rt::f3{v.p1[0], v.p1[1], v.p1[2]};
		p.cam.right = rt::f3{v.p2[0] - v.p1[0], v.p2[1] - v.p1[1], v.p2[2] - v.p1[2]};
		p.cam.up = rt::f3{v.p3[0] - v.p1[0], v.p3[1] - v.p1[1], v.p3[2] - v.p1[2]};
		p.cam.aperture = v.aperture, p.cam.spread_angle = v.spreadAngle, p.cam.clamp_value = cam->clampValue;
		p.cam.blue_noise = (c->sampler == 1 && c->have_blue_noise) ? c->d_blue_noise.as<uint32_t>() : nullptr;
	}
	p.fr = c->fr;
	p.fr.spp = (uint32_t)c->spp;
	p.fr.sample_base = c->sample_origin + c->samples_done;
	p.fr.probe_pixel = c->probe_y * c->W + c->probe_x;
	p.max_depth = (uint32_t)c->max_depth;
	p.parity_no_jitter = c->jitter == 1;
	// LDS top-of-tree cache: the first nodes (breadth-first top, bvh::collapse4) of the BLAS with the most nodes
	p.lds_first = 0, p.lds_count = 0;
	{
		// (... among the trees the rays walk: the meshes whose instances went into the world tree are not among them; that tree is)
		uint32_t big_base = 0, big_count = 0;
		for (size_t mi = 0; mi < c->meshes.size(); mi++)
		{
			const MeshRec &m = c->meshes[mi];
			const bool in_world = c->wtree.valid && mi < c->wtree.mesh_all.size() && c->wtree.mesh_all[mi];
			if (m.used && !in_world && m.n4_count > big_count)
				big_base = (uint32_t)m.n4_base, big_count = m.n4_count;
		}
		if (c->wtree.valid && c->wtree.resident && c->wtree.n4.size() > big_count)
			big_base = c->wtree.n4_base, big_count = (uint32_t)c->wtree.n4.size();
		const uint32_t cap = rtk::max_lds_nodes();
		const uint32_t want = c->lds_nodes < 0 ? cap : std::min<uint32_t>((uint32_t)c->lds_nodes, cap);
		if (big_count && want)
			p.lds_first = big_base, p.lds_count = std::min<uint32_t>(want, big_count);
	}
	p.refill = (uint32_t)c->refill & ((c->packet_ok && c->nodes4f_current) ? 15u : 7u);
	p.textured = c->textured ? 1u : 0u;
}

static int sync_all(rfwhip_context *c)
{
	for (int i = 0; i < rfwhip_context::MAX_SUB; i++)
	{
		if (c->sub_stream[i])
			RF_TRY(dm::sync(c->sub_stream[i]));
		if (c->conn_stream[i])
			RF_TRY(dm::sync(c->conn_stream[i]));
	}
	RF_TRY(dm::sync(c->stream));
	// what this context enqueued on a CALLER's stream still reads or writes its memory (MarkId says what): resize, cleanup and the
	// scene setters must not free or rewrite anything under it
	for (StreamMark &m : c->marks)
		RF_TRY(m.sync());
	return 0;
}

static int ensure_sub_batches(rfwhip_context *c, int subs)
{
	if (!c->events_ready)
	{
		RF_TRY(dm::event_create(&c->ev_prologue));
		for (int r = 0; r < rfwhip_context::MAX_RING; r++)
			RF_TRY(dm::event_create(&c->ev_resolve[r]));
		RF_TRY(dm::event_create(&c->ev_present_in));
		RF_TRY(dm::event_create(&c->adaptive_pub.ev));
		RF_TRY(dm::event_create(&c->order_pub.ev));
		RF_TRY(dm::event_create(&c->entry_pub.ev));
		for (int i = 0; i < rfwhip_context::MAX_SUB; i++)
		{
			RF_TRY(dm::event_create(&c->ev_sub_done[i]));
			RF_TRY(dm::event_create(&c->ev_conn_last[i]));
			for (int d = 0; d < rt::MAX_DEPTH_SLOTS; d++)
			{
				RF_TRY(dm::event_create(&c->ev_shade[i][d]));
				RF_TRY(dm::event_create(&c->ev_conn[i][d]));
			}
		}
		c->events_ready = true;
	}
	for (int i = 0; i < subs; i++)
	{
		if (!c->sub_stream[i])
			RF_TRY(dm::stream_create(&c->sub_stream[i]));
		if (!c->conn_stream[i])
			RF_TRY(dm::stream_create(&c->conn_stream[i]));
		if (i > 0 && !c->d_counters_sub[i].p)
		{
			RF_TRY(c->d_counters_sub[i].ensure(sizeof(rt::WaveCounters)));
			RF_TRY(dm::zero(c->d_counters_sub[i].p, sizeof(rt::WaveCounters), c->stream));
			RF_TRY(dm::sync(c->stream));
		}
	}
	return 0;
}

// How many items the launches of depth d of a pt call should be SIZED for (grids only: every kernel reads its real count on the
// device and works through whatever it finds).  The host never reads a counter between bounces, so every launch used to get a grid
// for the primary count — for the deeper waves of a small call a chip-wide persistent grid whose waves find a few dozen rays each.
// Paths per primary at depth d: from the counts of the last frame this context waited for (rfwhip_get_stats; same scene, any spp),
// with a quarter of headroom; before there is one — and after every rfwhip_update(), until a frame of the new scene has been
// waited for — a half per depth.  shade = false: the traversal launch of depth d — extension rays of depth d and the shadow rays
// of depth d - 1 beside them; true: the shade launch of depth d.
static uint32_t depth_items(const rfwhip_context *c, uint32_t n, int d, bool shade)
{
	if (d <= 0)
		return n;
	const rfwhip_render_stats &st = c->stats;
	double ext = 1.0, prev = 1.0, shadow_per_path = 0.8;
	if (st.primaryCount > 0 && c->depth_stats_valid) // (after rfwhip_update the counts of the last frame describe another scene)
	{
		const double p = (double)st.primaryCount, r1 = (double)st.secondaryCount / p, rdeep = (double)st.deepCount / p;
		// (deepCount adds up every depth >= 2: taken as the bound for each of them)
		ext = d == 1 ? r1 : rdeep, prev = d == 1 ? 1.0 : (d == 2 ? r1 : rdeep);
		shadow_per_path = std::min(1.0, (double)st.shadowCount / std::max(1.0, p * (0.7 + r1 + rdeep))) + 0.1;
	}
	else
		for (int k = 0; k < d; k++)
			prev = ext, ext *= 0.5;
	const double want = shade ? ext : std::max(ext, prev * shadow_per_path);
	const double items = std::min(1.0, 1.25 * want + 0.02) * (double)n;
	return (uint32_t)std::max(1.0, items);
}

// ---- the primary wave's camera-ordered node table (primary_order.h) ----------------------------------------------------------------
// Does a render call of `paths` path slots use it?  RFWHIP_PRIMARY_ORDER says never / always; otherwise when the pass is noise beside
// the call's primary wave even if the camera moves with every call: the pass reads and writes the table once, 2 x table bytes, at
// ~0.3 ps per byte of HBM traffic; a primary path costs ~32 ps of the packet kernel (4.2 ms per 133 M, DESIGN_LOG.md).  One path slot
// per byte moved puts the pass at 1 % of the primary wave (measured: DESIGN_LOG.md, round 8).  Small interactive frames keep the
// kernel that sorts for itself.
static bool primary_order_wanted(const rfwhip_context *c, size_t paths)
{
	if (c->primary_order == 0 || c->integrator != 1 || !c->packet_ok || !c->nodes4f_current || !(c->refill & 8) || !c->nodes4_live)
		return false;
	if (c->primary_order == 1)
		return true;
	return paths >= 2 * c->nodes4_live * sizeof(rt::Node4f);
}

// The table for camera position `pos`, rewritten on the main stream when it is stale: another position (by its bits), or d_nodes4f
// rewritten since (every rfwhip_update that changes a tree, a pose, a refit or an instance's transform ends in ensure_nodes4f).  The
// primary waves of the calls in flight read the table on their sub-batch streams: the rewrite waits for their ev_sub_done — every
// one of them has been waited for by its own call's epilogue on this stream already, the waits here say so where it matters.
static int ensure_primary_order(rfwhip_context *c, const rt::f3 &pos)
{
	uint32_t bits[3];
	memcpy(&bits[0], &pos.x, 4), memcpy(&bits[1], &pos.y, 4), memcpy(&bits[2], &pos.z, 4);
	if (c->ord_valid && c->ord_version == c->nodes4f_version && !memcmp(bits, c->ord_cam, sizeof(bits)))
		return 0;
	const size_t bytes = c->node4_capacity * sizeof(rt::Node4f);
	if (bytes > c->d_nodes4f_ord.cap)
		RF_TRY(sync_all(c)); // (the buffer moves)
	RF_TRY(c->d_nodes4f_ord.ensure(bytes));
	RF_TRY(c->order_pub.before_rewrite(c));
	const rt::Node4f *in = c->d_nodes4f.as<rt::Node4f>();
	rt::Node4f *out = c->d_nodes4f_ord.as<rt::Node4f>();
	StageTimer t(c, KF_PRIMARY_ORDER, -1);
	const float cam[3] = {pos.x, pos.y, pos.z};
	uint32_t at = 0; // ranges ascend (rfwhip_update); what lies between them is copied as it is
	bool run_ordered = false;
	uint32_t run_first = 0, run_count = 0;
	float run_origin[3] = {0, 0, 0};
	auto flush = [&]() {
		if (run_count)
			rtk::launch_order4f(in, out, run_first, run_count, run_origin, run_ordered, c->stream);
		run_count = 0;
	};
	auto add = [&](uint32_t first, uint32_t count, bool ordered, const float *origin) { // (neighbours handled alike: one launch)
		if (!count)
			return;
		if (run_count && run_first + run_count == first && run_ordered == ordered && (!ordered || !memcmp(run_origin, origin, 12)))
		{
			run_count += count;
			return;
		}
		flush();
		run_first = first, run_count = count, run_ordered = ordered;
		if (ordered)
			memcpy(run_origin, origin, 12);
	};
	for (const OrderRange &r : c->ord_ranges)
	{
		if (r.first < at || (size_t)r.first + r.count > c->nodes4_live)
			continue; // (never: the layout's ranges are disjoint)
		add(at, r.first - at, false, nullptr);
		float o[3] = {cam[0], cam[1], cam[2]};
		if (r.object_space)
			for (int k = 0; k < 3; k++)
				o[k] = r.inv[4 * k] * cam[0] + r.inv[4 * k + 1] * cam[1] + r.inv[4 * k + 2] * cam[2] + r.inv[4 * k + 3];
		add(r.first, r.count, true, o);
		at = r.first + r.count;
	}
	add(at, (uint32_t)c->nodes4_live - at, false, nullptr);
	flush();
	t.stop(0);
	c->kernel_launches[KF_PRIMARY_ORDER]++;
	RF_TRY(dm::last_launch_error());
	RF_TRY(c->order_pub.publish(c->stream));
	c->ord_valid = true, c->ord_version = c->nodes4f_version;
	memcpy(c->ord_cam, bits, sizeof(bits));
	return 0;
}

// ---- the primary wave's entry snapshot (primary_entry.h) --------------------------------------------------------------------------
// It rides on the ordered table (the caller has just made that current) and needs ONE origin for a group's rays: no lens.  The per-ray
// counters of count_traversal keep the meaning of a walk from the root, so a counting call starts there.
// The pass is a thread per record that walks some ten nodes in double precision: 0.57 ms for the 2.07 M records of a 1080p frame in
// groups of 64 (0.28 ns per record), against 19.6 ps per path of the primary wave that starts from them (2.6 ms per 133 M;
// DESIGN_LOG.md, round 9) — 2 % of the call's primary wave from 720 paths per record.  Below that a pass per call would eat a fifth
// of what it saves or more, so by the rule (-1) a smaller call gets records only when its view is the previous call's: a camera at
// rest, whose calls all reuse them (a converging render: 256 spp per call and record on the bench).  1 makes them for every view.
constexpr size_t PRIMARY_ENTRY_PATHS_PER_RECORD = 720;
static bool primary_entry_wanted(const rfwhip_context *c, const rtk::Params &base)
{
	return c->primary_entry != 0 && base.cam.aperture == 0.0f && c->count_traversal == 0;
}

// The records for this view, frame and table, rewritten on the main stream when any of them has changed (compared by their bits).
// Readers and the rewrite are ordered like the ordered table's (ensure_primary_order).
// *use: the call's primary wave starts from the records
static int ensure_primary_entry(rfwhip_context *c, const rtk::Params &base, size_t paths, bool *use)
{
	*use = false;
	uint32_t key[32] = {};
	static_assert(sizeof(rt::f3) == 12, "four vectors of the view");
	memcpy(&key[0], &base.cam.pos, 12), memcpy(&key[3], &base.cam.p1, 12), memcpy(&key[6], &base.cam.right, 12), memcpy(&key[9], &base.cam.up, 12);
	memcpy(&key[12], &base.fr.inv_w, 4), memcpy(&key[13], &base.fr.inv_h, 4);
	key[14] = base.fr.W, key[15] = base.fr.H, key[16] = base.fr.tiles_x, key[17] = base.fr.slots, key[18] = base.fr.sgroup_log2;
	key[19] = base.fr.local_rows, key[20] = base.fr.rank, key[21] = base.fr.world;
	key[22] = (uint32_t)c->order_pub.serial, key[23] = (uint32_t)(c->order_pub.serial >> 32);
	key[24] = base.sc.instance_count ? base.sc.tlas_root_entry : rtk::PRIMARY_ENTRY_NO_ROOT;
	const bool at_rest = !memcmp(key, c->ent_last_key, sizeof(key));
	memcpy(c->ent_last_key, key, sizeof(key));
	*use = true;
	if (c->ent_valid && !memcmp(key, c->ent_key, sizeof(key)))
		return 0;
	const uint32_t groups = (uint32_t)(((size_t)base.fr.slots << base.fr.sgroup_log2) >> 6);
	if (c->primary_entry < 0 && !at_rest && paths < PRIMARY_ENTRY_PATHS_PER_RECORD * groups)
	{
		*use = false;
		return 0;
	}
	const size_t bytes = (size_t)groups * rtk::primary_entry_words() * 4;
	if (bytes > c->d_primary_entry.cap)
		RF_TRY(sync_all(c)); // (the buffer moves)
	RF_TRY(c->d_primary_entry.ensure(bytes));
	RF_TRY(c->entry_pub.before_rewrite(c));
	StageTimer t(c, KF_PRIMARY_ENTRY, -1);
	rtk::launch_primary_entry(c->d_nodes4f_ord.as<rt::Node4f>(), key[24], base.cam, base.fr, c->d_primary_entry.as<uint32_t>(), groups, c->stream);
	t.stop(0);
	c->kernel_launches[KF_PRIMARY_ENTRY]++;
	RF_TRY(dm::last_launch_error());
	RF_TRY(c->entry_pub.publish(c->stream));
	c->ent_valid = true;
	memcpy(c->ent_key, key, sizeof(key));
	return 0;
}

// One render call = `spp` samples per pixel.  The samples are cut into up to `streams` sub-batches that run the whole
// wavefront pipeline concurrently on their own HIP streams (own slices of the path buffers, own device counters):
// every traversal kernel ends with a tail in which a few long rays keep a handful of waves busy — a chain of ~150
// dependent node fetches at ~1 us each out of the Infinity Cache — and the other sub-batches' kernels fill the CUs
// during that tail.  The accumulator is touched by one resolve kernel over all sub-batches at the end (stream 0).
extern "C" int rfwhip_render(rfwhip_context *c, const rfwhip_camera *cam, int status)
{
	CTX_ENTER(c);
	if (!cam)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_render: null camera");
	if (!c->W || !c->H)
		return set_error(RFWHIP_ERR_STATE, "rfwhip_render before rfwhip_init");
	if (c->scene_dirty)
		return set_error(RFWHIP_ERR_STATE, "rfwhip_render: scene changed since the last rfwhip_update()");
	if (c->sky_stale)
		RF_TRY(update_sky_sampling(c));
	if (c->lt_stale)
		RF_TRY(update_light_tree(c));
	if (c->sampler == 1 && !c->have_blue_noise)
		return set_error(RFWHIP_ERR_STATE, "sampler=bluenoise needs rfwhip_set_blue_noise() first");
	if (c->integrator == 0 && (c->adaptive_sampling || c->adaptive_live))
		return set_error(RFWHIP_ERR_STATE, "rfwhip_render: adaptive_sampling needs integrator=pt");
	if (c->max_depth + 2 > rt::MAX_DEPTH_SLOTS)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "max_depth %d too large", c->max_depth);
	const size_t paths = (size_t)c->fr.slots * (size_t)c->spp;
	if (paths >= (1ull << 31))
		return set_error(RFWHIP_ERR_UNSUPPORTED, "spp batch too large: %zu path slots (limit 2^31)", paths);
	if (c->integrator == 1 && !c->nodes4f_current && c->packet_ok && (c->refill & 8))
	{
		// (`refill` bit 3 came on after the last update: the packet form's float node table is written now, once)
		RF_TRY(ensure_nodes4f(c));
		RF_TRY(dm::sync(c->stream));
	}
	// Sub-batches: a call is cut into up to `streams` concurrent sub-batches only when that leaves every one at least
	// `sub_batch_paths` path slots and there are four of them: since the bounce / shadow / primary kernels keep their lanes
	// filled themselves, ONE sub-batch whose calls alternate between two sets of wave buffers / streams / counters (so that
	// consecutive calls overlap each other's kernel tails, connection waves on a side stream) is as fast or faster up to
	// ~200 M path slots (MI355X, 1080p terrain, Msamples/s as one sub-batch on the ring / cut into four — 16 spp: 2635 / 2366,
	// 32 spp: 2693 / 2515, 64 spp: 2741 / 2665; beyond that the ring's four sets of path state no longer fit comfortably).
	const long long want = (long long)paths / c->sub_batch_paths;
	int subs = (int)std::min<long long>(std::min(std::min(c->streams, (int)rfwhip_context::MAX_SUB), c->spp), want);
	if (subs < std::min(4, c->streams))
		subs = 1;
	const bool alternate = subs == 1;
	// sample groups of the slot layout (rt_core.h): the largest power of two <= sample_group at which every sub-batch begins
	uint32_t sgroup_log2 = 0;
	while ((2 << sgroup_log2) <= c->sample_group)
	{
		const int g = 2 << sgroup_log2;
		bool ok = c->spp % g == 0;
		for (int k = 1; k < subs && ok; k++)
			ok = (int)((long long)c->spp * k / subs) % g == 0;
		if (!ok)
			break;
		sgroup_log2++;
	}
	// ring of buffer sets: a single-sub-batch call uses set (call number mod ring) of everything — up to `ring` calls are
	// in flight, each a full-size launch chain; a call cut into sub-batches double-buffers its radiance only.  The ring is as
	// deep as the setting allows and the device's free memory holds (264 B of path state per slot and ring entry: 1080p at
	// 64 spp = 133 M slots = 35 GB per entry); when it does not fit, 2 and then 1 entries are tried before the call fails.
	// the extension / shadow queues are filled in blocks (rt_types.h: QUEUE_BLOCK): every sub-batch's slice of the per-ray
	// buffers has room for the void entries of its waves' last blocks behind the rays
	const size_t pad = rtk::queue_pad((uint32_t)std::min<size_t>(paths, 0xFFFFFFFFu));
	int ring = alternate ? c->ring : 2;
	for (;;)
	{
		const size_t wave_slots = alternate ? (size_t)ring * (paths + pad) : paths + (size_t)subs * pad;
		const size_t rad0 = alternate ? (size_t)ring * paths : paths, rad1 = alternate ? 0 : paths;
		const bool fits_as_is = wave_slots <= c->wave_capacity && rad0 <= c->rad_capacity[0] && rad1 <= c->rad_capacity[1];
		if (alternate && ring > 1 && !fits_as_is)
		{
			size_t free_b = 0, total_b = 0;
			dm::mem_info(&free_b, &total_b);
			const double avail = 0.94 * ((double)free_b + (double)wave_bytes_held(c));
			if ((double)wave_slots * WAVE_SLOT_BYTES + (double)(rad0 + rad1) * RAD_SLOT_BYTES > avail)
			{
				ring = ring > 2 ? 2 : 1;
				continue;
			}
		}
		if (ring != c->ring_active || paths != c->paths_active || subs != c->subs_active)
		{
			// the calls in flight lay their records out for another ring / batch size
			RF_TRY(sync_all(c));
			for (int r = 0; r < rfwhip_context::MAX_RING; r++)
				c->resolve_recorded[r] = false;
			c->ring_active = ring, c->paths_active = paths, c->subs_active = subs, c->call_slot = 0;
		}
		const int rc = ensure_wave_buffers(c, wave_slots, rad0, rad1);
		if (rc && alternate && ring > 1) // (the estimate was too optimistic: another process, fragmentation)
		{
			ring = ring > 2 ? 2 : 1;
			continue;
		}
		RF_TRY(rc);
		break;
	}
	RF_TRY(ensure_sub_batches(c, alternate ? ring : subs));
	const bool pipelined = c->render_in_flight; // the caller enqueues calls without waiting for them in between
	if (!c->render_in_flight)
	{
		c->render_t0 = std::chrono::steady_clock::now();
		c->render_in_flight = true;
	}
	void *s0 = c->stream;
	// ---- prologue on stream 0 ----
	if (c->marks[MK_PRESENT].pending)
	{
		// a present enqueued on the caller's stream (rfwhip_read_local_framebuffer_stream) still reads the accumulator: the main
		// stream runs behind it from here on, so whoever waits for the main stream has waited for the present
		RF_TRY(c->marks[MK_PRESENT].wait_on(s0));
		c->marks[MK_PRESENT].pending = false;
	}
	if (status == RFWHIP_RESET)
	{
		RF_TRY(dm::zero(c->d_acc.p, (size_t)c->fr.local_rows * c->W * sizeof(f4), s0));
		c->samples_done = 0;
		RF_TRY(noise_clear(c, c->fr.local_rows, c->W, s0));
		// decorrelated reset frames for the denoiser's temporal stage: the sample indices go on where the last frame's ended
		// (mod 256: the blue-noise sampler's table)
		c->sample_origin = c->dn_temporal ? (uint32_t)(c->samples_total % 256u) : 0u;
		c->dn_reset_since = true;
	}
	if (c->adaptive_live && c->adaptive_mask_moved)
	{
		RF_TRY(c->adaptive_pub.publish(s0));
		c->adaptive_mask_moved = false;
	}
	const rtk::AdaptiveView ad = c->adaptive_live ? adaptive_view(c) : rtk::AdaptiveView{};
	const uint32_t packets = (c->W / 4u) * (c->H / 2u);
	if (c->integrator == 0 && c->jitter == 0)
	{
		// per-packet xor128 states for the whole batch (global packet order => image independent of world)
		StageTimer tg(c, KF_GENERATE, -1);
		if (!c->jump_table_uploaded)
		{
			RF_TRY(c->d_jump_table.ensure(c->jump_table.size() * 4));
			RF_TRY(dm::h2d(c->d_jump_table.p, c->jump_table.data(), c->jump_table.size() * 4, s0));
			c->jump_table_uploaded = true;
		}
		if ((size_t)std::max(1u, packets) * c->spp * 16 > c->d_packet_rng.cap)
			RF_TRY(sync_all(c));
		RF_TRY(c->d_packet_rng.ensure((size_t)std::max(1u, packets) * c->spp * 16));
		if (packets)
			rtk::launch_rng_states(c->d_packet_rng.as<uint32_t>(), c->rng_state, c->d_jump_table.as<uint32_t>(), packets,
								   (uint32_t)c->spp, s0);
		tg.stop();
		xor128_jump(c->jump_table, c->rng_state, (unsigned long long)packets * 32ull * (unsigned long long)c->spp);
	}
	const bool rng_prologue = c->integrator == 0 && c->jitter == 0;
	if (rng_prologue)
		RF_TRY(dm::event_record(c->ev_prologue, s0));
	const bool count = c->count_traversal != 0;
	const uint32_t row_group = std::max(1u, (c->fr.tiles_x << sgroup_log2) / 4u); // primary wave: one row of 8x8 tiles per XCD group
	const uint32_t par = c->call_slot;							 // buffer set of this call
	const uint32_t prev = (par + (uint32_t)ring - 1u) % (uint32_t)ring; // ... and of the previous one
	// (sky sampling: the sky is a light of its own — a scene without lights still has shadow rays then)
	const bool connect = c->integrator == 1 && (total_light_count(c) > 0 || c->sky_view.pick > 0.0f) && c->max_depth > 0;
	// Connection waves on a second stream hide the kernel tails of a call that runs alone (1 spp frames, wait after every
	// call: 1.56 -> 1.43 ms).  When the caller pipelines its calls, the ring of buffer sets already keeps up to four launch
	// chains in flight and the extra kernels only evict each other's working sets (1 spp: 1.17 ms without, 1.38 ms with the
	// side stream; 16 spp: 13.2 / 14.1 ms), and the same holds beside other sub-batches (4 sub-batches, 128 spp: -9 %).
	// extension rays of depth d + 1 and shadow rays of depth d in one launch (both in persistent-lane form): one tail per depth
	const bool fused = connect && c->fuse != 0 && (c->refill & 3) == 3 && c->overlap != 1;
	const bool side = connect && !fused && (c->overlap == 1 || (c->overlap < 0 && subs == 1 && !pipelined));
	rtk::Params base;
	fill_params(c, cam, base);
	set_sample_group(base.fr, sgroup_log2);
	c->sgroup_last = sgroup_log2;
	// the primary wave's camera-ordered node table, where the packet form runs and the call is large enough (primary_order_wanted):
	// rewritten here, on the main stream, when the camera has moved or the trees have changed
	const rt::Node4f *ordered = nullptr;
	if (primary_order_wanted(c, paths) && rtk::primary_packet_walk(base, (uint32_t)((size_t)c->fr.slots * (size_t)(c->spp / subs))))
	{
		RF_TRY(ensure_primary_order(c, base.cam.pos));
		ordered = c->d_nodes4f_ord.as<rt::Node4f>();
	}
	// ... and the entry snapshot of this view, behind it (primary_entry_wanted)
	const uint32_t *entry = nullptr;
	if (ordered && primary_entry_wanted(c, base))
	{
		bool use = false;
		RF_TRY(ensure_primary_entry(c, base, paths, &use));
		if (use)
			entry = c->d_primary_entry.as<uint32_t>();
	}
	c->primary_entry_last = entry != nullptr;
	base.wv.primary_entry = entry;
	base.wv.rad = alternate ? c->d_rad[0].as<f4>() + paths * par : c->d_rad[par].as<f4>();
	// the connections always add into their own buffer, on a side stream or not: the image is then bit-identical whichever way
	// a call is scheduled (e.g. the ranks of a strip split against the single-rank image)
	base.wv.rad_nee = !connect ? nullptr : (alternate ? c->d_rad_nee[0].as<f4>() + paths * par : c->d_rad_nee[par].as<f4>());
	// ---- sub-batches: each on its own stream; nothing here waits for the previous call's resolve ----
	const int first_slot = alternate ? (int)par : 0;
	for (int k = 0; k < subs; k++)
	{
		const int i = first_slot + k; // which set of streams / counters / buffer slices
		void *s = c->sub_stream[i], *sc = side ? c->conn_stream[i] : c->sub_stream[i];
		const uint32_t s_begin = (uint32_t)((long long)c->spp * k / subs), s_end = (uint32_t)((long long)c->spp * (k + 1) / subs);
		const uint32_t spp_i = s_end - s_begin;
		if (!spp_i)
			continue;
		if (rng_prologue)
			RF_TRY(dm::stream_wait_event(s, c->ev_prologue));
		if (c->resolve_recorded[par]) // the resolve of the call `ring` calls ago read this radiance set
			RF_TRY(dm::stream_wait_event(s, c->ev_resolve[par]));
		// Several sub-batches start together, behind the previous call's resolve: they render the same pixels, and while they
		// run in step their kernels share BVH nodes in the L2s (letting them drift apart costs 2-4 %)
		if (subs > 1 && c->resolve_recorded[prev])
			RF_TRY(dm::stream_wait_event(s, c->ev_resolve[prev]));
		if (c->conn_used[i]) // the previous call's connection waves still use this sub-batch's counters and shadow buffers
			RF_TRY(dm::stream_wait_event(s, c->ev_conn_last[i]));
		if (c->adaptive_live) // the mask this call reads: the state after the previous call
			RF_TRY(c->adaptive_pub.acquire(i, s));
		if (ordered) // the ordered table, if it was rewritten since this stream last read it
			RF_TRY(c->order_pub.acquire(i, s));
		if (entry) // ... and the snapshot's records
			RF_TRY(c->entry_pub.acquire(i, s));
		rtk::Params p = base;
		const size_t off_rad = (size_t)c->fr.slots * s_begin; // this sub-batch's slice of the radiance buffers of the call
		const size_t off = alternate ? (paths + pad) * par : off_rad + (size_t)k * pad; // and of every per-ray buffer (padded)
		for (int q = 0; q < 2; q++)
			p.wv.org[q] += off, p.wv.dir[q] += off, p.wv.thr[q] += off;
		p.wv.hit += off, p.wv.hit_inst += off, p.wv.hit0 += off, p.wv.hit0_inst += off;
		p.wv.rad += off_rad;
		if (p.wv.rad_nee)
			p.wv.rad_nee += off_rad;
		if (p.wv.packet_rng)
			p.wv.packet_rng += (size_t)s_begin * packets * 4;
		if (i > 0)
			p.wv.counters = c->d_counters_sub[i].as<rt::WaveCounters>();
		p.fr.spp = spp_i;
		p.fr.sample_base = c->sample_origin + c->samples_done + s_begin;
		const uint32_t n = c->fr.slots * spp_i;
		// packet form of the depth-0 connection wave: where the packet traversal can run (float node table, trees within its stack),
		// a wave's shadow rays are neighbours (sample groups of >= 8) and the batch's slots leave room for the light's bin
		p.fr.shadow_bins = 0u;
		if (c->integrator == 1 && connect && (c->shadow_packets > 0 || (c->shadow_packets < 0 && c->shadow_packets_auto_on)) && (p.refill & 8u) &&
			sgroup_log2 >= 3u && !side)
			for (uint32_t b = rt::SHADOW_BIN_BITS; b >= 1u && !p.fr.shadow_bins; b--) // (as many bin bits as the batch's slots leave room for)
				if ((unsigned long long)n <= (1ull << rt::shadow_slot_bits(b)))
					p.fr.shadow_bins = b;
		// flags of the 64-slot groups the packet form of the primary wave finishes (this slice's own bytes: slices begin anywhere)
		p.wv.hit0_done = c->integrator == 1 && c->group_flags && rtk::primary_packet_form(p, n) && (size_t)i < HIT0_DONE_PAD / 2
							 ? c->d_hit0_done.as<unsigned char>() + (off >> 6) + (size_t)i
							 : nullptr;
		rtk::launch_init_counters(p.wv.counters, n, s);
		uint32_t queue = 0; // every traversal launch pulls from its own chunk queue
		bool conn_now = false;
		bool sp_side_pending = false; // k_shadow_packet of this sub-batch runs on its connection stream and nobody has waited for it yet
		if (c->integrator == 0)
		{
			p.depth = 0, p.group = row_group, p.queue = queue++;
			StageTimer te(c, KF_EXTEND, 0, s);
			rtk::launch_extend(p, rtk::GEN_PARITY, count, n, s);
			te.stop();
			p.queue = queue++;
			StageTimer ts(c, KF_SHADE, -1, s);
			rtk::launch_shade_parity(p, count, n, s);
			ts.stop();
		}
		else
		{
			rtk::Params pa = p; // fused: the connection wave of the previous depth, launched together with this depth's extension wave
			bool pa_pending = false;
			for (int d = 0; d <= c->max_depth; d++)
			{
				p.depth = (uint32_t)d;
				p.group = d == 0 ? row_group : 16u;
				p.queue = queue++;
				// shadow-ray buffers of this depth's parity: shade(d) writes them, connect(d) reads them
				p.wv.sh_org = c->d_sh_org[d & 1].as<f4>() + off, p.wv.sh_dir = c->d_sh_dir[d & 1].as<f4>() + off;
				p.wv.sh_rad = c->d_sh_rad[d & 1].as<f4>() + off;
				StageTimer te(c, KF_EXTEND, d, s);
				// (grid sizes of the deeper launches: from the paths EXPECTED there, not from the primary count — depth_items)
				const uint32_t n_ext = depth_items(c, n, d, false), n_shade = depth_items(c, n, d, true);
				te.fused = pa_pending;
				if (pa_pending && sp_side_pending) // (the depth-0 connection wave on the side stream zeroes slots this launch's shadow rays add into)
				{
					RF_TRY(dm::stream_wait_event(s, c->ev_conn[i][0]));
					sp_side_pending = false;
				}
				if (pa_pending)
					rtk::launch_trace_fused(p, pa, count, n_ext, s); // extension rays of depth d + shadow rays of depth d - 1
				else if (d == 0 && c->adaptive_live)
					rtk::launch_extend_masked(p, ad.mask, count, n, s, ordered);
				else
					rtk::launch_extend(p, d == 0 ? rtk::GEN_PT : rtk::GEN_BUFFER, count, d == 0 ? n : n_ext, s, d == 0 ? ordered : nullptr);
				if (d == 0 && ordered)
					c->order_pub.read_by(i);
				if (d == 0 && entry)
					c->entry_pub.read_by(i);
				pa_pending = false;
				te.stop();
				if (side && d >= 2 && d < c->max_depth) // connect(d - 2) read the buffers shade(d) is about to write
					RF_TRY(dm::stream_wait_event(s, c->ev_conn[i][d - 2]));
				StageTimer ts(c, KF_SHADE, -1, s);
				if (material_maps_on(c)) // (k_shade_pt_maps<SKY, LT>)
					rtk::launch_shade_pt_maps(p, c->sky_view, c->lt_view, c->light_sampling != 0, n_shade, s);
				else if (c->light_sampling) // (linear | tree: k_shade_pt_lt; the view's nodes are null in linear)
					rtk::launch_shade_pt_lt(p, c->sky_view, c->lt_view, n_shade, s);
				else
					rtk::launch_shade_pt(p, c->sky_view, n_shade, s);
				ts.stop();
				// The one place where a path's light depends on other pixels: the connections of depth d are traced only when some path
				// of the sub-batch went on to depth d + 1 (connection_count: the reference's host loop).  A frame always has such a
				// path; the few active tiles of an adaptive call may not, so the call says so itself (adaptive.h)
				if (c->adaptive_live && connect && d < c->max_depth)
					rtk::launch_adaptive_connections(p.wv.counters, (uint32_t)d, s);
				// The connection wave of depth d runs beside extend / shade of depth d + 1 on its own stream (it adds into
				// rad_nee, they into rad).  The connections of the last shade call are never traced
				// (CUDART/src/Context.cpp:109-120): the shade kernel does not emit them, and no wave is launched for them.
				if (connect && d < c->max_depth)
				{
					if (d == 0 && p.fr.shadow_bins)
					{
						// the connections of the primary vertices, sorted by light, as packets (their own launch: the extension wave of
						// depth 1 then runs without them)
						p.group = 16u, p.queue = queue++;
						void *const sp_stream = c->shadow_side ? c->conn_stream[i] : s;
						if (c->shadow_side)
						{
							// beside the extension wave of depth 1, on the sub-batch's connection stream; the connection wave of depth 1
							// (which adds into the slots this one zeroes) waits for it below
							RF_TRY(dm::event_record(c->ev_shade[i][0], s));
							RF_TRY(dm::stream_wait_event(sp_stream, c->ev_shade[i][0]));
						}
						StageTimer tc(c, KF_CONNECT, -1, sp_stream);
						rtk::launch_shadow_packets(p, count, depth_items(c, n, 1, false), sp_stream);
						tc.stop();
						if (c->shadow_side)
						{
							RF_TRY(dm::event_record(c->ev_conn[i][0], sp_stream));
							sp_side_pending = true;
						}
						continue;
					}
					if (fused)
					{
						pa = p, pa.group = 16u, pa.queue = queue++;
						pa_pending = true; // (d < max_depth: the next depth's extension wave takes it along)
						continue;
					}
					if (side)
					{
						RF_TRY(dm::event_record(c->ev_shade[i][d], s));
						RF_TRY(dm::stream_wait_event(sc, c->ev_shade[i][d]));
					}
					if (sp_side_pending) // (not fused: the depth-0 connection wave on the side stream zeroes slots this wave adds into,
					{					 // and reads the parity-0 shadow buffers shade(d + 1) rewrites; extend / shade of depth 1 overlap it)
						RF_TRY(dm::stream_wait_event(s, c->ev_conn[i][0]));
						sp_side_pending = false;
					}
					p.group = 16u, p.queue = queue++;
					StageTimer tc(c, KF_CONNECT, -1, sc);
					rtk::launch_connect(p, count, depth_items(c, n, d + 1, false), sc);
					tc.stop();
					if (side)
					{
						RF_TRY(dm::event_record(c->ev_conn[i][d], sc));
						conn_now = true;
					}
				}
			}
		}
		if (sp_side_pending) // (nothing deeper waited for it: the sub-batch is done when it is)
			RF_TRY(dm::stream_wait_event(s, c->ev_conn[i][0]));
		RF_TRY(dm::event_record(c->ev_sub_done[i], s));
		if (conn_now)
			RF_TRY(dm::event_record(c->ev_conn_last[i], sc));
		c->conn_used[i] = conn_now;
	}
	// ---- epilogue on the main stream: one resolve over every sample of the call ----
	for (int i = first_slot; i < first_slot + subs; i++)
	{
		RF_TRY(dm::stream_wait_event(s0, c->ev_sub_done[i]));
		if (c->conn_used[i])
			RF_TRY(dm::stream_wait_event(s0, c->ev_conn_last[i]));
	}
	{
		StageTimer tf(c, KF_FINALIZE, -1);
		if (c->adaptive_live)
			rtk::launch_resolve_adaptive(base, c->d_noise.as<float>(), ad, s0);
		else if (c->noise_live)
			rtk::launch_resolve_noise(base, c->d_noise.as<float>(), c->samples_done, s0);
		else
			rtk::launch_resolve(base, s0);
		tf.stop();
	}
	RF_TRY(dm::event_record(c->ev_resolve[par], s0));
	if (c->adaptive_live)
	{
		// the tiles' counts go on; after every adaptive_every-th call the metric at those counts decides which tiles retire.  Only
		// then does the mask move: the next primary waves wait for the record behind it, and on other calls for nothing
		const bool decide = ++c->adaptive_calls % (uint32_t)c->adaptive_every == 0u;
		rtk::launch_adaptive_step(ad, (uint32_t)c->spp, false, s0);
		if (decide)
		{
			StageTimer tn(c, KF_NOISE, -1);
			rtk::launch_noise_metric_adaptive(noise_view(c, c->d_noise.as<float>(), c->W, c->H, c->fr.local_rows, (uint32_t)c->rank, (uint32_t)c->world, 2u), ad.n_tile, false, s0);
			tn.stop();
			rtk::launch_adaptive_step(ad, 0u, true, s0);
			RF_TRY(c->adaptive_pub.publish(s0));
		}
	}
	c->resolve_recorded[par] = true;
	c->call_slot = (par + 1u) % (uint32_t)ring;
	RF_TRY(dm::last_launch_error());
	c->subs_last = subs, c->subs_first = first_slot;
	c->last_wave_off = alternate ? (paths + pad) * par : 0;
	c->samples_done += (uint32_t)c->spp;
	c->samples_total += (uint64_t)c->spp, c->frame_serial++;
	c->totals.samples += (uint64_t)c->W * c->H * (uint64_t)c->spp / (uint64_t)c->world;
	c->last_cam = *cam, c->have_last_cam = true; // (the denoiser's guide pass traces this camera's centre rays)
	return RFWHIP_OK;
}

extern "C" int rfwhip_wait(rfwhip_context *c)
{
	CTX_ENTER(c);
	// every render call ends with its resolve on the main stream, behind the events of all its sub-batch and connection
	// streams: the main stream alone tells when the enqueued frames are done (one synchronisation instead of up to 17)
	RF_TRY(dm::sync(c->stream));
	RF_TRY(c->marks[MK_PRESENT].sync());
	if (c->stage_timing) // (the denoiser's timed spans on a gather stream are read below)
		RF_TRY(c->marks[MK_DENOISE].sync());
	// wave counters of the last frame, summed over its sub-batches.  A sub-batch's connection wave of depth d ran only
	// if its depth d + 1 had extension rays (k_connect / k_trace_stream: connection_count)
	rt::WaveCounters wc;
	RF_TRY(dm::d2h(&wc, c->subs_first == 0 ? c->d_counters.p : c->d_counters_sub[c->subs_first].p, sizeof(wc), c->stream));
	uint32_t stack_overflow = wc.stack_overflow;
	const rt::WaveCounters wc0 = wc; // (as read: the sums below fold the other sub-batches' counts into wc)
	std::vector<rt::WaveCounters> more;
	// (adaptive sampling: "one path went on" written by k_adaptive_connections, adaptive.h, is no ray — its queue is empty)
	uint32_t ext_marks[rt::MAX_DEPTH_SLOTS] = {};
	auto count_marks = [&](const rt::WaveCounters &w) {
		for (int d = 1; d < rt::MAX_DEPTH_SLOTS; d++)
			ext_marks[d] += c->adaptive_live && w.ext[d] == 1u && w.ext_n[d] == 0u;
	};
	count_marks(wc);
	for (int d = 0; d + 1 < rt::MAX_DEPTH_SLOTS; d++)
		if (!wc.ext[d + 1])
			wc.shadow[d] = 0;
	for (int i = c->subs_first + 1; i < c->subs_first + c->subs_last; i++)
	{
		rt::WaveCounters w2;
		RF_TRY(dm::d2h(&w2, c->d_counters_sub[i].p, sizeof(w2), c->stream));
		more.push_back(w2);
		count_marks(w2);
		stack_overflow += w2.stack_overflow;
		for (int d = 0; d < rt::MAX_DEPTH_SLOTS; d++)
		{
			wc.ext[d] += w2.ext[d];
			if (d + 1 < rt::MAX_DEPTH_SLOTS && w2.ext[d + 1])
				wc.shadow[d] += w2.shadow[d];
		}
	}
	for (int d = 1; d < rt::MAX_DEPTH_SLOTS; d++)
		wc.ext[d] -= ext_marks[d];
	// k_trace_fused: the shadow rays' share of each depth's launch, from the workgroups' tick sums since the last wait (over the
	// counter sets of the last frame's sub-batches: the frames of a pipelined series render the same scene)
	double shadow_share[rt::MAX_DEPTH_SLOTS];
	{
		unsigned long long sums[rt::MAX_DEPTH_SLOTS][2] = {};
		auto fold = [&](int slot, const rt::WaveCounters &w) {
			for (int d = 0; d < rt::MAX_DEPTH_SLOTS; d++)
				for (int k = 0; k < 2; k++)
				{
					sums[d][k] += w.fused_ticks[d][k] - c->fused_ticks_at_wait[slot][d][k];
					c->fused_ticks_at_wait[slot][d][k] = w.fused_ticks[d][k];
				}
		};
		fold(c->subs_first, wc0);
		for (size_t k = 0; k < more.size(); k++)
			fold(c->subs_first + 1 + (int)k, more[k]);
		// k_shadow_packet: light bins per sorted run of the frames since the last wait.  Many bins per run = the first vertices of
		// neighbouring pixels do not agree about their lights: packets of 64 then mix many directions.  Measured: terrain 3.6 bins per
		// run, + 8 %; atrium (an interior lit from all sides) 5.5, + 0.6 %; the threshold, half of the 16 bins, is beyond what was measured
		unsigned long long runs = 0, bins = 0;
		auto fold_sp = [&](int slot, const rt::WaveCounters &w) {
			runs += w.sp_runs - c->sp_at_wait[slot][0], bins += w.sp_bins - c->sp_at_wait[slot][1];
			c->sp_at_wait[slot][0] = w.sp_runs, c->sp_at_wait[slot][1] = w.sp_bins;
		};
		fold_sp(c->subs_first, wc0);
		for (size_t k = 0; k < more.size(); k++)
			fold_sp(c->subs_first + 1 + (int)k, more[k]);
		if (runs)
		{
			c->shadow_bins_per_run = (double)bins / (double)runs;
			c->shadow_packets_auto_on = c->shadow_bins_per_run <= SHADOW_PACKET_MAX_BINS_PER_RUN;
		}
		for (int d = 0; d < rt::MAX_DEPTH_SLOTS; d++)
		{
			const double tot = (double)sums[d][0] + (double)sums[d][1];
			shadow_share[d] = tot > 0.0 ? (double)sums[d][1] / tot : 0.5;
		}
	}
	if (wc.probe_valid)
		c->probe_inst = wc.probe_inst, c->probe_prim = wc.probe_prim, c->probe_dist = wc.probe_dist;
	rfwhip_render_stats &st = c->stats;
	c->depth_stats_valid = true;
	const float anim = st.animationTime;
	memset(&st, 0, sizeof(st));
	st.animationTime = anim;
	{
		// ext[0] counts path slots (8x8 tiles, padded at the image border); primary RAYS exist for real pixels only
		uint32_t owned_rows = 0;
		for (uint32_t y = 0; y < c->H; y++)
			owned_rows += rt::strip_owner(y / rt::STRIP_ROWS, (uint32_t)c->world) == (uint32_t)c->rank;
		const uint32_t samples = c->fr.slots ? wc.ext[0] / c->fr.slots : 0u;
		st.primaryCount = owned_rows * c->W * samples;
	}
	st.secondaryCount = wc.ext[1];
	for (int d = 2; d < rt::MAX_DEPTH_SLOTS; d++)
		st.deepCount += wc.ext[d];
	for (int d = 0; d < rt::MAX_DEPTH_SLOTS; d++)
		st.shadowCount += wc.shadow[d];
	for (const TimedSpan &sp : c->spans)
	{
		float ms = dm::event_ms(sp.a, sp.b);
		if (sp.fused && sp.depth >= 0 && sp.depth < rt::MAX_DEPTH_SLOTS)
		{
			// (one launch, two stages: the shadow rays' share goes where a host of the reference looks for it — shadowTime, context.h:63)
			const float shadow_ms = ms * (float)shadow_share[sp.depth];
			st.shadowTime += shadow_ms, c->kernel_ms[KF_CONNECT] += shadow_ms;
			ms -= shadow_ms;
		}
		c->kernel_ms[sp.family] += ms;
		switch (sp.family)
		{
		case KF_EXTEND:
			if (sp.depth == 0)
				st.primaryTime += ms;
			else if (sp.depth == 1)
				st.secondaryTime += ms;
			else
				st.deepTime += ms;
			break;
		case KF_GENERATE:
			st.primaryTime += ms;
			break;
		case KF_SHADE:
			st.shadeTime += ms;
			break;
		case KF_CONNECT:
			st.shadowTime += ms;
			break;
		case KF_FINALIZE:
			st.finalizeTime += ms;
			break;
		default:
			if (KindTimes *kt = c->kind_times(sp.family)) // (the span's depth is the kernel's index in its family)
				if (sp.depth >= 0 && sp.depth < kt->count)
					kt->add(sp.depth, ms);
			break;
		}
	}
	c->spans.clear();
	c->events_used = 0;
	if (c->render_in_flight)
	{
		st.renderTime = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - c->render_t0).count();
		c->render_in_flight = false;
	}
	// (reported last: the bookkeeping above is complete, so the context stays usable after the error)
	if (stack_overflow)
		return set_error(RFWHIP_ERR_STATE, "traversal stack overflow: %u entries dropped in the last frame (the image is wrong)", stack_overflow);
	return RFWHIP_OK;
}

// =================================================================================================================
// present
// =================================================================================================================
extern "C" uint32_t rfwhip_local_rows(const rfwhip_context *c) { return c ? local_rows_of(c) : 0u; }

static int present(rfwhip_context *c, f4 *dst_device, int full)
{
	rtk::Params p;
	fill_params(c, nullptr, p);
	const float scale = c->samples_done ? 1.0f / (float)c->samples_done : 0.0f;
	if (c->adaptive_live) // (a tile's pixels hold n_tile samples)
		rtk::launch_present_adaptive(p, dst_device, adaptive_view(c), full, c->stream);
	else
		rtk::launch_present(p, dst_device, scale, full, c->stream);
	RF_TRY(dm::last_launch_error());
	return 0;
}

// ---- denoiser of the presented image (setting "denoise"; work items: denoise.h) -------------------------------------------------
static int dn_ensure(rfwhip_context *c)
{
	const size_t px = (size_t)c->W * c->H;
	RF_TRY(c->d_dn_guides.ensure_exact(2 * px * sizeof(f4) + sizeof(f4))); // (+ the guide pass's stack-overflow counter)
	RF_TRY(c->d_dn_img.ensure_exact(2 * px * sizeof(f4)));
	RF_TRY(c->d_dn_var.ensure_exact(2 * px * sizeof(float)));
	if (c->dn_temporal)
	{
		RF_TRY(c->d_dn_prev.ensure_exact(px * sizeof(f4)));
		RF_TRY(c->d_dn_ids.ensure_exact(2 * px * sizeof(uint32_t)));
		RF_TRY(c->d_dn_hist.ensure_exact(2 * px * (sizeof(f4) + 3 * sizeof(float))));
		if (c->dn_motion)
			RF_TRY(c->d_dn_surf.ensure_exact(px * sizeof(f4)));
	}
	return 0;
}

// per instance: the scene version of the update that last changed it (the temporal stage's instance test).  Uploaded on the
// stage's stream in front of it whenever the device copy is missing or stale, so the kernel never reads a table that is not there
// (the host copy changes only in rfwhip_update, after sync_all: no stage in flight still reads the device copy)
static int dn_inst_ver_current(rfwhip_context *c, void *stream)
{
	if (!c->dn_inst_ver_stale && c->d_dn_inst_ver.p)
		return 0;
	const size_t n = c->dn_inst_ver.size();
	RF_TRY(c->d_dn_inst_ver.ensure(std::max<size_t>(n, 1) * sizeof(uint32_t)));
	RF_TRY(dm::h2d(c->d_dn_inst_ver.p, c->dn_inst_ver.data(), n * sizeof(uint32_t), stream));
	c->dn_inst_ver_stale = false;
	return 0;
}

static rtk::DnView dn_view(rfwhip_context *c, f4 *in, f4 *out)
{
	rtk::DnView d;
	const size_t px = (size_t)c->W * c->H;
	d.W = c->W, d.H = c->H;
	d.ga = c->d_dn_guides.as<f4>(), d.gb = d.ga + px;
	d.in = in, d.out = out;
	d.img[0] = c->d_dn_img.as<f4>(), d.img[1] = d.img[0] + px;
	d.var[0] = c->d_dn_var.as<float>(), d.var[1] = d.var[0] + px;
	d.sigma_l = c->dn_sigma_l, d.sigma_n = c->dn_sigma_n, d.sigma_z = c->dn_sigma_z;
	d.iterations = (uint32_t)c->dn_iterations;
	d.overflow = (uint32_t *)(d.gb + px);
	d.id = c->dn_temporal ? c->d_dn_ids.as<uint32_t>() : nullptr;
	d.hist = nullptr;
	return d;
}

// the temporal stage's view: F = the last render, P = the stage record of the last presented frame; history set rd -> wr
static rtk::DnTemporal dn_temporal_view(rfwhip_context *c, const rtk::Params &p, int rd, int wr)
{
	rtk::DnTemporal t;
	const size_t px = (size_t)c->W * c->H;
	t.cam = p.cam, t.pcam = c->dn_t_pcam, t.fr = p.fr;
	t.pgb = c->d_dn_prev.as<f4>();
	t.id = c->d_dn_ids.as<uint32_t>(), t.pid = t.id + px;
	t.inst_ver = c->d_dn_inst_ver.as<uint32_t>(), t.n_inst = (uint32_t)c->dn_inst_ver.size(), t.pscene = c->dn_t_pscene;
	float *const mom = (float *)(c->d_dn_hist.as<f4>() + 2 * px), *const n = mom + 4 * px;
	t.col_in = c->d_dn_hist.as<f4>() + (size_t)rd * px;
	t.mom_in = mom + (size_t)rd * 2 * px, t.n_in = n + (size_t)rd * px;
	t.mom_out = mom + (size_t)wr * 2 * px, t.n_out = n + (size_t)wr * px;
	t.alpha = c->dn_alpha, t.usable = c->dn_t_usable ? 1u : 0u;
	return t;
}
static f4 *dn_hist_colour(rfwhip_context *c, int set) { return c->d_dn_hist.as<f4>() + (size_t)set * c->W * c->H; }

// P's guides (normal | z | gradient) and instance ids are kept before anything overwrites them for a new frame: only while a frame
// rendered after P waits to be presented (a guide pass for P itself — after an rfwhip_update — is not P's history)
static int dn_save_prev(rfwhip_context *c, void *stream)
{
	if (!c->dn_have_pres || !c->dn_guides_pres || c->frame_serial == c->dn_pres_serial ||
		(c->dn_prev_ok && c->dn_saved_serial == c->dn_pres_serial))
		return 0;
	const size_t px = (size_t)c->W * c->H;
	RF_TRY(dm::d2d(c->d_dn_prev.p, c->d_dn_guides.as<f4>() + px, px * sizeof(f4), stream));
	RF_TRY(dm::d2d(c->d_dn_ids.as<uint32_t>() + px, c->d_dn_ids.p, px * sizeof(uint32_t), stream));
	c->dn_prev_ok = true, c->dn_saved_serial = c->dn_pres_serial;
	return 0;
}

// the guides of the full image for the camera of the last render, unless they are current (camera by value, scene, size)
static int dn_guides(rfwhip_context *c, void *stream)
{
	if (!c->have_last_cam)
		return set_error(RFWHIP_ERR_STATE, "denoise: no frame has been rendered (the guides need the camera of a render)");
	RF_TRY(dn_ensure(c));
	// (current guides belong to the scene of the last rfwhip_update — the one the image was rendered with — even while set_* calls
	// since then wait for the next update)
	if (c->guides_valid && c->guide_scene == c->scene_version && c->guide_W == c->W && c->guide_H == c->H &&
		!memcmp(&c->guide_cam, &c->last_cam, sizeof(rfwhip_camera)))
		return 0;
	if (c->scene_dirty)
		return set_error(RFWHIP_ERR_STATE, "denoise: the guides must be traced, but the scene changed since the last rfwhip_update()");
	if (c->dn_temporal)
		RF_TRY(dn_save_prev(c, stream));
	rtk::Params p;
	fill_params(c, &c->last_cam, p);
	const rtk::DnView d = dn_view(c, nullptr, nullptr);
	RF_TRY(dm::zero(d.overflow, sizeof(uint32_t), stream));
	StageTimer t(c, KF_DENOISE, -1, stream);
	const bool motion = c->dn_temporal && c->dn_motion;
	rtk::launch_denoise_guides(p, d, motion ? c->d_dn_surf.as<f4>() : nullptr, stream, c->material_maps && c->mask_present);
	t.stop(2);
	RF_TRY(dm::last_launch_error());
	c->dn_g_rec_ok = motion;
	if (motion)
	{
		// what this pass traced (no set_* call is pending: scene_dirty is false here)
		c->dn_g_rec.assign(c->instances.size(), DnInstSnap());
		for (size_t i = 0; i < c->instances.size(); i++)
		{
			const InstRec &in = c->instances[i];
			DnInstSnap &r = c->dn_g_rec[i];
			if (!in.used || in.mesh >= c->meshes.size())
				continue;
			r.used = true, r.mesh = in.mesh, r.generation = c->meshes[in.mesh].generation, r.edits = c->meshes[in.mesh].edits;
			memcpy(r.transform, in.transform, sizeof(r.transform));
		}
		for (auto &m : c->meshes)
			m.dn_g_edits = m.edits;
	}
	c->guides_valid = true, c->guide_cam = c->last_cam, c->guide_scene = c->scene_version, c->guide_W = c->W, c->guide_H = c->H;
	c->dn_guides_pres = false;
	return 0;
}

// the guide pass's traversal-stack overflow counter (synchronises the context's stream)
static int dn_check_overflow(rfwhip_context *c)
{
	uint32_t n = 0;
	RF_TRY(dm::d2h(&n, dn_view(c, nullptr, nullptr).overflow, sizeof(n), c->stream));
	if (n)
		return set_error(RFWHIP_ERR_STATE, "denoise: traversal stack overflow in the guide pass: %u entries dropped (the guides are wrong)", n);
	return 0;
}

// "denoise_motion": the stage's per-instance table.  For a new presented frame F it is built from P's record and the record of F's
// guide pass, and kept; a further read of F uses it again while no rfwhip_update and no mesh edit followed — after one, the
// current vertices and the snapshots may be another frame's, and every instance that is not STILL restarts.
static void dn_rows(const float *M, float *rows) // column-major 4 x 4 -> rows 0..2, row-major 3 x 4
{
	for (int r = 0; r < 3; r++)
		for (int k = 0; k < 4; k++)
			rows[4 * r + k] = M[4 * k + r];
}
static int dn_motion_view(rfwhip_context *c, bool new_frame, void *stream, rtk::DnMotion &mv)
{
	const size_t n = c->dn_inst_ver.size();
	if (new_frame)
	{
		c->dn_mtab.assign(n, rtk::DnMotionInst{});
		for (size_t i = 0; i < n; i++)
		{
			rtk::DnMotionInst &e = c->dn_mtab[i];
			e.state = rtk::DN_M_RESTART;
			if (c->dn_inst_ver[i] <= c->dn_t_pscene)
			{
				e.state = rtk::DN_M_STILL;
				continue;
			}
			if (!c->dn_t_usable || !c->dn_p_rec_ok || !c->dn_g_rec_ok || i >= c->dn_p_rec.size() || i >= c->dn_g_rec.size())
				continue;
			const DnInstSnap &P = c->dn_p_rec[i], &G = c->dn_g_rec[i];
			if (!P.used || !G.used || P.mesh != G.mesh || P.generation != G.generation || G.mesh >= c->meshes.size())
				continue;
			const MeshRec &m = c->meshes[G.mesh];
			// the current vertices must be the ones F's guide pass traced, and P's either the same or the snapshot taken of P
			if (!m.used || !m.d_verts.p || m.generation != G.generation || m.edits != G.edits)
				continue;
			const f4 *prev = nullptr;
			if (P.edits == G.edits)
				prev = m.d_verts.as<f4>();
			else if (m.dn_snap_pres == c->dn_pres_id && m.d_dn_snap.p)
				prev = m.d_dn_snap.as<f4>();
			if (!prev)
				continue;
			e.state = rtk::DN_M_MOVED;
			dn_rows(P.transform, e.mp), dn_rows(G.transform, e.mf);
			e.cur = m.d_verts.as<f4>(), e.prev = prev;
			e.indices = m.indexed ? m.d_indices.as<uint32_t>() : nullptr;
			e.tri_count = (uint32_t)m.triCount, e.vert_count = (uint32_t)m.vertexCount;
		}
		c->dn_mtab_scene = (uint32_t)c->scene_version, c->dn_mtab_edits = c->dn_edit_count, c->dn_mtab_stale = true;
	}
	else if (c->dn_mtab.size() != n || c->dn_mtab_scene != (uint32_t)c->scene_version || c->dn_mtab_edits != c->dn_edit_count)
	{
		c->dn_mtab.assign(n, rtk::DnMotionInst{});
		for (size_t i = 0; i < n; i++)
			c->dn_mtab[i].state = c->dn_inst_ver[i] <= c->dn_t_pscene ? rtk::DN_M_STILL : rtk::DN_M_RESTART;
		c->dn_mtab_scene = (uint32_t)c->scene_version, c->dn_mtab_edits = c->dn_edit_count, c->dn_mtab_stale = true;
	}
	if (c->dn_mtab_stale || !c->d_dn_minst.p)
	{
		RF_TRY(c->d_dn_minst.ensure(std::max<size_t>(n, 1) * sizeof(rtk::DnMotionInst)));
		RF_TRY(dm::h2d(c->d_dn_minst.p, c->dn_mtab.data(), n * sizeof(rtk::DnMotionInst), stream));
		c->dn_mtab_stale = false;
	}
	mv.inst = c->d_dn_minst.as<rtk::DnMotionInst>(), mv.surf = c->d_dn_surf.as<f4>(), mv.dump = nullptr;
	return 0;
}

// filter the full image `in` (W x H float4 on this context's device) into `out` (may be `in`), enqueued on `stream`.  `presented`:
// the image of the last render handed out (world-1 read, group / comm gather): the temporal stage runs when it is on — once per
// frame with a new history set; a further read of the same frame runs it again from the same history into the same set
static int dn_filter(rfwhip_context *c, f4 *in, f4 *out, void *stream, bool presented)
{
	if (!presented || !c->dn_temporal)
	{
		RF_TRY(dn_guides(c, stream));
		StageTimer t(c, KF_DENOISE, -1, stream);
		rtk::launch_denoise_filter(dn_view(c, in, out), nullptr, nullptr, stream);
		t.stop(1 + c->dn_iterations);
		return dm::last_launch_error();
	}
	RF_TRY(dn_ensure(c));
	const bool new_frame = !c->dn_have_pres || c->frame_serial != c->dn_pres_serial;
	if (new_frame)
		RF_TRY(dn_save_prev(c, stream)); // (before the guide pass of F may overwrite P's guides)
	RF_TRY(dn_guides(c, stream));
	rtk::Params p;
	fill_params(c, &c->last_cam, p);
	if (new_frame)
	{
		// the history is usable after a RESET since P, at P's size, with P's guides kept
		c->dn_t_usable = c->dn_have_pres && c->dn_prev_ok && c->dn_saved_serial == c->dn_pres_serial && c->dn_reset_since &&
						 c->dn_pres_W == c->W && c->dn_pres_H == c->H;
		c->dn_t_pcam = c->dn_pres_cam, c->dn_t_pscene = c->dn_pres_scene;
	}
	const int rd = new_frame ? c->dn_hist_cur : c->dn_hist_cur ^ 1, wr = rd ^ 1;
	RF_TRY(dn_inst_ver_current(c, stream));
	rtk::DnView d = dn_view(c, in, out);
	d.hist = dn_hist_colour(c, wr);
	const rtk::DnTemporal tv = dn_temporal_view(c, p, rd, wr);
	rtk::DnMotion mv;
	const bool motion = c->dn_motion != 0;
	if (motion)
		RF_TRY(dn_motion_view(c, new_frame, stream, mv));
	StageTimer t(c, KF_DENOISE, -1, stream);
	rtk::launch_denoise_filter(d, &tv, motion ? &mv : nullptr, stream);
	t.stop(2 + c->dn_iterations);
	RF_TRY(dm::last_launch_error());
	if (new_frame)
	{
		if (motion)
		{
			// F becomes P: its guide pass's instances, and per mesh the edit count that pass traced
			c->dn_p_rec = c->dn_g_rec, c->dn_p_rec_ok = c->dn_g_rec_ok;
			for (auto &m : c->meshes)
				m.dn_p_edits = m.dn_g_edits;
		}
		c->dn_pres_id++;
		c->dn_hist_cur = wr, c->dn_have_pres = true, c->dn_pres_serial = c->frame_serial;
		c->dn_pres_cam = p.cam, c->dn_pres_scene = (uint32_t)c->guide_scene, c->dn_pres_W = c->W, c->dn_pres_H = c->H;
		c->dn_guides_pres = true, c->dn_reset_since = false;
	}
	return 0;
}

// the root's side of a group / comm gather (rfwhip_group.cpp): the full image on `hip_stream`, in place, when denoise is on
int rfwhip_internal_denoise_stream(rfwhip_context *c, void *rgba_device, void *hip_stream)
{
	CTX_ENTER(c);
	if (!c->denoise || !c->have_last_cam) // (nothing rendered yet: the accumulator is empty)
		return RFWHIP_OK;
	RF_TRY(ensure_sub_batches(c, 1));
	RF_TRY(dn_filter(c, (f4 *)rgba_device, (f4 *)rgba_device, hip_stream, true));
	return c->marks[MK_DENOISE].record(hip_stream, true);
}

extern "C" int rfwhip_read_framebuffer_device(rfwhip_context *c, void *rgba_device)
{
	CTX_ENTER(c);
	if (!rgba_device)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "null destination");
	if (c->world != 1)
		return set_error(RFWHIP_ERR_STATE, "rfwhip_read_framebuffer*: this rank owns 1/%d of the image; gather local "
											"framebuffers and call rfwhip_deinterleave_device", c->world);
	if (!c->W)
		return set_error(RFWHIP_ERR_STATE, "no render target");
	RF_TRY(present(c, (f4 *)rgba_device, 1));
	if (c->denoise && c->have_last_cam) // (before the first render the accumulator is empty: nothing to filter, no camera to trace)
	{
		RF_TRY(dn_filter(c, (f4 *)rgba_device, (f4 *)rgba_device, c->stream, true));
		RF_TRY(dn_check_overflow(c));
	}
	return dm::sync(c->stream);
}

extern "C" int rfwhip_read_framebuffer(rfwhip_context *c, float *rgba_host)
{
	CTX_ENTER(c);
	if (!rgba_host)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "null destination");
	const size_t bytes = (size_t)c->W * c->H * sizeof(f4);
	RF_TRY(c->d_present.ensure(bytes));
	RF_TRY(dm::zero(c->d_present.p, bytes, c->stream));
	RF_TRY(rfwhip_read_framebuffer_device(c, c->d_present.p));
	return dm::d2h(rgba_host, c->d_present.p, bytes, c->stream);
}

// ---- display stage (settings "display_*"; work item: display.h) -----------------------------------------------------------------
static size_t display_pixel_bytes(int format) { return format == RFWHIP_DISPLAY_RGBA8 ? 4u : sizeof(f4); }
static int display_check_format(const char *who, int format)
{
	if (format != RFWHIP_DISPLAY_RGBA8 && format != RFWHIP_DISPLAY_RGBA32F)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s: unknown display format %d", who, format);
	return RFWHIP_OK;
}
// ---- exposure meter (settings "display_exposure*"; work items: metering.h) ------------------------------------------------------
static_assert(sizeof(rfwhip_meter_stats) == sizeof(rtk::MeterRecord) && sizeof(rtk::MeterRecord) == 32, "rfwhip.h: the meter's record is the kernels' (kernels.h)");
static_assert(RFWHIP_METER_BINS == (int)rtk::MT_BINS, "rfwhip.h restates the histogram's size");
static const rtk::MeterRecord k_meter_fresh = {1.0f, 0.0f, 0.0f, 0.0f, 0u, 0u, 0u, 0u}; // before any step: E = 1, steps = 0
// the record and the summed histogram (a fresh record the first time) and room for the partial records of `pixels` pixels
static int meter_ensure(rfwhip_context *c, size_t pixels)
{
	if (!c->d_meter_rec.p)
	{
		RF_TRY(c->d_meter_rec.ensure(sizeof(rtk::MeterRecord)));
		RF_TRY(c->d_meter_hist.ensure(rtk::MT_RECORD * sizeof(uint32_t)));
		RF_TRY(dm::h2d(c->d_meter_rec.p, &k_meter_fresh, sizeof(k_meter_fresh), c->stream));
		RF_TRY(dm::zero(c->d_meter_hist.p, rtk::MT_RECORD * sizeof(uint32_t), c->stream));
		RF_TRY(dm::sync(c->stream));
		c->meter_manual_stale = true;
	}
	const size_t need = (size_t)std::max(1u, rtk::meter_records((uint32_t)pixels)) * rtk::MT_RECORD * sizeof(uint32_t);
	if (need > c->d_meter_part.cap)
	{
		RF_TRY(sync_all(c)); // (a step in flight writes the records this reallocates)
		RF_TRY(c->d_meter_part.ensure(need));
	}
	return 0;
}
static rtk::MeterParams meter_params(const rfwhip_context *c)
{
	rtk::MeterParams m;
	m.low = (double)c->exposure_low, m.high = (double)c->exposure_high;
	m.log2_key = (float)log2((double)c->exposure_key);
	m.ev = c->exposure_ev, m.ev_min = c->exposure_min_ev, m.ev_max = c->exposure_max_ev, m.speed = c->exposure_speed, m.pad = 0u;
	return m;
}
// behind work on the record enqueued on `stream`: a caller's stream is remembered by an event (rfwhip_get_meter, sync_all)
static int meter_mark(rfwhip_context *c, void *stream)
{
	return stream == c->stream ? 0 : c->marks[MK_METER].record(stream, true);
}
// the reduce on `records` partial records in d_meter_part, enqueued on `stream`
static int meter_reduce(rfwhip_context *c, uint32_t records, void *stream)
{
	StageTimer t(c, KF_METER_REDUCE, -1, stream);
	rtk::launch_meter_reduce(c->d_meter_part.as<uint32_t>(), records, c->d_meter_hist.as<uint32_t>(), meter_params(c),
							 c->d_meter_rec.as<rtk::MeterRecord>(), stream);
	t.stop(1);
	RF_TRY(dm::last_launch_error());
	c->meter_manual_stale = true; // (a step writes E)
	c->meter_have = false;		  // (... and the record is this image's: rfwhip_read_display* claims it for its frame)
	return meter_mark(c, stream);
}
// ONE STEP on the full W x H image `img`, enqueued on `stream`: two launches, nothing comes back to the host
static int meter_step(rfwhip_context *c, const f4 *img, void *stream)
{
	const size_t px = (size_t)c->W * c->H;
	RF_TRY(meter_ensure(c, px));
	rtk::MeterView v;
	v.in = img, v.pixels = (uint32_t)px, v.partial = c->d_meter_part.as<uint32_t>();
	{
		StageTimer t(c, KF_METER_HIST, -1, stream);
		rtk::launch_meter_hist(v, stream);
		t.stop(1);
	}
	RF_TRY(dm::last_launch_error());
	return meter_reduce(c, rtk::meter_records(v.pixels), stream);
}

// ---- bloom (settings "display_bloom*"; work items: bloom.h) ---------------------------------------------------------------------
constexpr uint32_t BLOOM_MAX_LEVELS = 8u;
// texels in front of level `level` (1-based) in d_bloom_pyr, and that level's size
static size_t bloom_level_offset(uint32_t W, uint32_t H, uint32_t level, uint32_t *w, uint32_t *h)
{
	size_t off = 0;
	for (uint32_t k = 1u;; k++)
	{
		W = (W + 1u) >> 1, H = (H + 1u) >> 1;
		if (k == level)
			break;
		off += (size_t)W * H;
	}
	*w = W, *h = H;
	return off;
}
// the pyramid of the target's size (all BLOOM_MAX_LEVELS levels: display_bloom_levels may change between chains), the bloomed image
// and the two floats of d_bloom_one: [0] = 1, the E of an unexposed display; [1] = the E rfwhip_bloom_image was given
static int bloom_ensure(rfwhip_context *c)
{
	if (!c->d_bloom_one.p)
	{
		static const float one[2] = {1.0f, 1.0f};
		RF_TRY(c->d_bloom_one.ensure(sizeof(one)));
		RF_TRY(dm::h2d(c->d_bloom_one.p, one, sizeof(one), c->stream));
		RF_TRY(dm::sync(c->stream));
	}
	uint32_t w, h;
	const size_t pyr = bloom_level_offset(c->W, c->H, BLOOM_MAX_LEVELS + 1u, &w, &h) * sizeof(f4), img = (size_t)c->W * c->H * sizeof(f4);
	if (pyr > c->d_bloom_pyr.cap || img > c->d_bloom_out.cap || !c->d_bloom_pyr.p || !c->d_bloom_out.p)
	{
		RF_TRY(sync_all(c)); // (a chain in flight writes the buffers this reallocates)
		RF_TRY(c->d_bloom_pyr.ensure(pyr));
		RF_TRY(c->d_bloom_out.ensure(img));
	}
	return 0;
}
// the chain on the full W x H image `in` with the exposure *E (a device float), enqueued on `stream`: d_bloom_out is the bloomed
// image, the levels stay in d_bloom_pyr as U_k.  A chain on another stream than the previous one waits for that one — and for the
// display kernel that read its image — first
static int bloom_chain(rfwhip_context *c, const f4 *in, const float *E, void *stream)
{
	RF_TRY(bloom_ensure(c));
	if (c->marks[MK_BLOOM].stream != stream)
		RF_TRY(c->marks[MK_BLOOM].wait_on(stream)); // (nothing before the first record)
	rtk::BloomParams b;
	b.intensity = c->bloom_intensity, b.threshold = c->bloom_threshold, b.knee = c->bloom_knee, b.scatter = c->bloom_scatter;
	const uint32_t n = rtk::bloom_levels(c->W, c->H, (uint32_t)c->bloom_levels);
	f4 *lv[BLOOM_MAX_LEVELS + 1];
	uint32_t w[BLOOM_MAX_LEVELS + 1], h[BLOOM_MAX_LEVELS + 1];
	lv[0] = nullptr, w[0] = c->W, h[0] = c->H;
	for (uint32_t k = 1u; k <= n; k++)
		lv[k] = c->d_bloom_pyr.as<f4>() + bloom_level_offset(c->W, c->H, k, &w[k], &h[k]);
	// (a span per launch, its `depth` the kernel: 0 down0, 1 down, 2 up, 3 apply)
	for (uint32_t k = 0u; k < n; k++)
	{
		rtk::BloomDownView v;
		v.src = k ? lv[k] : in, v.dst = lv[k + 1u], v.W = w[k], v.H = h[k], v.Wn = w[k + 1u], v.Hn = h[k + 1u], v.E = E;
		StageTimer t(c, KF_BLOOM, k ? 1 : 0, stream);
		if (k == 0u)
			rtk::launch_bloom_down0(v, b, stream);
		else
			rtk::launch_bloom_down(v, stream);
		t.stop(1);
	}
	for (uint32_t k = n - 1u; k >= 1u; k--)
	{
		rtk::BloomUpView v;
		v.level = lv[k], v.next = lv[k + 1u], v.W = w[k], v.H = h[k], v.Wn = w[k + 1u], v.Hn = h[k + 1u];
		StageTimer t(c, KF_BLOOM, 2, stream);
		rtk::launch_bloom_up(v, b, stream);
		t.stop(1);
	}
	rtk::BloomApplyView a;
	a.in = in, a.next = lv[1], a.out = c->d_bloom_out.as<f4>(), a.W = c->W, a.H = c->H, a.Wn = w[1], a.Hn = h[1];
	{
		StageTimer t(c, KF_BLOOM, 3, stream);
		rtk::launch_bloom_apply(a, b, stream);
		t.stop(1);
	}
	c->bloom_ran = n;
	return dm::last_launch_error();
}
// behind the last reader of d_bloom_out on `stream` (the main stream too: the next chain may run elsewhere; sync_all waits for the
// main stream itself)
static int bloom_mark(rfwhip_context *c, void *stream) { return c->marks[MK_BLOOM].record(stream, stream != c->stream); }

// ---- colour grading and dither (settings "display_grade*", "display_wb_temperature", "display_dither"; work items: display_grade.h) ----
static void mat3_mul(const double a[9], const double b[9], double o[9])
{
	for (int i = 0; i < 3; i++)
		for (int j = 0; j < 3; j++)
			o[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}
static void mat3_inv(const double m[9], double o[9])
{
	const double c0 = m[4] * m[8] - m[5] * m[7], c1 = m[5] * m[6] - m[3] * m[8], c2 = m[3] * m[7] - m[4] * m[6];
	const double det = m[0] * c0 + m[1] * c1 + m[2] * c2;
	o[0] = c0 / det, o[1] = (m[2] * m[7] - m[1] * m[8]) / det, o[2] = (m[1] * m[5] - m[2] * m[4]) / det;
	o[3] = c1 / det, o[4] = (m[0] * m[8] - m[2] * m[6]) / det, o[5] = (m[2] * m[3] - m[0] * m[5]) / det;
	o[6] = c2 / det, o[7] = (m[1] * m[6] - m[0] * m[7]) / det, o[8] = (m[0] * m[4] - m[1] * m[3]) / det;
}
// the white point of T kelvin on the Planckian locus as XYZ with Y = 1 (the cubic-spline approximation of include/rfwhip.h)
static void grade_white(double T, double xyz[3])
{
	const double x = T <= 4000.0 ? -0.2661239e9 / (T * T * T) - 0.2343589e6 / (T * T) + 0.8776956e3 / T + 0.179910
								 : -3.0258469e9 / (T * T * T) + 2.1070379e6 / (T * T) + 0.2226347e3 / T + 0.240390;
	const double y = T <= 2222.0	? -1.1063814 * x * x * x - 1.34811020 * x * x + 2.18555832 * x - 0.20219683
					 : T <= 4000.0 ? -0.9549476 * x * x * x - 1.37418593 * x * x + 2.09137015 * x - 0.16748867
									: 3.0817580 * x * x * x - 5.87338670 * x * x + 3.75112997 * x - 0.37001483;
	xyz[0] = x / y, xyz[1] = 1.0, xyz[2] = (1.0 - x - y) / y;
}
// M_wb = M_xyz->rgb B^-1 diag(rho_6500 / rho_T) B M_rgb->xyz, in double, stored as float32
static void grade_wb_matrix(double T, float out[9])
{
	static const double B[9] = {0.8951, 0.2664, -0.1614, -0.7502, 1.7135, 0.0367, 0.0389, -0.0685, 1.0296};
	static const double RGB2XYZ[9] = {0.4124564, 0.3575761, 0.1804375, 0.2126729, 0.7151522, 0.0721750, 0.0193339, 0.1191920, 0.9503041};
	double wt[3], w0[3], Bi[9], X2R[9], D[9] = {}, t0[9], t1[9], M[9];
	grade_white(T, wt), grade_white(6500.0, w0);
	for (int i = 0; i < 3; i++)
	{
		const double rt_ = B[3 * i] * wt[0] + B[3 * i + 1] * wt[1] + B[3 * i + 2] * wt[2];
		const double r0 = B[3 * i] * w0[0] + B[3 * i + 1] * w0[1] + B[3 * i + 2] * w0[2];
		D[4 * i] = r0 / rt_;
	}
	mat3_inv(B, Bi), mat3_inv(RGB2XYZ, X2R);
	mat3_mul(B, RGB2XYZ, t0), mat3_mul(D, t0, t1), mat3_mul(Bi, t1, t0), mat3_mul(X2R, t0, M);
	for (int i = 0; i < 9; i++)
		out[i] = (float)M[i];
}
// what k_display_graded takes: the flags name the steps that are not at the identity
static rtk::GradeView grade_view(rfwhip_context *c, bool exposed)
{
	rtk::GradeView g;
	memset(&g, 0, sizeof(g));
	g.rec = exposed ? c->d_meter_rec.as<rtk::MeterRecord>() : nullptr;
	g.lut = c->lut_n ? c->d_grade_lut.as<f4>() : nullptr, g.n = c->lut_n;
	g.flags = (exposed ? rtk::GR_EXPOSED : 0u) | (c->grade_temperature != 6500.0f ? rtk::GR_WB : 0u) | (c->grade_sat != 1.0f ? rtk::GR_SAT : 0u) |
			  (c->lut_n ? rtk::GR_LUT : 0u) | (c->grade_dither ? rtk::GR_DITHER : 0u);
	for (int i = 0; i < 3; i++)
	{
		if (c->grade_slope[i] != 1.0f || c->grade_offset[i] != 0.0f || c->grade_power[i] != 1.0f)
			g.flags |= rtk::GR_CDL_R << i;
		g.slope[i] = c->grade_slope[i], g.offset[i] = c->grade_offset[i], g.power[i] = c->grade_power[i];
	}
	memcpy(g.wb, c->grade_wb, sizeof(g.wb));
	g.sat = c->grade_sat;
	return g;
}

// one launch on `stream`: the full W x H float4 image `in` -> `out` in `format`, with the context's display settings.
// display_exposure = auto: the exposed kernel with the record's E — `step`: behind one step of the meter on `in`;
// manual with display_exposure_ev != 0: the exposed kernel with E = exp2(ev), written into the record when it is not there yet;
// manual, ev = 0: k_display, as without the meter
static int display_enqueue(rfwhip_context *c, const f4 *in, void *out, float brightness, float contrast, int format, void *stream, bool step)
{
	rtk::DisplayView v;
	v.W = c->W, v.H = c->H, v.in = in, v.out = out;
	v.brightness = brightness, v.contrast = contrast;
	v.tonemap = (uint32_t)c->display_tonemap, v.fxaa = (uint32_t)c->display_fxaa, v.srgb = (uint32_t)c->display_srgb;
	v.format = (uint32_t)format;
	const bool exposed = c->exposure_auto || c->exposure_ev != 0.0f;
	if (c->exposure_auto)
	{
		if (step)
			RF_TRY(meter_step(c, in, stream));
		else
			RF_TRY(meter_ensure(c, 0));
	}
	else if (exposed)
	{
		RF_TRY(meter_ensure(c, 0));
		if (c->meter_manual_stale)
		{
			c->meter_manual_E = exp2f(c->exposure_ev);
			RF_TRY(dm::h2d(c->d_meter_rec.p, &c->meter_manual_E, sizeof(float), stream)); // (E is the record's first word)
			RF_TRY(meter_mark(c, stream));
			c->meter_manual_stale = false;
		}
	}
	// display_bloom = 1: the bloom chain on `in` under that E (the record's first word), behind the meter's step; the display kernel
	// reads the chain's image
	if (c->bloom_on)
	{
		RF_TRY(bloom_ensure(c));
		RF_TRY(bloom_chain(c, in, exposed ? c->d_meter_rec.as<float>() : c->d_bloom_one.as<float>(), stream));
		v.in = c->d_bloom_out.as<f4>();
	}
	{
		// display_grade = 1: the graded kernel in place of either, behind the same steps
		StageTimer t(c, c->grade_on ? KF_GRADE : KF_DISPLAY, -1, stream);
		if (c->grade_on)
			rtk::launch_display_graded(v, grade_view(c, exposed), stream);
		else if (exposed)
		{
			rtk::ExposureView e;
			e.rec = c->d_meter_rec.as<rtk::MeterRecord>();
			rtk::launch_display_exposed(v, e, stream);
		}
		else
			rtk::launch_display(v, stream);
		t.stop(1);
	}
	RF_TRY(dm::last_launch_error());
	if (c->grade_on && c->lut_n && stream != c->stream) // (the kernel read the LUT on a caller's stream)
		RF_TRY(c->marks[MK_GRADE].record(stream, true));
	return c->bloom_on ? bloom_mark(c, stream) : 0;
}
// brightness and contrast of the presented image: the camera of the last render; before the first one the reference's defaults
// (Camera.cpp:8-9)
static void display_camera(const rfwhip_context *c, float &brightness, float &contrast)
{
	brightness = c->have_last_cam ? c->last_cam.brightness : 0.05f;
	contrast = c->have_last_cam ? c->last_cam.contrast : 1.0f;
}

extern "C" int rfwhip_display_stream(rfwhip_context *c, const void *rgba_device, void *out_device, int format, void *hip_stream)
{
	CTX_ENTER(c);
	if (!rgba_device || !out_device)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "null image");
	if (rgba_device == out_device)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_display_stream: in place is not allowed (FXAA reads the neighbours of a pixel)");
	RF_TRY(display_check_format("rfwhip_display_stream", format));
	if (!c->W)
		return set_error(RFWHIP_ERR_STATE, "no render target");
	float b, k;
	display_camera(c, b, k);
	return display_enqueue(c, (const f4 *)rgba_device, out_device, b, k, format, hip_stream, true); // (auto: every call is a step)
}

extern "C" int rfwhip_read_display_device(rfwhip_context *c, int format, void *out_device)
{
	CTX_ENTER(c);
	if (!out_device)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "null destination");
	RF_TRY(display_check_format("rfwhip_read_display*", format));
	if (c->world != 1)
		return set_error(RFWHIP_ERR_STATE, "rfwhip_read_display*: this rank owns 1/%d of the image; the display stage runs on the "
											"gathered image (rfwhip_group_read_display, rfwhip_display_stream)", c->world);
	if (!c->W)
		return set_error(RFWHIP_ERR_STATE, "no render target");
	// present -> denoise when on -> display
	const size_t bytes = (size_t)c->W * c->H * sizeof(f4);
	RF_TRY(c->d_present.ensure(bytes));
	RF_TRY(dm::zero(c->d_present.p, bytes, c->stream));
	RF_TRY(rfwhip_read_framebuffer_device(c, c->d_present.p));
	float b, k;
	display_camera(c, b, k);
	// auto exposure: one step per render call — a further read of the same frame under the same settings shows it with the same E
	const bool step = c->exposure_auto && (!c->meter_have || c->meter_serial != c->frame_serial);
	RF_TRY(display_enqueue(c, c->d_present.as<f4>(), out_device, b, k, format, c->stream, step));
	if (step)
		c->meter_have = true, c->meter_serial = c->frame_serial;
	return dm::sync(c->stream);
}

extern "C" int rfwhip_read_display(rfwhip_context *c, int format, void *out_host)
{
	CTX_ENTER(c);
	if (!out_host)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "null destination");
	RF_TRY(display_check_format("rfwhip_read_display*", format));
	const size_t bytes = (size_t)c->W * c->H * display_pixel_bytes(format);
	RF_TRY(c->d_display.ensure(bytes));
	RF_TRY(rfwhip_read_display_device(c, format, c->d_display.p));
	return dm::d2h(out_host, c->d_display.p, bytes, c->stream); // (only the format's bytes travel)
}

extern "C" int rfwhip_display_image(rfwhip_context *c, const float *rgba_in, float brightness, float contrast, int format, void *out_host)
{
	CTX_ENTER(c);
	if (!rgba_in || !out_host)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "null image");
	RF_TRY(display_check_format("rfwhip_display_image", format));
	if (!c->W)
		return set_error(RFWHIP_ERR_STATE, "no render target");
	RF_TRY(sync_all(c));
	const size_t px = (size_t)c->W * c->H;
	RF_TRY(c->d_present.ensure(px * sizeof(f4)));
	RF_TRY(c->d_display.ensure(px * display_pixel_bytes(format)));
	RF_TRY(dm::h2d(c->d_present.p, rgba_in, px * sizeof(f4), c->stream));
	RF_TRY(display_enqueue(c, c->d_present.as<f4>(), c->d_display.p, brightness, contrast, format, c->stream, true));
	RF_TRY(dm::d2h(out_host, c->d_display.p, px * display_pixel_bytes(format), c->stream));
	return dm::sync(c->stream);
}

// ---- baseline JPEG (settings "display_jpeg_*"; work items and kernels: display_jpeg.h) ----------------------------------------------
static_assert(sizeof(rfwhip_jpeg_stats) == sizeof(rtk::JpegRecord) && sizeof(rtk::JpegRecord) == 32, "rfwhip.h: the JPEG record is the kernels' (kernels.h)");
// T.81 Annex K.1 (natural order), the zigzag sequence, Annex K.3 (BITS and HUFFVAL; the two DC tables share their values)
static const uint8_t k_jpeg_q[2][64] = {
	{16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
	 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
	{17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
	 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
static const uint8_t k_jpeg_zz[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
									  35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
static const uint8_t k_jpeg_bits[4][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},	  // DC luminance
										   {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},  // AC luminance
										   {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},	  // DC chrominance
										   {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}}; // AC chrominance
static const uint8_t k_jpeg_dc_val[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const uint8_t k_jpeg_ac_val[2][162] = {
	{0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
	 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
	 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
	 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
	 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
	 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
	{0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
	 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
	 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
	 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
	 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
	 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
// the scaled table of a quality (IJG): s = 5000 / quality below 50, else 200 - 2 quality; Q = clamp((base s + 50) / 100, 1, 255)
static void jpeg_quant_table(int table, int quality, uint16_t out[64])
{
	const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
	for (int i = 0; i < 64; i++)
		out[i] = (uint16_t)std::min(std::max(((int)k_jpeg_q[table][i] * s + 50) / 100, 1), 255);
}
// canonical codes of one table: out[symbol] = code | length << 16 (0: the symbol has no code)
static void jpeg_huffman(const uint8_t bits[16], const uint8_t *vals, uint32_t *out, size_t out_n)
{
	for (size_t i = 0; i < out_n; i++)
		out[i] = 0u;
	uint32_t code = 0u;
	size_t k = 0;
	for (uint32_t len = 1; len <= 16u; len++, code <<= 1)
		for (uint32_t n = 0; n < bits[len - 1u]; n++, k++, code++)
			if (vals[k] < out_n)
				out[vals[k]] = code | (len << 16);
}
static void jpeg_tables(rtk::JpegTables &t)
{
	// K[u][x] = round(8192 a(u) cos((2 x + 1) u pi / 16)): 8192 / sqrt(8) in row 0, below it 4096 cos(n pi / 16) for n = 1 .. 7
	static const int cs[8] = {4096, 4017, 3784, 3406, 2896, 2276, 1567, 799};
	for (int u = 0; u < 8; u++)
		for (int x = 0; x < 8; x++)
		{
			int n = ((2 * x + 1) * u) % 32, sign = 1;
			if (n > 16)
				n = 32 - n;
			if (n > 8)
				n = 16 - n, sign = -1;
			t.K[u * 8 + x] = u == 0 ? 2896 : sign * (n == 8 ? 0 : cs[n]);
		}
	for (int z = 0; z < 64; z++)
		t.zz[z] = k_jpeg_zz[z], t.izz[k_jpeg_zz[z]] = (uint8_t)z;
	for (int table = 0; table < 2; table++)
	{
		jpeg_huffman(k_jpeg_bits[2 * table], k_jpeg_dc_val, t.dc[table], 12);
		jpeg_huffman(k_jpeg_bits[2 * table + 1], k_jpeg_ac_val[table], t.ac[table], 256);
	}
}
// SOI, APP0, DQT, SOF0, DHT, DRI, SOS: JP_HEADER bytes
static void jpeg_header(const rfwhip_context *c, uint8_t *h)
{
	size_t n = 0;
	const auto put8 = [&](uint32_t b) { h[n++] = (uint8_t)b; };
	const auto put16 = [&](uint32_t w) { put8(w >> 8), put8(w & 255u); };
	put16(0xFFD8);
	put16(0xFFE0), put16(16);
	for (const uint8_t b : {0x4A, 0x46, 0x49, 0x46, 0x00, 0x01, 0x01, 0x00, 0x00, 0x01, 0x00, 0x01, 0x00, 0x00})
		put8(b);
	put16(0xFFDB), put16(2 + 2 * 65);
	for (int table = 0; table < 2; table++)
	{
		uint16_t q[64];
		jpeg_quant_table(table, c->jpeg_quality, q);
		put8((uint32_t)table);
		for (int z = 0; z < 64; z++)
			put8(q[k_jpeg_zz[z]]);
	}
	put16(0xFFC0), put16(17), put8(8), put16(c->H), put16(c->W), put8(3);
	put8(1), put8(c->jpeg_sub ? 0x22 : 0x11), put8(0), put8(2), put8(0x11), put8(1), put8(3), put8(0x11), put8(1);
	put16(0xFFC4), put16(2 + 2 * (17 + 12) + 2 * (17 + 162));
	for (int k = 0; k < 4; k++) // DC0, AC0, DC1, AC1
	{
		put8((uint32_t)((k & 1) << 4 | (k >> 1)));
		for (int i = 0; i < 16; i++)
			put8(k_jpeg_bits[k][i]);
		if (k & 1)
			for (int i = 0; i < 162; i++)
				put8(k_jpeg_ac_val[k >> 1][i]);
		else
			for (int i = 0; i < 12; i++)
				put8(k_jpeg_dc_val[i]);
	}
	put16(0xFFDD), put16(4), put16((uint32_t)c->jpeg_restart);
	put16(0xFFDA), put16(12), put8(3), put8(1), put8(0x00), put8(2), put8(0x11), put8(3), put8(0x11), put8(0), put8(63), put8(0);
	(void)n; // == JP_HEADER (tests/test_display_jpeg.py holds the header to the model's byte for byte)
}
// the geometry of the target under the current settings, and the capacity that always suffices: the header, every block at its
// worst case, two marker bytes per interval
static void jpeg_geometry(const rfwhip_context *c, rtk::JpegView &v)
{
	const uint32_t M = c->jpeg_sub ? 16u : 8u;
	v.W = c->W, v.H = c->H, v.sub = (uint32_t)c->jpeg_sub;
	v.mcus_x = (c->W + M - 1u) / M, v.mcus = v.mcus_x * ((c->H + M - 1u) / M);
	v.bpm = c->jpeg_sub ? 6u : 3u, v.blocks = v.mcus * v.bpm;
	v.ri = (uint32_t)c->jpeg_restart, v.intervals = (v.mcus + v.ri - 1u) / v.ri;
}
static uint64_t jpeg_bound(const rtk::JpegView &v) { return (uint64_t)rtk::JP_HEADER + (uint64_t)v.blocks * rtk::JP_BLOCK_BYTES + 2ull * v.intervals; }
static int jpeg_check_target(const rfwhip_context *c, const char *who)
{
	if (!c->W)
		return set_error(RFWHIP_ERR_STATE, "no render target");
	if (c->W > 65535u || c->H > 65535u)
		return set_error(RFWHIP_ERR_UNSUPPORTED, "%s: a JPEG is at most 65535 pixels wide and high, the target is %u x %u", who, c->W, c->H);
	return RFWHIP_OK;
}
// the four kernels on `stream`: W x H RGBA8 at `rgba8` -> the stream at `out` (cap bytes, >= JP_HEADER) and the record at `rec`
static int jpeg_enqueue(rfwhip_context *c, const void *rgba8, void *out, size_t cap, void *rec, void *stream)
{
	rtk::JpegView v;
	memset(&v, 0, sizeof(v));
	jpeg_geometry(c, v);
	if (jpeg_bound(v) + 3ull * v.intervals > 0xFFFFFFFFull)
		return set_error(RFWHIP_ERR_UNSUPPORTED, "display_jpeg: a %u x %u target is too large for the encoder's 32-bit offsets", c->W, c->H);
	// one scratch: an encode on another stream has to be through with it
	if (c->marks[MK_JPEG].stream != stream)
		RF_TRY(c->marks[MK_JPEG].sync());
	if (!c->d_jpeg_tab.p)
	{
		rtk::JpegTables t;
		jpeg_tables(t);
		RF_TRY(c->d_jpeg_tab.ensure(sizeof(t)));
		RF_TRY(dm::h2d(c->d_jpeg_tab.p, &t, sizeof(t), c->stream));
		RF_TRY(dm::sync(c->stream));
	}
	const size_t need[4] = {(size_t)v.blocks * 128u, (size_t)v.blocks * rtk::JP_BLOCK_BYTES + 3u * (size_t)v.intervals, (size_t)v.intervals * 8u, (size_t)v.intervals * 4u};
	DevBuf *buf[4] = {&c->d_jpeg_coef, &c->d_jpeg_slots, &c->d_jpeg_counts, &c->d_jpeg_offsets};
	for (int k = 0; k < 4; k++)
		if (need[k] > buf[k]->cap || !buf[k]->p)
		{
			RF_TRY(sync_all(c)); // (an encode in flight uses the buffer this reallocates)
			if (stream != c->stream)
				RF_TRY(dm::sync(stream));
			RF_TRY(buf[k]->ensure(need[k]));
		}
	v.rgba = (const uint32_t *)rgba8, v.tab = c->d_jpeg_tab.as<rtk::JpegTables>();
	jpeg_quant_table(0, c->jpeg_quality, v.q[0]), jpeg_quant_table(1, c->jpeg_quality, v.q[1]);
	v.coef = c->d_jpeg_coef.as<int16_t>(), v.slots = c->d_jpeg_slots.as<uint8_t>();
	v.counts = c->d_jpeg_counts.as<uint32_t>(), v.offsets = c->d_jpeg_offsets.as<uint32_t>();
	v.rec = (rtk::JpegRecord *)rec, v.out = (uint8_t *)out, v.cap = (uint32_t)std::min<size_t>(cap, 0xFFFFFFFFu);
	uint8_t header[rtk::JP_HEADER];
	jpeg_header(c, header);
	RF_TRY(dm::h2d(out, header, sizeof(header), stream));
	void (*const launch[4])(const rtk::JpegView &, void *) = {rtk::launch_jpeg_blocks, rtk::launch_jpeg_entropy, rtk::launch_jpeg_offsets, rtk::launch_jpeg_pack};
	for (int k = 0; k < 4; k++)
	{
		StageTimer t(c, KF_JPEG, k, stream);
		launch[k](v, stream);
		t.stop(1);
		RF_TRY(dm::last_launch_error());
	}
	c->jpeg_coef_blocks = v.blocks;
	return c->marks[MK_JPEG].record(stream, true);
}

extern "C" int rfwhip_display_jpeg_bound(rfwhip_context *c, size_t *bytes)
{
	CTX_ENTER(c);
	if (!bytes)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_display_jpeg_bound: null argument");
	RF_TRY(jpeg_check_target(c, "rfwhip_display_jpeg_bound"));
	rtk::JpegView v;
	memset(&v, 0, sizeof(v));
	jpeg_geometry(c, v);
	*bytes = (size_t)jpeg_bound(v);
	return RFWHIP_OK;
}

extern "C" int rfwhip_display_jpeg_stream(rfwhip_context *c, const void *rgba8_device, void *out_device, size_t cap, void *record_device, void *hip_stream)
{
	CTX_ENTER(c);
	if (!rgba8_device || !out_device || !record_device)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_display_jpeg_stream: null argument");
	RF_TRY(jpeg_check_target(c, "rfwhip_display_jpeg_stream"));
	if (cap < rtk::JP_HEADER)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_display_jpeg_stream: cap = %zu bytes does not hold the header of %u bytes", cap, rtk::JP_HEADER);
	return jpeg_enqueue(c, rgba8_device, out_device, cap, record_device, hip_stream);
}

// the RGBA8 image in d_display -> the stream in `out_host`: the record first, then exactly its bytes
static int jpeg_read_back(rfwhip_context *c, const char *who, void *out_host, size_t cap, size_t *bytes)
{
	rtk::JpegView v;
	memset(&v, 0, sizeof(v));
	jpeg_geometry(c, v);
	// (the device's capacity: the caller's, never more than the bound and never less than the header — the record then names the
	// stream's length whether it fitted or not)
	const size_t dev_cap = (size_t)std::min<uint64_t>(jpeg_bound(v), std::max<uint64_t>(cap, rtk::JP_HEADER));
	RF_TRY(c->d_jpeg_rec.ensure(sizeof(rtk::JpegRecord)));
	if (dev_cap > c->d_jpeg_out.cap || !c->d_jpeg_out.p)
	{
		RF_TRY(sync_all(c));
		RF_TRY(c->d_jpeg_out.ensure(dev_cap));
	}
	RF_TRY(jpeg_enqueue(c, c->d_display.p, c->d_jpeg_out.p, dev_cap, c->d_jpeg_rec.p, c->stream));
	rtk::JpegRecord r;
	RF_TRY(dm::d2h(&r, c->d_jpeg_rec.p, sizeof(r), c->stream));
	c->marks[MK_JPEG].pending = false; // (the stream is idle)
	c->jpeg_rec_host = r;
	if (bytes)
		*bytes = r.bytes;
	if (r.overflow || (size_t)r.bytes > cap)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s: the stream has %u bytes, cap is %zu", who, r.bytes, cap);
	return dm::d2h(out_host, c->d_jpeg_out.p, r.bytes, c->stream);
}

extern "C" int rfwhip_read_display_jpeg(rfwhip_context *c, void *out_host, size_t cap, size_t *bytes)
{
	CTX_ENTER(c);
	if (!out_host && cap)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_read_display_jpeg: null destination");
	RF_TRY(jpeg_check_target(c, "rfwhip_read_display_jpeg"));
	// present -> denoise when on -> display (RGBA8) -> encode
	RF_TRY(c->d_display.ensure((size_t)c->W * c->H * 4u));
	RF_TRY(rfwhip_read_display_device(c, RFWHIP_DISPLAY_RGBA8, c->d_display.p));
	return jpeg_read_back(c, "rfwhip_read_display_jpeg", out_host, cap, bytes);
}

extern "C" int rfwhip_jpeg_image(rfwhip_context *c, const void *rgba8_in, void *out_host, size_t cap, size_t *bytes)
{
	CTX_ENTER(c);
	if (!rgba8_in || (!out_host && cap))
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_jpeg_image: null image");
	RF_TRY(jpeg_check_target(c, "rfwhip_jpeg_image"));
	RF_TRY(sync_all(c));
	const size_t px = (size_t)c->W * c->H;
	RF_TRY(c->d_display.ensure(px * 4u));
	RF_TRY(dm::h2d(c->d_display.p, rgba8_in, px * 4u, c->stream));
	return jpeg_read_back(c, "rfwhip_jpeg_image", out_host, cap, bytes);
}

extern "C" int rfwhip_get_jpeg(rfwhip_context *c, rfwhip_jpeg_stats *stats)
{
	CTX_ENTER(c);
	if (!stats)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_get_jpeg: null argument");
	if (!c->jpeg_rec_host.header)
		return set_error(RFWHIP_ERR_STATE, "rfwhip_get_jpeg: no stream has been read back");
	memcpy(stats, &c->jpeg_rec_host, sizeof(*stats));
	return RFWHIP_OK;
}

extern "C" int rfwhip_read_jpeg_coefficients(rfwhip_context *c, int16_t *out, size_t cap_blocks, uint32_t *blocks)
{
	CTX_ENTER(c);
	if (!c->jpeg_coef_blocks)
		return set_error(RFWHIP_ERR_STATE, "rfwhip_read_jpeg_coefficients: nothing has been encoded");
	if (blocks)
		*blocks = c->jpeg_coef_blocks;
	if (!out)
		return RFWHIP_OK; // (the count alone)
	if (cap_blocks < c->jpeg_coef_blocks)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_read_jpeg_coefficients: %u blocks, room for %zu", c->jpeg_coef_blocks, cap_blocks);
	RF_TRY(sync_all(c));
	return dm::d2h(out, c->d_jpeg_coef.p, (size_t)c->jpeg_coef_blocks * 128u, c->stream);
}

// ---- image textures (work items and kernels: texture_decode.h) -----------------------------------------------------------------------
static_assert(sizeof(rfwhip_texture_decode_record) == sizeof(rtk::TexRecord) && sizeof(rtk::TexRecord) == 32, "rfwhip.h: the decode record is the kernels' (texture_decode.h)");
static_assert(rtk::TD_INVALID == RFWHIP_ERR_INVALID_ARGUMENT && rtk::TD_UNSUPPORTED == RFWHIP_ERR_UNSUPPORTED, "texture_decode.h answers rfwhip.h's codes");
static_assert(rtk::TD_FLIP_ROWS == RFWHIP_TEXSRC_FLIP_ROWS && rtk::TD_LINEARIZE_REFERENCE == RFWHIP_TEXSRC_LINEARIZE_REFERENCE &&
				  rtk::TD_LINEARIZE_SRGB == RFWHIP_TEXSRC_LINEARIZE_SRGB && rtk::TD_ERR_TRUNCATED == RFWHIP_TEXDEC_ERR_TRUNCATED &&
				  rtk::TD_ERR_RUN == RFWHIP_TEXDEC_ERR_RUN && rtk::TD_ERR_NOCODE == RFWHIP_TEXDEC_ERR_NOCODE && rtk::TD_ERR_MARKER == RFWHIP_TEXDEC_ERR_MARKER,
			  "texture_decode.h restates rfwhip.h's flags");

// one source of a decode: a walked JPEG stream, or RGBA8 pixels
struct TdJob
{
	bool jpeg = false;
	const void *data = nullptr;
	size_t bytes = 0;
	uint32_t W = 0, H = 0, mods = 0;
	rtk::TdInfo info;
};
// host arrays an enqueued copy still reads: alive until the stream has been waited for
struct TdKeep
{
	std::vector<std::vector<int16_t>> coef;
	std::vector<std::vector<uint32_t>> words;
};
static int td_check_flags(const char *who, uint32_t flags)
{
	if (flags & ~7u)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s: unknown flags 0x%x", who, flags);
	if ((flags & RFWHIP_TEXSRC_LINEARIZE_REFERENCE) && (flags & RFWHIP_TEXSRC_LINEARIZE_SRGB))
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s: two linearisations at once", who);
	return 0;
}
// the scratch for every job of a call, sized once (a growing buffer waits for the work in flight first)
static int td_reserve(rfwhip_context *c, const std::vector<TdJob> &jobs)
{
	size_t need[8] = {0, 0, sizeof(rtk::TdTables), 0, 0, 0, 0, 0};
	bool srgb = false;
	for (const TdJob &j : jobs)
	{
		srgb = srgb || (j.mods & rtk::TD_LINEARIZE_SRGB);
		need[6] = std::max(need[6], (size_t)rtk::td_tiles(j.W, j.H) * 4u);
		if (!j.jpeg)
		{
			need[7] = std::max(need[7], (size_t)j.W * j.H * 4u);
			continue;
		}
		rtk::TexdecView v;
		size_t planes = 0;
		rtk::td_view_geometry(j.info, v, &planes);
		need[0] = std::max(need[0], j.bytes), need[1] = std::max(need[1], j.info.ranges.size() * 4u);
		need[3] = std::max(need[3], (size_t)j.info.blocks * 128u), need[4] = std::max(need[4], (size_t)j.info.intervals * 4u);
		need[5] = std::max(need[5], planes);
	}
	DevBuf *buf[8] = {&c->d_td_stream, &c->d_td_ranges, &c->d_td_tab, &c->d_td_coef, &c->d_td_flags, &c->d_td_planes, &c->d_td_alpha, &c->d_td_src};
	for (int k = 0; k < 8; k++)
		if (need[k] && (need[k] > buf[k]->cap || !buf[k]->p))
		{
			RF_TRY(sync_all(c));
			RF_TRY(buf[k]->ensure(need[k]));
		}
	if (srgb && !c->d_td_lin.p)
	{
		uint8_t lin[256];
		rtk::td_srgb_table(lin);
		RF_TRY(c->d_td_lin.ensure(sizeof(lin)));
		RF_TRY(dm::h2d(c->d_td_lin.p, lin, sizeof(lin), c->stream));
		RF_TRY(dm::sync(c->stream));
	}
	return 0;
}
// one job on the context's stream: level 0 (and with `mips` the chain behind it) at `out`, the record at `rec`
static int td_enqueue(rfwhip_context *c, const TdJob &j, uint32_t *out, rtk::TexRecord *rec, bool mips, TdKeep &keep)
{
	void *const s = c->stream;
	rtk::TexdecView v;
	memset(&v, 0, sizeof(v));
	v.W = j.W, v.H = j.H, v.mods = j.mods, v.out = out, v.rec = rec, v.alpha = c->d_td_alpha.as<uint32_t>();
	v.lin = c->d_td_lin.as<uint8_t>(), v.tiles = mips ? rtk::td_tiles(j.W, j.H) : 0u, v.path = rtk::TD_PATH_NONE;
	const auto run = [&](int kind, void (*launch)(const rtk::TexdecView &, void *)) {
		StageTimer t(c, KF_TEXDEC, kind, s);
		launch(v, s);
		t.stop(1);
		return dm::last_launch_error();
	};
	if (j.jpeg)
	{
		rtk::td_view_geometry(j.info, v, nullptr);
		v.coef = c->d_td_coef.as<int16_t>(), v.flags = c->d_td_flags.as<uint32_t>(), v.planes = c->d_td_planes.as<uint8_t>();
		v.tab = c->d_td_tab.as<rtk::TdTables>();
		RF_TRY(dm::h2d(c->d_td_tab.p, &j.info.tab, sizeof(rtk::TdTables), s));
		const bool device = c->td_entropy == 2 || (c->td_entropy == 0 && j.info.ri != 0u);
		v.path = device ? rtk::TD_PATH_DEVICE : rtk::TD_PATH_HOST;
		if (device)
		{
			v.stream = c->d_td_stream.as<uint8_t>(), v.ranges = c->d_td_ranges.as<uint32_t>();
			RF_TRY(dm::h2d(c->d_td_stream.p, j.data, j.bytes, s));
			RF_TRY(dm::h2d(c->d_td_ranges.p, j.info.ranges.data(), j.info.ranges.size() * 4u, s));
			RF_TRY(run(0, rtk::launch_texdec_zero));
			RF_TRY(run(1, rtk::launch_texdec_entropy));
		}
		else // the same item, serially over the host's arrays; the words go up
		{
			keep.coef.emplace_back((size_t)v.blocks * 64u, (int16_t)0);
			keep.words.emplace_back((size_t)v.intervals, 0u);
			rtk::TexdecView h = v;
			h.stream = (const uint8_t *)j.data, h.ranges = j.info.ranges.data(), h.tab = &j.info.tab;
			h.coef = keep.coef.back().data(), h.flags = keep.words.back().data();
			rtk::td_host_entropy(h);
			RF_TRY(dm::h2d(c->d_td_coef.p, h.coef, (size_t)v.blocks * 128u, s));
			RF_TRY(dm::h2d(c->d_td_flags.p, h.flags, (size_t)v.intervals * 4u, s));
		}
		RF_TRY(run(2, rtk::launch_texdec_idct));
		c->td_coef_blocks = v.blocks;
	}
	else
	{
		v.src = c->d_td_src.as<uint32_t>();
		RF_TRY(dm::h2d(c->d_td_src.p, j.data, (size_t)j.W * j.H * 4u, s));
	}
	RF_TRY(run(3, rtk::launch_texdec_color));
	if (mips)
		RF_TRY(run(4, rtk::launch_tex_mips));
	return run(5, rtk::launch_texdec_finish);
}
static int td_error_of_record(const char *who, size_t index, const rtk::TexRecord &r)
{
	if (!r.errors)
		return 0;
	return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s: texture %zu: the entropy data is corrupt (%s%s%s%s)", who, index,
					 (r.errors & rtk::TD_ERR_TRUNCATED) ? " an interval ends inside a code;" : "", (r.errors & rtk::TD_ERR_RUN) ? " a zero run passes coefficient 63;" : "",
					 (r.errors & rtk::TD_ERR_NOCODE) ? " bits that are no Huffman code;" : "", (r.errors & rtk::TD_ERR_MARKER) ? " a marker inside an interval;" : "");
}

extern "C" int rfwhip_image_info(const void *data, size_t bytes, rfwhip_image_info_t *info)
{
	if (!data || !info)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_image_info: null argument");
	rtk::TdInfo t;
	const int rc = rtk::td_walk((const uint8_t *)data, bytes, t);
	memset(info, 0, sizeof(*info));
	info->width = t.W, info->height = t.H, info->components = t.ncomp, info->h_sampling = t.hs, info->v_sampling = t.vs;
	info->restart_interval = t.ri, info->intervals = t.intervals, info->supported = rc == rtk::TD_OK;
	snprintf(info->reason, sizeof(info->reason), "%s", t.msg);
	if (rc == rtk::TD_INVALID)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_image_info: %s", t.msg);
	return RFWHIP_OK;
}

extern "C" int rfwhip_png_unfilter(const uint8_t *in, size_t rows, size_t row_bytes, size_t bpp, uint8_t *out)
{
	if (!in || !out || !bpp)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_png_unfilter: null argument");
	if (rtk::td_png_unfilter(in, rows, row_bytes, bpp, out))
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_png_unfilter: a filter type above 4");
	return RFWHIP_OK;
}

extern "C" int rfwhip_set_texture_sources(rfwhip_context *c, const rfwhip_texture_source *src, size_t count)
{
	CTX_ENTER(c);
	const char *const who = "rfwhip_set_texture_sources";
	if (count && !src)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s: null array", who);
	// 1. every header, and the layout of the one table
	std::vector<rt::TexDesc> desc(count);
	std::vector<TdJob> jobs(count);
	std::vector<f4> f4s;
	uint64_t n_u32 = 0;
	for (size_t i = 0; i < count; i++)
	{
		const rfwhip_texture_source &t = src[i];
		rt::TexDesc &d = desc[i];
		TdJob &j = jobs[i];
		memset(&d, 0, sizeof(d));
		if (!t.data)
			return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s: texture %zu has no data", who, i);
		if (t.kind == RFWHIP_TEXSRC_TEXELS)
		{
			d.type = t.type, d.width = t.width, d.height = t.height, d.texelCount = t.texelCount;
			if (!t.texelCount || (t.type != RFWHIP_TEX_UINT && t.type != RFWHIP_TEX_FLOAT4))
				return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s: texture %zu has no texels or an unknown type %u", who, i, t.type);
			if (t.type == RFWHIP_TEX_FLOAT4)
			{
				d.offset = (uint32_t)f4s.size();
				f4s.insert(f4s.end(), (const f4 *)t.data, (const f4 *)t.data + t.texelCount);
				continue;
			}
		}
		else if (t.kind == RFWHIP_TEXSRC_JPEG || t.kind == RFWHIP_TEXSRC_RGBA8)
		{
			if (td_check_flags(who, t.flags))
				return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s: texture %zu: flags 0x%x", who, i, t.flags);
			j.jpeg = t.kind == RFWHIP_TEXSRC_JPEG, j.data = t.data, j.bytes = t.bytes, j.mods = t.flags, j.W = t.width, j.H = t.height;
			if (j.jpeg)
			{
				const int rc = rtk::td_walk((const uint8_t *)t.data, t.bytes, j.info);
				if (rc)
					return set_error(rc, "%s: texture %zu: %s", who, i, j.info.msg);
				j.W = j.info.W, j.H = j.info.H;
			}
			else if (!j.W || !j.H || j.W > 65535u || j.H > 65535u || t.bytes != (size_t)j.W * j.H * 4u)
				return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s: texture %zu: %u x %u RGBA8 pixels in %zu bytes", who, i, j.W, j.H, t.bytes);
			if ((uint64_t)j.W * j.H > 0x3FFFFFFFull)
				return set_error(RFWHIP_ERR_UNSUPPORTED, "%s: texture %zu: %u x %u texels", who, i, j.W, j.H);
			d.type = RFWHIP_TEX_UINT, d.width = j.W, d.height = j.H, d.texelCount = rtk::td_chain_texels(j.W, j.H);
		}
		else
			return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s: texture %zu has unknown kind %u", who, i, t.kind);
		d.offset = (uint32_t)n_u32, n_u32 += d.texelCount;
		if (n_u32 > 0xFFFFFFFFull)
			return set_error(RFWHIP_ERR_UNSUPPORTED, "%s: more than 2^32 texels", who);
	}
	// 2. a new table beside the current one: the current one stays whatever happens below
	RF_TRY(sync_all(c));
	std::vector<TdJob> work;
	for (const TdJob &j : jobs)
		if (j.data)
			work.push_back(j);
	RF_TRY(td_reserve(c, work));
	DevBuf n_desc, n_tex, n_f4, n_rec;
	const auto drop = [&](int rc) {
		(void)dm::sync(c->stream);
		n_desc.free_(), n_tex.free_(), n_f4.free_(), n_rec.free_();
		return rc;
	};
	std::vector<rtk::TexRecord> records(count, rtk::TexRecord{0, 0, 0, 0, 0, 0, 0, 0});
	TdKeep keep;
	int rc = n_desc.ensure(desc.size() * sizeof(rt::TexDesc));
	rc = rc ? rc : n_tex.ensure((size_t)n_u32 * 4u);
	rc = rc ? rc : n_f4.ensure(f4s.size() * sizeof(f4));
	rc = rc ? rc : n_rec.ensure(count * sizeof(rtk::TexRecord));
	rc = rc ? rc : dm::h2d(n_desc.p, desc.data(), desc.size() * sizeof(rt::TexDesc), c->stream);
	rc = rc ? rc : dm::h2d(n_f4.p, f4s.data(), f4s.size() * sizeof(f4), c->stream);
	rc = rc ? rc : dm::h2d(n_rec.p, records.data(), count * sizeof(rtk::TexRecord), c->stream);
	for (size_t i = 0; i < count && !rc; i++)
	{
		uint32_t *slot = n_tex.as<uint32_t>() + desc[i].offset;
		if (src[i].kind == RFWHIP_TEXSRC_TEXELS)
			rc = src[i].type == RFWHIP_TEX_UINT ? dm::h2d(slot, src[i].data, (size_t)desc[i].texelCount * 4u, c->stream) : 0;
		else
			rc = td_enqueue(c, jobs[i], slot, n_rec.as<rtk::TexRecord>() + i, true, keep);
	}
	rc = rc ? rc : dm::d2h(records.data(), n_rec.p, count * sizeof(rtk::TexRecord), c->stream);
	if (rc)
		return drop(rc);
	for (size_t i = 0; i < count; i++)
		if (td_error_of_record(who, i, records[i]))
			return drop(RFWHIP_ERR_INVALID_ARGUMENT);
	// 3. the new table takes the place of the old one
	std::swap(c->d_textures, n_desc), std::swap(c->d_tex_u32, n_tex), std::swap(c->d_tex_f4, n_f4), std::swap(c->d_td_rec, n_rec);
	n_desc.free_(), n_tex.free_(), n_f4.free_(), n_rec.free_();
	c->texture_count = (uint32_t)count, c->tex_desc_host = desc, c->td_records = records;
	update_maps_present(c);
	c->scene_dirty = true;
	return RFWHIP_OK;
}

extern "C" int rfwhip_get_texture_decode(rfwhip_context *c, size_t index, rfwhip_texture_decode_record *record)
{
	CTX_ENTER(c);
	if (record && index == (size_t)-1 && c->td_hook_ran) // the record of the last rfwhip_decode_image
	{
		memcpy(record, &c->td_hook_record, sizeof(*record));
		return RFWHIP_OK;
	}
	if (!record || index >= c->td_records.size())
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_get_texture_decode: texture %zu of %zu", index, c->td_records.size());
	memcpy(record, &c->td_records[index], sizeof(*record));
	return RFWHIP_OK;
}

extern "C" int rfwhip_read_texture(rfwhip_context *c, size_t index, void *out, size_t cap_texels, size_t *texels)
{
	CTX_ENTER(c);
	if (index >= c->tex_desc_host.size())
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_read_texture: texture %zu of %zu", index, c->tex_desc_host.size());
	const rt::TexDesc &d = c->tex_desc_host[index];
	if (texels)
		*texels = d.texelCount;
	if (!out)
		return RFWHIP_OK;
	if (cap_texels < d.texelCount)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_read_texture: %u texels, room for %zu", d.texelCount, cap_texels);
	RF_TRY(sync_all(c));
	if (d.type == RFWHIP_TEX_FLOAT4)
		return dm::d2h(out, c->d_tex_f4.as<f4>() + d.offset, (size_t)d.texelCount * sizeof(f4), c->stream);
	return dm::d2h(out, c->d_tex_u32.as<uint32_t>() + d.offset, (size_t)d.texelCount * 4u, c->stream);
}

extern "C" int rfwhip_decode_image(rfwhip_context *c, const void *data, size_t bytes, uint32_t flags, void *out_rgba8_host, size_t cap_texels,
								   uint32_t *w, uint32_t *h)
{
	CTX_ENTER(c);
	if (!data)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_decode_image: null stream");
	RF_TRY(td_check_flags("rfwhip_decode_image", flags));
	std::vector<TdJob> job(1);
	TdJob &j = job[0];
	j.jpeg = true, j.data = data, j.bytes = bytes, j.mods = flags;
	const int rc = rtk::td_walk((const uint8_t *)data, bytes, j.info);
	if (rc)
		return set_error(rc, "rfwhip_decode_image: %s", j.info.msg);
	j.W = j.info.W, j.H = j.info.H;
	if (w)
		*w = j.W;
	if (h)
		*h = j.H;
	const size_t px = (size_t)j.W * j.H;
	if (!out_rgba8_host)
		return RFWHIP_OK;
	if (cap_texels < px)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_decode_image: %zu texels, room for %zu", px, cap_texels);
	RF_TRY(sync_all(c));
	RF_TRY(td_reserve(c, job));
	if (px * 4u + 32u > c->d_td_out.cap || !c->d_td_out.p)
		RF_TRY(c->d_td_out.ensure(px * 4u + 32u));
	TdKeep keep;
	rtk::TexRecord *rec = (rtk::TexRecord *)(c->d_td_out.as<uint8_t>() + px * 4u);
	int e = td_enqueue(c, j, c->d_td_out.as<uint32_t>(), rec, false, keep);
	rtk::TexRecord r;
	e = e ? e : dm::d2h(&r, rec, sizeof(r), c->stream);
	if (e)
	{
		(void)dm::sync(c->stream);
		return e;
	}
	c->td_hook_record = r, c->td_hook_ran = true;
	RF_TRY(td_error_of_record("rfwhip_decode_image", 0, r));
	return dm::d2h(out_rgba8_host, c->d_td_out.p, px * 4u, c->stream);
}

extern "C" int rfwhip_read_texture_coefficients(rfwhip_context *c, int16_t *out, size_t cap_blocks, uint32_t *blocks)
{
	CTX_ENTER(c);
	if (!c->td_coef_blocks)
		return set_error(RFWHIP_ERR_STATE, "rfwhip_read_texture_coefficients: nothing has been decoded");
	if (blocks)
		*blocks = c->td_coef_blocks;
	if (!out)
		return RFWHIP_OK; // (the count alone)
	if (cap_blocks < c->td_coef_blocks)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_read_texture_coefficients: %u blocks, room for %zu", c->td_coef_blocks, cap_blocks);
	RF_TRY(sync_all(c));
	return dm::d2h(out, c->d_td_coef.p, (size_t)c->td_coef_blocks * 128u, c->stream);
}

// ---- the sky's loaders (work items and kernels: sky_load.h) -----------------------------------------------------------------------
static_assert(sizeof(rfwhip_sky_table_record) == sizeof(rtk::SkyTabRecord) && sizeof(rfwhip_sky_alias) == sizeof(rtk::SkyAliasEntry) &&
				  sizeof(rtk::SkyAliasEntry) == sizeof(rt::SkyAlias) && sizeof(rtk::SkyF4) == sizeof(f4),
			  "rfwhip.h: the sky table's records are the kernels' (sky_load.h, rt_types.h)");
static_assert(rtk::SKY_INVALID == RFWHIP_ERR_INVALID_ARGUMENT && rtk::SKY_UNSUPPORTED == RFWHIP_ERR_UNSUPPORTED && rtk::SKY_FLIP_ROWS == RFWHIP_SKYSRC_FLIP_ROWS &&
				  rtk::SKY_ERR_ZERO == RFWHIP_SKYHDR_ERR_ZERO && rtk::SKY_ERR_OVERRUN == RFWHIP_SKYHDR_ERR_OVERRUN &&
				  rtk::SKY_ERR_TRUNCATED == RFWHIP_SKYHDR_ERR_TRUNCATED && rtk::SKYTAB_VALID == RFWHIP_SKYTAB_VALID && rtk::SKYTAB_DEVICE == RFWHIP_SKYTAB_DEVICE,
			  "sky_load.h restates rfwhip.h's codes and flags");

extern "C" int rfwhip_hdr_info(const void *data, size_t bytes, rfwhip_hdr_info_t *info)
{
	if (!data || !info)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_hdr_info: null argument");
	rtk::SkyHdrInfo t;
	const int rc = rtk::skyhdr_walk((const uint8_t *)data, bytes, t);
	memset(info, 0, sizeof(*info));
	info->width = t.W, info->height = t.H, info->exposure = t.exposure, info->rle = t.rle_lines != 0u, info->supported = rc == rtk::SKY_OK;
	snprintf(info->reason, sizeof(info->reason), "%s", t.msg);
	if (rc == rtk::SKY_INVALID)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_hdr_info: %s", t.msg);
	return RFWHIP_OK;
}

extern "C" int rfwhip_set_sky_hdr(rfwhip_context *c, const void *data, size_t bytes, uint32_t flags)
{
	CTX_ENTER(c);
	const char *const who = "rfwhip_set_sky_hdr";
	if (!data)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s: null file", who);
	if (flags & ~(uint32_t)RFWHIP_SKYSRC_FLIP_ROWS)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s: unknown flags 0x%x", who, flags);
	rtk::SkyHdrInfo info;
	const int walked = rtk::skyhdr_walk((const uint8_t *)data, bytes, info);
	if (walked)
		return set_error(walked, "%s: %s", who, info.msg);
	// a new sky beside the current one: the current one stays whatever happens below
	RF_TRY(sync_all(c));
	void *const s = c->stream;
	const size_t n = (size_t)info.W * info.H, items = (size_t)info.H * 4u;
	DevBuf n_sky, d_stream, d_ranges, d_planes, d_flags;
	const auto drop = [&](int rc) {
		(void)dm::sync(s);
		n_sky.free_(), d_stream.free_(), d_ranges.free_(), d_planes.free_(), d_flags.free_();
		return rc;
	};
	int rc = n_sky.ensure(n * sizeof(f4));
	rc = rc ? rc : d_stream.ensure(bytes);
	rc = rc ? rc : d_ranges.ensure(info.ranges.size() * 4u);
	rc = rc ? rc : d_flags.ensure(items * 4u);
	if (info.rle_lines)
		rc = rc ? rc : d_planes.ensure(items * info.W);
	rc = rc ? rc : dm::h2d(d_stream.p, data, bytes, s);
	rc = rc ? rc : dm::h2d(d_ranges.p, info.ranges.data(), info.ranges.size() * 4u, s);
	if (rc)
		return drop(rc);
	rtk::SkyHdrView v;
	memset(&v, 0, sizeof(v));
	v.stream = d_stream.as<uint8_t>(), v.ranges = d_ranges.as<uint32_t>(), v.planes = d_planes.as<uint8_t>(), v.flags = d_flags.as<uint32_t>();
	v.out = n_sky.as<rtk::SkyF4>(), v.W = info.W, v.H = info.H, v.mods = flags;
	const auto run = [&](int kind, void (*launch)(const rtk::SkyHdrView &, void *)) {
		StageTimer t(c, KF_SKYLOAD, kind, s);
		launch(v, s);
		t.stop(1);
		return dm::last_launch_error();
	};
	std::vector<uint32_t> words;
	if (info.rle_lines) // (a file of flat scanlines has no planes to expand)
	{
		words.resize(items);
		rc = run(0, rtk::launch_skyhdr_planes);
	}
	rc = rc ? rc : run(1, rtk::launch_skyhdr_texels);
	if (!rc && info.rle_lines)
		rc = dm::d2h(words.data(), d_flags.p, items * 4u, s);
	rc = rc ? rc : dm::sync(s);
	if (rc)
		return drop(rc);
	for (size_t i = 0; i < words.size(); i++)
		if (words[i]) // (the walk refuses these streams: a flag here is the kernel disagreeing with it)
			return drop(set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s: scanline %zu: component %zu is corrupt (flags 0x%x)", who, i / 4u, i % 4u, words[i]));
	std::swap(c->d_sky, n_sky);
	drop(0);
	c->sky_w = info.W, c->sky_h = info.H;
	c->sky_version++;
	c->scene_dirty = true;
	return RFWHIP_OK;
}

extern "C" int rfwhip_read_sky(rfwhip_context *c, float *out_rgba, size_t cap_texels, uint32_t *width, uint32_t *height)
{
	CTX_ENTER(c);
	if (width)
		*width = c->sky_w;
	if (height)
		*height = c->sky_h;
	if (!out_rgba)
		return RFWHIP_OK; // (the sizes alone)
	const size_t n = (size_t)c->sky_w * c->sky_h;
	if (cap_texels < n)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_read_sky: %zu texels, room for %zu", n, cap_texels);
	RF_TRY(sync_all(c));
	return dm::d2h(out_rgba, c->d_sky.p, n * sizeof(f4), c->stream);
}

static int sky_table_on_device(rfwhip_context *c, const double *weights, uint32_t n, DevBuf &table, rtk::SkyTabRecord *record)
{
	void *const s = c->stream;
	const uint32_t nb1 = rtk::skytab_blocks(n), nb2 = rtk::skytab_blocks(nb1);
	DevBuf b_w, b_d, b_e, b_part, b_t1d, b_t1e, b_t2d, b_t2e, b_c1, b_c2, b_omega, b_rec;
	DevBuf *const all[12] = {&b_w, &b_d, &b_e, &b_part, &b_t1d, &b_t1e, &b_t2d, &b_t2e, &b_c1, &b_c2, &b_omega, &b_rec};
	const size_t need[12] = {(size_t)n * 8u, (size_t)n * 8u, (size_t)n * 8u, (size_t)nb1 * sizeof(rtk::SkyPartial), (size_t)nb1 * 8u, (size_t)nb1 * 8u,
							 (size_t)nb2 * 8u, (size_t)nb2 * 8u, (size_t)nb1 * 4u, (size_t)nb2 * 4u, weights ? 0u : (size_t)c->sky_h * 8u, sizeof(rtk::SkyTabRecord)};
	const auto drop = [&](int rc) {
		(void)dm::sync(s);
		for (DevBuf *b : all)
			b->free_();
		return rc;
	};
	int rc = table.ensure((size_t)n * sizeof(rtk::SkyAliasEntry));
	for (int k = 0; k < 12 && !rc; k++)
		rc = need[k] ? all[k]->ensure_exact(need[k]) : 0;
	std::vector<double> omega; // the rows' solid angles, as skysamp::build_alias has them: no device cos enters the numbers
	if (!rc && weights)
		rc = dm::h2d(b_w.p, weights, (size_t)n * 8u, s);
	else if (!rc)
	{
		const double pi = 3.14159265358979323846;
		omega.resize(c->sky_h);
		for (uint32_t j = 0; j < c->sky_h; j++)
			omega[j] = (2.0 * pi / c->sky_w) * (std::cos(pi * j / c->sky_h) - std::cos(pi * (j + 1) / c->sky_h));
		rc = dm::h2d(b_omega.p, omega.data(), omega.size() * 8u, s);
	}
	if (rc)
		return drop(rc);
	rtk::SkyTabView v;
	memset(&v, 0, sizeof(v));
	v.sky = weights ? nullptr : c->d_sky.as<rtk::SkyF4>(), v.omega = b_omega.as<double>(), v.W = weights ? 1u : c->sky_w;
	v.w = b_w.as<double>(), v.D = b_d.as<double>(), v.E = b_e.as<double>(), v.part = b_part.as<rtk::SkyPartial>();
	v.t1d = b_t1d.as<double>(), v.t1e = b_t1e.as<double>(), v.t2d = b_t2d.as<double>(), v.t2e = b_t2e.as<double>();
	v.c1 = b_c1.as<uint32_t>(), v.c2 = b_c2.as<uint32_t>(), v.rec = b_rec.as<rtk::SkyTabRecord>(), v.table = table.as<rtk::SkyAliasEntry>();
	v.n = n, v.nb1 = nb1, v.nb2 = nb2;
	void (*const chain[7])(const rtk::SkyTabView &, void *) = {rtk::launch_skytab_weights, rtk::launch_skytab_total, rtk::launch_skytab_scan_block,
																rtk::launch_skytab_scan_super, rtk::launch_skytab_scan_top, rtk::launch_skytab_scan_apply,
																rtk::launch_skytab_assign};
	for (int k = 0; k < 7 && !rc; k++)
	{
		StageTimer t(c, KF_SKYLOAD, 2 + k, s);
		chain[k](v, s);
		t.stop(1);
		rc = dm::last_launch_error();
	}
	rc = rc ? rc : dm::d2h(record, b_rec.p, sizeof(*record), s);
	return drop(rc);
}

extern "C" int rfwhip_read_sky_table(rfwhip_context *c, rfwhip_sky_alias *out, size_t cap_entries, size_t *entries, rfwhip_sky_table_record *record)
{
	CTX_ENTER(c);
	if (!c->sky_sampling)
		return set_error(RFWHIP_ERR_STATE, "rfwhip_read_sky_table: sky_sampling is off, there is no table");
	if (c->sky_stale || c->sky_table_of != c->sky_version || c->sky_table_by != c->sky_table)
		RF_TRY(update_sky_sampling(c));
	const size_t n = c->sky_total > 0.0 ? (size_t)c->sky_w * c->sky_h : 0u;
	if (entries)
		*entries = n;
	if (record)
		memcpy(record, &c->sky_record, sizeof(*record));
	if (!out || cap_entries < n || !n)
		return RFWHIP_OK; // (the count and the record alone)
	RF_TRY(sync_all(c));
	return dm::d2h(out, c->d_sky_alias.p, n * sizeof(rt::SkyAlias), c->stream);
}

extern "C" int rfwhip_sky_alias_from_weights(rfwhip_context *c, const double *weights, size_t n, rfwhip_sky_alias *table_out, rfwhip_sky_table_record *record_out)
{
	CTX_ENTER(c);
	if (!weights || !table_out || !record_out || !n)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_sky_alias_from_weights: null argument or no weights");
	if (n >= (1ull << 31))
		return set_error(RFWHIP_ERR_UNSUPPORTED, "rfwhip_sky_alias_from_weights: %zu weights (the table indexes 2^31)", n);
	RF_TRY(sync_all(c));
	DevBuf table;
	rtk::SkyTabRecord r;
	int rc = sky_table_on_device(c, weights, (uint32_t)n, table, &r);
	rc = rc ? rc : dm::d2h(table_out, table.p, n * sizeof(rt::SkyAlias), c->stream);
	table.free_();
	if (!rc)
		memcpy(record_out, &r, sizeof(r));
	return rc;
}

extern "C" int rfwhip_bloom_image(rfwhip_context *c, const float *rgba_in, float exposure, float *rgba_out)
{
	CTX_ENTER(c);
	if (!rgba_in || !rgba_out)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_bloom_image: null image");
	if (!(exposure >= 0.0f && exposure < INFINITY))
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_bloom_image: the exposure must be a finite number >= 0");
	if (!c->W)
		return set_error(RFWHIP_ERR_STATE, "no render target");
	RF_TRY(sync_all(c));
	const size_t px = (size_t)c->W * c->H;
	RF_TRY(c->d_present.ensure(px * sizeof(f4)));
	RF_TRY(bloom_ensure(c));
	RF_TRY(dm::h2d(c->d_present.p, rgba_in, px * sizeof(f4), c->stream));
	RF_TRY(dm::h2d(c->d_bloom_one.as<float>() + 1, &exposure, sizeof(float), c->stream));
	RF_TRY(bloom_chain(c, c->d_present.as<f4>(), c->d_bloom_one.as<float>() + 1, c->stream));
	RF_TRY(bloom_mark(c, c->stream));
	RF_TRY(dm::d2h(rgba_out, c->d_bloom_out.p, px * sizeof(f4), c->stream));
	return dm::sync(c->stream);
}

extern "C" int rfwhip_read_bloom_level(rfwhip_context *c, int level, float *out, size_t cap, uint32_t *w, uint32_t *h)
{
	CTX_ENTER(c);
	if (!c->W)
		return set_error(RFWHIP_ERR_STATE, "no render target");
	if (!c->bloom_ran)
		return set_error(RFWHIP_ERR_STATE, "rfwhip_read_bloom_level: no bloom chain has run");
	if (level < 1 || level > (int)c->bloom_ran)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_read_bloom_level: level %d, the last chain ran levels 1 .. %u", level, c->bloom_ran);
	uint32_t lw, lh;
	const size_t off = bloom_level_offset(c->W, c->H, (uint32_t)level, &lw, &lh);
	if (w)
		*w = lw;
	if (h)
		*h = lh;
	if (!out)
		return RFWHIP_OK; // (the size alone)
	if (cap < (size_t)lw * lh * 4u)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_read_bloom_level: level %d is %u x %u float4, room for %zu floats", level, lw, lh, cap);
	RF_TRY(sync_all(c));
	RF_TRY(dm::d2h(out, c->d_bloom_pyr.as<f4>() + off, (size_t)lw * lh * sizeof(f4), c->stream));
	return dm::sync(c->stream);
}

extern "C" int rfwhip_set_display_lut(rfwhip_context *c, const float *rgb, uint32_t n)
{
	CTX_ENTER(c);
	if (!rgb || n == 0u)
	{
		RF_TRY(sync_all(c)); // (a graded display kernel in flight reads the table)
		c->lut_host.clear(), c->lut_n = 0;
		c->d_grade_lut.free_();
		return RFWHIP_OK;
	}
	if (n < rtk::GR_LUT_MIN || n > rtk::GR_LUT_MAX)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_set_display_lut: the size must lie in [2, 65], got %u", n);
	const size_t count = (size_t)n * n * n;
	for (size_t i = 0; i < count * 3u; i++)
		if (!(rgb[i] >= -FLT_MAX && rgb[i] <= FLT_MAX))
			return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_set_display_lut: entry %zu is not finite", i / 3u);
	std::vector<float> wide(count * 4u);
	for (size_t i = 0; i < count; i++)
		wide[4 * i] = rgb[3 * i], wide[4 * i + 1] = rgb[3 * i + 1], wide[4 * i + 2] = rgb[3 * i + 2], wide[4 * i + 3] = 0.0f;
	// into a buffer of its own, swapped in once the copy has landed: a failure on the way leaves the old LUT whole
	DevBuf fresh;
	int rc = fresh.ensure(count * sizeof(f4));
	if (!rc)
		rc = dm::h2d(fresh.p, wide.data(), count * sizeof(f4), c->stream);
	if (!rc)
		rc = dm::sync(c->stream);
	if (!rc)
		rc = sync_all(c); // (a graded display kernel in flight reads the old table)
	if (rc)
	{
		fresh.free_();
		return rc;
	}
	std::swap(c->d_grade_lut.p, fresh.p), std::swap(c->d_grade_lut.cap, fresh.cap);
	fresh.free_();
	c->lut_host.assign(rgb, rgb + count * 3u), c->lut_n = n;
	return RFWHIP_OK;
}

// .cube text: "#" comments, TITLE, LUT_3D_SIZE n, DOMAIN_MIN 0 0 0 / DOMAIN_MAX 1 1 1, then n^3 lines of three numbers, red fastest
extern "C" int rfwhip_set_display_lut_cube(rfwhip_context *c, const char *text, size_t len)
{
	CTX_ENTER(c);
	if (!text)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_set_display_lut_cube: null text");
	const std::string all(text, len);
	std::vector<float> rgb;
	uint32_t n = 0u;
	size_t pos = 0, line_no = 0;
	while (pos < all.size())
	{
		size_t end = all.find('\n', pos);
		if (end == std::string::npos)
			end = all.size();
		std::string line = all.substr(pos, end - pos);
		pos = end + 1, line_no++;
		const size_t first = line.find_first_not_of(" \t\r");
		if (first == std::string::npos || line[first] == '#')
			continue;
		const size_t last = line.find_last_not_of(" \t\r");
		line = line.substr(first, last - first + 1);
		const size_t sp = line.find_first_of(" \t");
		const std::string word = line.substr(0, sp), rest = sp == std::string::npos ? "" : line.substr(sp + 1);
		if (word == "TITLE")
			continue;
		if (word == "LUT_1D_SIZE" || word == "LUT_1D_INPUT_RANGE")
			return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_set_display_lut_cube: line %zu: a 1D LUT is not supported", line_no);
		if (word == "LUT_3D_SIZE")
		{
			char *e = nullptr;
			const long v = strtol(rest.c_str(), &e, 10);
			while (e && (*e == ' ' || *e == '\t'))
				e++;
			if (n || !e || e == rest.c_str() || *e || v < (long)rtk::GR_LUT_MIN || v > (long)rtk::GR_LUT_MAX)
				return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_set_display_lut_cube: line %zu: LUT_3D_SIZE must be given once, a whole number in [2, 65]", line_no);
			n = (uint32_t)v;
			continue;
		}
		const bool dmin = word == "DOMAIN_MIN", dmax = word == "DOMAIN_MAX";
		float f[3];
		char tail = 0;
		const int got = sscanf((dmin || dmax) ? rest.c_str() : line.c_str(), "%f %f %f %c", &f[0], &f[1], &f[2], &tail);
		if (dmin || dmax)
		{
			const float want = dmin ? 0.0f : 1.0f;
			if (got != 3 || f[0] != want || f[1] != want || f[2] != want)
				return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_set_display_lut_cube: line %zu: the only domain accepted is DOMAIN_MIN 0 0 0 / DOMAIN_MAX 1 1 1", line_no);
			continue;
		}
		if (got != 3 || !((word[0] >= '0' && word[0] <= '9') || word[0] == '-' || word[0] == '+' || word[0] == '.'))
			return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_set_display_lut_cube: line %zu: not a keyword of a 3D LUT and not three numbers", line_no);
		if (!n)
			return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_set_display_lut_cube: line %zu: an entry in front of LUT_3D_SIZE", line_no);
		if (rgb.size() >= (size_t)n * n * n * 3u)
			return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_set_display_lut_cube: more than %u^3 entries", n);
		rgb.insert(rgb.end(), f, f + 3);
	}
	if (!n)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_set_display_lut_cube: no LUT_3D_SIZE");
	if (rgb.size() != (size_t)n * n * n * 3u)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_set_display_lut_cube: %zu entries, LUT_3D_SIZE %u needs %zu", rgb.size() / 3u, n, (size_t)n * n * n);
	return rfwhip_set_display_lut(c, rgb.data(), n);
}

extern "C" int rfwhip_get_display_lut(rfwhip_context *c, float *rgb, size_t cap, uint32_t *n)
{
	CTX_ENTER(c);
	if (n)
		*n = c->lut_n;
	if (!rgb)
		return RFWHIP_OK; // (the size alone)
	if (cap < c->lut_host.size())
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_get_display_lut: the LUT holds %zu floats, room for %zu", c->lut_host.size(), cap);
	if (!c->lut_host.empty())
		memcpy(rgb, c->lut_host.data(), c->lut_host.size() * sizeof(float));
	return RFWHIP_OK;
}

extern "C" int rfwhip_grade_colors(rfwhip_context *c, int which, size_t count, const float *rgb_in, float *rgb_out)
{
	CTX_ENTER(c);
	if (count && (!rgb_in || !rgb_out))
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_grade_colors: null colours");
	if (which != 0 && which != 1)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_grade_colors: which must be 0 (white balance, CDL, saturation) or 1 (the LUT), got %d", which);
	if (!c->W)
		return set_error(RFWHIP_ERR_STATE, "no render target");
	if (count == 0)
		return RFWHIP_OK;
	if (count >= (1ull << 30))
		return set_error(RFWHIP_ERR_UNSUPPORTED, "rfwhip_grade_colors: too many colours");
	RF_TRY(sync_all(c));
	DevBuf d_in, d_out;
	int rc = d_in.ensure(count * 3u * sizeof(float));
	if (!rc)
		rc = d_out.ensure(count * 3u * sizeof(float));
	if (!rc)
		rc = dm::h2d(d_in.p, rgb_in, count * 3u * sizeof(float), c->stream);
	if (!rc)
	{
		rtk::launch_kat_grade(grade_view(c, false), which, d_in.as<float>(), d_out.as<float>(), (uint32_t)count, c->stream);
		rc = dm::last_launch_error();
	}
	if (!rc)
		rc = dm::d2h(rgb_out, d_out.p, count * 3u * sizeof(float), c->stream);
	d_in.free_(), d_out.free_();
	return rc;
}

extern "C" int rfwhip_get_meter(rfwhip_context *c, rfwhip_meter_stats *stats)
{
	CTX_ENTER(c);
	if (!stats)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_get_meter: null stats");
	if (!c->W)
		return set_error(RFWHIP_ERR_STATE, "no render target");
	RF_TRY(sync_all(c));
	RF_TRY(meter_ensure(c, 0));
	return dm::d2h(stats, c->d_meter_rec.p, sizeof(*stats), c->stream);
}

extern "C" int rfwhip_read_meter_histogram(rfwhip_context *c, uint32_t *bins, uint32_t *excluded)
{
	CTX_ENTER(c);
	if (!bins)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_read_meter_histogram: null bins");
	if (!c->W)
		return set_error(RFWHIP_ERR_STATE, "no render target");
	RF_TRY(sync_all(c));
	RF_TRY(meter_ensure(c, 0));
	uint32_t h[rtk::MT_RECORD];
	RF_TRY(dm::d2h(h, c->d_meter_hist.p, sizeof(h), c->stream));
	memcpy(bins, h, rtk::MT_BINS * sizeof(uint32_t));
	if (excluded)
		*excluded = h[rtk::MT_BINS];
	return RFWHIP_OK;
}

extern "C" int rfwhip_meter_reset(rfwhip_context *c)
{
	CTX_ENTER(c);
	if (!c->W)
		return set_error(RFWHIP_ERR_STATE, "no render target");
	RF_TRY(sync_all(c));
	RF_TRY(meter_ensure(c, 0));
	RF_TRY(dm::h2d(c->d_meter_rec.p, &k_meter_fresh, sizeof(k_meter_fresh), c->stream));
	RF_TRY(dm::zero(c->d_meter_hist.p, rtk::MT_RECORD * sizeof(uint32_t), c->stream));
	c->meter_have = false, c->meter_manual_stale = true;
	return dm::sync(c->stream);
}

// the record and, where asked for, the histogram, after the step(s) enqueued on the context's stream
static int meter_answer(rfwhip_context *c, rfwhip_meter_stats *stats, uint32_t *bins)
{
	RF_TRY(dm::d2h(stats, c->d_meter_rec.p, sizeof(*stats), c->stream));
	if (bins)
		RF_TRY(dm::d2h(bins, c->d_meter_hist.p, rtk::MT_BINS * sizeof(uint32_t), c->stream));
	return RFWHIP_OK;
}

extern "C" int rfwhip_meter_image(rfwhip_context *c, const float *rgba_in, rfwhip_meter_stats *stats, uint32_t *bins)
{
	CTX_ENTER(c);
	if (!rgba_in || !stats)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_meter_image: null image or stats");
	if (!c->W)
		return set_error(RFWHIP_ERR_STATE, "no render target");
	RF_TRY(sync_all(c));
	const size_t px = (size_t)c->W * c->H;
	RF_TRY(c->d_present.ensure(px * sizeof(f4)));
	RF_TRY(dm::h2d(c->d_present.p, rgba_in, px * sizeof(f4), c->stream));
	RF_TRY(meter_step(c, c->d_present.as<f4>(), c->stream));
	return meter_answer(c, stats, bins);
}

extern "C" int rfwhip_meter_histogram(rfwhip_context *c, const uint32_t *bins, uint32_t excluded, rfwhip_meter_stats *stats)
{
	CTX_ENTER(c);
	if (!bins || !stats)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_meter_histogram: null bins or stats");
	if (!c->W)
		return set_error(RFWHIP_ERR_STATE, "no render target");
	unsigned long long total = 0;
	for (uint32_t b = 0; b < rtk::MT_BINS; b++)
		total += bins[b];
	if (total > 0xFFFFFFFFull)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_meter_histogram: the counts add up to %llu, more than 2^32 - 1", total);
	RF_TRY(sync_all(c));
	RF_TRY(meter_ensure(c, 0));
	uint32_t h[rtk::MT_RECORD] = {};
	memcpy(h, bins, rtk::MT_BINS * sizeof(uint32_t));
	h[rtk::MT_BINS] = excluded;
	RF_TRY(dm::h2d(c->d_meter_part.p, h, sizeof(h), c->stream)); // (posed as the one partial record of a pass)
	RF_TRY(meter_reduce(c, 1u, c->stream));
	return meter_answer(c, stats, nullptr);
}

// ---- noise estimate (settings "noise_*"; work items: noise.h) -----------------------------------------------------------------------
// the metric on `moments` (local layout of `rows` x W) for n samples per pixel: two launches on the context's stream and the 32-byte
// record back on the host; the error map and the tile records stay in d_noise_map / d_noise_tiles
// n_tile != null (adaptive sampling): n per tile
static int noise_metric(rfwhip_context *c, const float *moments, uint32_t W, uint32_t H, uint32_t rows, uint32_t rank, uint32_t world,
						uint32_t n, rtk::NoiseTotal *total, const uint32_t *n_tile = nullptr)
{
	const uint32_t tiles = rtk::noise_tiles_x(W) * (rows / rtk::NZ_TILE_Y);
	if (c->adaptive_live && (size_t)rows * W * sizeof(float) > c->d_noise_map.cap)
		RF_TRY(sync_all(c)); // (rfwhip_noise_image on a larger image: a decision call in flight writes these buffers)
	RF_TRY(c->d_noise_map.ensure((size_t)rows * W * sizeof(float)));
	RF_TRY(c->d_noise_tiles.ensure((size_t)tiles * sizeof(rtk::NoiseTile)));
	RF_TRY(c->d_noise_total.ensure(sizeof(rtk::NoiseTotal)));
	const rtk::NoiseView v = noise_view(c, moments, W, H, rows, rank, world, n);
	{
		StageTimer t(c, KF_NOISE, -1);
		if (n_tile)
			rtk::launch_noise_metric_adaptive(v, n_tile, true, c->stream);
		else
			rtk::launch_noise_metric(v, c->stream);
		t.stop(2);
	}
	RF_TRY(dm::last_launch_error());
	RF_TRY(dm::d2h(total, c->d_noise_total.p, sizeof(*total), c->stream));
	return dm::sync(c->stream);
}
static void noise_fill_stats(const rfwhip_context *c, const rtk::NoiseTotal &t, uint64_t samples, rfwhip_noise_stats *st)
{
	st->samples = samples, st->pixels = t.pixels, st->converged = t.converged;
	st->mean_error = t.pixels ? t.sum_e / (double)t.pixels : 0.0;
	st->max_error = t.max_e, st->threshold = c->noise_threshold;
}
// the metric on the context's own moments
static int noise_own(rfwhip_context *c, const char *who, rtk::NoiseTotal *total)
{
	if (!c->noise_estimate)
		return set_error(RFWHIP_ERR_STATE, "%s: noise_estimate is off", who);
	if (!c->noise_live)
		return set_error(RFWHIP_ERR_STATE, "%s: noise_estimate came on after the accumulation began; render with RFWHIP_RESET first", who);
	if (c->samples_done < 2u)
		return set_error(RFWHIP_ERR_STATE, "%s: %u samples per pixel, the estimate needs 2", who, c->samples_done);
	// (the last render's resolve is on the context's stream: the metric runs behind it)
	return noise_metric(c, c->d_noise.as<float>(), c->W, c->H, c->fr.local_rows, (uint32_t)c->rank, (uint32_t)c->world, c->samples_done, total,
						c->adaptive_live ? c->d_ad_n.as<uint32_t>() : nullptr);
}

extern "C" int rfwhip_get_noise(rfwhip_context *c, rfwhip_noise_stats *stats)
{
	CTX_ENTER(c);
	if (!stats)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "null stats");
	rtk::NoiseTotal t;
	RF_TRY(noise_own(c, "rfwhip_get_noise", &t));
	noise_fill_stats(c, t, c->samples_done, stats);
	return RFWHIP_OK;
}

extern "C" int rfwhip_read_noise_map(rfwhip_context *c, float *e)
{
	CTX_ENTER(c);
	if (!e)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "null map");
	if (c->world != 1)
		return set_error(RFWHIP_ERR_STATE, "rfwhip_read_noise_map: this rank owns 1/%d of the image", c->world);
	rtk::NoiseTotal t;
	RF_TRY(noise_own(c, "rfwhip_read_noise_map", &t));
	RF_TRY(dm::d2h(e, c->d_noise_map.p, (size_t)c->W * c->H * sizeof(float), c->stream)); // (world 1: local row = image row)
	return dm::sync(c->stream);
}

extern "C" int rfwhip_read_noise_tiles(rfwhip_context *c, rfwhip_noise_tile *records, size_t cap, uint32_t *tiles_x, uint32_t *tiles_y)
{
	CTX_ENTER(c);
	if (!records || !tiles_x || !tiles_y)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "null destination");
	const uint32_t tx = rtk::noise_tiles_x(c->W), ty = c->fr.local_rows / rtk::NZ_TILE_Y;
	if (c->noise_estimate && c->W && cap < (size_t)tx * ty)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_read_noise_tiles: room for %zu records, the context has %u x %u tiles", cap, tx, ty);
	rtk::NoiseTotal t;
	RF_TRY(noise_own(c, "rfwhip_read_noise_tiles", &t));
	*tiles_x = tx, *tiles_y = ty;
	RF_TRY(dm::d2h(records, c->d_noise_tiles.p, (size_t)tx * ty * sizeof(rtk::NoiseTile), c->stream));
	return dm::sync(c->stream);
}

extern "C" int rfwhip_read_noise_moments(rfwhip_context *c, float *sumY, float *m2)
{
	CTX_ENTER(c);
	if (!sumY || !m2)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "null destination");
	if (c->world != 1)
		return set_error(RFWHIP_ERR_STATE, "rfwhip_read_noise_moments: this rank owns 1/%d of the image", c->world);
	if (!c->noise_estimate || !c->noise_live)
		return set_error(RFWHIP_ERR_STATE, "rfwhip_read_noise_moments: %s", !c->noise_estimate ? "noise_estimate is off" : "noise_estimate came on after the accumulation began; render with RFWHIP_RESET first");
	const size_t px = (size_t)c->W * c->H;
	std::vector<float> both(px * 2u);
	RF_TRY(dm::d2h(both.data(), c->d_noise.p, px * 2u * sizeof(float), c->stream));
	RF_TRY(dm::sync(c->stream));
	for (size_t i = 0; i < px; i++)
		sumY[i] = both[2u * i], m2[i] = both[2u * i + 1u];
	return RFWHIP_OK;
}

extern "C" int rfwhip_noise_merge(rfwhip_context *c, size_t pixels, uint32_t n_a, const float *sumY_a, const float *m2_a, uint32_t S,
								  const float *samples_rgb, float *sumY_out, float *m2_out)
{
	CTX_ENTER(c);
	if (!sumY_a || !m2_a || !samples_rgb || !sumY_out || !m2_out)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "null array");
	if (!pixels || !S || pixels > (1u << 24) || S > 4096u)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_noise_merge: 1 .. 2^24 pixels and 1 .. 4096 samples, got %zu and %u", pixels, S);
	RF_TRY(sync_all(c));
	const size_t sb = pixels * S * 3u * sizeof(float), mb = pixels * 2u * sizeof(float);
	RF_TRY(c->d_noise_in.ensure(sb + mb));
	std::vector<float> both(pixels * 2u);
	for (size_t i = 0; i < pixels; i++)
		both[2u * i] = sumY_a[i], both[2u * i + 1u] = m2_a[i];
	float *d_samples = c->d_noise_in.as<float>(), *d_mom = d_samples + pixels * S * 3u;
	RF_TRY(dm::h2d(d_samples, samples_rgb, sb, c->stream));
	RF_TRY(dm::h2d(d_mom, both.data(), mb, c->stream));
	rtk::launch_noise_merge(d_samples, d_mom, (uint32_t)pixels, n_a, S, c->stream);
	RF_TRY(dm::last_launch_error());
	RF_TRY(dm::d2h(both.data(), d_mom, mb, c->stream));
	RF_TRY(dm::sync(c->stream));
	for (size_t i = 0; i < pixels; i++)
		sumY_out[i] = both[2u * i], m2_out[i] = both[2u * i + 1u];
	return RFWHIP_OK;
}

extern "C" int rfwhip_noise_image(rfwhip_context *c, uint32_t W, uint32_t H, uint32_t n, const float *sumY, const float *m2,
								  rfwhip_noise_stats *stats, float *e_map, rfwhip_noise_tile *tiles)
{
	CTX_ENTER(c);
	if (!sumY || !m2 || !stats)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "null array");
	if (!W || !H || W > 65536u || H > 65536u || (size_t)W * H > (1u << 26))
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_noise_image: bad size %ux%u", W, H);
	if (n < 2u)
		return set_error(RFWHIP_ERR_STATE, "rfwhip_noise_image: %u samples per pixel, the estimate needs 2", n);
	RF_TRY(sync_all(c));
	const uint32_t rows = (H + rt::STRIP_ROWS - 1) / rt::STRIP_ROWS * rt::STRIP_ROWS; // (a world-1 context's local rows)
	const size_t px = (size_t)W * H, lpx = (size_t)W * rows;
	std::vector<float> both(lpx * 2u, 0.0f);
	for (size_t i = 0; i < px; i++)
		both[2u * i] = sumY[i], both[2u * i + 1u] = m2[i];
	RF_TRY(c->d_noise_in.ensure(lpx * 2u * sizeof(float)));
	RF_TRY(dm::h2d(c->d_noise_in.p, both.data(), lpx * 2u * sizeof(float), c->stream));
	rtk::NoiseTotal t;
	RF_TRY(noise_metric(c, c->d_noise_in.as<float>(), W, H, rows, 0u, 1u, n, &t));
	noise_fill_stats(c, t, n, stats);
	if (e_map)
		RF_TRY(dm::d2h(e_map, c->d_noise_map.p, px * sizeof(float), c->stream));
	if (tiles)
		RF_TRY(dm::d2h(tiles, c->d_noise_tiles.p, (size_t)t.tiles * sizeof(rtk::NoiseTile), c->stream));
	return dm::sync(c->stream);
}

// ---- adaptive sampling (settings "adaptive_*"; work items: adaptive.h) --------------------------------------------------------------
static int adaptive_own(rfwhip_context *c, const char *who)
{
	if (!c->adaptive_live)
		return set_error(RFWHIP_ERR_STATE, "%s: %s", who, c->adaptive_sampling ? "adaptive_sampling came on after the accumulation began; render with RFWHIP_RESET first" : "adaptive_sampling is off");
	return RFWHIP_OK;
}
// the real pixels of noise tile (tx, ty) of this rank
static uint32_t adaptive_tile_pixels(const rfwhip_context *c, uint32_t tx, uint32_t ty)
{
	const uint32_t w = std::min(rtk::NZ_TILE_X, c->W - tx * rtk::NZ_TILE_X);
	uint32_t rows = 0;
	for (uint32_t r = 0; r < rtk::NZ_TILE_Y; r++)
	{
		const uint32_t yl = ty * rtk::NZ_TILE_Y + r;
		rows += rt::strip_of_local(yl / rt::STRIP_ROWS, (uint32_t)c->rank, (uint32_t)c->world) * rt::STRIP_ROWS + yl % rt::STRIP_ROWS < c->H;
	}
	return w * rows;
}
// the tiles' state as the last render call enqueued leaves it
static int adaptive_read(rfwhip_context *c, std::vector<uint32_t> &n, std::vector<unsigned char> &active)
{
	const uint32_t tiles = rtk::noise_tiles_x(c->W) * (c->fr.local_rows / rtk::NZ_TILE_Y);
	n.resize(tiles), active.resize(tiles);
	RF_TRY(dm::d2h(n.data(), c->d_ad_n.p, (size_t)tiles * 4u, c->stream));
	RF_TRY(dm::d2h(active.data(), c->d_ad_active.p, tiles, c->stream));
	return dm::sync(c->stream);
}

extern "C" int rfwhip_get_adaptive(rfwhip_context *c, rfwhip_adaptive_stats *stats)
{
	CTX_ENTER(c);
	if (!stats)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "null stats");
	RF_TRY(adaptive_own(c, "rfwhip_get_adaptive"));
	std::vector<uint32_t> n;
	std::vector<unsigned char> active;
	RF_TRY(adaptive_read(c, n, active));
	rfwhip_adaptive_stats st = {0, 0, 0, 0, 0, 0};
	const uint32_t ntx = rtk::noise_tiles_x(c->W);
	for (uint32_t t = 0; t < (uint32_t)n.size(); t++)
	{
		const uint64_t px = adaptive_tile_pixels(c, t % ntx, t / ntx);
		if (!px)
			continue; // (the padded rows below the image)
		st.tiles++, st.pixels += px, st.samples_taken += px * n[t];
		if (active[t])
			st.active_tiles++, st.active_pixels += px;
	}
	st.samples_uniform = st.pixels * c->samples_done;
	*stats = st;
	return RFWHIP_OK;
}

extern "C" int rfwhip_read_adaptive_tiles(rfwhip_context *c, uint32_t *n, uint8_t *active, size_t cap, uint32_t *tiles_x, uint32_t *tiles_y)
{
	CTX_ENTER(c);
	if (!n || !active || !tiles_x || !tiles_y)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "null destination");
	RF_TRY(adaptive_own(c, "rfwhip_read_adaptive_tiles"));
	const uint32_t tx = rtk::noise_tiles_x(c->W), ty = c->fr.local_rows / rtk::NZ_TILE_Y;
	if (cap < (size_t)tx * ty)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_read_adaptive_tiles: room for %zu tiles, the context has %u x %u", cap, tx, ty);
	std::vector<uint32_t> hn;
	std::vector<unsigned char> ha;
	RF_TRY(adaptive_read(c, hn, ha));
	memcpy(n, hn.data(), hn.size() * 4u), memcpy(active, ha.data(), ha.size());
	*tiles_x = tx, *tiles_y = ty;
	return RFWHIP_OK;
}

extern "C" int rfwhip_adaptive_set_tiles(rfwhip_context *c, const uint8_t *active, size_t count)
{
	CTX_ENTER(c);
	if (!active)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "null flags");
	RF_TRY(adaptive_own(c, "rfwhip_adaptive_set_tiles"));
	const rtk::AdaptiveView a = adaptive_view(c);
	if (count != a.count)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_adaptive_set_tiles: %zu flags, the context has %u tiles", count, a.count);
	RF_TRY(sync_all(c));
	std::vector<uint32_t> n;
	std::vector<unsigned char> cur;
	RF_TRY(adaptive_read(c, n, cur));
	// (flags only clear: a retired tile stays retired)
	std::vector<unsigned char> mask((size_t)a.tiles_x * (c->fr.local_rows / rt::TILE), 1);
	for (uint32_t t = 0; t < a.count; t++)
	{
		cur[t] = cur[t] && active[t];
		const uint32_t ty = t / a.ntx, sx = (t % a.ntx) * (rtk::NZ_TILE_X / rt::TILE);
		for (uint32_t k = 0; k < rtk::NZ_TILE_X / rt::TILE; k++)
			if (sx + k < a.tiles_x)
				mask[(size_t)ty * a.tiles_x + sx + k] = cur[t];
	}
	RF_TRY(dm::h2d(a.active, cur.data(), cur.size(), c->stream));
	RF_TRY(dm::h2d(a.mask, mask.data(), mask.size(), c->stream));
	RF_TRY(dm::sync(c->stream));
	c->adaptive_mask_moved = true; // (the next call's sub-batch streams wait for the main stream once more: plain order, nothing is in flight)
	return RFWHIP_OK;
}

extern "C" int rfwhip_read_local_framebuffer_device(rfwhip_context *c, void *rgba_device)
{
	CTX_ENTER(c);
	if (!rgba_device)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "null destination");
	if (!c->W)
		return set_error(RFWHIP_ERR_STATE, "no render target");
	RF_TRY(present(c, (f4 *)rgba_device, 0));
	return dm::sync(c->stream);
}

// Stream-ordered variants: nothing blocks the host.  The present runs on the CALLER's stream after everything this
// context has enqueued so far; the context's next render waits (on the device) until that present has read the
// accumulator.  With torch.distributed the caller passes torch's current stream, so the RCCL gather that follows is
// ordered behind the present by plain stream order, and the next frame's kernels overlap the gather.
extern "C" int rfwhip_read_local_framebuffer_stream(rfwhip_context *c, void *rgba_device, void *hip_stream)
{
	CTX_ENTER(c);
	if (!rgba_device)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "null destination");
	if (!c->W)
		return set_error(RFWHIP_ERR_STATE, "no render target");
	RF_TRY(ensure_sub_batches(c, 1)); // creates ev_present_in
	RF_TRY(dm::event_record(c->ev_present_in, c->stream));
	RF_TRY(dm::stream_wait_event(hip_stream, c->ev_present_in));
	rtk::Params p;
	fill_params(c, nullptr, p);
	const float scale = c->samples_done ? 1.0f / (float)c->samples_done : 0.0f;
	if (c->adaptive_live)
		rtk::launch_present_adaptive(p, (f4 *)rgba_device, adaptive_view(c), 0, hip_stream);
	else
		rtk::launch_present(p, (f4 *)rgba_device, scale, 0, hip_stream);
	RF_TRY(dm::last_launch_error());
	return c->marks[MK_PRESENT].record(hip_stream, true);
}

extern "C" int rfwhip_deinterleave_stream(rfwhip_context *c, const void *gathered_device, void *rgba_device, void *hip_stream)
{
	CTX_ENTER(c);
	if (!gathered_device || !rgba_device)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "null buffer");
	rtk::launch_deinterleave((const f4 *)gathered_device, (f4 *)rgba_device, c->W, c->H, local_rows_of(c), (uint32_t)c->world, hip_stream);
	return dm::last_launch_error();
}

extern "C" int rfwhip_get_placement(rfwhip_context *c, int *device_ordinal, int *rank, int *world)
{
	CTX_ENTER(c);
	if (device_ordinal)
		*device_ordinal = c->device;
	if (rank)
		*rank = c->rank;
	if (world)
		*world = c->world;
	return RFWHIP_OK;
}

extern "C" int rfwhip_get_target_size(rfwhip_context *c, uint32_t *width, uint32_t *height)
{
	CTX_ENTER(c);
	if (width)
		*width = c->W;
	if (height)
		*height = c->H;
	return RFWHIP_OK;
}

extern "C" int rfwhip_deinterleave_device(rfwhip_context *c, const void *gathered_device, void *rgba_device)
{
	CTX_ENTER(c);
	if (!gathered_device || !rgba_device)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "null buffer");
	rtk::launch_deinterleave((const f4 *)gathered_device, (f4 *)rgba_device, c->W, c->H, local_rows_of(c), (uint32_t)c->world, c->stream);
	RF_TRY(dm::last_launch_error());
	return dm::sync(c->stream);
}

// =================================================================================================================
// probe / stats / settings / hooks
// =================================================================================================================
extern "C" int rfwhip_set_probe_index(rfwhip_context *c, uint32_t x, uint32_t y)
{
	CTX_ENTER(c);
	c->probe_x = x, c->probe_y = y;
	return RFWHIP_OK;
}
extern "C" int rfwhip_get_probe_results(rfwhip_context *c, uint32_t *inst, uint32_t *prim, float *dist)
{
	CTX_ENTER(c);
	if (inst)
		*inst = c->probe_inst;
	if (prim)
		*prim = c->probe_prim;
	if (dist)
		*dist = c->probe_dist;
	return RFWHIP_OK;
}
extern "C" int rfwhip_get_stats(rfwhip_context *c, rfwhip_render_stats *stats)
{
	CTX_ENTER(c);
	if (!stats)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "null stats");
	*stats = c->stats;
	return RFWHIP_OK;
}

// =================================================================================================================
// settings: one row per key — how a value is parsed and stored (nothing: read-only), how it is printed, whether
// rfwhip_get_settings lists it.  rfwhip_set_setting / rfwhip_get_setting / rfwhip_get_settings are lookups in k_settings.
// =================================================================================================================
struct Setting
{
	const char *key;
	int (*set)(rfwhip_context *c, const char *key, const char *value); // nullptr: read-only, a set answers "unknown setting"
	int (*get)(rfwhip_context *c, char *out, size_t cap);
	bool listed;
};

// ---- the recurring row kinds (lenient ones parse with atoi: "abc" is 0) ----
static int set_enum2(int &dst, const char *key, const char *value, const char *name0, const char *name1)
{
	if (strcmp(value, name0) && strcmp(value, name1))
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s must be \"%s\" or \"%s\"", key, name0, name1);
	dst = !strcmp(value, name1);
	return RFWHIP_OK;
}
static int set_flag(int &dst, const char *value)
{
	dst = atoi(value) != 0;
	return RFWHIP_OK;
}
static int set_int_in(int &dst, const char *key, const char *value, int lo, int hi)
{
	const int n = atoi(value);
	if (n < lo || n > hi)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s must be in [%d, %d]", key, lo, hi);
	dst = n;
	return RFWHIP_OK;
}
static int set_whole_in(int &dst, const char *key, const char *value, long lo, long hi) // strict: the whole of `value` is one whole number in [lo, hi]
{
	char *end = nullptr;
	const long n = strtol(value, &end, 10);
	if (!end || *end || end == value || n < lo || n > hi)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s must be a whole number in [%ld, %ld]", key, lo, hi);
	dst = (int)n;
	return RFWHIP_OK;
}
static int parse_01(const char *key, const char *value, bool *on) // strict: exactly "0" or "1"
{
	if (strcmp(value, "0") && strcmp(value, "1"))
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s must be \"0\" or \"1\"", key);
	*on = value[0] == '1';
	return RFWHIP_OK;
}
// strict: the whole of `value` is one number that `ok` accepts ("" reads as 0 unless the row refuses it); `must` completes
// "<key> must ..."
static int set_float(float &dst, const char *key, const char *value, bool (*ok)(float), const char *must, bool empty_is_zero = true)
{
	char *end = nullptr;
	const float f = strtof(value, &end);
	if (!end || *end || (end == value && !empty_is_zero) || !ok(f))
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s must %s", key, must);
	dst = f;
	return RFWHIP_OK;
}
// strict: one number for the three channels, or three separated by blanks; every one must pass `ok`, else nothing changes
static int set_float3(float dst[3], const char *key, const char *value, bool (*ok)(float), const char *must)
{
	float f[3];
	int n = 0;
	const char *p = value;
	for (; n < 3; n++)
	{
		while (*p == ' ' || *p == '\t')
			p++;
		if (!*p)
			break;
		char *end = nullptr;
		f[n] = strtof(p, &end);
		if (!end || end == p || !ok(f[n]))
			return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s must %s", key, must);
		p = end;
	}
	while (*p == ' ' || *p == '\t')
		p++;
	if (*p || (n != 1 && n != 3))
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s must %s", key, must);
	for (int i = 0; i < 3; i++)
		dst[i] = f[n == 1 ? 0 : i];
	return RFWHIP_OK;
}
static int set_sigma(float &dst, const char *key, const char *value)
{
	return set_float(dst, key, value, [](float f) { return f >= 0.0f && f < 1e30f; }, "be a finite number >= 0");
}
// denoise_temporal / denoise_motion: turning one on clears the history, traces the guides again with what the stage needs
// and, where `ensure` says the stage will run, (re)allocates its buffers
static int set_denoise_stage(rfwhip_context *c, int &stage, const char *key, const char *value, bool (*ensure)(const rfwhip_context *))
{
	bool on;
	RF_TRY(parse_01(key, value, &on));
	if (on && !stage)
	{
		RF_TRY(sync_all(c)); // (a stage in flight may still read the buffers this reallocates)
		stage = 1;
		dn_clear_history(c);
		c->guides_valid = false;
		if (ensure(c))
			RF_TRY(dn_ensure(c));
	}
	stage = on;
	return RFWHIP_OK;
}
// display_exposure*: the record's E (manual mode) and the frame rfwhip_read_display* metered are those of the old settings
static int exposure_changed(rfwhip_context *c)
{
	c->meter_have = false, c->meter_manual_stale = true;
	return RFWHIP_OK;
}
// one end of an ordered pair (display_exposure_low < _high in [0, 1]; _min_ev <= _max_ev in [-64, 64]): a value that breaks the
// range or the order is refused and both ends keep their values
static int set_exposure_pair(rfwhip_context *c, float &lo, float &hi, bool set_lo, const char *key, const char *value, const char *must)
{
	const bool window = &lo == &c->exposure_low;
	float f = 0.0f;
	RF_TRY(set_float(f, key, value, [](float x) { return x >= -64.0f && x <= 64.0f; }, must, false));
	const float nlo = set_lo ? f : lo, nhi = set_lo ? hi : f;
	if (window ? !(f >= 0.0f && f <= 1.0f && nlo < nhi) : !(nlo <= nhi))
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s must %s", key, must);
	lo = nlo, hi = nhi;
	return exposure_changed(c);
}
static int put(char *out, size_t cap, const char *fmt, ...) __attribute__((format(printf, 3, 4)));
static int put(char *out, size_t cap, const char *fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(out, cap, fmt, ap);
	va_end(ap);
	return RFWHIP_OK;
}
// a family's table as its *_time setting prints it: the milliseconds by kernel, then the launches, one space between any two
static int put_kind_times(char *out, size_t cap, const KindTimes &t)
{
	char line[640]; // (9 floats of at most 47 characters, 9 counts of at most 10, the spaces)
	int at = 0;
	for (int k = 0; k < t.count; k++)
		at += snprintf(line + at, sizeof(line) - (size_t)at, "%.6f ", t.ms[k]);
	for (int k = 0; k < t.count; k++)
		at += snprintf(line + at, sizeof(line) - (size_t)at, k + 1 < t.count ? "%u " : "%u", t.launches[k]);
	return put(out, cap, "%s", line);
}

#define SET [](rfwhip_context * c, const char *key, const char *value) -> int
#define GET [](rfwhip_context * c, char *out, size_t cap) -> int
#define GET_INT(member) GET { return put(out, cap, "%d", c->member); }
#define ENUM2(member, name0, name1) SET { return set_enum2(c->member, key, value, name0, name1); }, GET { return put(out, cap, "%s", c->member ? name1 : name0); }
#define FLAG(member) SET { return set_flag(c->member, value); }, GET_INT(member)
#define INT_IN(member, lo, hi) SET { return set_int_in(c->member, key, value, lo, hi); }, GET_INT(member)
#define SIGMA(member) SET { return set_sigma(c->member, key, value); }, GET { return put(out, cap, "%g", c->member); }
static const Setting k_settings[] = {
	// ---- listed by rfwhip_get_settings, in this order ----
	{"integrator", SET {
		 if (set_enum2(c->integrator, key, value, "parity", "pt"))
			 return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "integrator must be \"parity\" or \"pt\", got \"%s\"", value);
		 return RFWHIP_OK; },
	 GET { return put(out, cap, "%s", c->integrator ? "pt" : "parity"); }, true},
	{"spp", INT_IN(spp, 1, 4096), true},
	{"max_depth", INT_IN(max_depth, 0, rt::MAX_DEPTH_SLOTS - 2), true},
	{"jitter", ENUM2(jitter, "xor128", "center"), true},
	{"stage_timing", FLAG(stage_timing), true},
	{"count_traversal", FLAG(count_traversal), true},
	{"lds_nodes", SET { c->lds_nodes = std::max(-1, atoi(value)); return RFWHIP_OK; }, GET_INT(lds_nodes), true},
	{"refill", SET { c->refill = atoi(value) & 15; return RFWHIP_OK; }, GET_INT(refill), true},
	{"streams", INT_IN(streams, 1, rfwhip_context::MAX_SUB), true},
	{"sampler", ENUM2(sampler, "hash", "bluenoise"), true},
	{"builder", ENUM2(builder, "host", "device"), true},
	{"overlap", SET {
		 if (set_int_in(c->overlap, key, value, -1, 1))
			 return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "overlap must be -1 (by launch size), 0 or 1");
		 return RFWHIP_OK; },
	 GET_INT(overlap), true},
	{"sub_batch_paths", SET {
		 const long long n = atoll(value);
		 if (n < 1)
			 return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "sub_batch_paths must be >= 1");
		 c->sub_batch_paths = n;
		 return RFWHIP_OK; },
	 GET { return put(out, cap, "%lld", c->sub_batch_paths); }, true},
	{"ring", INT_IN(ring, 1, rfwhip_context::MAX_RING), true},
	{"sample_group", SET {
		 const int n = atoi(value);
		 if (n < 1 || n > 64 || (n & (n - 1)))
			 return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "sample_group must be a power of two in [1, 64]");
		 c->sample_group = n;
		 return RFWHIP_OK; },
	 GET_INT(sample_group), true},
	{"flat_instances", SET {
		 c->scene_dirty = true; // takes effect with the next rfwhip_update()
		 return set_flag(c->flat_instances, value); },
	 GET_INT(flat_instances), true},
	{"flatten_bytes", SET {
		 c->flatten_bytes = std::max(0ll, atoll(value));
		 c->scene_dirty = true;
		 return RFWHIP_OK; },
	 GET { return put(out, cap, "%lld", c->flatten_bytes); }, true},
	{"fuse", FLAG(fuse), true},
	{"shadow_packets", SET {
		 const int v = atoi(value);
		 c->shadow_packets = v < 0 ? -1 : (v != 0);
		 c->shadow_packets_auto_on = true;
		 return RFWHIP_OK; },
	 GET_INT(shadow_packets), true},
	{"shadow_side", FLAG(shadow_side), true},
	{"group_flags", FLAG(group_flags), true},
	{"denoise", SET {
		 bool on;
		 RF_TRY(parse_01(key, value, &on));
		 if (on && c->W && c->rank == 0) // (the root filters the gathered image; other ranks never do)
			 RF_TRY(dn_ensure(c)); // (buffers of the full image: allocated when the setting is first turned on)
		 if (on && !c->denoise)
			 dn_clear_history(c);
		 c->denoise = on;
		 return RFWHIP_OK; },
	 GET_INT(denoise), true},
	{"denoise_iterations", INT_IN(dn_iterations, 1, 8), true},
	{"denoise_sigma_luminance", SIGMA(dn_sigma_l), true},
	{"denoise_sigma_normal", SIGMA(dn_sigma_n), true},
	{"denoise_sigma_depth", SIGMA(dn_sigma_z), true},
	{"denoise_temporal", SET { // (guides: traced again with the instance ids)
		 return set_denoise_stage(c, c->dn_temporal, key, value, [](const rfwhip_context *c) { return c->W && c->rank == 0; }); },
	 GET_INT(dn_temporal), true},
	{"denoise_alpha", SET { return set_float(c->dn_alpha, key, value, [](float f) { return f > 0.0f && f <= 1.0f; }, "be in (0, 1]"); },
	 GET { return put(out, cap, "%g", c->dn_alpha); }, true},
	{"sky_sampling", SET {
		 bool on;
		 RF_TRY(parse_01(key, value, &on));
		 c->sky_sampling = on;
		 c->sky_stale = true; // (the next render builds the table, on the sky of the last rfwhip_update)
		 return RFWHIP_OK; },
	 GET_INT(sky_sampling), true},
	{"sky_pick", SET {
		 RF_TRY(set_float(c->sky_pick, key, value, [](float f) { return f == -1.0f || (f >= 0.0f && f <= 1.0f); },
						  "be -1 (auto) or a probability in [0, 1]", false));
		 c->sky_stale = true;
		 return RFWHIP_OK; },
	 GET { return put(out, cap, "%g", c->sky_pick); }, true},
	{"denoise_motion", SET { // (guides: traced again with the surface record)
		 return set_denoise_stage(c, c->dn_motion, key, value, [](const rfwhip_context *c) { return c->W && c->rank == 0 && c->dn_temporal; }); },
	 GET_INT(dn_motion), true},
	// ---- unlisted ----
	// (self-arming primary kernels: round 4's switch, removed with the variant in round 5 — accepted and ignored, like refill bit 2)
	{"arm", SET { return RFWHIP_OK; }, GET { return put(out, cap, "0"); }, false},
	// read-only: would the next large pt call take the packet form of the depth-0 connection wave?
	{"shadow_packets_on", nullptr, GET { return put(out, cap, "%d", (c->shadow_packets > 0 || (c->shadow_packets < 0 && c->shadow_packets_auto_on)) && c->packet_ok && c->nodes4f_current && (c->refill & 8) ? 1 : 0); }, false},
	// the primary wave's entry snapshot (primary_entry.h): 1 wherever the camera-ordered table is used, without a lens and without
	// count_traversal (primary_entry_wanted; no value forces it where those fail); -1 there too, where the pass pays: calls of 720
	// paths per record or more, and smaller ones from the second call with the same view on (ensure_primary_entry); 0 never
	{"primary_entry", SET {
		 const int v = atoi(value);
		 c->primary_entry = v < 0 ? -1 : (v != 0);
		 return RFWHIP_OK; },
	 GET_INT(primary_entry), false},
	// read-only: did the primary wave of the last render call start from the snapshot?
	{"primary_entry_on", nullptr, GET { return put(out, cap, "%d", c->primary_entry_last ? 1 : 0); }, false},
	// read-only: light bins per sorted run of the last waited frames, see shadow_packets
	{"shadow_bins_per_run", nullptr, GET { return put(out, cap, "%.3f", c->shadow_bins_per_run); }, false},
	// read-only: which kernel variants the render calls launch (for hosts that label their measurements: bench.py)
	{"textured", nullptr, GET { return put(out, cap, "%d", c->textured ? 1 : 0); }, false}, // some material carries a texture / normal map: k_shade_pt<true>
	// material maps: the alpha mask of slot 9 and the roughness / metallic maps of slots 7 / 6 in the pt
	// integrator.  A change makes the guides stale: the guide pass honours the mask
	{"material_maps", SET {
		 bool on;
		 RF_TRY(parse_01(key, value, &on));
		 if ((int)on != c->material_maps)
			 c->guides_valid = false;
		 c->material_maps = on;
		 return RFWHIP_OK; },
	 GET_INT(material_maps), false},
	// read-only: the next render's pt shade waves run k_shade_pt_maps (the setting is on and some material has such a map)
	{"material_maps_on", nullptr, GET { return put(out, cap, "%d", material_maps_on(c) ? 1 : 0); }, false},
	// the pt primary wave runs in packet form (k_primary_packet) for sample groups >= 2 or large launches
	{"packet", nullptr, GET { return put(out, cap, "%d", (c->packet_ok && (c->refill & 8)) ? 1 : 0); }, false},
	// triangles in the world tree of the last rfwhip_update (0: none)
	{"world_tree", nullptr, GET { return put(out, cap, "%zu", c->wtree.valid ? c->wtree.tris : (size_t)0); }, false},
	// how a next-event vertex picks its light and weights it: reference = the reference's estimator (the
	// default kernels), linear = its potentials with consistent weights, tree = the light tree with the same weights
	{"light_sampling", SET {
		 static const char *const names[] = {"reference", "linear", "tree"};
		 int mode = -1;
		 for (int k = 0; k < 3; k++)
			 if (!strcmp(value, names[k]))
				 mode = k;
		 if (mode < 0)
			 return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s must be \"reference\", \"linear\" or \"tree\"", key);
		 c->light_sampling = mode;
		 c->lt_stale = true; // (the next render builds or drops the tree, on the lights of the last rfwhip_set_lights)
		 return RFWHIP_OK; },
	 GET { return put(out, cap, "%s", c->light_sampling == 2 ? "tree" : c->light_sampling == 1 ? "linear" : "reference"); }, false},
	// the display stage (display.h): what rfwhip_read_display* / rfwhip_display_* apply to the presented image
	{"display_tonemap", ENUM2(display_tonemap, "aces", "none"), false},
	{"display_fxaa", SET {
		 bool on;
		 RF_TRY(parse_01(key, value, &on));
		 c->display_fxaa = on;
		 return RFWHIP_OK; },
	 GET_INT(display_fxaa), false},
	{"display_srgb", SET {
		 bool on;
		 RF_TRY(parse_01(key, value, &on));
		 c->display_srgb = on;
		 return RFWHIP_OK; },
	 GET_INT(display_srgb), false},
	// the exposure meter (metering.h): how rfwhip_read_display* / rfwhip_display_* expose the image they show.
	// A change of any of them makes the next read of the same frame meter it again
	{"display_exposure", SET {
		 RF_TRY(set_enum2(c->exposure_auto, key, value, "manual", "auto"));
		 return exposure_changed(c); },
	 GET { return put(out, cap, "%s", c->exposure_auto ? "auto" : "manual"); }, false},
	{"display_exposure_ev", SET {
		 RF_TRY(set_float(c->exposure_ev, key, value, [](float f) { return f >= -32.0f && f <= 32.0f; }, "be a finite number in [-32, 32]", false));
		 return exposure_changed(c); },
	 GET { return put(out, cap, "%g", c->exposure_ev); }, false},
	{"display_exposure_key", SET {
		 RF_TRY(set_float(c->exposure_key, key, value, [](float f) { return f > 0.0f && f < 1e30f; }, "be a finite number > 0", false));
		 return exposure_changed(c); },
	 GET { return put(out, cap, "%g", c->exposure_key); }, false},
	{"display_exposure_low", SET { return set_exposure_pair(c, c->exposure_low, c->exposure_high, true, key, value, "be in [0, 1] and below display_exposure_high"); },
	 GET { return put(out, cap, "%g", c->exposure_low); }, false},
	{"display_exposure_high", SET { return set_exposure_pair(c, c->exposure_low, c->exposure_high, false, key, value, "be in [0, 1] and above display_exposure_low"); },
	 GET { return put(out, cap, "%g", c->exposure_high); }, false},
	{"display_exposure_speed", SET {
		 RF_TRY(set_float(c->exposure_speed, key, value, [](float f) { return f > 0.0f && f <= 1.0f; }, "be in (0, 1]", false));
		 return exposure_changed(c); },
	 GET { return put(out, cap, "%g", c->exposure_speed); }, false},
	{"display_exposure_min_ev", SET { return set_exposure_pair(c, c->exposure_min_ev, c->exposure_max_ev, true, key, value, "be a finite number in [-64, 64], at most display_exposure_max_ev"); },
	 GET { return put(out, cap, "%g", c->exposure_min_ev); }, false},
	{"display_exposure_max_ev", SET { return set_exposure_pair(c, c->exposure_min_ev, c->exposure_max_ev, false, key, value, "be a finite number in [-64, 64], at least display_exposure_min_ev"); },
	 GET { return put(out, cap, "%g", c->exposure_max_ev); }, false},
	// bloom (bloom.h): the glow pyramid rfwhip_read_display* / rfwhip_display_* add in front of the tone map
	{"display_bloom", SET {
		 bool on;
		 RF_TRY(parse_01(key, value, &on));
		 c->bloom_on = on;
		 return on && c->W ? bloom_ensure(c) : RFWHIP_OK; },
	 GET_INT(bloom_on), false},
	{"display_bloom_intensity", SET { return set_float(c->bloom_intensity, key, value, [](float f) { return f >= 0.0f && f <= 16.0f; }, "be in [0, 16]", false); },
	 GET { return put(out, cap, "%g", c->bloom_intensity); }, false},
	{"display_bloom_threshold", SET { return set_float(c->bloom_threshold, key, value, [](float f) { return f >= 0.0f && f < 1e30f; }, "be a finite number >= 0", false); },
	 GET { return put(out, cap, "%g", c->bloom_threshold); }, false},
	{"display_bloom_knee", SET { return set_float(c->bloom_knee, key, value, [](float f) { return f >= 0.0f && f <= 1.0f; }, "be in [0, 1]", false); },
	 GET { return put(out, cap, "%g", c->bloom_knee); }, false},
	{"display_bloom_scatter", SET { return set_float(c->bloom_scatter, key, value, [](float f) { return f >= 0.0f && f <= 1.0f; }, "be in [0, 1]", false); },
	 GET { return put(out, cap, "%g", c->bloom_scatter); }, false},
	{"display_bloom_levels", SET {
		 char *end = nullptr;
		 const long n = strtol(value, &end, 10);
		 if (!end || *end || end == value || n < 1 || n > (long)BLOOM_MAX_LEVELS)
			 return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s must be a whole number in [1, 8]", key);
		 c->bloom_levels = (int)n;
		 return RFWHIP_OK; },
	 GET_INT(bloom_levels), false},
	// (read-only, stage_timing = 1) family 12 by kernel since its last reset: the milliseconds of k_bloom_down0, k_bloom_down,
	// k_bloom_up, k_bloom_apply, then their launches
	{"display_bloom_time", nullptr, GET { return put_kind_times(out, cap, c->bloom_times); }, false},
	// colour grading and dither (display_grade.h): k_display_graded in place of the display kernel
	{"display_grade", SET {
		 bool on;
		 RF_TRY(parse_01(key, value, &on));
		 c->grade_on = on;
		 return RFWHIP_OK; },
	 GET_INT(grade_on), false},
	{"display_wb_temperature", SET {
		 float t = 0.0f;
		 RF_TRY(set_float(t, key, value, [](float f) { return f >= 1667.0f && f <= 25000.0f; }, "be a temperature in kelvin in [1667, 25000]", false));
		 c->grade_temperature = t;
		 grade_wb_matrix((double)t, c->grade_wb);
		 return RFWHIP_OK; },
	 GET { return put(out, cap, "%g", c->grade_temperature); }, false},
	{"display_grade_slope", SET { return set_float3(c->grade_slope, key, value, [](float f) { return f >= 0.0f && f <= FLT_MAX; }, "be one or three finite numbers >= 0"); },
	 GET { return put(out, cap, "%g %g %g", c->grade_slope[0], c->grade_slope[1], c->grade_slope[2]); }, false},
	{"display_grade_offset", SET { return set_float3(c->grade_offset, key, value, [](float f) { return f >= -FLT_MAX && f <= FLT_MAX; }, "be one or three finite numbers"); },
	 GET { return put(out, cap, "%g %g %g", c->grade_offset[0], c->grade_offset[1], c->grade_offset[2]); }, false},
	{"display_grade_power", SET { return set_float3(c->grade_power, key, value, [](float f) { return f > 0.0f && f <= FLT_MAX; }, "be one or three finite numbers > 0"); },
	 GET { return put(out, cap, "%g %g %g", c->grade_power[0], c->grade_power[1], c->grade_power[2]); }, false},
	{"display_grade_saturation", SET { return set_float(c->grade_sat, key, value, [](float f) { return f >= 0.0f && f <= 4.0f; }, "be in [0, 4]", false); },
	 GET { return put(out, cap, "%g", c->grade_sat); }, false},
	{"display_dither", SET {
		 bool on;
		 RF_TRY(parse_01(key, value, &on));
		 c->grade_dither = on;
		 return RFWHIP_OK; },
	 GET_INT(grade_dither), false},
	// (read-only) the size n of the LUT of rfwhip_set_display_lut, 0 without one
	{"display_lut", nullptr, GET { return put(out, cap, "%u", c->lut_n); }, false},
	// (read-only, stage_timing = 1) family 13 since its last reset: the milliseconds of k_display_graded, then its launches
	{"display_grade_time", nullptr, GET { return put(out, cap, "%.6f %u", c->kernel_ms[KF_GRADE], c->kernel_launches[KF_GRADE]); }, false},
	// baseline JPEG (display_jpeg.h): strict whole numbers; a refused value leaves the setting as it was
	{"display_jpeg_quality", SET { return set_whole_in(c->jpeg_quality, key, value, 1, 100); }, GET_INT(jpeg_quality), false},
	{"display_jpeg_subsampling", SET { return set_enum2(c->jpeg_sub, key, value, "444", "420"); },
	 GET { return put(out, cap, "%s", c->jpeg_sub ? "420" : "444"); }, false},
	{"display_jpeg_restart", SET { return set_whole_in(c->jpeg_restart, key, value, 1, 65535); }, GET_INT(jpeg_restart), false},
	// (read-only) the length of the last stream this library read back (rfwhip_read_display_jpeg, rfwhip_jpeg_image), 0 before
	{"display_jpeg_bytes", nullptr, GET { return put(out, cap, "%u", c->jpeg_rec_host.bytes); }, false},
	// (read-only, stage_timing = 1) family 14 by kernel since its last reset: the milliseconds of k_jpeg_blocks, k_jpeg_entropy,
	// k_jpeg_offsets, k_jpeg_pack, then their launches
	{"display_jpeg_time", nullptr, GET { return put_kind_times(out, cap, c->jpeg_times); }, false},
	// image textures (texture_decode.h): which side decodes the entropy data; auto = the device when the stream
	// has restart intervals, the host when it has none
	{"texture_entropy", SET {
		 const int k = !strcmp(value, "auto") ? 0 : !strcmp(value, "host") ? 1 : !strcmp(value, "device") ? 2 : -1;
		 if (k < 0)
			 return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s must be auto, host or device", key);
		 c->td_entropy = k;
		 return RFWHIP_OK; },
	 GET { return put(out, cap, "%s", c->td_entropy == 1 ? "host" : c->td_entropy == 2 ? "device" : "auto"); }, false},
	// (read-only, stage_timing = 1) family 15 by kernel since its last reset: the milliseconds of k_texdec_zero, k_texdec_entropy,
	// k_texdec_idct, k_texdec_color, k_tex_mips, k_texdec_finish, then their launches
	{"texture_decode_time", nullptr, GET { return put_kind_times(out, cap, c->texdec_times); }, false},
	// the sky's loaders (sky_load.h): who builds the alias table of sky_sampling; a change rebuilds it
	{"sky_table", SET {
		 const int k = !strcmp(value, "host") ? 0 : !strcmp(value, "device") ? 1 : -1;
		 if (k < 0)
			 return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s must be host or device", key);
		 c->sky_table = k;
		 c->sky_stale = true;
		 return RFWHIP_OK; },
	 GET { return put(out, cap, "%s", c->sky_table == 1 ? "device" : "host"); }, false},
	// (read-only, stage_timing = 1) family 17 by kernel since its last reset: the milliseconds of k_skyhdr_planes, k_skyhdr_texels,
	// k_skytab_weights, k_skytab_total, k_skytab_scan_block, k_skytab_scan_super, k_skytab_scan_top, k_skytab_scan_apply,
	// k_skytab_assign, then their launches
	{"sky_load_time", nullptr, GET { return put_kind_times(out, cap, c->skyload_times); }, false},
	// the noise estimate (noise.h): the moments beside the accumulator and the two definitions of the metric
	{"noise_estimate", SET {
		 bool on;
		 RF_TRY(parse_01(key, value, &on));
		 if (!on && (c->adaptive_sampling || c->adaptive_live))
			 return set_error(RFWHIP_ERR_STATE, c->adaptive_sampling ? "noise_estimate: adaptive_sampling is on and needs it; turn that off first"
																	 : "noise_estimate: the accumulation is an adaptive one; render with RFWHIP_RESET first");
		 if (!on && c->noise_estimate)
		 {
			 RF_TRY(sync_all(c)); // (a resolve in flight may still write the moments)
			 c->d_noise.free_(), c->d_noise_map.free_(), c->d_noise_tiles.free_(), c->d_noise_total.free_();
			 c->noise_live = false;
		 }
		 c->noise_estimate = on; // (on: the moments begin with the next RESET or rfwhip_init)
		 return RFWHIP_OK; },
	 GET_INT(noise_estimate), false},
	// adaptive sampling (adaptive.h); on and off with the next RESET or rfwhip_init
	{"adaptive_sampling", SET {
		 bool on;
		 RF_TRY(parse_01(key, value, &on));
		 if (on && !c->noise_estimate)
			 return set_error(RFWHIP_ERR_STATE, "adaptive_sampling needs noise_estimate=1");
		 c->adaptive_sampling = on;
		 return RFWHIP_OK; },
	 GET_INT(adaptive_sampling), false},
	{"adaptive_min_samples", SET { return set_int_in(c->adaptive_min_samples, key, value, 2, 1 << 30); }, GET_INT(adaptive_min_samples), false},
	{"adaptive_every", SET { return set_int_in(c->adaptive_every, key, value, 1, 64); }, GET_INT(adaptive_every), false},
	{"noise_floor", SET { return set_float(c->noise_floor, key, value, [](float f) { return f > 0.0f && f < 1e30f; }, "be a finite number > 0", false); },
	 GET { return put(out, cap, "%g", c->noise_floor); }, false},
	{"noise_threshold", SET { return set_float(c->noise_threshold, key, value, [](float f) { return f > 0.0f && f < 1e30f; }, "be a finite number > 0", false); },
	 GET { return put(out, cap, "%g", c->noise_threshold); }, false},
	// moving emitters (light_follow.h): rfwhip_update derives the bound area lights on the device and refits the tree
	{"lights_follow_geometry", SET {
		 bool on;
		 RF_TRY(parse_01(key, value, &on));
		 if (on && !c->lights_follow)
			 c->lf_dirty = true; // (turned on: the next rfwhip_update refreshes)
		 c->lights_follow = on;
		 return RFWHIP_OK; },
	 GET_INT(lights_follow), false},
	// read-only: bound area lights at the last refresh (0 while the setting is off); refits of the light tree since it was built
	{"lights_bound", nullptr, GET { return put(out, cap, "%u", c->lights_follow ? c->lights_bound : 0u); }, false},
	{"light_tree_refits", nullptr, GET { return put(out, cap, "%u", c->lt_refits); }, false},
	// read-only: nodes of the light tree the next render would use (0: none, or light_sampling is not tree)
	{"light_tree", nullptr, GET {
		 if (c->lt_stale)
			 RF_TRY(update_light_tree(c));
		 return put(out, cap, "%u", c->lt_view.node_count); },
	 false},
	// read-only: p > 0, the pt shade waves run k_shade_pt_sky
	{"sky", nullptr, GET {
		 if (c->sky_stale && !c->scene_dirty)
			 RF_TRY(update_sky_sampling(c));
		 return put(out, cap, "%d", c->sky_view.pick > 0.0f ? 1 : 0); },
	 false},
};
#undef SET
#undef GET
#undef GET_INT
#undef ENUM2
#undef FLAG
#undef INT_IN
#undef SIGMA

static const Setting *find_setting(const char *key)
{
	for (const Setting &s : k_settings)
		if (!strcmp(s.key, key))
			return &s;
	return nullptr;
}

extern "C" int rfwhip_set_setting(rfwhip_context *c, const char *key, const char *value)
{
	CTX_ENTER(c);
	if (!key || !value)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "null key/value");
	const Setting *s = find_setting(key);
	if (!s || !s->set)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "unknown setting \"%s\"", key);
	return s->set(c, key, value);
}

extern "C" int rfwhip_get_setting(rfwhip_context *c, const char *key, char *value, size_t cap)
{
	CTX_ENTER(c);
	if (!key || !value || !cap)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "null key/value");
	const Setting *s = find_setting(key);
	if (!s)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "unknown setting \"%s\"", key);
	return s->get(c, value, cap);
}

extern "C" int rfwhip_get_settings(rfwhip_context *c, const char **keys, size_t cap)
{
	(void)c;
	size_t n = 0;
	for (const Setting &s : k_settings)
		if (s.listed)
		{
			if (keys && n < cap)
				keys[n] = s.key;
			n++;
		}
	return (int)n;
}

extern "C" int rfwhip_get_counters(rfwhip_context *c, rfwhip_counters *out, int reset)
{
	CTX_ENTER(c);
	if (!out)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "null counters");
	RF_TRY(sync_all(c));
	memset(out, 0, sizeof(*out));
	for (int i = 0; i < rfwhip_context::MAX_SUB; i++)
	{
		void *buf = i == 0 ? c->d_counters.p : c->d_counters_sub[i].p;
		if (!buf)
			continue;
		rt::WaveCounters wc;
		RF_TRY(dm::d2h(&wc, buf, sizeof(wc), c->stream));
		out->rays_extend += wc.rays_extend, out->rays_shadow += wc.rays_shadow;
		out->inner_extend += wc.inner_extend, out->tris_extend += wc.tris_extend;
		out->inner_shadow += wc.inner_shadow, out->tris_shadow += wc.tris_shadow;
		out->shaded += wc.shaded;
		out->lds_extend += wc.lds_extend, out->lds_shadow += wc.lds_shadow;
		// the device-side clock of the extend stage: launches already folded + the ones of the most recent call
		out->extend_ticks += wc.ext_ticks, out->extend_launches_timed += wc.ext_timed;
		for (int d = 0; d < rt::MAX_DEPTH_SLOTS; d++)
			if (wc.t_last[d] > wc.t_first[d])
				out->extend_ticks += wc.t_last[d] - wc.t_first[d], out->extend_launches_timed++;
		if (reset)
		{
			wc.rays_extend = wc.rays_shadow = wc.inner_extend = wc.tris_extend = wc.inner_shadow = wc.tris_shadow = wc.shaded = 0;
			wc.lds_extend = wc.lds_shadow = 0;
			wc.ext_ticks = 0, wc.ext_timed = 0;
			for (int d = 0; d < rt::MAX_DEPTH_SLOTS; d++)
				wc.t_first[d] = ~0ull, wc.t_last[d] = 0ull;
			RF_TRY(dm::h2d(buf, &wc, sizeof(wc), c->stream));
			RF_TRY(dm::sync(c->stream));
		}
	}
	out->samples = c->totals.samples;
	if (reset)
		c->totals.samples = 0;
	return RFWHIP_OK;
}

extern "C" int rfwhip_get_kernel_time(rfwhip_context *c, int which, float *ms, uint32_t *launches, int reset)
{
	CTX_ENTER(c);
	if (which < 0 || which >= KF_COUNT)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "kernel family %d out of range", which);
	static_assert(KF_METER_HIST == 9 && KF_METER_REDUCE == 10 && KF_PRIMARY_ORDER == 11 && KF_BLOOM == 12 && KF_GRADE == 13 && KF_JPEG == 14 && KF_TEXDEC == 15 && KF_PRIMARY_ENTRY == 16 && KF_SKYLOAD == 17 && KF_RIG == 18, "rfwhip.h numbers the families");
	if (ms)
		*ms = c->kernel_ms[which];
	if (launches)
		*launches = c->kernel_launches[which];
	if (reset)
		c->kernel_ms[which] = 0.0f, c->kernel_launches[which] = 0;
	if (KindTimes *kt = reset ? c->kind_times(which) : nullptr)
		kt->reset();
	return RFWHIP_OK;
}

extern "C" int rfwhip_read_denoise_guides(rfwhip_context *c, float *albedo, float *normal_depth)
{
	CTX_ENTER(c);
	if (!c->W)
		return set_error(RFWHIP_ERR_STATE, "no render target");
	if (c->world != 1 && c->rank != 0)
		return set_error(RFWHIP_ERR_STATE, "rfwhip_read_denoise_guides: the guides live on the root (rank 0)");
	RF_TRY(sync_all(c));
	RF_TRY(dn_guides(c, c->stream));
	RF_TRY(dn_check_overflow(c));
	const size_t px = (size_t)c->W * c->H;
	std::vector<f4> g(2 * px);
	RF_TRY(dm::d2h(g.data(), c->d_dn_guides.p, 2 * px * sizeof(f4), c->stream));
	for (size_t i = 0; i < px; i++)
	{
		if (albedo)
			for (int k = 0; k < 4; k++)
				albedo[4 * i + k] = (&g[i].x)[k];
		if (normal_depth)
		{
			uint32_t e;
			memcpy(&e, &g[px + i].x, 4);
			const rt::f3 n = rtk::dn_normal(e);
			normal_depth[4 * i] = n.x, normal_depth[4 * i + 1] = n.y, normal_depth[4 * i + 2] = n.z, normal_depth[4 * i + 3] = g[px + i].y;
		}
	}
	return RFWHIP_OK;
}

// What rfwhip_read_denoise_history / _motion run the presented frame's stage once more with, from the same history into the same set
// (the bits it wrote): the presented image in d_present, the guides, the params of last_cam, the history sets (*rd -> *wr), the
// instance versions and the view
static int dn_replay_setup(rfwhip_context *c, rtk::Params &p, int *rd, int *wr, rtk::DnView &d)
{
	RF_TRY(sync_all(c));
	RF_TRY(c->d_present.ensure((size_t)c->W * c->H * sizeof(f4)));
	RF_TRY(present(c, c->d_present.as<f4>(), 1));
	RF_TRY(dn_guides(c, c->stream));
	fill_params(c, &c->last_cam, p);
	*wr = c->dn_hist_cur, *rd = *wr ^ 1;
	RF_TRY(dn_inst_ver_current(c, c->stream));
	d = dn_view(c, c->d_present.as<f4>(), c->d_present.as<f4>());
	d.hist = dn_hist_colour(c, *wr);
	return 0;
}

extern "C" int rfwhip_read_denoise_history(rfwhip_context *c, float *pre_rgbl, float *var, float *hist_rgbl, float *moments, float *length)
{
	CTX_ENTER(c);
	if (!c->W)
		return set_error(RFWHIP_ERR_STATE, "no render target");
	if (c->world != 1)
		return set_error(RFWHIP_ERR_STATE, "rfwhip_read_denoise_history: world-1 contexts only (a group's root filters gathered images)");
	if (!c->denoise || !c->dn_temporal || !c->dn_have_pres || c->frame_serial != c->dn_pres_serial)
		return set_error(RFWHIP_ERR_STATE, "rfwhip_read_denoise_history: the last render has not been presented with denoise and "
											"denoise_temporal on");
	// the stage of the presented frame once more, for I~ and var
	const size_t px = (size_t)c->W * c->H;
	rtk::Params p;
	rtk::DnView d;
	int rd, wr;
	RF_TRY(dn_replay_setup(c, p, &rd, &wr, d));
	rtk::DnMotion mv;
	if (c->dn_motion)
		RF_TRY(dn_motion_view(c, false, c->stream, mv));
	{
		StageTimer t(c, KF_DENOISE, -1, c->stream);
		rtk::launch_denoise_temporal(d, dn_temporal_view(c, p, rd, wr), c->dn_motion ? &mv : nullptr, c->stream);
		t.stop(2);
	}
	RF_TRY(dm::last_launch_error());
	const rtk::DnTemporal tv = dn_temporal_view(c, p, rd, wr);
	std::vector<f4> img(px), col(px);
	std::vector<float> v(px), mom(2 * px), n(px);
	RF_TRY(dm::d2h(img.data(), d.img[0], px * sizeof(f4), c->stream));
	RF_TRY(dm::d2h(v.data(), d.var[0], px * sizeof(float), c->stream));
	RF_TRY(dm::d2h(col.data(), d.hist, px * sizeof(f4), c->stream));
	RF_TRY(dm::d2h(mom.data(), tv.mom_out, 2 * px * sizeof(float), c->stream));
	RF_TRY(dm::d2h(n.data(), tv.n_out, px * sizeof(float), c->stream));
	RF_TRY(dm::sync(c->stream));
	// (invalid pixels: the stage writes no I~ / var; 0 here)
	std::vector<f4> gb(px);
	RF_TRY(dm::d2h(gb.data(), c->d_dn_guides.as<f4>() + px, px * sizeof(f4), c->stream));
	for (size_t i = 0; i < px; i++)
	{
		const bool valid = gb[i].y >= 0.0f;
		for (int k = 0; k < 4; k++)
		{
			if (pre_rgbl)
				pre_rgbl[4 * i + k] = valid ? (&img[i].x)[k] : 0.0f;
			if (hist_rgbl)
				hist_rgbl[4 * i + k] = (&col[i].x)[k];
		}
		if (var)
			var[i] = valid ? v[i] : 0.0f;
		if (moments)
			moments[2 * i] = mom[2 * i], moments[2 * i + 1] = mom[2 * i + 1];
		if (length)
			length[i] = n[i];
	}
	return RFWHIP_OK;
}

extern "C" int rfwhip_read_denoise_motion(rfwhip_context *c, int32_t *state, float *prev_position, float *prev_normal)
{
	CTX_ENTER(c);
	if (!c->W)
		return set_error(RFWHIP_ERR_STATE, "no render target");
	if (c->world != 1)
		return set_error(RFWHIP_ERR_STATE, "rfwhip_read_denoise_motion: world-1 contexts only (a group's root filters gathered images)");
	if (!c->denoise || !c->dn_temporal || !c->dn_motion || !c->dn_have_pres || c->frame_serial != c->dn_pres_serial)
		return set_error(RFWHIP_ERR_STATE, "rfwhip_read_denoise_motion: the last render has not been presented with denoise, "
											"denoise_temporal and denoise_motion on");
	// the stage of the presented frame once more, with the per-pixel record written
	const size_t px = (size_t)c->W * c->H;
	rtk::Params p;
	rtk::DnView d;
	int rd, wr;
	RF_TRY(dn_replay_setup(c, p, &rd, &wr, d));
	rtk::DnMotion mv;
	RF_TRY(dn_motion_view(c, false, c->stream, mv));
	DevBuf dump;
	RF_TRY(dump.ensure_exact(8 * px * sizeof(float)));
	mv.dump = dump.as<float>();
	rtk::launch_denoise_temporal(d, dn_temporal_view(c, p, rd, wr), &mv, c->stream);
	int rc = dm::last_launch_error();
	std::vector<float> rec(8 * px);
	if (!rc)
		rc = dm::d2h(rec.data(), dump.p, 8 * px * sizeof(float), c->stream);
	if (!rc)
		rc = dm::sync(c->stream);
	dump.free_();
	if (rc)
		return rc;
	for (size_t i = 0; i < px; i++)
	{
		if (state)
			state[i] = (int32_t)rec[8 * i];
		for (int k = 0; k < 3; k++)
		{
			if (prev_position)
				prev_position[3 * i + k] = rec[8 * i + 1 + k];
			if (prev_normal)
				prev_normal[3 * i + k] = rec[8 * i + 4 + k];
		}
	}
	return RFWHIP_OK;
}

extern "C" int rfwhip_denoise_image(rfwhip_context *c, const float *rgba_in, float *rgba_out)
{
	CTX_ENTER(c);
	if (!rgba_in || !rgba_out)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "null image");
	if (!c->W)
		return set_error(RFWHIP_ERR_STATE, "no render target");
	if (c->world != 1 && c->rank != 0)
		return set_error(RFWHIP_ERR_STATE, "rfwhip_denoise_image: the guides live on the root (rank 0)");
	RF_TRY(sync_all(c));
	const size_t bytes = (size_t)c->W * c->H * sizeof(f4);
	RF_TRY(c->d_present.ensure(bytes));
	RF_TRY(dm::h2d(c->d_present.p, rgba_in, bytes, c->stream));
	RF_TRY(dn_filter(c, c->d_present.as<f4>(), c->d_present.as<f4>(), c->stream, false)); // (spatial only: not a presented frame)
	RF_TRY(dm::d2h(rgba_out, c->d_present.p, bytes, c->stream));
	return dm::sync(c->stream);
}

extern "C" int rfwhip_read_primary_hits(rfwhip_context *c, float *t, int32_t *prim, int32_t *inst, float *u, float *v)
{
	CTX_ENTER(c);
	if (!c->W || c->wave_capacity == 0)
		return set_error(RFWHIP_ERR_STATE, "no frame rendered yet");
	RF_TRY(sync_all(c));
	// the first sample of the most recent call's first sub-batch lives in that sub-batch's first sample group
	rt::FrameView fr = c->fr;
	set_sample_group(fr, c->sgroup_last);
	const size_t slots = (size_t)c->fr.slots << fr.sgroup_log2;
	std::vector<f4> h(slots);
	std::vector<int> hi(slots);
	RF_TRY(dm::d2h(h.data(), c->d_hit0.as<f4>() + c->last_wave_off, slots * sizeof(f4), c->stream));
	RF_TRY(dm::d2h(hi.data(), c->d_hit0_inst.as<int>() + c->last_wave_off, slots * 4, c->stream));
	const size_t n = (size_t)c->W * c->H;
	for (size_t i = 0; i < n; i++)
	{
		if (t)
			t[i] = 1e34f;
		if (prim)
			prim[i] = -1;
		if (inst)
			inst[i] = -1;
		if (u)
			u[i] = 0;
		if (v)
			v[i] = 0;
	}
	const bool parity = c->integrator == 0;
	for (uint32_t yl = 0; yl < c->fr.local_rows; yl++)
	{
		const uint32_t y = rt::strip_of_local(yl / rt::STRIP_ROWS, (uint32_t)c->rank, (uint32_t)c->world) * rt::STRIP_ROWS + yl % rt::STRIP_ROWS;
		if (y >= c->H)
			continue;
		for (uint32_t x = 0; x < c->W; x++)
		{
			if (parity && (x >= (c->W / 4u) * 4u || y >= (c->H / 2u) * 2u))
				continue;
			const uint32_t tile = (yl / rt::TILE) * c->fr.tiles_x + x / rt::TILE;
			const size_t slot = (size_t)rt::pixel_to_slot(fr, tile, rt::tile_pix(x % rt::TILE, yl % rt::TILE), 0u);
			const size_t o = (size_t)y * c->W + x;
			int pr;
			memcpy(&pr, &h[slot].w, 4);
			if (pr == rt::HIT_MISS_SHADED) // (a miss the primary kernel shaded itself: kernels.hip, primary_finish_item)
				pr = -1;
			if (t)
				t[o] = h[slot].x;
			if (u)
				u[o] = h[slot].y;
			if (v)
				v[o] = h[slot].z;
			if (prim)
				prim[o] = pr;
			if (inst)
				inst[o] = pr >= 0 ? hi[slot] : -1;
		}
	}
	return RFWHIP_OK;
}

// The caller's rays through one form of the traversal (rfwhip.h: rfwhip_trace_rays_form): the product's launchers on the context's
// own wave buffers, with the counters a render's shade stages would have left (queue lengths, "paths went on").
struct FormRays
{
	size_t n = 0;
	const float *org = nullptr, *dir = nullptr, *t_max = nullptr;
	const uint32_t *tag = nullptr;
};
static int trace_form(rfwhip_context *c, const char *who, int form, uint32_t grid_items, uint32_t bins, const FormRays &e, float t_min, float t_max,
					  float *t, int32_t *prim, int32_t *inst, float *u, float *v, const FormRays &a, float *visible, uint64_t *launch_counters)
{
	if (form < RFWHIP_FORM_LANE_CLOSEST || form > RFWHIP_FORM_PACKET_ANY)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s: unknown form %d", who, form);
	const bool closest = form == RFWHIP_FORM_LANE_CLOSEST || form == RFWHIP_FORM_STREAM_CLOSEST || form == RFWHIP_FORM_FUSED;
	const bool any = form >= RFWHIP_FORM_LANE_ANY;
	const size_t ne = closest ? e.n : 0, na = any ? a.n : 0;
	if ((ne && (!e.org || !e.dir)) || (na && (!a.org || !a.dir || !a.t_max)))
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s: null rays", who);
	if (c->scene_dirty)
		return set_error(RFWHIP_ERR_STATE, "%s: scene changed since the last rfwhip_update()", who);
	if (ne >= (1ull << 31) || na >= (1ull << 31))
		return set_error(RFWHIP_ERR_UNSUPPORTED, "%s: too many rays", who);
	const bool packet = form == RFWHIP_FORM_PACKET_ANY;
	if (packet && (bins < 1u || bins > rt::SHADOW_BIN_BITS))
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s: %u bin bits (1..%u)", who, bins, rt::SHADOW_BIN_BITS);
	if (form == RFWHIP_FORM_LANE_CLOSEST && e.tag)
		for (size_t i = 0; i < ne; i++)
			if (e.tag[i] == rt::RAY_VOID)
				return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s: the one-ray-per-lane closest-hit form has no void entries (ray %zu)", who, i);
	for (size_t i = 0; i < ne && e.tag; i++)
		if (e.tag[i] != rt::RAY_VOID && e.tag[i] >= (1u << 31))
			return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s: tag %zu is no slot word (below 2^31) and not void", who, i);
	// occlusion set: the slot of every entry, unique and inside the visibility buffer
	const uint32_t slot_bits = packet ? rt::shadow_slot_bits(bins) : 32u;
	std::vector<uint32_t> slot_of(na, rt::RAY_VOID);
	{
		std::vector<uint8_t> taken(na, 0);
		for (size_t i = 0; i < na; i++)
		{
			const uint32_t w = a.tag ? a.tag[i] : (uint32_t)i;
			if (w == rt::RAY_VOID)
				continue;
			if (w >> 31)
				return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s: tag %zu of the occlusion set is no slot word (below 2^31: the bin ends at bit 30) and not void", who, i);
			const uint32_t sl = packet ? w & ((1u << slot_bits) - 1u) : w;
			if (sl >= na)
				return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s: slot %u of ray %zu outside the %zu slots of the call", who, sl, i, na);
			if (taken[sl])
				return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "%s: duplicate slot %u (ray %zu): the result is folded into its slot by a read-modify-write", who, sl, i);
			taken[sl] = 1, slot_of[i] = sl;
		}
	}
	if (ne + na == 0)
		return RFWHIP_OK;
	RF_TRY(sync_all(c)); // the wave buffers are shared with the sub-batch streams of a render in flight
	const size_t cap = std::max(ne, na);
	RF_TRY(ensure_wave_buffers(c, std::max(cap, c->wave_capacity), std::max(na, c->rad_capacity[0]), c->rad_capacity[1]));
	void *s = c->stream;
	if (packet)
	{
		RF_TRY(ensure_nodes4f(c));
		if (!(c->packet_ok && c->nodes4f_current && (c->refill & 8)))
			return set_error(RFWHIP_ERR_UNSUPPORTED, "%s: the packet traversal cannot run on this scene (its trees exceed the packet stack, or refill bit 3 is off)", who);
	}
	rtk::Params p;
	fill_params(c, nullptr, p);
	std::vector<f4> o4(cap), d4(cap);
	const auto word = [](uint32_t wd) {
		float f;
		memcpy(&f, &wd, 4);
		return f;
	};
	if (ne)
	{
		const bool ranged = form == RFWHIP_FORM_LANE_CLOSEST;
		for (size_t i = 0; i < ne; i++)
		{
			o4[i] = f4{e.org[3 * i], e.org[3 * i + 1], e.org[3 * i + 2], ranged ? t_min : word(e.tag ? e.tag[i] : (uint32_t)i)};
			d4[i] = f4{e.dir[3 * i], e.dir[3 * i + 1], e.dir[3 * i + 2], ranged ? t_max : 0.0f};
		}
		// the closest-hit waves of odd depth read the odd buffers: org/dir carry (origin, t_min | tag) and (direction, t_max | -)
		RF_TRY(dm::h2d(c->d_org[1].p, o4.data(), ne * sizeof(f4), s));
		RF_TRY(dm::h2d(c->d_dir2[1].p, d4.data(), ne * sizeof(f4), s));
		// a record no kernel writes stays recognisable
		std::vector<f4> h(ne, f4{NAN, NAN, NAN, word((uint32_t)RFWHIP_FORM_SENTINEL_PRIM)});
		std::vector<int> hi(ne, (int)RFWHIP_FORM_SENTINEL_PRIM);
		RF_TRY(dm::h2d(c->d_hit.p, h.data(), ne * sizeof(f4), s));
		RF_TRY(dm::h2d(c->d_hit_inst.p, hi.data(), ne * 4, s));
	}
	f4 *const vis_buf = packet ? c->d_rad_nee[0].as<f4>() : c->d_rad[0].as<f4>();
	if (na)
	{
		for (size_t i = 0; i < na; i++)
		{
			o4[i] = f4{a.org[3 * i], a.org[3 * i + 1], a.org[3 * i + 2], word(a.tag ? a.tag[i] : (uint32_t)i)};
			d4[i] = f4{a.dir[3 * i], a.dir[3 * i + 1], a.dir[3 * i + 2], a.t_max[i]};
		}
		RF_TRY(dm::h2d(c->d_sh_org[0].p, o4.data(), na * sizeof(f4), s));
		RF_TRY(dm::h2d(c->d_sh_dir[0].p, d4.data(), na * sizeof(f4), s));
		std::vector<f4> one(na, f4{1.0f, 0.0f, 0.0f, 0.0f});
		RF_TRY(dm::h2d(c->d_sh_rad[0].p, one.data(), na * sizeof(f4), s));
		// the slots the queue names start at 0 (1 for the packet form, whose occluded rays zero theirs); every other slot holds the
		// sentinel
		std::vector<f4> vis(na, f4{RFWHIP_FORM_UNTOUCHED, 0.0f, 0.0f, 0.0f});
		for (size_t i = 0; i < na; i++)
			if (slot_of[i] != rt::RAY_VOID)
				vis[slot_of[i]].x = packet ? 1.0f : 0.0f;
		RF_TRY(dm::h2d(vis_buf, vis.data(), na * sizeof(f4), s));
	}
	// the counters as the shade stages of a render would have left them: queue lengths, and "paths went on" (connection_count)
	const uint32_t de = form == RFWHIP_FORM_FUSED ? 3u : 1u, da = packet ? 0u : (form == RFWHIP_FORM_FUSED ? 2u : 1u);
	rtk::launch_init_counters(p.wv.counters, 0, s);
	RF_TRY(dm::last_launch_error());
	rt::WaveCounters w0;
	RF_TRY(dm::d2h(&w0, c->d_counters.p, sizeof(w0), s));
	if (ne)
		w0.ext[de] = w0.ext_n[de] = (uint32_t)ne;
	if (na)
	{
		w0.shadow[da] = w0.shadow_n[da] = (uint32_t)na;
		if (!w0.ext[da + 1])
			w0.ext[da + 1] = 1u;
	}
	RF_TRY(dm::h2d(c->d_counters.p, &w0, sizeof(w0), s));
	const bool count = launch_counters != nullptr || c->count_traversal != 0;
	const uint32_t items = grid_items ? grid_items : (uint32_t)cap;
	p.group = 16;
	p.wv.sh_org = c->d_sh_org[0].as<f4>(), p.wv.sh_dir = c->d_sh_dir[0].as<f4>(), p.wv.sh_rad = c->d_sh_rad[0].as<f4>();
	p.wv.rad = c->d_rad[0].as<f4>(), p.wv.rad_nee = nullptr;
	switch (form)
	{
	case RFWHIP_FORM_LANE_CLOSEST:
		p.depth = 1, p.queue = 0;
		rtk::launch_extend(p, rtk::GEN_RANGED, count, items, s);
		break;
	case RFWHIP_FORM_STREAM_CLOSEST:
		p.depth = 1, p.queue = 0, p.refill |= 1u;
		rtk::launch_extend(p, rtk::GEN_BUFFER, count, items, s);
		break;
	case RFWHIP_FORM_LANE_ANY:
		p.depth = 1, p.queue = 0, p.refill &= ~2u;
		rtk::launch_connect(p, count, items, s);
		break;
	case RFWHIP_FORM_STREAM_ANY:
		p.depth = 1, p.queue = 0, p.refill |= 2u;
		rtk::launch_connect(p, count, items, s);
		break;
	case RFWHIP_FORM_FUSED:
	{
		p.refill |= 3u;
		rtk::Params pa = p;
		p.depth = 3, p.queue = 0;
		pa.depth = 2, pa.queue = 1;
		rtk::launch_trace_fused(p, pa, count, items, s);
		break;
	}
	default:
		p.depth = 0, p.queue = 0, p.fr.shadow_bins = bins, p.wv.rad_nee = c->d_rad_nee[0].as<f4>();
		rtk::launch_shadow_packets(p, count, items, s);
		break;
	}
	RF_TRY(dm::last_launch_error());
	rt::WaveCounters wc;
	RF_TRY(dm::d2h(&wc, c->d_counters.p, sizeof(wc), s));
	if (launch_counters)
	{
		launch_counters[0] = wc.rays_extend - w0.rays_extend, launch_counters[1] = wc.rays_shadow - w0.rays_shadow;
		launch_counters[2] = wc.sp_runs - w0.sp_runs, launch_counters[3] = wc.stack_overflow;
	}
	if (ne)
	{
		std::vector<f4> h(ne);
		std::vector<int> hi(ne);
		RF_TRY(dm::d2h(h.data(), c->d_hit.p, ne * sizeof(f4), s));
		RF_TRY(dm::d2h(hi.data(), c->d_hit_inst.p, ne * 4, s));
		for (size_t i = 0; i < ne; i++)
		{
			int pr;
			memcpy(&pr, &h[i].w, 4);
			if (t)
				t[i] = h[i].x;
			if (u)
				u[i] = h[i].y;
			if (v)
				v[i] = h[i].z;
			if (prim)
				prim[i] = pr;
			if (inst)
				inst[i] = pr >= 0 ? hi[i] : -1;
		}
	}
	if (na && visible)
	{
		std::vector<f4> vis(na);
		RF_TRY(dm::d2h(vis.data(), vis_buf, na * sizeof(f4), s));
		for (size_t i = 0; i < na; i++)
			visible[i] = vis[i].x;
	}
	if (wc.stack_overflow)
		return set_error(RFWHIP_ERR_STATE, "traversal stack overflow: %u entries dropped", wc.stack_overflow);
	return RFWHIP_OK;
}

extern "C" int rfwhip_trace_rays(rfwhip_context *c, size_t n, const float *org, const float *dir, float t_min, float t_max,
								 float *t, int32_t *prim, int32_t *inst, float *u, float *v)
{
	CTX_ENTER(c);
	FormRays e;
	e.n = n, e.org = org, e.dir = dir;
	return trace_form(c, "rfwhip_trace_rays", RFWHIP_FORM_LANE_CLOSEST, 0u, 0u, e, t_min, t_max, t, prim, inst, u, v, FormRays(), nullptr, nullptr);
}

extern "C" int rfwhip_trace_rays_form(rfwhip_context *c, int form, uint32_t grid_items, uint32_t bins, size_t n, const float *org, const float *dir,
									  const uint32_t *tag, float *t, int32_t *prim, int32_t *inst, float *u, float *v, size_t n_any,
									  const float *org_any, const float *dir_any, const float *t_max_any, const uint32_t *tag_any,
									  float *visible, uint64_t *launch_counters)
{
	CTX_ENTER(c);
	FormRays e, a;
	e.n = n, e.org = org, e.dir = dir, e.tag = tag;
	a.n = n_any, a.org = org_any, a.dir = dir_any, a.t_max = t_max_any, a.tag = tag_any;
	return trace_form(c, "rfwhip_trace_rays_form", form, grid_items, bins, e, 1e-5f, 1e34f, t, prim, inst, u, v, a, visible, launch_counters);
}

static_assert(sizeof(rfwhip_area_light) == sizeof(rt::AreaLight) && sizeof(rfwhip_point_light) == sizeof(rt::PointLight) &&
				  sizeof(rfwhip_spot_light) == sizeof(rt::SpotLight),
			  "rfwhip_set_lights hands its arrays to the light tree's builder as the kernels' records");
static_assert(RFWHIP_KAT_LT_SAMPLE == rtk::KAT_LT_SAMPLE && RFWHIP_KAT_LT_PICK_PROB == rtk::KAT_LT_PICK_PROB, "kernels.h restates the light-tree functions");
static_assert(RFWHIP_KAT_METER_BIN == rtk::KAT_METER_BIN, "kernels.h restates the meter's function");
static_assert(RFWHIP_KAT_SURFACE_MAPS == rtk::KAT_SURFACE_MAPS, "kernels.h restates the material maps' function");
static_assert(RFWHIP_KAT_IN == 24 && RFWHIP_KAT_OUT == 8, "kat_item's record layout (kernels.hip)");
static_assert(RFWHIP_STRIP_ROWS == (int)rt::STRIP_ROWS, "rfwhip.h: rfwhip_row_owner() restates rt::strip_owner()");
static_assert(sizeof(rfwhip_adaptive_stats) == 48, "rfwhip.h: six uint64");
static_assert(sizeof(rfwhip_noise_tile) == sizeof(rtk::NoiseTile) && sizeof(rtk::NoiseTotal) == 32 && sizeof(rfwhip_noise_stats) == 40,
			  "rfwhip.h: the noise records are the kernels' (kernels.h)");
extern "C" int rfwhip_kat(rfwhip_context *c, int function, size_t n, const float *in, float *out)
{
	CTX_ENTER(c);
	if (n && (!in || !out))
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_kat: null records");
	if (function < 0 || function > RFWHIP_KAT_SURFACE_MAPS)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_kat: unknown function %d", function);
	if ((function == RFWHIP_KAT_POINT_ON_LIGHT || function == RFWHIP_KAT_LIGHT_PICK_PROB) && c->scene_dirty)
		return set_error(RFWHIP_ERR_STATE, "rfwhip_kat: the light functions use the lights of the last rfwhip_update()");
	if ((function == RFWHIP_KAT_SKY_SAMPLE || function == RFWHIP_KAT_SKY_PDF) && !c->scene_dirty && c->sky_stale)
		RF_TRY(update_sky_sampling(c));
	if ((function == RFWHIP_KAT_SKY_SAMPLE || function == RFWHIP_KAT_SKY_PDF) && (c->scene_dirty || !c->sky_view.table))
		return set_error(RFWHIP_ERR_STATE, "rfwhip_kat: the sky functions use the table of the last rfwhip_update() with sky_sampling=1 and a sky with light");
	if (function == RFWHIP_KAT_LT_SAMPLE || function == RFWHIP_KAT_LT_PICK_PROB)
	{
		if (c->scene_dirty || c->light_sampling != 2)
			return set_error(RFWHIP_ERR_STATE, "rfwhip_kat: the light-tree functions use the tree of the last rfwhip_update() with light_sampling=tree");
		if (c->lt_stale)
			RF_TRY(update_light_tree(c));
		// (the kernel indexes the path table with the light a record names)
		for (size_t i = 0; i < n && function == RFWHIP_KAT_LT_PICK_PROB; i++)
		{
			uint32_t light;
			memcpy(&light, in + i * RFWHIP_KAT_IN + 8, sizeof(light));
			if (light >= total_light_count(c))
				return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_kat: record %zu names light %u of %u", i, light, total_light_count(c));
		}
	}
	if (function == RFWHIP_KAT_BLUE_NOISE && !c->have_blue_noise)
		return set_error(RFWHIP_ERR_STATE, "rfwhip_kat: no blue-noise table (rfwhip_set_blue_noise)");
	const bool surface_fn = function == RFWHIP_KAT_SURFACE_LAYERS || function == RFWHIP_KAT_SURFACE_MAPS;
	if ((function == RFWHIP_KAT_TEX_FETCH || surface_fn) && c->scene_dirty)
		return set_error(RFWHIP_ERR_STATE, "rfwhip_kat: the texture functions use the scene of the last rfwhip_update()");
	// (the kernel indexes the scene's tables with what the records name: every index is checked here)
	for (size_t i = 0; i < n && (function == RFWHIP_KAT_TEX_FETCH || surface_fn); i++)
	{
		uint32_t ub[7];
		memcpy(ub, in + i * RFWHIP_KAT_IN, sizeof(ub));
		if (function == RFWHIP_KAT_TEX_FETCH)
		{
			if (ub[0] >= c->texture_count)
				return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_kat: record %zu names texture %u of %u", i, ub[0], c->texture_count);
			if (ub[1] > 1u || ub[5] < 1u || ub[5] > 65536u || ub[6] < 1u || ub[6] > 65536u)
				return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_kat: record %zu: form %u, size %u x %u", i, ub[1], ub[5], ub[6]);
			continue;
		}
		if (ub[0] >= c->instances.size() || !c->instances[ub[0]].used || c->instances[ub[0]].mesh >= c->meshes.size() ||
			!c->meshes[c->instances[ub[0]].mesh].used)
			return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_kat: record %zu names instance %u", i, ub[0]);
		if (ub[1] >= c->meshes[c->instances[ub[0]].mesh].triCount)
			return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_kat: record %zu names triangle %u of instance %u", i, ub[1], ub[0]);
	}
	if (n == 0)
		return RFWHIP_OK;
	if (n >= (1ull << 31))
		return set_error(RFWHIP_ERR_UNSUPPORTED, "rfwhip_kat: too many records");
	RF_TRY(sync_all(c));
	DevBuf d_in, d_out;
	int rc = d_in.ensure(n * RFWHIP_KAT_IN * sizeof(float));
	if (!rc)
		rc = d_out.ensure(n * RFWHIP_KAT_OUT * sizeof(float));
	if (!rc)
		rc = dm::h2d(d_in.p, in, n * RFWHIP_KAT_IN * sizeof(float), c->stream);
	if (!rc)
	{
		rtk::Params p;
		fill_params(c, nullptr, p);
		p.cam.blue_noise = c->have_blue_noise ? c->d_blue_noise.as<uint32_t>() : nullptr;
		rtk::launch_kat(p, c->sky_view, c->lt_view, function, d_in.as<float>(), d_out.as<float>(), (uint32_t)n, c->stream);
		rc = dm::last_launch_error();
	}
	if (!rc)
		rc = dm::d2h(out, d_out.p, n * RFWHIP_KAT_OUT * sizeof(float), c->stream);
	d_in.free_(), d_out.free_();
	return rc;
}

extern "C" int rfwhip_get_bvh(rfwhip_context *c, size_t mesh_index, rfwhip_bvh_node *nodes, size_t node_cap,
							  uint32_t *prim_indices, size_t prim_cap, size_t *node_count, size_t *prim_count)
{
	CTX_ENTER(c);
	if (mesh_index >= c->meshes.size() || !c->meshes[mesh_index].used)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_get_bvh: no mesh %zu", mesh_index);
	MeshRec &m = c->meshes[mesh_index];
	if (m.device_built)
	{
		// no host copy exists: fetched on demand (this is a debugging / test hook, not part of the build path)
		if (node_count)
			*node_count = m.node_count2;
		if (prim_count)
			*prim_count = m.triCount;
		RF_TRY(sync_all(c));
		const uint32_t nb = m.resident ? m.node_base : 0u, tb = m.resident ? m.tri_base : 0u;
		if (nodes && node_cap)
		{
			const size_t n = std::min<size_t>(node_cap, m.node_count2);
			const rt::Node *src = m.resident ? c->d_nodes.as<rt::Node>() + m.node_base : m.d_b_nodes.as<rt::Node>();
			RF_TRY(dm::d2h(nodes, src, n * sizeof(rt::Node), c->stream));
			for (size_t k = 0; k < n; k++) // device entries -> the reference layout (bvh_node.h:23-28), mesh-local
			{
				if (nodes[k].count > 0)
					nodes[k].left_first = (int32_t)(((uint32_t)nodes[k].left_first & rt::ENTRY_FIRST_MASK) - tb);
				else if (nodes[k].count < 0)
					nodes[k].left_first = (int32_t)(((uint32_t)nodes[k].left_first & rt::ENTRY_INDEX_MASK) - nb);
			}
		}
		if (prim_indices && prim_cap)
		{
			std::vector<f4> tv(3 * m.triCount);
			const f4 *src = m.resident ? c->d_tri_verts.as<f4>() + 3ull * m.tri_base : m.d_b_tri_verts.as<f4>();
			RF_TRY(dm::d2h(tv.data(), src, tv.size() * sizeof(f4), c->stream));
			for (size_t k = 0; k < std::min<size_t>(prim_cap, m.triCount); k++)
				memcpy(&prim_indices[k], &tv[3 * k].w, 4);
		}
		return RFWHIP_OK;
	}
	if (node_count)
		*node_count = m.bvh.nodes.size();
	if (prim_count)
		*prim_count = m.bvh.order.size();
	if (nodes && node_cap)
	{
		const size_t n = std::min(node_cap, m.bvh.nodes.size());
		if (m.resident)
		{
			RF_TRY(sync_all(c));
			RF_TRY(dm::d2h(nodes, c->d_nodes.as<rt::Node>() + m.node_base, n * sizeof(rt::Node), c->stream));
			for (size_t k = 0; k < n; k++) // device nodes carry packed entries: hand out the reference layout
				nodes[k].left_first = m.bvh.nodes[k].left_first;
		}
		else
			memcpy(nodes, m.bvh.nodes.data(), n * sizeof(rt::Node));
	}
	if (prim_indices && prim_cap)
		memcpy(prim_indices, m.bvh.order.data(), std::min(prim_cap, m.bvh.order.size()) * 4);
	return RFWHIP_OK;
}

extern "C" int rfwhip_get_light_tree(rfwhip_context *c, rfwhip_light_tree_node *nodes, size_t node_cap, rfwhip_light_tree_path *paths,
									 size_t light_cap)
{
	static_assert(sizeof(rfwhip_light_tree_node) == sizeof(rt::LightTreeNode) && sizeof(rfwhip_light_tree_path) == sizeof(rt::LightTreePath),
				  "rfwhip_abi.h restates the light tree's records");
	if (!c)
		return -set_error(RFWHIP_ERR_INVALID_ARGUMENT, "null context");
	if (c->cleaned)
		return -set_error(RFWHIP_ERR_STATE, "context already cleaned up");
	if (dm::use(c->device))
		return -RFWHIP_ERR_HIP;
	if (c->lt_stale && update_light_tree(c))
		return -RFWHIP_ERR_STATE;
	if (c->light_sampling != 2)
		return 0;
	if (sync_all(c))
		return -RFWHIP_ERR_STATE;
	// no host copy is kept: fetched on demand (a test hook)
	if (nodes && node_cap && c->lt_view.nodes &&
		dm::d2h(nodes, c->lt_view.nodes, std::min<size_t>(node_cap, c->lt_view.node_count) * sizeof(rt::LightTreeNode), c->stream))
		return -RFWHIP_ERR_STATE;
	if (paths && light_cap && c->lt_view.paths &&
		dm::d2h(paths, c->lt_view.paths, std::min<size_t>(light_cap, total_light_count(c)) * sizeof(rt::LightTreePath), c->stream))
		return -RFWHIP_ERR_STATE;
	return (int)c->lt_view.node_count;
}

extern "C" int rfwhip_get_bvh4(rfwhip_context *c, size_t mesh_index, void *nodes4c, void *nodes4f, uint32_t *src4, size_t node_cap,
							   float *tri_verts, size_t tri_cap, rfwhip_bvh4_info *info)
{
	CTX_ENTER(c);
	if (mesh_index >= c->meshes.size() || !c->meshes[mesh_index].used)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_get_bvh4: no mesh %zu", mesh_index);
	const MeshRec &m = c->meshes[mesh_index];
	if (!m.resident)
		return set_error(RFWHIP_ERR_STATE, "rfwhip_get_bvh4: mesh %zu is not resident (rfwhip_update places it)", mesh_index);
	if (info)
	{
		info->n4_base = m.n4_base, info->n4_count = m.n4_count, info->tri_base = m.tri_base, info->tri_count = (uint32_t)m.triCount;
		info->node_base = m.node_base, info->node_count2 = m.node_count2;
		info->stack_need = m.stack_need, info->device_built = m.device_built ? 1u : 0u;
	}
	RF_TRY(sync_all(c));
	const size_t n4 = std::min<size_t>(node_cap, m.n4_count), nt = std::min<size_t>(tri_cap, m.triCount);
	if (nodes4c && n4)
		RF_TRY(dm::d2h(nodes4c, c->d_nodes4.as<rt::Node4c>() + m.n4_base, n4 * sizeof(rt::Node4c), c->stream));
	if (src4 && n4)
		RF_TRY(dm::d2h(src4, c->d_nodes4_src.as<uint32_t>() + 4ull * m.n4_base, 4 * n4 * sizeof(uint32_t), c->stream));
	if (tri_verts && nt)
		RF_TRY(dm::d2h(tri_verts, c->d_tri_verts.as<f4>() + 3ull * m.tri_base, 3 * nt * sizeof(f4), c->stream));
	if (nodes4f && n4)
	{
		if (c->nodes4f_current)
			RF_TRY(dm::d2h(nodes4f, c->d_nodes4f.as<rt::Node4f>() + m.n4_base, n4 * sizeof(rt::Node4f), c->stream));
		else
		{
			// the float table is written only when the packet traversal can run: expand the slice with the same kernel
			DevBuf tmp;
			int rc = tmp.ensure(n4 * sizeof(rt::Node4f));
			if (!rc)
			{
				rtk::launch_expand4(c->d_nodes4.as<rt::Node4c>() + m.n4_base, tmp.as<rt::Node4f>(), (uint32_t)n4, c->stream);
				rc = dm::last_launch_error();
			}
			if (!rc)
				rc = dm::d2h(nodes4f, tmp.p, n4 * sizeof(rt::Node4f), c->stream);
			tmp.free_();
			RF_TRY(rc);
		}
	}
	return RFWHIP_OK;
}

// ---- moving emitters (setting "lights_follow_geometry"; work items: light_follow.h) ---------------------------------------------
extern "C" int rfwhip_read_area_lights(rfwhip_context *c, rfwhip_area_light *out, size_t cap)
{
	CTX_ENTER(c);
	const size_t n = std::min<size_t>(cap, c->lc.areaLightCount);
	if (n && !out)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_read_area_lights: null array");
	if (n)
		RF_TRY(dm::d2h(out, c->d_area.p, n * sizeof(rfwhip_area_light), c->stream));
	RF_TRY(dm::sync(c->stream));
	return (int)c->lc.areaLightCount;
}

extern "C" int rfwhip_light_tree_refit(rfwhip_context *c, rfwhip_light_tree_node *nodes, size_t node_count, const rfwhip_area_light *area,
									   size_t n_area, const uint8_t *bound)
{
	CTX_ENTER(c);
	if (!nodes || !node_count || (n_area && !area))
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_light_tree_refit: null array");
	if (node_count >= (1ull << 31) || (node_count != 1 && (node_count & 1)))
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_light_tree_refit: %zu nodes is not the size of a light tree", node_count);
	const uint32_t n_spatial = node_count == 1 ? 1u : (uint32_t)(node_count / 2);
	if (n_area > n_spatial)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_light_tree_refit: %zu area lights, but the tree holds %u lights", n_area, n_spatial);
	rtk::LightTreeLevels lv{};
	if (!lighttree::levels(reinterpret_cast<const rt::LightTreeNode *>(nodes), node_count, n_spatial, lv.first, lv.count, rtk::LT_MAX_LEVELS, lv.levels))
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_light_tree_refit: the nodes are not a tree as rfwhip_get_light_tree returns it");
	RF_TRY(sync_all(c));
	const std::vector<uint8_t> all(bound ? 0 : n_area, 1);
	DevBuf d_nodes, d_area, d_bound, d_touched;
	int rc = d_nodes.ensure(node_count * sizeof(rt::LightTreeNode));
	if (!rc)
		rc = d_area.ensure(std::max<size_t>(1, n_area) * sizeof(rt::AreaLight));
	if (!rc)
		rc = d_bound.ensure(std::max<size_t>(1, n_area));
	if (!rc)
		rc = d_touched.ensure(node_count);
	if (!rc)
		rc = dm::h2d(d_nodes.p, nodes, node_count * sizeof(rt::LightTreeNode), c->stream);
	if (!rc && n_area)
		rc = dm::h2d(d_area.p, area, n_area * sizeof(rt::AreaLight), c->stream);
	if (!rc && n_area)
		rc = dm::h2d(d_bound.p, bound ? bound : all.data(), n_area, c->stream);
	if (!rc)
	{
		rtk::launch_light_tree_refit(d_nodes.as<rt::LightTreeNode>(), lv, d_area.as<rt::AreaLight>(), (uint32_t)n_area,
									 d_bound.as<unsigned char>(), d_touched.as<unsigned char>(), c->stream);
		rc = dm::last_launch_error();
	}
	if (!rc)
		rc = dm::d2h(nodes, d_nodes.p, node_count * sizeof(rt::LightTreeNode), c->stream);
	const int rs = dm::sync(c->stream); // (on every path: nothing enqueued may outlive the buffers)
	rc = rc ? rc : rs;
	d_nodes.free_(), d_area.free_(), d_bound.free_(), d_touched.free_();
	return rc;
}

#if defined(RFWHIP_HOST_EMULATION)
// ---- the emulation libraries only (tests/test_primary_order.py): not declared in rfwhip.h, not in the product ----
// the primary wave's ordering item (primary_order.h) on n caller-supplied rt::Node4f records (host memory, `out` another array)
extern "C" RFWHIP_API int rfwhip_emu_order4f(const void *in, void *out, uint32_t n, const float *origin, int ordered)
{
	if (!in || !out || !origin || in == out)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_emu_order4f: two node arrays and an origin");
	rtk::launch_order4f((const rt::Node4f *)in, (rt::Node4f *)out, 0u, n, origin, ordered != 0, nullptr);
	return dm::sync(nullptr); // (the deferred-stream variant: stream 0 — a context's main stream — has run it)
}
// the entry snapshot of the context's last render call that made one (primary_entry.h; tests/test_primary_entry.py): what the pass
// read and what it wrote.  info[0..31] = the key of the records (view, frame, table serial, root: ensure_primary_entry), info[32] =
// words per record, info[33] = records, info[34] = nodes of the camera-ordered table, info[35] = 1 if there are records at all.
// nodes / records (either may be null): the table and the records, as many bytes / words as the caps allow
extern "C" RFWHIP_API int rfwhip_emu_primary_entry(rfwhip_context *c, uint32_t *info, void *nodes, size_t nodes_cap_bytes, uint32_t *records,
												   size_t records_cap_words)
{
	if (!c || !info)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_emu_primary_entry: a context and 36 words");
	RF_TRY(sync_all(c));
	memcpy(info, c->ent_key, sizeof(c->ent_key));
	const size_t groups = c->ent_valid ? (((size_t)c->ent_key[17] << c->ent_key[18]) >> 6) : 0;
	info[32] = rtk::primary_entry_words(), info[33] = (uint32_t)groups, info[34] = (uint32_t)c->nodes4_live, info[35] = c->ent_valid ? 1u : 0u;
	if (nodes && c->ent_valid)
		memcpy(nodes, c->d_nodes4f_ord.p, std::min(nodes_cap_bytes, c->nodes4_live * sizeof(rt::Node4f)));
	if (records && c->ent_valid)
		memcpy(records, c->d_primary_entry.p, std::min(records_cap_words, groups * info[32]) * 4);
	return RFWHIP_OK;
}
#endif

#if defined(RFWHIP_HOST_EMULATION) && defined(RFWHIP_EMU_STREAMS) && RFWHIP_EMU_STREAMS
// ---- the deferred-stream emulation library only (tests/test_schedule.py): not declared in rfwhip.h, not in the product ----
// policy: 0 = in enqueue order, 1 = latest ready operation first, 2 = seeded random, 3 = latest first over everything enqueued
// (emu_streams.h).  Runs everything still pending (in enqueue order) first and resets the counters of rfwhip_emu_schedule_stats.
extern "C" RFWHIP_API int rfwhip_emu_set_schedule(int policy, unsigned seed)
{
	if (policy < emu_streams::INORDER || policy > emu_streams::EAGER)
		return set_error(RFWHIP_ERR_INVALID_ARGUMENT, "rfwhip_emu_set_schedule: unknown policy %d", policy);
	emu_streams::state().policy = emu_streams::INORDER; // (what is still pending runs as the host issued it)
	emu_streams::set_schedule(policy, seed);
	return RFWHIP_OK;
}
// since the last rfwhip_emu_set_schedule: the closures run, how many of them ran while an operation enqueued before them and
// needed by the same sync point had not run yet, and the launches of the packet form of the depth-0 connection wave
extern "C" RFWHIP_API int rfwhip_emu_schedule_stats(unsigned long long *ran, unsigned long long *out_of_order,
												   unsigned long long *shadow_packet_launches)
{
	const emu_streams::State &S = emu_streams::state();
	if (ran)
		*ran = S.ran;
	if (out_of_order)
		*out_of_order = S.out_of_order;
	if (shadow_packet_launches)
		*shadow_packet_launches = S.shadow_packet_launches;
	return RFWHIP_OK;
}
#endif
