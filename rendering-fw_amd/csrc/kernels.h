// kernels.h — host-callable launchers of the wavefront stages (implemented in kernels.hip).
#pragma once
#include "rt_types.h"
#include <stddef.h>

namespace rtk
{

struct Params
{
	rt::SceneView sc;
	rt::WaveView wv;
	rt::CamView cam;
	rt::FrameView fr;
	uint32_t depth;		// pathLength of this wave
	uint32_t max_depth; // MAX_PATH_LENGTH
	uint32_t parity_no_jitter;
	uint32_t lds_first; // Node4 range every traversal workgroup keeps in LDS: the top of the largest BLAS
	uint32_t lds_count; // (0 = off, <= max_lds_nodes())
	uint32_t queue;		// which WaveCounters::work[] row this launch pulls its chunks from
	uint32_t group;		// chunks per XCD group (one row of tiles for the primary wave)
	uint32_t refill;	// incoherent waves: lanes that finish a ray pull the next one (persistent lanes)
	uint32_t textured;	// some material carries a texture / normal map: the shade kernel variant with the texture layers
};

enum GenMode
{
	GEN_BUFFER = 0, // rays come from the wave buffers (depth >= 1)
	GEN_PT = 1,		// generate pt primary rays   (CUDART generatePrimaryRay)
	GEN_PARITY = 2, // generate parity primary rays (EmbreeRT GenerateRay8 draw order)
	GEN_RANGED = 3	// rays from the wave buffers with per-ray (t_min, t_max) in the w components (rfwhip_trace_rays)
};

typedef void *stream_t; // hipStream_t

// The denoiser's buffers and knobs (denoise.h): full image, W x H pixels, row-major
struct DnView
{
	uint32_t W, H;
	rt::f4 *ga, *gb;	  // guides: albedo | valid, octahedral normal | z | dz/dx | dz/dy
	rt::f4 *in, *out;	  // the image to filter and where the result goes (may be the same buffer)
	rt::f4 *img[2];		  // ping-pong demodulated irradiance (rgb, luminance)
	float *var[2];		  // ping-pong variance of the luminance
	float sigma_l, sigma_n, sigma_z;
	uint32_t iterations;  // 1..8 passes, step 2^i
	uint32_t *overflow;	  // the guide pass's own traversal-stack overflow counter (not the render's wave counters)
	uint32_t *id;		  // the guide pass's instance index per pixel (DN_NO_INST: invalid), or null (temporal stage off)
	rt::f4 *hist;		  // where pass 0 writes its demodulated output (the temporal stage's colour history), or null
};

// The temporal stage of the denoiser (denoise.h dn_temporal_item): frame F's camera, the previous presented frame P's camera,
// guides and instance ids, and the two history sets (read P's, write F's)
struct DnTemporal
{
	rt::CamView cam, pcam;		 // F's and P's cameras (pos, p1, right, up)
	rt::FrameView fr;			 // F's frame (1 / W, 1 / H of the centre rays)
	const rt::f4 *pgb;			 // P's guides (normal | z | dz/dx | dz/dy)
	const uint32_t *id, *pid;	 // F's and P's instance ids
	const uint32_t *inst_ver;	 // per instance: the scene version of the update that last changed it
	uint32_t n_inst, pscene;	 // instances, and the scene version of P's guides
	const rt::f4 *col_in;		 // P's history: colour, moments (mu1, mu2), length
	const float *mom_in, *n_in;
	float *mom_out, *n_out;		 // F's moments and length (the colour goes through DnView::hist)
	float alpha;
	uint32_t usable;			 // 0: every pixel starts fresh (no history is read)
};

// Motion in the temporal stage (setting "denoise_motion"; denoise.h dn_temporal_motion_item).  Per instance: what the host decided
// (DN_M_STILL / DN_M_MOVED / DN_M_RESTART) and, for MOVED, the transforms at P's guides and now (rows 0..2, row-major 3 x 4) and
// the mesh's object-space vertices now and at P's guides (the same array for a mesh nobody edited since)
constexpr uint32_t DN_M_INVALID = 0u, DN_M_STILL = 1u, DN_M_MOVED = 2u, DN_M_RESTART = 3u; // (rfwhip_read_denoise_motion's states)
struct alignas(16) DnMotionInst
{
	float mp[12], mf[12];
	const rt::f4 *cur, *prev;
	const uint32_t *indices; // three per triangle, or null: triangle k has the vertices 3 k .. 3 k + 2
	uint32_t state, tri_count, vert_count, pad;
};
struct DnMotion
{
	const DnMotionInst *inst; // DnTemporal::n_inst records
	const rt::f4 *surf;		  // per pixel, from the guide pass: (primitive, u, v, 0)
	float *dump;			  // rfwhip_read_denoise_motion: 8 floats per pixel (state, X_P, n'_p, 0), or null
};

// The display stage (display.h): the full W x H float4 image `in` -> one pixel per pixel in `out` (in != out)
struct DisplayView
{
	uint32_t W, H;
	const rt::f4 *in;
	void *out;					// W x H uint32 (format 0, RFWHIP_DISPLAY_RGBA8) or W x H float4 (format 1, RFWHIP_DISPLAY_RGBA32F)
	float brightness, contrast; // the camera's (rfwhip_camera)
	uint32_t tonemap;			// 0 aces, 1 none
	uint32_t fxaa, srgb, format;
};

// The exposure meter (metering.h).  A histogram is MT_BINS bins; a record of one is MT_RECORD words: the bins, then `excluded`,
// padded to whole 16-byte rows (the reduce reads four bins per lane)
constexpr uint32_t MT_BINS = 256u, MT_RECORD = MT_BINS + 4u;
// The 32-byte record k_meter_reduce leaves on the device (= rfwhip_meter_stats) ...
struct MeterRecord
{
	float E, l, l_target, lambda; // the exposure 2^l, l after adaptation, its clamped target, the window's mean log2 luminance
	uint32_t valid, excluded;	  // pixels counted into the histogram / left out of it (the last metered image)
	uint32_t steps, reserved;	  // steps taken since the last reset
};
// ... what a step is taken with (the display_exposure_* settings; log2_key: log2 of the key, computed in double) ...
struct MeterParams
{
	double low, high;
	float log2_key, ev, ev_min, ev_max, speed;
	uint32_t pad;
};
// ... the histogram pass's view: `pixels` float4 pixels in, one partial record of MT_RECORD words per MT_RANGE pixels out ...
struct MeterView
{
	const rt::f4 *in;
	uint32_t pixels;
	uint32_t *partial;
};
// ... and the exposed display's: E of the record, a scalar load (DisplayView stays what it was)
struct ExposureView
{
	const MeterRecord *rec;
};

// Bloom (bloom.h): the display_bloom_* settings as the kernels take them ...
struct BloomParams
{
	float intensity, threshold, knee, scatter;
};
// ... a down pass: the W x H texels of `src` (the image itself for the first one) -> the Wn x Hn texels of `dst`, Wn = (W + 1) >> 1;
// E: the exposure behind the prefilter, one float on the device (the first pass alone reads it) ...
struct BloomDownView
{
	const rt::f4 *src;
	rt::f4 *dst;
	uint32_t W, H, Wn, Hn;
	const float *E;
};
// ... an up pass: level k (W x H, D_k in, U_k out) and level k + 1 (`next`, Wn x Hn) ...
struct BloomUpView
{
	rt::f4 *level;
	const rt::f4 *next;
	uint32_t W, H, Wn, Hn;
};
// ... and the apply pass: the W x H image `in`, level 1 (`next`, Wn x Hn) -> `out` (in != out)
struct BloomApplyView
{
	const rt::f4 *in;
	const rt::f4 *next;
	rt::f4 *out;
	uint32_t W, H, Wn, Hn;
};

// Colour grading and dither (display_grade.h): what k_display_graded takes beside the DisplayView.  flags: the GR_* bits of the steps
// that are NOT at the identity, set by the host; rec: the record whose E the kernel applies (GR_EXPOSED, else unread);
// lut: n^3 float4, red fastest (GR_LUT, else unread); wb: M_wb row by row
constexpr uint32_t GR_EXPOSED = 1u, GR_WB = 2u, GR_CDL_R = 4u, GR_CDL_G = 8u, GR_CDL_B = 16u, GR_SAT = 32u, GR_LUT = 64u, GR_DITHER = 128u;
constexpr uint32_t GR_LUT_MIN = 2u, GR_LUT_MAX = 65u; // a LUT's size n: at most 65^3 x 16 bytes = 4.4 MB
struct GradeView
{
	const MeterRecord *rec;
	const rt::f4 *lut;
	uint32_t n, flags;
	float wb[9];
	float slope[3], offset[3], power[3];
	float sat;
};

// Baseline JPEG of the RGBA8 display image (display_jpeg.h).  JP_HEADER: the bytes in front of the entropy data, built by the host;
// JP_BLOCK_BYTES: the worst case of one block in an interval's slot — a block's code is at most JP_STRIP_WORDS x 32 bits = 208
// bytes, and every byte may be an 0xFF with a 0x00 behind it
constexpr uint32_t JP_HEADER = 613u, JP_STRIP_WORDS = 52u, JP_BLOCK_BYTES = 8u * JP_STRIP_WORDS;
// the constant tables, built once by the host: K = the DCT's integer matrix, row by row; zz[z] = the natural index of zigzag
// position z, izz its inverse; dc / ac[table][symbol] = the Annex K.3 Huffman code in the low 16 bits, its length above
struct JpegTables
{
	int32_t K[64];
	uint8_t zz[64], izz[64];
	uint32_t dc[2][12], ac[2][256];
};
// what k_jpeg_offsets leaves (= rfwhip_jpeg_stats): bytes = the whole stream, header and markers included, also when it did not fit
struct JpegRecord
{
	uint32_t bytes, intervals, mcus, blocks, stuffed, overflow, header, pad;
};
// rgba: W x H RGBA8, R in the lowest byte; sub: 0 = "444", 1 = "420"; bpm = blocks per MCU (3 | 6); ri = MCUs per restart interval;
// q[table][natural index] = the scaled quantisation tables; coef: blocks x 64 int16; slots: blocks x JP_BLOCK_BYTES + 3 x intervals
// bytes; counts: per interval its bytes and its stuffed bytes; offsets: per interval its place in `out`; out: cap bytes
struct JpegView
{
	const uint32_t *rgba;
	uint32_t W, H, sub, mcus_x, mcus, bpm, blocks, ri, intervals, cap;
	const JpegTables *tab;
	uint16_t q[2][64];
	int16_t *coef;
	uint8_t *slots;
	uint32_t *counts, *offsets;
	JpegRecord *rec;
	uint8_t *out;
};

// The noise estimate (noise.h).  One record per NZ_TILE_X x NZ_TILE_Y noise tile (= rfwhip_noise_tile) and the one record k_noise_final leaves
constexpr uint32_t NZ_TILE_X = 32, NZ_TILE_Y = 8;
struct NoiseTile
{
	float sum_e, max_e;
	uint32_t pixels, converged;
};
struct NoiseTotal // 32 bytes: all the host reads back
{
	double sum_e;
	unsigned long long pixels, converged;
	float max_e;
	uint32_t tiles;
};
// the metric's view of a rank's pixels, in the local layout of the accumulator (local_rows x W, row yl = a row of one of the
// rank's strips): moments in, error map / tile records / total out
struct NoiseView
{
	uint32_t W, H, local_rows, rank, world;
	uint32_t n;			  // samples per pixel (>= 2)
	const float *moments; // 2 per local pixel: sumY, M2
	float *e_map;		  // local_rows x W; 0 where there is no pixel (rows >= H of the last strip)
	NoiseTile *tiles;	  // ceil(W / 32) x local_rows / 8, row-major
	NoiseTotal *total;
	float floor_, threshold;
};
// adaptive sampling (adaptive.h): the per-tile state of a rank beside the tile records of the metric
struct AdaptiveView
{
	uint32_t ntx, count;   // noise tiles per row, and in all (= ntx * local_rows / 8)
	uint32_t tiles_x;	   // slot tiles per row (FrameView::tiles_x): the mask's row length
	uint32_t min_samples;  // adaptive_min_samples
	uint32_t *n_tile;	   // samples the tile's pixels hold
	unsigned char *active; // 1 until the tile retires
	unsigned char *mask;   // one byte per slot tile, tiles_x x local_rows / 8 (padded to whole words): 1 = trace
	const NoiseTile *tiles;
};

// capacity of the LDS top-of-tree cache the kernels were built with
uint32_t max_lds_nodes();

// device properties used for grid sizing
void set_device_cus(int cus);

// zero the per-render wave counters (ext/shadow/probe) and set ext[0] = primary_count
void launch_init_counters(rt::WaveCounters *c, uint32_t primary_count, stream_t s);
void launch_set_ext_count(rt::WaveCounters *c, uint32_t depth, uint32_t count, stream_t s);
void launch_rng_states(uint32_t *states, const uint32_t base_state[4], const uint32_t *jump_table,
					   uint32_t packets_per_sample, uint32_t spp, stream_t s);
// ordered (GEN_PT in packet form only): the camera-ordered copy of SceneView::nodes4f (launch_order4f) — the primary wave reads it
// in place of nodes4f and takes every node's children as they come; null: the primary wave sorts them itself
void launch_extend(const Params &p, int gen, bool count, uint32_t max_items, stream_t s, const rt::Node4f *ordered = nullptr);
bool primary_packet_form(const Params &p, uint32_t max_items); // the pt primary wave of such a launch fills WaveView::hit0_done
bool primary_packet_walk(const Params &p, uint32_t max_items); // ... and walks the tree once per wave (the emulation's does too)
void launch_shade_parity(const Params &p, bool count, uint32_t max_items, stream_t s);
uint32_t queue_pad(uint32_t max_items); // extra slots per queue and launch for the void entries of unfinished blocks
// sky.pick > 0 (setting sky_sampling): the sky variant k_shade_pt_sky, which takes the table as an argument of its own (Params, and
// with it every other kernel's code, stays what it was)
void launch_shade_pt(const Params &p, const rt::SkyView &sky, uint32_t max_items, stream_t s);
// light_sampling = linear | tree: k_shade_pt_lt (lt.nodes null: linear); sky as above (pick == 0: no sky sampling)
void launch_shade_pt_lt(const Params &p, const rt::SkyView &sky, const rt::LightTreeView &lt, uint32_t max_items, stream_t s);
// material_maps = 1 and a material with an alpha, roughness or metallic map: k_shade_pt_maps<SKY, LT> in place of either of the two
// above (with_lt false: light_sampling = reference, lt unread; sky as above)
void launch_shade_pt_maps(const Params &p, const rt::SkyView &sky, const rt::LightTreeView &lt, bool with_lt, uint32_t max_items, stream_t s);
void launch_connect(const Params &p, bool count, uint32_t max_items, stream_t s);
// the connection wave of depth 0 in packet form: runs of the shadow queue sorted by the chosen light's bin (FrameView::shadow_bins),
// one wave-uniform occlusion traversal per 64 rays of the sorted order
void launch_shadow_packets(const Params &p, bool count, uint32_t max_items, stream_t s);
// the extension rays of pe.depth and the shadow rays of pa.depth (= pe.depth - 1) in one launch (both with persistent lanes)
void launch_trace_fused(const Params &pe, const Params &pa, bool count, uint32_t max_items, stream_t s);
void launch_resolve(const Params &p, stream_t s);
// noise_estimate = 1: k_resolve_noise, the resolve that also folds the call's samples into the two moments per local pixel
// (noise.h; n_a = samples per pixel before this call).  The moments are arguments of their own: Params stays what it was
void launch_resolve_noise(const Params &p, float *moments, uint32_t n_a, stream_t s);
// the step update alone on given samples (rfwhip_noise_merge): samples_rgb = pixels x S x 3 floats, moments = 2 per pixel, in place
void launch_noise_merge(const float *samples_rgb, float *moments, uint32_t pixels, uint32_t n_a, uint32_t S, stream_t s);
// the metric: k_noise_tiles (error map + one record per tile) and k_noise_final (one workgroup, the tiles in index order)
void launch_noise_metric(const NoiseView &v, stream_t s);
uint32_t noise_tiles_x(uint32_t W);
// adaptive_sampling = 1 (adaptive.h).  The pt primary wave with the mask as an argument of its own (k_primary_packet_masked /
// k_extend_masked: Params, and every other kernel's code, stay what they were), ...
void launch_extend_masked(const Params &p, const unsigned char *mask, bool count, uint32_t max_items, stream_t s, const rt::Node4f *ordered = nullptr);
// ... k_resolve_adaptive (launch_resolve_noise for the pixels of active tiles, n_a per tile), k_present_adaptive (scale per tile), ...
void launch_resolve_adaptive(const Params &p, float *moments, const AdaptiveView &a, stream_t s);
void launch_present_adaptive(const Params &p, rt::f4 *out, const AdaptiveView &a, int full, stream_t s);
// ... the metric with n per tile (final: k_noise_final behind it, as launch_noise_metric; else the tile records alone), ...
void launch_noise_metric_adaptive(const NoiseView &v, const uint32_t *n_tile, bool final, stream_t s);
// ... and k_adaptive_step: n_tile += add on active tiles; decide: retire by the tile records
void launch_adaptive_step(const AdaptiveView &a, uint32_t add, bool decide, stream_t s);
void launch_adaptive_reset(const AdaptiveView &a, stream_t s); // n_tile = 0, every tile active
// k_adaptive_connections: behind the shade launch of `depth`, the connections of that depth are traced whatever the other tiles do
void launch_adaptive_connections(rt::WaveCounters *c, uint32_t depth, stream_t s);
// rfwhip_kat: `function` (RFWHIP_KAT_*) on n records of 24 floats -> n records of 8 floats (device pointers)
// (KAT_LT_*: the functions of k_kat_lt, RFWHIP_KAT_LT_* of rfwhip_abi.h; every other function runs in k_kat)
constexpr int KAT_LT_SAMPLE = 17, KAT_LT_PICK_PROB = 18;
constexpr int KAT_SURFACE_MAPS = 20; // (RFWHIP_KAT_SURFACE_MAPS: k_kat_maps)
void launch_kat(const Params &p, const rt::SkyView &sky, const rt::LightTreeView &lt, int function, const float *in, float *out, uint32_t n, stream_t s);
// out: local layout (local_rows x W) when full == 0, else full image (H x W; world must be 1)
void launch_present(const Params &p, rt::f4 *out, float scale, int full, stream_t s);
// the denoiser's guide pass (p: scene, camera and FrameView of the full image) = guide kernel + depth-gradient kernel
// surf != null ("denoise_motion"): the guide kernel's variant that also writes the surface record per pixel
// maps (material_maps = 1 and a material with an alpha mask): the variant that honours the mask, k_dn_guides_maps
void launch_denoise_guides(const Params &p, const DnView &d, rt::f4 *surf, stream_t s, bool maps = false);
// demodulation + variance (with t, then the temporal stage), d.iterations a-trous passes, remodulation into d.out:
// 1 (+ 1 with t) + d.iterations launches
// m != null (with t): the stage's motion variant k_dn_temporal_motion
void launch_denoise_filter(const DnView &d, const DnTemporal *t, const DnMotion *m, stream_t s);
// demodulation + the temporal stage, into d.img[0] / d.var[0] (rfwhip_read_denoise_history): 2 launches
void launch_denoise_temporal(const DnView &d, const DnTemporal &t, const DnMotion *m, stream_t s);
// the display stage: one launch of k_display (fxaa: the LDS-tiled kernel; else its halo-free pointwise variant)
void launch_display(const DisplayView &v, stream_t s);
// ... and its exposed twin k_display_exposed: every colour channel times e.rec->E in front of the tone step (metering.h)
void launch_display_exposed(const DisplayView &v, const ExposureView &e, stream_t s);
// the exposure meter (metering.h).  k_meter_hist: meter_records(v.pixels) partial records; k_meter_reduce: one workgroup sums `records`
// of them into hist (MT_RECORD words: the bins, then excluded) and takes a step on rec (rfwhip_meter_histogram
// poses a caller's histogram as one record)
uint32_t meter_records(uint32_t pixels);
void launch_meter_hist(const MeterView &v, stream_t s);
void launch_meter_reduce(const uint32_t *partial, uint32_t records, uint32_t *hist, const MeterParams &m, MeterRecord *rec, stream_t s);
constexpr int KAT_METER_BIN = 19; // (RFWHIP_KAT_METER_BIN: k_kat_meter, metering.h)
// bloom (bloom.h), one launch each: k_bloom_down0 (the image -> level 1: sanitise, prefilter, Karis weights and the 4 x 4 filter),
// k_bloom_down (level k -> k + 1), k_bloom_up (U_k over D_k), k_bloom_apply (the output image).  bloom_levels: the levels a chain runs
uint32_t bloom_levels(uint32_t W, uint32_t H, uint32_t levels);
void launch_bloom_down0(const BloomDownView &v, const BloomParams &b, stream_t s);
void launch_bloom_down(const BloomDownView &v, stream_t s);
void launch_bloom_up(const BloomUpView &v, const BloomParams &b, stream_t s);
void launch_bloom_apply(const BloomApplyView &v, const BloomParams &b, stream_t s);
// colour grading and dither (display_grade.h): k_display_graded in place of k_display / k_display_exposed, and the known-answer
// kernel k_kat_grade: n records of three floats, which = 0 (white balance, CDL, saturation) | 1 (the LUT)
void launch_display_graded(const DisplayView &v, const GradeView &g, stream_t s);
void launch_kat_grade(const GradeView &g, int which, const float *in, float *out, uint32_t n, stream_t s);
// baseline JPEG (display_jpeg.h), in this order on one stream: k_jpeg_blocks, k_jpeg_entropy, k_jpeg_offsets, k_jpeg_pack
void launch_jpeg_blocks(const JpegView &v, stream_t s);
void launch_jpeg_entropy(const JpegView &v, stream_t s);
void launch_jpeg_offsets(const JpegView &v, stream_t s);
void launch_jpeg_pack(const JpegView &v, stream_t s);
// a guide record's normal, unpacked on the host (rfwhip_read_denoise_guides)
rt::f3 dn_normal(uint32_t octahedral);
void launch_deinterleave(const rt::f4 *gathered, rt::f4 *out, uint32_t W, uint32_t H, uint32_t local_rows,
						 uint32_t world, stream_t s);
// bottom-up refit of one BLAS after its vertices changed: leaf_order[i] = original primitive of leaf slot i
// nodes / tri_verts are the scene-wide arrays (device entries carry absolute indices); node_base / tri_base locate the
// BLAS in them; parents are BLAS-relative
void launch_refit(rt::Node *nodes, uint32_t node_base, const int *parents, uint32_t node_count, rt::f4 *tri_verts,
				  uint32_t tri_base, const rt::f4 *verts, const uint32_t *indices, uint32_t tri_count, uint32_t *flags,
				  stream_t s);

// Flat instances (rfwhip_update): the triangles of a mesh whose one instance has the identity transform are reached without
// entering an instance, so every one of them carries that instance's index (w of its second leaf-ordered vertex).
void launch_stamp_instance(rt::f4 *tri_verts, uint32_t tri_count, uint32_t instance, stream_t s);

// after a refit of the BVH2 boxes: re-quantise the child boxes of the compressed 4-wide nodes of the same BLAS; src4 = four
// BLAS-relative BVH2 node indices per 4-wide node (Node4::src of the host's collapse)
void launch_refresh4(rt::Node4c *nodes4, const uint32_t *src4, uint32_t count4, const rt::Node *blas_nodes2, stream_t s);
// traversal-stack entries the packet form of the primary wave holds: the 64 lanes of one VGPR minus the sentinel at the
// bottom and two slots of slack above the top (its three-entry push writes unconditionally); the host uses the per-lane
// kernels for a scene whose trees could need more
constexpr uint32_t PACKET_STACK = 61;
// every compressed node once more with float planes (rt::Node4f), for the packet traversal's scalar fetches
void launch_expand4(const rt::Node4c *nodes4, rt::Node4f *out, uint32_t count4, stream_t s);
// the primary wave's ordering pass (primary_order.h): nodes first .. first + count - 1 of `in` into the same nodes of `out`, their
// children near to far as seen from `origin` (ordered = false: copied as they are)
void launch_order4f(const rt::Node4f *in, rt::Node4f *out, uint32_t first, uint32_t count, const float origin[3], bool ordered, stream_t s);
// the primary wave's entry snapshot pass (primary_entry.h): the records of groups 0 .. groups - 1 of the frame's slot layout
// (groups = (fr.slots << fr.sgroup_log2) / 64) into out, primary_entry_words() words each; nodes: the camera-ordered table, root:
// SceneView::tlas_root_entry, PRIMARY_ENTRY_NO_ROOT without instances
constexpr uint32_t PRIMARY_ENTRY_NO_ROOT = 0xFFFFFFFEu; // (= ENTRY_DONE of rt_core.h, which the host side does not see)
uint32_t primary_entry_words();
void launch_primary_entry(const rt::Node4f *nodes, uint32_t root, const rt::CamView &cam, const rt::FrameView &fr, uint32_t *out, uint32_t groups, stream_t s);
// BVH construction on the device (lbvh.hip), end to end in mesh-local arrays (node_base = tri_base = n4_base = 0):
//   nodes / parents / flags   2 n entries   BVH2 in the reference's layout, device entries, one triangle per leaf
//   nodes4 / src4             <= n / 4 n    the compressed 4-wide nodes the rays fetch, breadth-first, + their BVH2 sources
//   tri_verts                 3 n           triangles in leaf (depth-first) order, w of vertex 0 = primitive id
// Only the result record comes back (the call synchronises the stream).  Returns 0, or 1 when the mesh has fewer than two
// triangles (build it on the host), > 1 on an error.
struct DeviceBuildResult
{
	uint32_t node_count, node4_count, stack_need;
	float bmin[3], bmax[3];
};
size_t device_build_scratch_bytes(uint32_t tri_count);
int launch_device_build(const rt::f4 *verts, const uint32_t *indices, uint32_t tri_count, void *scratch, size_t scratch_bytes,
						rt::Node *nodes, int *parents, uint32_t *flags, rt::Node4c *nodes4, uint32_t *src4, rt::f4 *tri_verts,
						DeviceBuildResult *out, stream_t s);
// mesh-local entries -> scene-wide indices, in place (rfwhip_update places a device-built mesh with two copies and this)
void launch_rebase(rt::Node *nodes, uint32_t node_count, uint32_t node_base, rt::Node4c *nodes4, uint32_t n4_count, uint32_t n4_base,
				   uint32_t tri_base, stream_t s);
// linear-blend skinning on the device (geometry/gltf/mesh.cpp:31-45): verts/vnormals <- base * sum(w_k * M[j_k]);
// mats: joint_count column-major 4x4
void launch_skin_vertices(rt::f4 *verts, rt::f4 *vnormals, const rt::f4 *base_verts, const rt::f4 *base_normals,
						  const uint32_t *joints4, const rt::f4 *weights4, const float *mats, uint32_t joint_count,
						  uint32_t vertex_count, stream_t s);
// morph targets on the device (geometry/gltf/mesh.cpp:127-147): verts / vnormals <- base + sum_j weights[j] * target_j;
// tgt_pos / tgt_nrm: [target][vertex] float4, weights: device array of target_count floats
void launch_morph_vertices(rt::f4 *verts, rt::f4 *vnormals, const rt::f4 *base_verts, const rt::f4 *base_normals,
						   const rt::f4 *tgt_pos, const rt::f4 *tgt_nrm, const float *weights, uint32_t target_count,
						   uint32_t vertex_count, stream_t s);
// update_triangles() of the same file for the shading records: vertex normals of the three corners + face normal
void launch_skin_shade(rt::TriShade *shade, const rt::f4 *verts, const rt::f4 *vnormals, const uint32_t *indices,
					   uint32_t tri_count, stream_t s);

// Moving emitters (setting "lights_follow_geometry"; work items: light_follow.h; formulas: include/rfwhip.h).
// One record per instance slot: the transform and normal matrix of the last rfwhip_set_instance (rows 0..2, row-major, the normal
// matrix's rows padded to four floats) and the mesh's current object-space vertices — the arrays the temporal stage's motion
// table points at (DnMotionInst::cur / indices), with the same rule for "the vertices of triangle k".  tri_count == 0: not in use.
struct alignas(16) LightInst
{
	float m[12], nrm[12];
	const rt::f4 *verts;
	const uint32_t *indices; // three per triangle, or null: triangle k has the vertices 3 k .. 3 k + 2
	uint32_t tri_count, shade_base;
	uint32_t pad[2];
};
struct LightFollowView
{
	rt::AreaLight *area; // the lights of the last rfwhip_set_lights: bound ones are rewritten in place
	const LightInst *inst;
	rt::TriShade *tri_shade; // scene-wide: a bound triangle's area (ex.x) is written beside its light's
	unsigned char *bound;	 // per area light: 1 bound, 0 unbound
	uint32_t *bound_count;	 // zeroed by the caller in front of the launch; the bound lights are added to it
	uint32_t n_area, n_inst;
};
// k_light_refresh: one area light per lane
void launch_light_refresh(const LightFollowView &v, stream_t s);
// The light tree's levels (light_tree.h lays the nodes out breadth first): level l is nodes [first[l], first[l] + count[l])
constexpr uint32_t LT_MAX_LEVELS = 32;
struct LightTreeLevels
{
	uint32_t first[LT_MAX_LEVELS], count[LT_MAX_LEVELS];
	uint32_t levels;
};
// Bottom-up refit of lo / hi / axis / cos_o over the existing topology: a leaf of a bound area light from its light, an inner node
// with such a leaf below from its two children; every other node keeps its bytes.  touched: one byte per node (scratch).  Levels
// wider than a workgroup get a launch each, deepest first; the levels above them run in ONE workgroup with a barrier between
// levels (k_lt_refit_top)
void launch_light_tree_refit(rt::LightTreeNode *nodes, const LightTreeLevels &lv, const rt::AreaLight *area, uint32_t n_area,
							 const unsigned char *bound, unsigned char *touched, stream_t s);

// image textures (texture_decode.h, kernel family 15), in this order on one stream: k_texdec_zero, k_texdec_entropy (the device path of
// the entropy decoding), k_texdec_idct, k_texdec_color (with v.src: the modifiers over an RGBA8 source), k_tex_mips, k_texdec_finish
struct TexdecView;
void launch_texdec_zero(const TexdecView &v, stream_t s);
void launch_texdec_entropy(const TexdecView &v, stream_t s);
void launch_texdec_idct(const TexdecView &v, stream_t s);
void launch_texdec_color(const TexdecView &v, stream_t s);
void launch_tex_mips(const TexdecView &v, stream_t s);
void launch_texdec_finish(const TexdecView &v, stream_t s);

// the sky's loaders (sky_load.h, kernel family 17).  A Radiance HDR decode: k_skyhdr_planes (skipped when every scanline is flat),
// k_skyhdr_texels.  The alias table: k_skytab_weights, k_skytab_total, k_skytab_scan_block, k_skytab_scan_super, k_skytab_scan_top,
// k_skytab_scan_apply, k_skytab_assign, in this order on one stream
struct SkyHdrView;
struct SkyTabView;
void launch_skyhdr_planes(const SkyHdrView &v, stream_t s);
void launch_skyhdr_texels(const SkyHdrView &v, stream_t s);
void launch_skytab_weights(const SkyTabView &v, stream_t s);
void launch_skytab_total(const SkyTabView &v, stream_t s);
void launch_skytab_scan_block(const SkyTabView &v, stream_t s);
void launch_skytab_scan_super(const SkyTabView &v, stream_t s);
void launch_skytab_scan_top(const SkyTabView &v, stream_t s);
void launch_skytab_scan_apply(const SkyTabView &v, stream_t s);
void launch_skytab_assign(const SkyTabView &v, stream_t s);

// animations (animation.h, kernel family 18).  k_rig_evaluate: ONE launch, a workgroup per entry of `calls`; table: the context's
// rigs by index (device memory, like calls)
struct RigView;
struct RigCall;
void launch_rig_evaluate(const RigView *table, const RigCall *calls, uint32_t count, stream_t s);

} // namespace rtk

// the types, the marker walk and the work items of the image textures (part 1 of the file)
#include "texture_decode.h"
// the types, the header walk and the work items of the sky's loaders (part 1 of the file)
#include "sky_load.h"
// the types, the validator and the work items of the animations (part 1 of the file)
#include "animation.h"
