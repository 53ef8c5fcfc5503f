// animation.h — glTF animations evaluated on the device: keyframes to joint matrices and morph weights (include/rfwhip.h,
// rfwhip_set_rig / rfwhip_bind_rig / rfwhip_animate / rfwhip_read_rig).  Kernel family 18.
//
// The file has two parts.  PART 1 (types, the host's validator, the work items, and the items run serially over plain host arrays) is
// included by kernels.h at file scope and needs nothing but this file: tests/animation_san_main.cpp includes it alone.  PART 2 (the
// HIP kernel and its launcher, or the emulation's launcher) is included by kernels.hip inside namespace rtk with
// ANIMATION_LAUNCHERS defined.  The kernel and the emulation run the same items in the same order.
//
// THE RULE is the one gltf.py follows (geometry/gltf/animation.cpp:231-322, 374-422 of the reference), as a function of the time
// alone — no key cursor survives a call.  Per channel, with its own key times t[0 .. n-1] (strictly increasing, validated):
//   time      if time > t[n-1] and t[n-1] > 0: time = fmodf(time, t[n-1]) (exact)
//   segment   k = the number of j in [1, n-2] with time > t[j], by a binary search of at most 32 steps
//   fraction  d = t[k+1] - t[k], f = (time - t[k]) / d; n == 1 or f <= 0: the FIRST key's value
//   STEP key k; LINEAR fmaf(f, b, R((1 - f) a)); CUBICSPLINE with t2 = R(f f), t3 = R(t2 f), m0 = R(d out_k), m1 = R(d in_k+1):
//     h10 = fmaf(-2, t2, t3) + f, h00 = fmaf(2, t3, fmaf(-3, t2, 1)), h01 = fmaf(-2, t3, R(3 t2)), h11 = t3 - t2,
//     value = fmaf(m1, h11, fmaf(p1, h01, fmaf(p0, h00, R(m0 h10))))
//   rotations are sampled per component like every other path and then divided by n = sqrtf(fmaf(w, w, fmaf(z, z, fmaf(y, y, R(x x)))))
//     (no slerp, no transcendental function); n zero or not finite: the identity (0, 0, 0, 1), counted in the status record.
//   The sampled value replaces the node's base translation, rotation, scale or weights.  A weights key holds the node's weight_count
//   scalars; a CUBICSPLINE one holds (in-tangent, value, out-tangent) per target, target after target.
// Per node:  local = T R S M.  R as gltf.py's _quat_to_mat: every product of two components rounded on its own (xx = R(x x), ...),
//   the diagonal 1 - 2 (yy + zz), the rest 2 (xy -+ zw); column j of R times s_j, one rounding; [RS | t] times the node's constant
//   matrix by the PRODUCT shape: c[r][c] = fmaf(a[r][3], b[3][c], fmaf(a[r][2], b[2][c], fmaf(a[r][1], b[1][c], R(a[r][0] b[0][c])))).
//   world[i] = world[parent] local[i], the same shape, level by level in the validator's depth-sorted order; a root's world is its local.
// Per skin:  inv = the closed affine inverse of world[mesh_node]: cofactors fmaf(a, b, -R(c d)) of the upper 3 x 3, det =
//   fmaf(a02, C02, fmaf(a01, C01, R(a00 C00))), inv3 = adjugate / det entry by entry, translation -(fmaf(i2, t2, fmaf(i1, t1, R(i0 t0)))),
//   last row 0 0 0 1.  det zero or not finite: the identity, counted in the status record.
// Per joint:  (inv world[joint]) ibm, two products of the shape above, stored column-major as launch_skin_vertices reads it.
// R(x) is rounded() of rt_core.h: a product rounded on its own, hidden from the compiler's contraction; fmaf is fused; division and
// square root are IEEE in every build.  Nothing else is left to the compiler, so EVERY value this file writes — local TRS, weights,
// world matrices, joint matrices, the status record — has the same bytes in the shipped build, the validation build and the
// emulation.
//
// LAUNCH  k_rig_evaluate: one workgroup of RIG_THREADS lanes per listed rig, every lane loops over its items in strides of the
// workgroup: reset (base TRS and weights), barrier, channels, barrier, locals, barrier, one barrier per level of the hierarchy,
// inverses, barrier, joints, and one lane writes the status record.  Local and world matrices live in LDS for rigs of at most
// RIG_LDS_NODES = 320 nodes: 2 x 64 B x 320 = 40 KiB of the CU's 160 KiB, four workgroups per CU; a larger rig uses its own global
// scratch range with the same items (a workgroup barrier orders global accesses of the workgroup as well).  No atomics, no
// recursion; every loop is bounded by a count the validator has checked.
#ifndef RFWHIP_ANIMATION_H
#define RFWHIP_ANIMATION_H

#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#ifndef RT_FN
#define RT_FN inline
#endif

namespace rtk
{

constexpr int RIG_OK = 0, RIG_INVALID = 1; // = RFWHIP_OK, RFWHIP_ERR_INVALID_ARGUMENT
// = RFWHIP_RIG_PATH_*, RFWHIP_RIG_METHOD_*, RFWHIP_RIG_READ_*
constexpr uint32_t RIG_TRANSLATION = 0u, RIG_ROTATION = 1u, RIG_SCALE = 2u, RIG_WEIGHTS = 3u;
constexpr uint32_t RIG_STEP = 0u, RIG_LINEAR = 1u, RIG_CUBICSPLINE = 2u;
constexpr uint32_t RIG_READ_TRS = 0u, RIG_READ_WORLD = 1u, RIG_READ_JOINTS = 2u, RIG_READ_WEIGHTS = 3u, RIG_READ_STATUS = 4u;
constexpr uint32_t RIG_BASE_POSE = 0xFFFFFFFFu; // = RFWHIP_RIG_BASE_POSE
constexpr uint32_t RIG_THREADS = 256u;
constexpr uint32_t RIG_LDS_NODES = 320u; // the LDS budget: two 4 x 4 float matrices per node, 40 KiB
constexpr uint32_t RIG_TRS = 10u;		 // floats of a node's local TRS: translation, rotation xyzw, scale

// = rfwhip_rig_node ... rfwhip_rig_status (include/rfwhip_abi.h), which part 1 does not see
struct RigNode
{
	int32_t parent;
	float translation[3], rotation[4], scale[3];
	uint32_t weight_offset;
	float matrix[16]; // column-major
	uint32_t weight_count, reserved[3];
};
struct RigSkin
{
	uint32_t mesh_node, joint_offset, joint_count, reserved;
};
struct RigAnim
{
	uint32_t channel_offset, channel_count;
};
struct RigChannel
{
	uint32_t node, path, method, key_count, time_offset, value_offset, value_count, reserved;
};
struct RigStatus
{
	float time;						// the given time after the wrap of the animation's first channel (as given for a base pose)
	uint32_t rotation_fallbacks;	// sampled rotations of zero or non-finite norm: the identity instead
	uint32_t inverse_fallbacks;		// skins whose mesh node had a zero or non-finite determinant: the identity instead
	uint32_t serial;				// counts the evaluations of this rig, from 1 (the record is zeroed with the rig; the kernel adds 1)
	uint32_t animation, reserved[3];
};
static_assert(sizeof(RigNode) == 128 && sizeof(RigSkin) == 16 && sizeof(RigAnim) == 8 && sizeof(RigChannel) == 32 && sizeof(RigStatus) == 32,
			  "the rig's records");
// = rfwhip_rig: the flat tables as a host hands them over
struct RigSource
{
	const RigNode *nodes;
	size_t node_count;
	const float *weights;
	size_t weight_count;
	const RigSkin *skins;
	size_t skin_count;
	const uint32_t *joints;
	const float *inverse_bind; // 16 floats per entry of `joints`, column-major
	size_t joint_count;
	const RigAnim *animations;
	size_t animation_count;
	const RigChannel *channels;
	size_t channel_count;
	const float *times;
	size_t time_count;
	const float *values;
	size_t value_count;
};
// One rig on the device.  The tables above, what the validator adds (order: the nodes sorted by depth; level_first: levels + 1
// offsets into it; item_skin / item_joint: per joint matrix to write, its skin and its entry of `joints`), and what an evaluation
// writes: trs, weights, world, joint_mats (item after item: skin after skin), status; local / inv / flags are scratch.
struct RigView
{
	const RigNode *nodes;
	const float *base_weights;
	const RigSkin *skins;
	const uint32_t *joints;
	const float *ibm;
	const RigAnim *anims;
	const RigChannel *channels;
	const float *times, *values;
	const uint32_t *order, *level_first, *item_skin, *item_joint;
	float *trs, *weights, *world, *local, *inv, *joint_mats;
	uint32_t *flags; // one word per channel of the rig, then one per skin
	RigStatus *status;
	uint32_t node_count, weight_count, skin_count, item_count, anim_count, channel_count, levels, pad;
};
// one entry of a call: these twelve bytes are all that travels per rig and frame
struct RigCall
{
	uint32_t rig, animation;
	float time;
};
static_assert(sizeof(RigCall) == 12, "a (rig, animation, time) triple");

RT_FN uint32_t rig_width(const RigNode &n, uint32_t path) { return path == RIG_ROTATION ? 4u : path == RIG_WEIGHTS ? n.weight_count : 3u; }

// ---- the host's validator -----------------------------------------------------------------------------------------------------
struct RigPlan
{
	std::vector<uint32_t> depth, order, level_first, item_skin, item_joint, out_offset; // out_offset: per skin, its first item
	uint32_t levels = 0;
	char msg[192] = {};
};
inline int rig_fail(RigPlan &o, const char *fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(o.msg, sizeof(o.msg), fmt, ap);
	va_end(ap);
	return RIG_INVALID;
}
inline bool rig_range(size_t offset, size_t count, size_t size) { return offset <= size && count <= size - offset; }
inline int rig_validate(const RigSource &r, RigPlan &o)
{
	static const char *const PATHS[4] = {"translation", "rotation", "scale", "weights"};
	constexpr size_t LIMIT = (size_t)1 << 28;
	if (!r.nodes || !r.node_count)
		return rig_fail(o, "a rig needs at least one node");
	if (r.node_count > LIMIT || r.weight_count > LIMIT || r.skin_count > LIMIT || r.joint_count > LIMIT || r.animation_count > LIMIT ||
		r.channel_count > LIMIT || r.time_count > LIMIT || r.value_count > LIMIT)
		return rig_fail(o, "a table with more than 2^28 entries");
	if ((r.weight_count && !r.weights) || (r.skin_count && !r.skins) || (r.joint_count && (!r.joints || !r.inverse_bind)) ||
		(r.animation_count && !r.animations) || (r.channel_count && !r.channels) || (r.time_count && !r.times) || (r.value_count && !r.values))
		return rig_fail(o, "a count > 0 with a null table");
	const uint32_t n = (uint32_t)r.node_count, UNKNOWN = 0xFFFFFFFFu;
	for (uint32_t i = 0; i < n; i++)
	{
		const RigNode &nd = r.nodes[i];
		if (nd.parent < -1 || nd.parent >= (int32_t)n)
			return rig_fail(o, "node %u: parent %d out of range (%u nodes)", i, nd.parent, n);
		if (!rig_range(nd.weight_offset, nd.weight_count, r.weight_count))
			return rig_fail(o, "node %u: weights %u + %u out of range (%zu weights)", i, nd.weight_offset, nd.weight_count, r.weight_count);
	}
	// depths, each node once: walk up to a node of known depth (or a root), then number the path on the way back
	o.depth.assign(n, UNKNOWN);
	std::vector<uint8_t> on_path(n, 0);
	std::vector<uint32_t> path;
	for (uint32_t i = 0; i < n; i++)
	{
		path.clear();
		int32_t j = (int32_t)i;
		while (j >= 0 && o.depth[(uint32_t)j] == UNKNOWN && !on_path[(uint32_t)j])
			on_path[(uint32_t)j] = 1, path.push_back((uint32_t)j), j = r.nodes[j].parent;
		if (j >= 0 && o.depth[(uint32_t)j] == UNKNOWN)
			return rig_fail(o, "node %d: parent cycle", j);
		uint32_t d = j < 0 ? 0u : o.depth[(uint32_t)j] + 1u;
		for (size_t k = path.size(); k-- > 0;)
			o.depth[path[k]] = d++, on_path[path[k]] = 0;
	}
	o.levels = 0;
	for (uint32_t i = 0; i < n; i++)
		o.levels = o.depth[i] + 1u > o.levels ? o.depth[i] + 1u : o.levels;
	o.level_first.assign(o.levels + 1u, 0u);
	for (uint32_t i = 0; i < n; i++)
		o.level_first[o.depth[i] + 1u]++;
	for (uint32_t l = 0; l < o.levels; l++)
		o.level_first[l + 1u] += o.level_first[l];
	o.order.assign(n, 0u);
	{
		std::vector<uint32_t> next(o.level_first.begin(), o.level_first.end() - 1);
		for (uint32_t i = 0; i < n; i++)
			o.order[next[o.depth[i]]++] = i;
	}
	// skins
	o.item_skin.clear(), o.item_joint.clear(), o.out_offset.clear();
	for (uint32_t s = 0; s < (uint32_t)r.skin_count; s++)
	{
		const RigSkin &sk = r.skins[s];
		if (sk.mesh_node >= n)
			return rig_fail(o, "skin %u: mesh node %u out of range (%u nodes)", s, sk.mesh_node, n);
		if (!sk.joint_count)
			return rig_fail(o, "skin %u has no joints", s);
		if (!rig_range(sk.joint_offset, sk.joint_count, r.joint_count))
			return rig_fail(o, "skin %u: joints %u + %u out of range (%zu joints)", s, sk.joint_offset, sk.joint_count, r.joint_count);
		o.out_offset.push_back((uint32_t)o.item_skin.size());
		for (uint32_t j = 0; j < sk.joint_count; j++)
		{
			if (r.joints[sk.joint_offset + j] >= n)
				return rig_fail(o, "skin %u: joint %u is node %u (%u nodes)", s, j, r.joints[sk.joint_offset + j], n);
			o.item_skin.push_back(s), o.item_joint.push_back(sk.joint_offset + j);
		}
		if (o.item_skin.size() > LIMIT)
			return rig_fail(o, "skin %u: more than 2^28 joint matrices", s);
	}
	// channels
	for (uint32_t c = 0; c < (uint32_t)r.channel_count; c++)
	{
		const RigChannel &ch = r.channels[c];
		if (ch.node >= n)
			return rig_fail(o, "channel %u: node %u out of range (%u nodes)", c, ch.node, n);
		if (ch.path > RIG_WEIGHTS)
			return rig_fail(o, "channel %u: path %u is none of translation, rotation, scale, weights", c, ch.path);
		if (ch.method > RIG_CUBICSPLINE)
			return rig_fail(o, "channel %u: method %u is none of STEP, LINEAR, CUBICSPLINE", c, ch.method);
		if (!ch.key_count)
			return rig_fail(o, "channel %u: key_count is 0", c);
		if (!rig_range(ch.time_offset, ch.key_count, r.time_count))
			return rig_fail(o, "channel %u: key times %u + %u out of range (%zu times)", c, ch.time_offset, ch.key_count, r.time_count);
		for (uint32_t k = 0; k < ch.key_count; k++)
		{
			const float t = r.times[ch.time_offset + k];
			if (!(t - t == 0.0f))
				return rig_fail(o, "channel %u: key time %u is not finite", c, k);
			if (k && !(t > r.times[ch.time_offset + k - 1u]))
				return rig_fail(o, "channel %u: key time %u is not greater than its predecessor", c, k);
		}
		const uint32_t w = rig_width(r.nodes[ch.node], ch.path);
		if (!w)
			return rig_fail(o, "channel %u: a weights channel on node %u, which has no weights", c, ch.node);
		const size_t want = (size_t)w * ch.key_count * (ch.method == RIG_CUBICSPLINE ? 3u : 1u);
		if (ch.value_count != want)
			return rig_fail(o, "channel %u: %u values, %s x %s x %u keys needs %zu", c, ch.value_count, PATHS[ch.path],
							ch.method == RIG_CUBICSPLINE ? "CUBICSPLINE" : ch.method == RIG_LINEAR ? "LINEAR" : "STEP", ch.key_count, want);
		if (!rig_range(ch.value_offset, ch.value_count, r.value_count))
			return rig_fail(o, "channel %u: values %u + %u out of range (%zu values)", c, ch.value_offset, ch.value_count, r.value_count);
	}
	// animations: ranges of channels; two channels of one animation on the same (node, path) would be two lanes writing one value
	std::vector<uint32_t> seen(4u * (size_t)n, UNKNOWN);
	for (uint32_t a = 0; a < (uint32_t)r.animation_count; a++)
	{
		const RigAnim &an = r.animations[a];
		if (!rig_range(an.channel_offset, an.channel_count, r.channel_count))
			return rig_fail(o, "animation %u: channels %u + %u out of range (%zu channels)", a, an.channel_offset, an.channel_count, r.channel_count);
		for (uint32_t c = an.channel_offset; c < an.channel_offset + an.channel_count; c++)
		{
			uint32_t &slot = seen[4u * (size_t)r.channels[c].node + r.channels[c].path];
			if (slot == a)
				return rig_fail(o, "channel %u: animation %u has another %s channel on node %u", c, a, PATHS[r.channels[c].path], r.channels[c].node);
			slot = a;
		}
	}
	return RIG_OK;
}

// ---- arithmetic with a fixed shape ---------------------------------------------------------------------------------------------
// rt_core.h's rounded(), restated because this part stands alone: an empty asm hides the product from the contraction pass
RT_FN float rig_r(float x)
{
#if defined(__HIP_DEVICE_COMPILE__)
	asm("" : "+v"(x));
#elif defined(__x86_64__)
	asm("" : "+x"(x));
#else
	volatile float y = x;
	x = y;
#endif
	return x;
}
RT_FN bool rig_finite(float x) { return x - x == 0.0f; }
// c = a b, column-major 4 x 4: the PRODUCT shape of the header
RT_FN void rig_mul(float *c, const float *a, const float *b)
{
	for (int col = 0; col < 4; col++)
		for (int row = 0; row < 4; row++)
			c[4 * col + row] = fmaf(a[12 + row], b[4 * col + 3],
									fmaf(a[8 + row], b[4 * col + 2], fmaf(a[4 + row], b[4 * col + 1], rig_r(a[row] * b[4 * col]))));
}
RT_FN void rig_identity(float *m)
{
	for (int i = 0; i < 16; i++)
		m[i] = (i % 5) ? 0.0f : 1.0f;
}

// ---- the work items --------------------------------------------------------------------------------------------------------------
// node i back to its base TRS; weight w back to its base
RT_FN void rig_reset_node(const RigView &v, uint32_t i)
{
	const RigNode &n = v.nodes[i];
	float *o = v.trs + (size_t)RIG_TRS * i;
	o[0] = n.translation[0], o[1] = n.translation[1], o[2] = n.translation[2];
	o[3] = n.rotation[0], o[4] = n.rotation[1], o[5] = n.rotation[2], o[6] = n.rotation[3];
	o[7] = n.scale[0], o[8] = n.scale[1], o[9] = n.scale[2];
}
RT_FN void rig_reset_weight(const RigView &v, uint32_t w) { v.weights[w] = v.base_weights[w]; }

RT_FN float rig_wrap(float time, float duration) { return (time > duration && duration > 0.0f) ? fmodf(time, duration) : time; }
// the number of j in [1, n - 2] with time > t[j]
RT_FN uint32_t rig_segment(const float *t, uint32_t n, float time)
{
	uint32_t lo = 1u, hi = n >= 2u ? n - 1u : 1u; // the first j in [lo, hi) with !(time > t[j]), or hi
	for (int step = 0; step < 32 && lo < hi; step++)
	{
		const uint32_t mid = lo + ((hi - lo) >> 1);
		if (time > t[mid])
			lo = mid + 1u;
		else
			hi = mid;
	}
	return lo - 1u;
}
// one component: a / b the values of keys k and k + 1, out_a / in_b their tangents (CUBICSPLINE only)
RT_FN float rig_blend(uint32_t method, float f, float d, float a, float b, float out_a, float in_b)
{
	if (method == RIG_STEP)
		return a;
	if (method == RIG_LINEAR)
		return fmaf(f, b, rig_r((1.0f - f) * a));
	const float t2 = rig_r(f * f), t3 = rig_r(t2 * f);
	const float m0 = rig_r(d * out_a), m1 = rig_r(d * in_b);
	const float h10 = fmaf(-2.0f, t2, t3) + f, h00 = fmaf(2.0f, t3, fmaf(-3.0f, t2, 1.0f)), h01 = fmaf(-2.0f, t3, rig_r(3.0f * t2)), h11 = t3 - t2;
	return fmaf(m1, h11, fmaf(b, h01, fmaf(a, h00, rig_r(m0 * h10))));
}
// channel c of the rig at `time`; returns 1 when a rotation fell back to the identity.  first: the channel that reports the time
RT_FN uint32_t rig_channel_item(const RigView &v, uint32_t c, float time, bool first)
{
	const RigChannel ch = v.channels[c];
	const RigNode &nd = v.nodes[ch.node];
	const float *t = v.times + ch.time_offset, *val = v.values + ch.value_offset;
	const uint32_t n = ch.key_count, w = rig_width(nd, ch.path);
	const bool cubic = ch.method == RIG_CUBICSPLINE, scalar = ch.path == RIG_WEIGHTS;
	time = rig_wrap(time, t[n - 1u]);
	if (first)
		v.status->time = time;
	uint32_t k = 0u;
	float f = 0.0f, d = 0.0f;
	if (n > 1u)
	{
		k = rig_segment(t, n, time);
		d = t[k + 1u] - t[k];
		f = (time - t[k]) / d;
	}
	const bool head = n == 1u || f <= 0.0f; // the first key's value
	if (head)
		k = 0u;
	float out[4] = {0.0f, 0.0f, 0.0f, 0.0f};
	float *dst = scalar ? v.weights + nd.weight_offset : v.trs + (size_t)RIG_TRS * ch.node + (ch.path == RIG_TRANSLATION ? 0u : ch.path == RIG_ROTATION ? 3u : 7u);
	for (uint32_t i = 0; i < w; i++)
	{
		// a key's entries: vectors are rows of w floats, three rows (in, value, out) per CUBICSPLINE key; a weights key holds
		// (in, value, out) per target
		const size_t a0 = scalar ? ((size_t)k * w + i) * (cubic ? 3u : 1u) : ((size_t)k * (cubic ? 3u : 1u)) * w + i;
		const size_t step = scalar ? 1u : w;				   // from in-tangent to value to out-tangent
		const size_t key = (size_t)w * (cubic ? 3u : 1u); // from key k to key k + 1
		const float a = val[a0 + (cubic ? step : 0u)];
		float x = a;
		if (!head && ch.method != RIG_STEP)
		{
			const float b = val[a0 + key + (cubic ? step : 0u)];
			x = rig_blend(ch.method, f, d, a, b, cubic ? val[a0 + 2u * step] : 0.0f, cubic ? val[a0 + key] : 0.0f);
		}
		if (ch.path == RIG_ROTATION)
			out[i] = x;
		else
			dst[i] = x;
	}
	if (ch.path != RIG_ROTATION)
		return 0u;
	const float len = sqrtf(fmaf(out[3], out[3], fmaf(out[2], out[2], fmaf(out[1], out[1], rig_r(out[0] * out[0])))));
	const bool ok = len > 0.0f && rig_finite(len);
	dst[0] = ok ? out[0] / len : 0.0f, dst[1] = ok ? out[1] / len : 0.0f, dst[2] = ok ? out[2] / len : 0.0f, dst[3] = ok ? out[3] / len : 1.0f;
	return ok ? 0u : 1u;
}
// local[i] = T R S M
RT_FN void rig_local_item(const RigView &v, float *local, uint32_t i)
{
	const float *p = v.trs + (size_t)RIG_TRS * i;
	const float x = p[3], y = p[4], z = p[5], w = p[6];
	const float xx = rig_r(x * x), yy = rig_r(y * y), zz = rig_r(z * z), xy = rig_r(x * y), xz = rig_r(x * z), yz = rig_r(y * z);
	const float xw = rig_r(x * w), yw = rig_r(y * w), zw = rig_r(z * w);
	float a[16];
	a[0] = rig_r((1.0f - 2.0f * (yy + zz)) * p[7]), a[1] = rig_r((2.0f * (xy + zw)) * p[7]), a[2] = rig_r((2.0f * (xz - yw)) * p[7]), a[3] = 0.0f;
	a[4] = rig_r((2.0f * (xy - zw)) * p[8]), a[5] = rig_r((1.0f - 2.0f * (xx + zz)) * p[8]), a[6] = rig_r((2.0f * (yz + xw)) * p[8]), a[7] = 0.0f;
	a[8] = rig_r((2.0f * (xz + yw)) * p[9]), a[9] = rig_r((2.0f * (yz - xw)) * p[9]), a[10] = rig_r((1.0f - 2.0f * (xx + yy)) * p[9]), a[11] = 0.0f;
	a[12] = p[0], a[13] = p[1], a[14] = p[2], a[15] = 1.0f;
	rig_mul(local + 16u * (size_t)i, a, v.nodes[i].matrix);
}
// entry `slot` of the depth-sorted order: world = world[parent] local (a root: its local)
RT_FN void rig_world_item(const RigView &v, const float *local, float *world, uint32_t slot)
{
	const uint32_t i = v.order[slot];
	const int32_t parent = v.nodes[i].parent;
	float *o = world + 16u * (size_t)i;
	if (parent < 0)
		for (int k = 0; k < 16; k++)
			o[k] = local[16u * (size_t)i + k];
	else
		rig_mul(o, world + 16u * (size_t)parent, local + 16u * (size_t)i);
}
// skin s: the affine inverse of its mesh node's world matrix; returns 1 when it fell back to the identity
RT_FN uint32_t rig_inverse_item(const RigView &v, const float *world, uint32_t s)
{
	const float *m = world + 16u * (size_t)v.skins[s].mesh_node;
	float *o = v.inv + 16u * (size_t)s;
	// a[r][c] = m[4 c + r]; C_rc: the cofactor of a[r][c]
	const float a00 = m[0], a10 = m[1], a20 = m[2], a01 = m[4], a11 = m[5], a21 = m[6], a02 = m[8], a12 = m[9], a22 = m[10];
	const float C00 = fmaf(a11, a22, -rig_r(a12 * a21)), C01 = fmaf(a12, a20, -rig_r(a10 * a22)), C02 = fmaf(a10, a21, -rig_r(a11 * a20));
	const float C10 = fmaf(a02, a21, -rig_r(a01 * a22)), C11 = fmaf(a00, a22, -rig_r(a02 * a20)), C12 = fmaf(a01, a20, -rig_r(a00 * a21));
	const float C20 = fmaf(a01, a12, -rig_r(a02 * a11)), C21 = fmaf(a02, a10, -rig_r(a00 * a12)), C22 = fmaf(a00, a11, -rig_r(a01 * a10));
	const float det = fmaf(a02, C02, fmaf(a01, C01, rig_r(a00 * C00)));
	if (!(det != 0.0f && rig_finite(det)))
	{
		rig_identity(o);
		return 1u;
	}
	// inv3[r][c] = C_cr / det
	const float i00 = C00 / det, i01 = C10 / det, i02 = C20 / det;
	const float i10 = C01 / det, i11 = C11 / det, i12 = C21 / det;
	const float i20 = C02 / det, i21 = C12 / det, i22 = C22 / det;
	const float t0 = m[12], t1 = m[13], t2 = m[14];
	o[0] = i00, o[1] = i10, o[2] = i20, o[3] = 0.0f;
	o[4] = i01, o[5] = i11, o[6] = i21, o[7] = 0.0f;
	o[8] = i02, o[9] = i12, o[10] = i22, o[11] = 0.0f;
	o[12] = -fmaf(i02, t2, fmaf(i01, t1, rig_r(i00 * t0)));
	o[13] = -fmaf(i12, t2, fmaf(i11, t1, rig_r(i10 * t0)));
	o[14] = -fmaf(i22, t2, fmaf(i21, t1, rig_r(i20 * t0)));
	o[15] = 1.0f;
	return 0u;
}
// joint matrix `item`: (inv[skin] world[joint]) ibm
RT_FN void rig_joint_item(const RigView &v, const float *world, uint32_t item)
{
	const uint32_t j = v.item_joint[item];
	float t[16];
	rig_mul(t, v.inv + 16u * (size_t)v.item_skin[item], world + 16u * (size_t)v.joints[j]);
	rig_mul(v.joint_mats + 16u * (size_t)item, t, v.ibm + 16u * (size_t)j);
}
// the channels of a call: [first, first + count)
RT_FN void rig_call_channels(const RigView &v, const RigCall &call, uint32_t &first, uint32_t &count)
{
	first = count = 0u;
	if (call.animation != RIG_BASE_POSE && call.animation < v.anim_count)
		first = v.anims[call.animation].channel_offset, count = v.anims[call.animation].channel_count;
}
// the status record, by one lane behind everything else: the flag words are added up left to right
RT_FN void rig_status_item(const RigView &v, const RigCall &call, uint32_t chan_first, uint32_t chan_count)
{
	uint32_t rot = 0u, inv = 0u;
	for (uint32_t c = 0; c < chan_count; c++)
		rot += v.flags[chan_first + c];
	for (uint32_t s = 0; s < v.skin_count; s++)
		inv += v.flags[v.channel_count + s];
	RigStatus st = *v.status;
	if (!chan_count)
		st.time = call.time;
	st.rotation_fallbacks = rot, st.inverse_fallbacks = inv, st.serial = st.serial + 1u, st.animation = chan_count ? call.animation : RIG_BASE_POSE;
	st.reserved[0] = st.reserved[1] = st.reserved[2] = 0u;
	*v.status = st;
}

// ---- the items run serially over host arrays (the emulation, the stand-alone program): a rig at a time, phase after phase ----
inline void rig_host_evaluate(const RigView *table, const RigCall *calls, uint32_t count)
{
	for (uint32_t b = 0; b < count; b++)
	{
		const RigCall call = calls[b];
		const RigView v = table[call.rig];
		uint32_t first, n;
		rig_call_channels(v, call, first, n);
		for (uint32_t i = 0; i < v.node_count; i++)
			rig_reset_node(v, i);
		for (uint32_t w = 0; w < v.weight_count; w++)
			rig_reset_weight(v, w);
		for (uint32_t c = 0; c < n; c++)
			v.flags[first + c] = rig_channel_item(v, first + c, call.time, c == 0u);
		for (uint32_t i = 0; i < v.node_count; i++)
			rig_local_item(v, v.local, i);
		for (uint32_t slot = 0; slot < v.node_count; slot++)
			rig_world_item(v, v.local, v.world, slot);
		for (uint32_t s = 0; s < v.skin_count; s++)
			v.flags[v.channel_count + s] = rig_inverse_item(v, v.world, s);
		for (uint32_t item = 0; item < v.item_count; item++)
			rig_joint_item(v, v.world, item);
		rig_status_item(v, call, first, n);
	}
}

} // namespace rtk
#endif // RFWHIP_ANIMATION_H

// =================================================================================================================================
// PART 2: the kernel and the launcher (kernels.hip, inside namespace rtk)
// =================================================================================================================================
#if defined(ANIMATION_LAUNCHERS) && !defined(RFWHIP_ANIMATION_LAUNCHERS_DONE)
#define RFWHIP_ANIMATION_LAUNCHERS_DONE
#if defined(RT_DEVICE_BUILD)

// (A template with one unused parameter, like the kernels of sky_load.h: it is emitted where its launcher first uses it, behind
// every kernel that existed before, so those keep their places in the code object.)
template <int LAST>
__global__ void __launch_bounds__(RIG_THREADS) k_rig_evaluate(const RigView *table, const RigCall *calls)
{
	__shared__ float s_local[16u * RIG_LDS_NODES], s_world[16u * RIG_LDS_NODES];
	const RigCall call = calls[blockIdx.x];
	const RigView v = table[call.rig];
	const uint32_t t = threadIdx.x;
	const bool lds = v.node_count <= RIG_LDS_NODES; // (uniform: every lane of the workgroup takes the same side)
	float *const local = lds ? s_local : v.local;
	float *const world = lds ? s_world : v.world;
	uint32_t first, n;
	rig_call_channels(v, call, first, n);
	for (uint32_t i = t; i < v.node_count; i += RIG_THREADS)
		rig_reset_node(v, i);
	for (uint32_t w = t; w < v.weight_count; w += RIG_THREADS)
		rig_reset_weight(v, w);
	__syncthreads();
	for (uint32_t c = t; c < n; c += RIG_THREADS)
		v.flags[first + c] = rig_channel_item(v, first + c, call.time, c == 0u);
	__syncthreads();
	for (uint32_t i = t; i < v.node_count; i += RIG_THREADS)
		rig_local_item(v, local, i);
	__syncthreads();
	for (uint32_t l = 0; l < v.levels; l++) // (v.levels is uniform: every lane reaches every barrier)
	{
		const uint32_t end = v.level_first[l + 1u];
		for (uint32_t slot = v.level_first[l] + t; slot < end; slot += RIG_THREADS)
			rig_world_item(v, local, world, slot);
		__syncthreads();
	}
	for (uint32_t s = t; s < v.skin_count; s += RIG_THREADS)
		v.flags[v.channel_count + s] = rig_inverse_item(v, world, s);
	if (lds) // the world matrices leave for rfwhip_read_rig
		for (uint32_t i = t; i < 16u * v.node_count; i += RIG_THREADS)
			v.world[i] = s_world[i];
	__syncthreads();
	for (uint32_t item = t; item < v.item_count; item += RIG_THREADS)
		rig_joint_item(v, world, item);
	if (!t)
		rig_status_item(v, call, first, n);
}

void launch_rig_evaluate(const RigView *table, const RigCall *calls, uint32_t count, stream_t s)
{
	if (count)
		hipLaunchKernelGGL(k_rig_evaluate<0>, dim3(count), dim3(RIG_THREADS), 0, (hipStream_t)s, table, calls);
}

#else // the emulation: the same items in the same order, serially

void launch_rig_evaluate(const RigView *table, const RigCall *calls, uint32_t count, stream_t s)
{
	EMU_DEFER(s, launch_rig_evaluate(table, calls, count, s));
	rig_host_evaluate(table, calls, count);
}
#endif
#endif
