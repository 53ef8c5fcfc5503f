// primary_entry.h — the work item of the primary wave's ENTRY SNAPSHOT pass.  Included by kernels.hip inside
// namespace rtk, behind primary_order.h: the device kernel (k_primary_entry) and the host emulation (kernels_emu.inc) run the same item.
//
// With sample groups of 64 a wave of the packet form of the primary wave (trace_packet, ORDERED) holds the 64 samples of ONE pixel:
// 64 rays from the camera position through one pixel.  Whatever the samples, such a wave starts at the root and walks the same chain
// of nodes down to the first leaf — a chain that depends on camera, pixel and tree only, and that every sample group and every
// sub-batch of a call, and every call with the same view, walks again.  The pass walks it ONCE per 64-slot group of one sample group
// of the slot layout (rt_core.h: group = (slot mod (g * slots)) / 64; g = 64: a pixel, smaller g: 64 / g neighbouring pixels) and
// leaves what the wave's stack would hold at the end of it: PRIMARY_ENTRY_K entry words in stack order, word 0 the bottom, the
// nearest on top, unused words ENTRY_DONE.  The wave loads the record into its stack and pops (trace_packet).
//   The candidate list starts as {root}.  While the top candidate is an inner node of the world-space tree (no leaf, no instance
//   leaf: below one lies another space), it is replaced by those of its children that the group's PYRAMID may touch, in table order
//   — the camera-ordered table's: near to far — the first on top.  A top candidate with no touched child is dropped.  The walk stops
//   when the list would outgrow K, or at the first leaf on top.  An empty list is legal: every ray of the group misses.
// Start point and child order never decide a closest hit (primary_order.h), and a candidate that no ray enters only costs its node
// step, so the test may err towards "touched" and never the other way.
//
// The pyramid test, in double precision (exactly rounded +, *, /, sqrt only, every product rounded on its own, pe_m: the emulation, the device and the float64
// model of tests/primary_entry_model.py then agree wherever it matters, and where they do not, both answers are right).
//   A ray of the group is O = cam.pos, D ~ q + right u + up v with q = p1 - pos, u in [x0, x1 + 1] / W, v in [y0, y1 + 1] / H: the
//   pixel rectangle of the group with jitter in [0, 1)^2 (pt_primary_ray).  The side plane at u = u0 holds the apex, the direction
//   `up` and a = q + right u0, so its normal is up x a — no difference of nearly equal corners — and
//       (up x a) . (q + right u + up v) = (u - u0) [up, q, right]:
//   signed by the triple product, the normal points inwards.  Likewise the other three.
//   A child is NOT touched when, for one unit normal n, every corner X of its box has  n . (X - pos) < -margin, which is tested on the
//   corner furthest along n with the largest margin of the eight:
//       margin = theta r + beta (|X|_1 + |pos|_1),    r = the distance of the furthest corner from pos.
//   theta bounds the angle between a real ray and the pyramid.  Per component k, pt_primary_ray rounds u and v (2^-24 relative: at
//   most 2^-24 |right_k| and 2^-24 |up_k| of the point), two fused multiply-adds (2^-24 of at most |p1_k| + |right_k| and |p1_k| +
//   |right_k| + |up_k|), the subtraction of the origin and normalize_r's rounded product (each 2^-24 of at most s_k = |p1_k| +
//   |right_k| + |up_k| + |pos_k|): less than 4 x 2^-24 s_k in all, a vector shorter than 2^-22 S with S = |s|_2, seen from the apex
//   at a distance of at least d (the apex's distance from the image plane) — an angle below 2^-22 S / d.  The pass takes
//   theta = 2^-18 + 2^-21 S / d: twice that, and 2^-18 for the triangle test's own tolerance, which reports hits on rays that pass a
//   triangle's edge by a few units of the last place (2^-22 or so of the distance).  At 1080p with the camera 60 units from the
//   origin theta is 3 % of a pixel's angle.  The cone {X: n . (X - pos) < -theta |X - pos|} is convex, so a box with its eight
//   corners inside holds no point of any real ray.  beta = 2^-19 covers what of that tolerance scales with the coordinates and not
//   with the distance, and the few double roundings of this test (the conversion of planes and origin is exact).
//   A view without an image plane (d = 0, not finite) gives the record {root}: today's start.
#pragma once

static_assert(PRIMARY_ENTRY_NO_ROOT == ENTRY_DONE, "kernels.h restates it for the host");
#ifndef RT_PRIMARY_ENTRY_K
#define RT_PRIMARY_ENTRY_K 8 // words per record (8 against 16: DESIGN_LOG.md round 9, step 0); at most 63, the wave's stack
#endif
constexpr uint32_t PRIMARY_ENTRY_K = RT_PRIMARY_ENTRY_K;
static_assert(PRIMARY_ENTRY_K >= 1u && PRIMARY_ENTRY_K <= 63u, "a record is loaded by lanes 1 .. K of a wave");

struct PePyramid
{
	double c[3], n[4][3]; // apex, inward unit normals
	double theta, c1;	  // c1 = |pos|_1
	bool ok, any;		  // ok: the planes exist; any: the group holds a pixel of the image
};

// the pixel rectangle of a group: the bounding rectangle of its 64 / g pixels that lie in the image
RT_FN bool pe_rect(const FrameView &fr, uint32_t group, uint32_t &x0, uint32_t &x1, uint32_t &y0, uint32_t &y1)
{
	const uint32_t gl = fr.sgroup_log2, pixels = 64u >> gl;
	bool any = false;
	x0 = y0 = 0xFFFFFFFFu, x1 = y1 = 0u;
	for (uint32_t j = 0; j < pixels; j++)
	{
		const PixelRef pr = slot_to_pixel(fr, group * 64u + (j << gl)); // (first sample group: sgroup 0)
		if (!pr.valid)
			continue;
		any = true;
		x0 = pr.x < x0 ? pr.x : x0, x1 = pr.x > x1 ? pr.x : x1;
		y0 = pr.y < y0 ? pr.y : y0, y1 = pr.y > y1 ? pr.y : y1;
	}
	return any;
}

// a product rounded on its own (rounded() of rt_core.h, for doubles: an empty asm hides it from the contraction pass; it emits nothing)
RT_FN double pe_m(double a, double b)
{
	double x = a * b;
#if defined(__HIP_DEVICE_COMPILE__)
	asm("" : "+v"(x));
#elif defined(__x86_64__)
	asm("" : "+x"(x));
#else
	volatile double y = x;
	x = y;
#endif
	return x;
}
RT_FN void pe_cross(const double a[3], const double b[3], double r[3])
{
	r[0] = pe_m(a[1], b[2]) - pe_m(a[2], b[1]), r[1] = pe_m(a[2], b[0]) - pe_m(a[0], b[2]), r[2] = pe_m(a[0], b[1]) - pe_m(a[1], b[0]);
}
RT_FN double pe_dot(const double a[3], const double b[3]) { return (pe_m(a[0], b[0]) + pe_m(a[1], b[1])) + pe_m(a[2], b[2]); }

RT_FN void pe_pyramid(const CamView &cam, const FrameView &fr, uint32_t group, PePyramid &py)
{
	uint32_t x0, x1, y0, y1;
	py.any = pe_rect(fr, group, x0, x1, y0, y1);
	py.ok = false;
	if (!py.any)
		return;
	const double c[3] = {cam.pos.x, cam.pos.y, cam.pos.z}, p1[3] = {cam.p1.x, cam.p1.y, cam.p1.z};
	const double rt[3] = {cam.right.x, cam.right.y, cam.right.z}, up[3] = {cam.up.x, cam.up.y, cam.up.z};
	const double u0 = pe_m((double)x0, (double)fr.inv_w), u1 = pe_m((double)x1 + 1.0, (double)fr.inv_w);
	const double v0 = pe_m((double)y0, (double)fr.inv_h), v1 = pe_m((double)y1 + 1.0, (double)fr.inv_h);
	double q[3], a[4][3], ru[3];
	for (int k = 0; k < 3; k++)
	{
		py.c[k] = c[k];
		q[k] = p1[k] - c[k];
		a[0][k] = q[k] + pe_m(rt[k], u0), a[1][k] = q[k] + pe_m(rt[k], u1); // the planes u = u0, u = u1 hold `up`
		a[2][k] = q[k] + pe_m(up[k], v0), a[3][k] = q[k] + pe_m(up[k], v1); // the planes v = v0, v = v1 hold `right`
	}
	pe_cross(rt, up, ru);
	const double area = sqrt(pe_dot(ru, ru)), triple = pe_dot(ru, q); // [right, up, q]
	const double d = fabs(triple) / area;
	double sk[3];
	for (int k = 0; k < 3; k++)
		sk[k] = ((fabs(p1[k]) + fabs(rt[k])) + fabs(up[k])) + fabs(c[k]);
	const double S = sqrt(pe_dot(sk, sk));
	py.c1 = fabs(c[0]) + fabs(c[1]) + fabs(c[2]);
	py.theta = 3.814697265625e-06 + pe_m(4.76837158203125e-07, S) / d;
	if (!(d > 0.0) || !(py.theta < 0.125)) // (also NaN)
		return;
	// (up x a) . right = [up, a, right] = [right, up, q] for u0 and u1 alike; (right x a) . up = -[right, up, q]
	const double s = triple > 0.0 ? 1.0 : -1.0;
	const double sign[4] = {s, -s, -s, s};
	for (int j = 0; j < 4; j++)
	{
		double n[3];
		pe_cross(j < 2 ? up : rt, a[j], n);
		const double len = sqrt(pe_dot(n, n));
		if (!(len > 0.0))
			return;
		for (int k = 0; k < 3; k++)
			py.n[j][k] = pe_m(n[k], sign[j]) / len;
	}
	py.ok = true;
}

// may a ray of the pyramid touch the box [lo, hi]?  (an inverted box: never)
RT_FN bool pe_touched(const PePyramid &py, const float lo[3], const float hi[3])
{
	if (lo[0] > hi[0] || lo[1] > hi[1] || lo[2] > hi[2])
		return false;
	double d0[3], d1[3], r2 = 0.0, x1 = 0.0;
	for (int k = 0; k < 3; k++)
	{
		d0[k] = (double)lo[k] - py.c[k], d1[k] = (double)hi[k] - py.c[k];
		r2 += fmax(pe_m(d0[k], d0[k]), pe_m(d1[k], d1[k]));
		x1 += fmax(fabs((double)lo[k]), fabs((double)hi[k]));
	}
	const double margin = pe_m(py.theta, sqrt(r2)) + pe_m(1.9073486328125e-06, x1 + py.c1);
	for (int j = 0; j < 4; j++)
	{
		const double *n = py.n[j];
		const double reach = (fmax(pe_m(n[0], d0[0]), pe_m(n[0], d1[0])) + fmax(pe_m(n[1], d0[1]), pe_m(n[1], d1[1]))) + fmax(pe_m(n[2], d0[2]), pe_m(n[2], d1[2]));
		if (reach < -margin)
			return false;
	}
	return true;
}

// the record of `group` into out[0 .. K - 1].  nodes: the table the primary wave will walk (the camera-ordered one), root: its
// start (SceneView::tlas_root_entry, ENTRY_DONE without instances); list: K words of working storage, `stride` words apart
RT_FN void primary_entry_item(const Node4f *nodes, uint32_t root, const CamView &cam, const FrameView &fr, uint32_t group, uint32_t *out,
							  uint32_t *list, uint32_t stride)
{
	PePyramid py;
	pe_pyramid(cam, fr, group, py);
	uint32_t n = 0;
	if (root != ENTRY_DONE && py.any)
		list[0] = root, n = 1u;
	// (every step drops a candidate or goes one level down: the bound only guards against a table that is no tree)
	for (uint32_t step = 0; py.ok && n && step < 4096u; step++)
	{
		const uint32_t top = list[(n - 1u) * stride];
		if (top & ENTRY_LEAF)
			break;
		const Node4f &nd = nodes[top & ENTRY_INDEX_MASK];
		uint32_t t[4], m = 0;
		for (int k = 0; k < 4; k++)
		{
			const float lo[3] = {nd.lo[0][k], nd.lo[1][k], nd.lo[2][k]}, hi[3] = {nd.hi[0][k], nd.hi[1][k], nd.hi[2][k]};
			const uint32_t e = nd.entry[k];
			if (e != ENTRY_EMPTY && pe_touched(py, lo, hi))
				t[m++] = e;
		}
		if (m && n - 1u + m > PRIMARY_ENTRY_K)
			break;
		n--;
		for (uint32_t k = m; k > 0u; k--)
			list[n++ * stride] = t[k - 1u];
	}
	for (uint32_t j = 0; j < PRIMARY_ENTRY_K; j++)
		out[j] = j < n ? list[j * stride] : ENTRY_DONE;
}
