// light_follow.h — the work items of setting "lights_follow_geometry" (include/rfwhip.h): the area lights of
// emissive geometry derived on the device from the current triangles and transforms, and the light tree refitted over its existing
// topology.  Included by kernels.hip inside namespace rtk: the device kernels (k_light_refresh, k_lt_refit_level, k_lt_refit_top)
// and the host emulation (kernels_emu.inc) run the same items.  Every product and sum below has a fixed shape (rt_core.h: fmaf /
// rounded), so the shipped build, the validation build and the emulation leave the same bytes in a light; the tree's cones go
// through acos / atan2 / sin / cos (m_*: the platform's, or rt_strict_math.h's in the validation build).
//
// REFRESH, one area light per lane (system::update_area_lights, system.cpp:1003-1024, on the device).  A light is BOUND when instIdx
// names an instance in use, triIdx is below the triangle count of its mesh and that triangle's lightTriIdx is >= 0; every other
// light keeps its bytes.  For a bound light, v_j the current object-space vertices of the triangle, M / Nm the instance's matrices:
//   vertex_j = M v_j              per coordinate fmaf(m2, z, fmaf(m1, y, rounded(m0 x))) + m3: four roundings
//   position = ((vertex0 + vertex1) + vertex2) * (1/3)f                                       three more
//   normal   = Nm N               N = the face normal of the triangle's shading record (n0.w, n1.w, n2.w), not renormalised
//   area     = 0.5 |(v1 - v0) x (v2 - v0)|   OBJECT space, like the reference's updateArea; also written to the shading record
//              (ex.x): skin_shade_item leaves ex.x alone, so after a pose or morph the record still held the bind pose's area
//   radiance, energy, triIdx, instIdx, dummy0, dummy1: the words that were there.
//
// REFIT.  A leaf of a bound area light: lo / hi = min / max of the light's three vertices, axis = its normalised normal, cos_o = 1
// (a zero or non-finite normal: axis (0, 0, 1), cos_o = -1, as lighttree::build has it).  An inner node with such a leaf below:
// lo / hi = min / max of its two children's (exact in float32), cone = the union of the two children's cones (Conty Estevez and
// Kulla 2018, Alg. 1) — see lf_cone_union for the margin that keeps it conservative in float32.  Nodes are visited level by level
// from the deepest up, one lane per node, a node reads only its own children: no atomics, the same lights give the same bytes.
#pragma once
#include <float.h>

// 16 aligned bytes of a record as they are (the int words of a light travel through float lanes untouched)
RT_FN f4 lf_ld4(const void *p)
{
	f4 r;
	__builtin_memcpy(&r, __builtin_assume_aligned(p, 16), 16);
	return r;
}
RT_FN void lf_st4(void *p, const f4 &v) { __builtin_memcpy(__builtin_assume_aligned(p, 16), &v, 16); }

// light i of the view; returns whether it is bound.  16-byte accesses: the four rows that carry a word to keep are read (64 B),
// the five rows with a geometry field are written (80 B); the radiance row never changes and is not touched
RT_FN bool lf_refresh_item(const LightFollowView &v, uint32_t i)
{
	char *const rec = reinterpret_cast<char *>(v.area + i);
	const f4 q0 = lf_ld4(rec), q3 = lf_ld4(rec + 48), q4 = lf_ld4(rec + 64), q5 = lf_ld4(rec + 80);
	const int tri = (int)fbits(q3.w), ii = (int)fbits(q4.w);
	bool bound = ii >= 0 && (uint32_t)ii < v.n_inst && tri >= 0;
	const LightInst *in = nullptr;
	if (bound)
	{
		in = v.inst + ii;
		bound = (uint32_t)tri < in->tri_count;
	}
	TriShade *sh = nullptr;
	if (bound)
	{
		sh = v.tri_shade + ((size_t)in->shade_base + (uint32_t)tri);
		bound = (int)fbits(sh->ex.z) >= 0; // lightTriIdx: the back-pointer of an emissive triangle (system.cpp:1021)
	}
	v.bound[i] = bound ? 1 : 0;
	if (!bound)
		return false;
	uint32_t a, b, c;
	if (in->indices)
		a = in->indices[3u * (uint32_t)tri], b = in->indices[3u * (uint32_t)tri + 1u], c = in->indices[3u * (uint32_t)tri + 2u];
	else
		a = 3u * (uint32_t)tri, b = a + 1u, c = a + 2u;
	const f3 v0 = xyz(in->verts[a]), v1 = xyz(in->verts[b]), v2 = xyz(in->verts[c]);
	const float *m = in->m, *nm = in->nrm;
	const f3 w0 = mk3(row_point_r(m, v0), row_point_r(m + 4, v0), row_point_r(m + 8, v0));
	const f3 w1 = mk3(row_point_r(m, v1), row_point_r(m + 4, v1), row_point_r(m + 8, v1));
	const f3 w2 = mk3(row_point_r(m, v2), row_point_r(m + 4, v2), row_point_r(m + 8, v2));
	const f3 pos = ((w0 + w1) + w2) * (1.0f / 3.0f);
	const f4 n0 = sh->n0, n1 = sh->n1, n2 = sh->n2, ex = sh->ex;
	const f3 N = mk3(n0.w, n1.w, n2.w);
	const f3 ln = mk3(row_dir_r(nm, N), row_dir_r(nm + 4, N), row_dir_r(nm + 8, N));
	const f3 cr = cross_r(v1 - v0, v2 - v0);
	const float area = 0.5f * sqrtf(dot_r(cr, cr));
	lf_st4(rec, mk4(pos.x, pos.y, pos.z, q0.w));
	lf_st4(rec + 16, mk4(ln.x, ln.y, ln.z, area));
	lf_st4(rec + 48, mk4(w0.x, w0.y, w0.z, q3.w));
	lf_st4(rec + 64, mk4(w1.x, w1.y, w1.z, q4.w));
	lf_st4(rec + 80, mk4(w2.x, w2.y, w2.z, q5.w));
	// Two lights on one triangle (two instances of one emissive mesh) are two lanes that read and write this row with no order
	// between them: formally a data race.  It is benign: both compute the area from the same object-space vertices, carry the same
	// three other words through, and so store identical bytes; whichever read sees whichever store, the row holds those bytes.
	sh->ex = mk4(area, ex.y, ex.z, ex.w);
	return true;
}

// ---- refit ----
constexpr float LF_PI = 3.14159274101257324f; // (float)pi: a hair above pi
// The margin of the cone union, in radians.  The cones united are the children's STORED ones: axis / |axis| exactly, half angle
// acos(cos_o) exactly; by induction each contains its lights' normals, up to the direction error of a leaf's float normalisation
// (<= 3 ulp per component: 2^-22 rad), which the first union above the leaf absorbs.  What float32 adds to Alg. 1:
//   theta_a, theta_b = acos(cos_o), theta_d = atan2(|a x b|, a.b): <= 4 ulp of a value below 4 each (the platform's functions are
//     within 2-3 ulp, rt_strict_math.h's within 2): 3 x 4 x 2^-22.  atan2 of the cross product, not acos of the dot product: the
//     latter turns a 2^-24 error of a dot product near 1 into 2^-12 rad; |a x b| is good to 2^-23 absolutely (cross_r: one rounding
//     per product), theta_d to 2^-22 — and the ratio does not care that a stored axis is a unit vector only to 2^-24;
//   theta = (theta_a + theta_d + theta_b) / 2 and theta_r = theta - theta_a: three roundings of values below 8: 3 x 2^-22;
//   the rotated axis a cos(theta_r) + (k^ x a) sin(theta_r): sin and cos to 4 ulp, six products and sums, the normalisation and
//     the stored float: <= 16 x 2^-24 = 2^-20 in direction;
//   sum < 20 x 2^-22 < 2^-17: LF_EPS, a factor of 1.6 above the count.
// One more term is not a constant: k^ = (a x b) / |a x b| turns by up to 2^-23 / |a x b| when a x b is short (axes nearly parallel
// or nearly opposite), and the rotated axis with it by theta_r times that: LF_KERR / |a x b| * theta_r with LF_KERR = 2^-22 (twice
// the bound).  Nearly parallel axes have theta_r <= theta_d / 2 ~ |a x b| / 2, so the term stays below 2^-22 there; nearly opposite
// ones pay up to pi 2^-23 / |a x b|.  Below |a x b| = 2^-20 = LF_KMIN the direction of a x b is noise: parallel axes (a.b > 0) keep
// a's axis with theta = max(theta_a, theta_d + theta_b), at most theta_d / 2 < 2^-20 wider than Alg. 1; opposite ones give up:
// cos_o = -1, as cone_union of the host build does for them.
// Last, cos_o = cos(theta + margin) - 2^-22: the cosine to 4 ulp of a value below 1 and the rounding of the difference.  Near
// theta = 0 this is what dominates: cos_o = 1 - 2^-22 is a half angle of 6.9e-4 rad, the price of a cosine stored in float32.
constexpr float LF_EPS = 7.62939453125e-6f;	   // 2^-17
constexpr float LF_KERR = 2.384185791015625e-7f; // 2^-22
constexpr float LF_KMIN = 9.5367431640625e-7f;   // 2^-20
constexpr float LF_COS_STEP = 2.384185791015625e-7f; // 2^-22

RT_FN float lf_theta(float cos_o) { return cos_o > -1.0f ? m_acosf(fminf(cos_o, 1.0f)) : LF_PI; } // (NaN: pi)

// the union of the cones (A, cos_a) and (B, cos_b) into (axis, cos_o)
RT_FN void lf_cone_union(f3 A, float cos_a, f3 B, float cos_b, f3 &axis, float &cos_o)
{
	float ta = lf_theta(cos_a), tb = lf_theta(cos_b);
	if (tb > ta)
	{
		const f3 T = A;
		A = B, B = T;
		const float t = ta, c = cos_a;
		ta = tb, tb = t, cos_a = cos_b, cos_b = c;
	}
	axis = A, cos_o = -1.0f;
	if (!(ta < LF_PI))
		return;
	const f3 k = cross_r(A, B);
	const float kl = sqrtf(dot_r(k, k)), d = dot_r(A, B);
	const float td = m_atan2f(kl, d);
	if (td + tb + LF_EPS <= ta) // (b's cone inside a's, with the margin to spare: a's cone as it is)
	{
		cos_o = cos_a;
		return;
	}
	float t = fmaxf(0.5f * ((ta + td) + tb), ta), margin = LF_EPS;
	if (!(kl > LF_KMIN))
	{
		if (!(d > 0.0f))
			return; // (opposite axes, or NaN: every direction)
		t = fmaxf(ta, td + tb);
	}
	else
	{
		const float tr = t - ta, inv = 1.0f / kl;
		const f3 kh = mk3(rounded(k.x * inv), rounded(k.y * inv), rounded(k.z * inv));
		const f3 kxa = cross_r(kh, A);
		const float cs = m_cosf(tr), sn = m_sinf(tr);
		axis = normalize_r(mk3(fmaf(kxa.x, sn, rounded(A.x * cs)), fmaf(kxa.y, sn, rounded(A.y * cs)), fmaf(kxa.z, sn, rounded(A.z * cs))));
		margin = fmaf(tr, LF_KERR * inv, LF_EPS);
	}
	t += margin;
	if (!(t < LF_PI - LF_EPS) || any_nan(axis))
	{
		axis = A;
		return;
	}
	cos_o = fmaxf(m_cosf(t) - LF_COS_STEP, -1.0f);
}

// a leaf of a bound area light, from its light
RT_FN void lf_refit_leaf(LightTreeNode &nd, const AreaLight &l)
{
	for (int a = 0; a < 3; a++)
	{
		nd.lo[a] = fminf(l.vertex0[a], fminf(l.vertex1[a], l.vertex2[a]));
		nd.hi[a] = fmaxf(l.vertex0[a], fmaxf(l.vertex1[a], l.vertex2[a]));
	}
	// (scaled by the largest component first: a normal of length 1e-30 is a direction, as it is to the host build's doubles)
	const float mx = fmaxf(fabsf(l.normal[0]), fmaxf(fabsf(l.normal[1]), fabsf(l.normal[2])));
	const bool ok = mx > 0.0f && mx <= FLT_MAX && l.normal[0] == l.normal[0] && l.normal[1] == l.normal[1] && l.normal[2] == l.normal[2];
	const f3 n = ok ? normalize_r(mk3(l.normal[0] / mx, l.normal[1] / mx, l.normal[2] / mx)) : mk3(0.0f, 0.0f, 1.0f);
	nd.axis[0] = n.x, nd.axis[1] = n.y, nd.axis[2] = n.z;
	nd.cos_o = ok ? 1.0f : -1.0f;
}
// an inner node from its two children
RT_FN void lf_refit_inner(LightTreeNode &nd, const LightTreeNode &L, const LightTreeNode &R)
{
	for (int a = 0; a < 3; a++)
		nd.lo[a] = fminf(L.lo[a], R.lo[a]), nd.hi[a] = fmaxf(L.hi[a], R.hi[a]);
	f3 axis;
	float cos_o;
	lf_cone_union(ld3(L.axis), L.cos_o, ld3(R.axis), R.cos_o, axis, cos_o);
	nd.axis[0] = axis.x, nd.axis[1] = axis.y, nd.axis[2] = axis.z;
	nd.cos_o = cos_o;
}
// node i: touched[i] = a bound area light's leaf, or an inner node with one below; such a node is rewritten
RT_FN void lf_refit_item(LightTreeNode *nodes, const AreaLight *area, uint32_t n_area, const unsigned char *bound, unsigned char *touched,
						 uint32_t i)
{
	LightTreeNode &nd = nodes[i];
	const uint32_t child = nd.child;
	if (!child)
	{
		const bool t = nd.light < n_area && bound[nd.light];
		touched[i] = t ? 1 : 0;
		if (t)
			lf_refit_leaf(nd, area[nd.light]);
		return;
	}
	const bool t = touched[child] | touched[child + 1u];
	touched[i] = t ? 1 : 0;
	if (t)
		lf_refit_inner(nd, nodes[child], nodes[child + 1u]);
}
