// denoise.h — the work items of the denoiser of the presented image (setting "denoise", include/rfwhip.h): a guide pass and
// SVGF's filter (Schied et al., HPG 2017): the spatial a-trous passes and its temporal stage.  Included by kernels.hip inside namespace rtk,
// after the other work items: the device kernels (kernels.hip) and the host emulation (kernels_emu.inc) run the same items.
//
// Guides, per pixel of the full W x H image (one centre ray from the lens centre, the closest-hit traversal of the path tracer):
//   ga = albedo (material colour after the texture layers, pt_textures), w = 1 valid / 0 invalid
//   gb = octahedral normal (two snorm16 in the bits of x: the shading normal after normal maps, facing the camera), z = distance
//        along the ray to the surface (-1 = invalid), dz/dx, dz/dy (central differences; one-sided at borders / invalid neighbours)
// A pixel is invalid when its ray misses, hits an emitter (a colour component > 1, pt_shade), or passes more than DN_MAX_ALPHA
// alpha-tested layers (the path tracer's pass-through: the ray goes on from I + 1e-5 D).
// Filter (valid pixels; invalid ones are copied bit for bit and never used as neighbours):
//   demodulate  I = c / max(albedo, 1e-3), l = lum(I); var = weighted variance of l over the valid 3x3 neighbours (weights w_z w_n)
//   pass i      step s = 2^i, 5x5 taps q = p + s (dx, dy), w = h(dx) h(dy) w_z w_n w_l, h = (1, 4, 6, 4, 1) / 16
//               w_z = exp(-|z_p - z_q| / (sigma_z |s (dx, dy) . grad z_p| + 1e-4)), w_n = max(0, n_p . n_q)^sigma_n,
//               w_l = exp(-|l_p - l_q| / (sigma_l sqrt(g3x3(var)_p) + 1e-10)), g3x3 = (1, 2, 1) / 4 x (1, 2, 1) / 4 over valid taps
//               I' = sum w I_q / sum w, var' = sum w^2 var_q / (sum w)^2, l' = lum(I')
//   remodulate  (last pass) out = I' max(albedo, 1e-3), out.w = c.w
// Fixed tap order, no atomics: the output depends on the input image and the guides only.
// Temporal stage (setting "denoise_temporal"; SVGF's reprojected history): dn_temporal_item follows the demodulation once per
// presented frame F.  It reprojects p's guide point X = pos_F + z_p D_p into the previous presented frame P (bilinear taps, each
// kept when it is consistent: inside, valid, the same unchanged instance, depth and normal within DN_T_*), blends I and the
// luminance moments with the history (n = min(n_P + 1, 64), a = max(alpha, 1 / n)) and takes var = max(0, mu2 - mu1^2) once
// n >= 4 (the 3x3 estimate before).  Pass 0 writes the colour history (its demodulated output).  A fresh pixel (no consistent
// tap, or no usable history) reads no history and gives the spatial filter's values bit for bit.
// Motion (setting "denoise_motion"; dn_temporal_motion_item, the same body): a pixel of an instance that moved or deformed since P
// and whose previous vertices are known (DnMotionInst::state == DN_M_MOVED) is reprojected through the previous position of its own
// surface point, X_P = M_P (w b_0 + u b_1 + v b_2), and its normal is carried back by the triangle's own deformation before the
// normal test.  The guide pass's variant dn_guide_surf_item keeps the hit's primitive and barycentrics for it (DnMotion::surf).
#pragma once

constexpr int DN_MAX_ALPHA = 8;			// alpha-tested layers a guide ray passes before the pixel is called invalid
constexpr float DN_ALBEDO_MIN = 1e-3f;	// demodulation floor per channel
constexpr int DN_TILE_X = 16, DN_TILE_Y = 16; // pixels of a 256-thread workgroup: 2 x 2 tiles of 8 x 8, one per wave64
// temporal stage (include/rfwhip.h "denoise_temporal" names the same constants)
constexpr float DN_T_DEPTH_GRAD = 2.0f;	 // depth test: |z_P(q) - |X - pos_P|| <= 2 (|dz/dx| + |dz/dy|) + 0.01 |X - pos_P|
constexpr float DN_T_DEPTH_REL = 0.01f;
constexpr float DN_T_NORMAL = 0.9f;		 // normal test: n_p . n_P(q) >= 0.9
constexpr float DN_T_MIN_WEIGHT = 0.01f; // a pixel whose consistent bilinear weights sum below this starts fresh
constexpr float DN_T_MAX_N = 64.0f;		 // history length cap
constexpr float DN_T_VAR_N = 3.99f;		 // from this history length on (4, less a margin for the rounding of the interpolated length:
										 // n_P is a weighted sum), the variance comes from the moments
constexpr uint32_t DN_NO_INST = 0xFFFFFFFFu; // instance id of an invalid guide pixel

RT_FN float dn_lum(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }

RT_FN float dn_sign(float v) { return v < 0.0f ? -1.0f : 1.0f; }
RT_FN uint32_t dn_oct_encode(f3 n)
{
	const float s = fabsf(n.x) + fabsf(n.y) + fabsf(n.z);
	float px = n.x / s, py = n.y / s;
	if (n.z < 0.0f)
	{
		const float ox = (1.0f - fabsf(py)) * dn_sign(px), oy = (1.0f - fabsf(px)) * dn_sign(py);
		px = ox, py = oy;
	}
	const int qx = (int)rintf(fminf(fmaxf(px, -1.0f), 1.0f) * 32767.0f), qy = (int)rintf(fminf(fmaxf(py, -1.0f), 1.0f) * 32767.0f);
	return ((uint32_t)qx & 0xFFFFu) | ((uint32_t)qy << 16);
}
RT_FN f3 dn_oct_decode(uint32_t e)
{
	float x = (float)(int16_t)(e & 0xFFFFu) * (1.0f / 32767.0f), y = (float)(int16_t)(e >> 16) * (1.0f / 32767.0f);
	const float z = 1.0f - fabsf(x) - fabsf(y);
	if (z < 0.0f)
	{
		const float ox = (1.0f - fabsf(y)) * dn_sign(x), oy = (1.0f - fabsf(x)) * dn_sign(y);
		x = ox, y = oy;
	}
	const float inv = 1.0f / sqrtf(x * x + y * y + z * z);
	return mk3(x * inv, y * inv, z * inv);
}

// pixel of thread t of workgroup (bx, by): the 8 x 8 tile of wave t / 64, row-major inside it
RT_FN bool dn_pixel(uint32_t bx, uint32_t by, uint32_t t, uint32_t W, uint32_t H, uint32_t &i)
{
	const uint32_t wave = t >> 6, lane = t & 63u;
	const uint32_t x = bx * DN_TILE_X + (wave & 1u) * TILE + (lane & 7u), y = by * DN_TILE_Y + (wave >> 1) * TILE + (lane >> 3);
	i = y * W + x;
	return x < W && y < H;
}

// ---- guide pass ---------------------------------------------------------------------------------------------------------
RT_FN void dn_guide_item(const Params &p, const DnView &d, uint32_t i, const TravStack &stk)
{
#define DN_BODY_SURF 0
#define DN_BODY_MAPS 0
#include "denoise_guide_body.h"
#undef DN_BODY_MAPS
#undef DN_BODY_SURF
}
// "denoise_motion": the same item, which also keeps the hit's primitive and barycentrics (surf[i] = (prim, u, v, 0))
RT_FN void dn_guide_surf_item(const Params &p, const DnView &d, f4 *surf, uint32_t i, const TravStack &stk)
{
#define DN_BODY_SURF 1
#define DN_BODY_MAPS 0
#include "denoise_guide_body.h"
#undef DN_BODY_MAPS
#undef DN_BODY_SURF
}
// material_maps: the same item, which also lets the alpha mask pass the ray through (pt_maps_alpha); surf may be null
RT_FN void dn_guide_maps_item(const Params &p, const DnView &d, f4 *surf, uint32_t i, const TravStack &stk)
{
#define DN_BODY_SURF 1
#define DN_BODY_MAPS 1
#include "denoise_guide_body.h"
#undef DN_BODY_MAPS
#undef DN_BODY_SURF
}

// screen-space depth gradient (a second kernel: it reads the neighbours' z); writes gb[i].z / .w only
RT_FN void dn_gradient_item(const DnView &d, uint32_t i)
{
	const uint32_t x = i % d.W, y = i / d.W;
	const float z = d.gb[i].y;
	if (z < 0.0f)
		return;
	auto zq = [&](int qx, int qy) -> float {
		if (qx < 0 || qy < 0 || qx >= (int)d.W || qy >= (int)d.H)
			return -1.0f;
		return d.gb[(uint32_t)qy * d.W + (uint32_t)qx].y;
	};
	auto diff = [&](float zm, float zp) -> float {
		if (zm >= 0.0f && zp >= 0.0f)
			return (zp - zm) * 0.5f;
		if (zp >= 0.0f)
			return zp - z;
		if (zm >= 0.0f)
			return z - zm;
		return 0.0f;
	};
	float *const g = (float *)&d.gb[i];
	g[2] = diff(zq((int)x - 1, (int)y), zq((int)x + 1, (int)y));
	g[3] = diff(zq((int)x, (int)y - 1), zq((int)x, (int)y + 1));
}

// ---- filter -------------------------------------------------------------------------------------------------------------
RT_FN float dn_w_z(const f4 &gp, const f4 &gq, float sigma_z, int sdx, int sdy)
{
	return expf(-fabsf(gp.y - gq.y) / (sigma_z * fabsf((float)sdx * gp.z + (float)sdy * gp.w) + 1e-4f));
}
RT_FN float dn_w_n(f3 np, f3 nq, float sigma_n) { return powf(fmaxf(0.0f, dot(np, nq)), sigma_n); }

// demodulation + the initial variance, into img (I, l) / var
RT_FN void dn_demod_item(const DnView &d, f4 *img, float *var, uint32_t i)
{
	const f4 gp = d.gb[i];
	if (gp.y < 0.0f)
		return;
	const int x = (int)(i % d.W), y = (int)(i / d.W);
	const f3 np = dn_oct_decode(fbits(gp.x));
	float w[9], l[9], sw = 0.0f, sl = 0.0f;
	for (int dy = -1; dy <= 1; dy++)
		for (int dx = -1; dx <= 1; dx++)
		{
			const int k = (dy + 1) * 3 + dx + 1, qx = x + dx, qy = y + dy;
			w[k] = 0.0f, l[k] = 0.0f;
			if (qx < 0 || qy < 0 || qx >= (int)d.W || qy >= (int)d.H)
				continue;
			const uint32_t q = (uint32_t)qy * d.W + (uint32_t)qx;
			const f4 gq = d.gb[q];
			if (gq.y < 0.0f)
				continue;
			const f4 a = d.ga[q], c = d.in[q];
			const float ir = c.x / fmaxf(a.x, DN_ALBEDO_MIN), ig = c.y / fmaxf(a.y, DN_ALBEDO_MIN), ib = c.z / fmaxf(a.z, DN_ALBEDO_MIN);
			l[k] = dn_lum(ir, ig, ib);
			w[k] = dn_w_z(gp, gq, d.sigma_z, dx, dy) * dn_w_n(np, dn_oct_decode(fbits(gq.x)), d.sigma_n);
			sw += w[k], sl += w[k] * l[k];
			if (k == 4)
				img[i] = mk4(ir, ig, ib, l[k]);
		}
	const float mean = sl / sw;
	float v = 0.0f;
	for (int k = 0; k < 9; k++)
		v += w[k] * (l[k] - mean) * (l[k] - mean);
	var[i] = v / sw;
}

// ---- temporal stage (after dn_demod_item when "denoise_temporal" is on) -----------------------------------------------------------
// The demodulation has written I, l and the 3x3 variance into img / var; this reprojects pixel i into the previous presented frame,
// blends with its history and chooses the variance, in place: img (I~, lum(I~)) / var; the moments and the history length into
// t.mom_out / t.n_out.  A fresh pixel leaves img / var as the demodulation wrote them: the spatial filter's values, bit for bit.
// Invalid pixels store n = 0.  (Reads and writes pixel i of img / var only.)
// Motion ("denoise_motion", dn_temporal_motion_item): a pixel whose instance changed since P and is DN_M_MOVED in m.inst takes X_P
// and n'_p below in place of X and n_p; every other pixel runs the code of the stage unchanged.
// m.dump (rfwhip_read_denoise_motion; null in a presented frame's stage): 8 floats per pixel, state | X_P | n'_p | 0.
RT_FN void dn_motion_dump(const DnMotion &m, uint32_t i, uint32_t state, f3 X, f3 n)
{
	float *const o = m.dump + 8u * (size_t)i;
	o[0] = (float)state, o[1] = X.x, o[2] = X.y, o[3] = X.z, o[4] = n.x, o[5] = n.y, o[6] = n.z, o[7] = 0.0f;
}
RT_FN f3 dn_xform(const float *M, f3 v) // rows 0..2 of a 4 x 4 matrix, 3 x 4 row-major
{
	return mk3(M[0] * v.x + M[1] * v.y + M[2] * v.z + M[3], M[4] * v.x + M[5] * v.y + M[6] * v.z + M[7],
			   M[8] * v.x + M[9] * v.y + M[10] * v.z + M[11]);
}
// the previous position of the surface point (prim, u, v) of a MOVED instance and p's normal carried back to P; false: degenerate
RT_FN bool dn_motion_point(const DnMotionInst &mi, const f4 sf, f3 &X, f3 &n)
{
	const uint32_t k = fbits(sf.x);
	if (k >= mi.tri_count)
		return false;
	uint32_t i0 = 3u * k, i1 = 3u * k + 1u, i2 = 3u * k + 2u;
	if (mi.indices)
		i0 = mi.indices[3u * k], i1 = mi.indices[3u * k + 1u], i2 = mi.indices[3u * k + 2u];
	if (i0 >= mi.vert_count || i1 >= mi.vert_count || i2 >= mi.vert_count)
		return false;
	const f4 a0 = mi.cur[i0], a1 = mi.cur[i1], a2 = mi.cur[i2], b0 = mi.prev[i0], b1 = mi.prev[i1], b2 = mi.prev[i2];
	const float u = sf.y, v = sf.z, w = 1.0f - u - v;
	const f3 A0 = dn_xform(mi.mf, xyz(a0)), B0 = dn_xform(mi.mp, xyz(b0));
	const f3 e1 = dn_xform(mi.mf, xyz(a1)) - A0, e2 = dn_xform(mi.mf, xyz(a2)) - A0;
	const f3 f1 = dn_xform(mi.mp, xyz(b1)) - B0, f2 = dn_xform(mi.mp, xyz(b2)) - B0;
	const f3 ca = cross(e1, e2), cb = cross(f1, f2);
	const float la = length(ca), dd = length(cb);
	if (!(la > 0.0f && la < 1e30f && dd > 0.0f && dd < 1e30f))
		return false;
	const f3 Na = ca * (1.0f / la), Nb = cb * (1.0f / dd);
	const float c1 = dot(e1, n), c2 = dot(e2, n), c3 = dot(Na, n);
	const f3 r = (cross(f2, Nb) * c1 + cross(Nb, f1) * c2) * (1.0f / dd) + Nb * c3;
	const float lr = length(r);
	if (!(lr > 0.0f && lr < 1e30f))
		return false;
	n = r * (1.0f / lr);
	X = dn_xform(mi.mp, xyz(b0) * w + xyz(b1) * u + xyz(b2) * v);
	return true;
}

RT_FN void dn_temporal_item(const DnView &d, const DnTemporal &t, f4 *img, float *var, uint32_t i)
{
#define DN_BODY_MOTION 0
#include "denoise_temporal_body.h"
#undef DN_BODY_MOTION
}
RT_FN void dn_temporal_motion_item(const DnView &d, const DnTemporal &t, const DnMotion &m, f4 *img, float *var, uint32_t i)
{
#define DN_BODY_MOTION 1
#include "denoise_temporal_body.h"
#undef DN_BODY_MOTION
}

// one a-trous pass of step `step`: src / vsrc -> dst / vdst, or (last) the remodulated image into d.out (may be d.in)
RT_FN void dn_pass_item(const DnView &d, uint32_t step, bool last, const f4 *src, const float *vsrc, f4 *dst, float *vdst, uint32_t i)
{
	const f4 gp = d.gb[i];
	if (gp.y < 0.0f)
	{
		if (last)
			d.out[i] = d.in[i];
		return;
	}
	const int x = (int)(i % d.W), y = (int)(i / d.W);
	// the luminance edge's scale: the variance blurred over the valid 3 x 3 neighbours
	float gv = 0.0f, gw = 0.0f;
	for (int dy = -1; dy <= 1; dy++)
		for (int dx = -1; dx <= 1; dx++)
		{
			const int qx = x + dx, qy = y + dy;
			if (qx < 0 || qy < 0 || qx >= (int)d.W || qy >= (int)d.H)
				continue;
			const uint32_t q = (uint32_t)qy * d.W + (uint32_t)qx;
			if (d.gb[q].y < 0.0f)
				continue;
			const float k = (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f);
			gv += k * vsrc[q], gw += k;
		}
	const float inv_l = 1.0f / (d.sigma_l * sqrtf(gv / gw) + 1e-10f);
	const f3 np = dn_oct_decode(fbits(gp.x));
	const float lp = src[i].w;
	const float h[5] = {1.0f / 16.0f, 4.0f / 16.0f, 6.0f / 16.0f, 4.0f / 16.0f, 1.0f / 16.0f};
	float sw = 0.0f, sv = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f;
	for (int dy = -2; dy <= 2; dy++)
		for (int dx = -2; dx <= 2; dx++)
		{
			const int sdx = (int)step * dx, sdy = (int)step * dy, qx = x + sdx, qy = y + sdy;
			if (qx < 0 || qy < 0 || qx >= (int)d.W || qy >= (int)d.H)
				continue;
			const uint32_t q = (uint32_t)qy * d.W + (uint32_t)qx;
			const f4 gq = d.gb[q];
			if (gq.y < 0.0f)
				continue;
			const f4 iq = src[q];
			const float w = h[dx + 2] * h[dy + 2] * dn_w_z(gp, gq, d.sigma_z, sdx, sdy) * dn_w_n(np, dn_oct_decode(fbits(gq.x)), d.sigma_n) *
							expf(-fabsf(lp - iq.w) * inv_l);
			sw += w, sr += w * iq.x, sg += w * iq.y, sb += w * iq.z;
			sv += w * w * vsrc[q];
		}
	const float inv = 1.0f / sw;
	const float r = sr * inv, g = sg * inv, b = sb * inv;
	if (last)
	{
		const f4 a = d.ga[i], c = d.in[i];
		d.out[i] = mk4(r * fmaxf(a.x, DN_ALBEDO_MIN), g * fmaxf(a.y, DN_ALBEDO_MIN), b * fmaxf(a.z, DN_ALBEDO_MIN), c.w);
	}
	else
	{
		dst[i] = mk4(r, g, b, dn_lum(r, g, b));
		vdst[i] = sv * inv * inv;
	}
	if (step == 1u && d.hist) // (the temporal stage: pass 0's demodulated output is the colour history)
		d.hist[i] = mk4(r, g, b, dn_lum(r, g, b));
}
