// display_grade.h — colour grading and dither for the display stage (settings "display_grade", "display_wb_temperature",
// "display_grade_*", "display_dither", include/rfwhip.h).  Included by kernels.hip inside namespace rtk, after
// display.h, metering.h and bloom.h: the device kernels (k_display_graded, k_kat_grade) and the host emulation (kernels_emu.inc) run
// the same items.
//
// Per texel, E = the exposure the display kernel would apply (the meter record's; absent: no multiplication), x the input colour:
//   x    <- x E                                                                                  (GR_EXPOSED)
//   LINEAR (GR_WB or any GR_CDL_* or GR_SAT; all at the identity: the whole block is skipped, x reaches dp_tone as it is):
//     c  = min(fmaxf(x, 0), 65504) per colour channel: a NaN channel is 0; alpha is untouched throughout
//     WB   c_i <- fmaf(M_i2, c_b, fmaf(M_i1, c_g, M_i0 c_r))                                      (GR_WB; M: 3 x 3, row i)
//     CDL  c_i <- powf(fmaxf(fmaf(c_i, slope_i, offset_i), 0), power_i)                           (GR_CDL_R / _G / _B, per channel;
//          power_i = 1: the clamped value itself, no powf)
//     SAT  Y = fmaf(0.0722, c_b, fmaf(0.7152, c_g, 0.2126 c_r));  c_i <- fmaf(sat, c_i - Y, Y)    (GR_SAT)
//   TONE v = dp_tone on the result (display.h, unchanged): v in [0, 1]
//   LUT  v <- clamp(tetra(L, v), 0, 1)                            (GR_LUT; the entries of L may lie outside [0, 1], v never does)
//          p = v (n - 1) per channel; i = min((int)p, n - 2); f = p - i; the fractions in descending order f_a >= f_b >= f_c, ties
//          in channel order r, g, b; V0 = L[i], V1 = one step along axis a, V2 = one further step along b, V3 = L[i + (1, 1, 1)];
//          w = (1 - f_a, f_a - f_b, f_b - f_c, f_c);  out = fmaf(w3, V3, fmaf(w2, V2, fmaf(w1, V1, w0 V0)))
//          L: n^3 float4 (r, g, b, 0), red fastest — one 16-byte load per vertex, the four fetched before the arithmetic
//   FXAA, ENCODE: display.h's dp_encoded, on the graded values
//   DITHER (RGBA8, GR_DITHER): byte = clamp(rint(255 v + d(x, y) - 0.5), 0, 255) for r, g, b, EVALUATED EXACTLY (dg_byte: the
//          product's rounding error is carried along, so a threshold is never decided by a rounding of 255 v + d); alpha as without.
//          d(x, y) = (B + 0.5) / 256, B = the 16 x 16 Bayer index of (x & 15, y & 15): with q = x ^ y, bit b (0 .. 3) of q is bit
//          2 (3 - b) + 1 of B and bit b of y is bit 2 (3 - b) (2 x 2: [[0, 2], [3, 1]]).  One pattern for the three channels, a pure
//          function of the pixel.
// Tint (white points off the Planckian locus) is out of scope: the white balance has one parameter, the temperature.
// The flags are wave-uniform (an argument of the kernel): a step at the identity costs one scalar branch and is NOT multiplied through,
// so display_grade = 1 with every parameter at its default is bit for bit display_grade = 0, infinities and NaNs included.
// Fixed operation order, explicit fmaf, no atomics.
#pragma once
#include <math.h>

// (GR_* flags, GR_LUT_MIN / _MAX: kernels.h — the host sets the flags and checks a LUT's size by them)
constexpr uint32_t GR_LINEAR = GR_WB | GR_CDL_R | GR_CDL_G | GR_CDL_B | GR_SAT;
static_assert(GR_CDL_G == GR_CDL_R << 1 && GR_CDL_B == GR_CDL_R << 2, "the host sets a channel's flag by a shift");

RT_FN float dg_luma(f3 c) { return fmaf(0.0722f, c.z, fmaf(0.7152f, c.y, 0.2126f * c.x)); }
// (power = 1: the clamped value itself — powf(t, 1) is t, and a library powf is the most expensive thing in this file; `power` is an
// argument of the kernel, so the test is a scalar branch)
RT_FN float dg_cdl(float c, float slope, float offset, float power)
{
	const float t = fmaxf(fmaf(c, slope, offset), 0.0f);
	return power == 1.0f ? t : powf(t, power);
}
// the LINEAR block on a colour that is already exposed
RT_FN f3 dg_linear(const GradeView &g, f3 c)
{
	c = mk3(fminf(fmaxf(c.x, 0.0f), DP_MAX_IN), fminf(fmaxf(c.y, 0.0f), DP_MAX_IN), fminf(fmaxf(c.z, 0.0f), DP_MAX_IN));
	if (g.flags & GR_WB)
		c = mk3(fmaf(g.wb[2], c.z, fmaf(g.wb[1], c.y, g.wb[0] * c.x)), fmaf(g.wb[5], c.z, fmaf(g.wb[4], c.y, g.wb[3] * c.x)),
				fmaf(g.wb[8], c.z, fmaf(g.wb[7], c.y, g.wb[6] * c.x)));
	if (g.flags & GR_CDL_R)
		c.x = dg_cdl(c.x, g.slope[0], g.offset[0], g.power[0]);
	if (g.flags & GR_CDL_G)
		c.y = dg_cdl(c.y, g.slope[1], g.offset[1], g.power[1]);
	if (g.flags & GR_CDL_B)
		c.z = dg_cdl(c.z, g.slope[2], g.offset[2], g.power[2]);
	if (g.flags & GR_SAT)
	{
		const float Y = dg_luma(c);
		c = mk3(fmaf(g.sat, c.x - Y, Y), fmaf(g.sat, c.y - Y, Y), fmaf(g.sat, c.z - Y, Y));
	}
	return c;
}
// tetra(L, v) for v in [0, 1]^3: every index lies in [0, n^3) because 0 <= i <= n - 2 per axis
RT_FN f3 dg_tetra(const GradeView &g, f3 v)
{
	const int n = (int)g.n;
	const float s = (float)(n - 1);
	const float pr = v.x * s, pg = v.y * s, pb = v.z * s;
	const int ir = (int)pr < n - 2 ? (int)pr : n - 2, ig = (int)pg < n - 2 ? (int)pg : n - 2, ib = (int)pb < n - 2 ? (int)pb : n - 2;
	const float fr = pr - (float)ir, fg = pg - (float)ig, fb = pb - (float)ib;
	const int sr = 1, sg = n, sb = n * n;
	int sa, sbb; // the steps along the axes of the largest and the middle fraction
	float fa, fm, fc;
	if (fr >= fg)
	{
		if (fg >= fb)
			sa = sr, sbb = sg, fa = fr, fm = fg, fc = fb;
		else if (fr >= fb)
			sa = sr, sbb = sb, fa = fr, fm = fb, fc = fg;
		else
			sa = sb, sbb = sr, fa = fb, fm = fr, fc = fg;
	}
	else
	{
		if (fr >= fb)
			sa = sg, sbb = sr, fa = fg, fm = fr, fc = fb;
		else if (fg >= fb)
			sa = sg, sbb = sb, fa = fg, fm = fb, fc = fr;
		else
			sa = sb, sbb = sg, fa = fb, fm = fg, fc = fr;
	}
	const int i0 = (ib * n + ig) * n + ir;
	const f4 V0 = g.lut[i0], V1 = g.lut[i0 + sa], V2 = g.lut[i0 + sa + sbb], V3 = g.lut[i0 + sr + sg + sb];
	const float w0 = 1.0f - fa, w1 = fa - fm, w2 = fm - fc, w3 = fc;
	return mk3(fmaf(w3, V3.x, fmaf(w2, V2.x, fmaf(w1, V1.x, w0 * V0.x))), fmaf(w3, V3.y, fmaf(w2, V2.y, fmaf(w1, V1.y, w0 * V0.y))),
			   fmaf(w3, V3.z, fmaf(w2, V2.z, fmaf(w1, V1.z, w0 * V0.z))));
}
// one texel up to the LDS tile: exposure, the LINEAR block, the tone map, the LUT.  With flags = 0 this is dp_tone(v, in)
// (the three routes in front of dp_tone are written out, each the expression of the kernel it stands for — k_display's, k_display_exposed's
// — so that the compiler contracts x E + offset here where it does there)
RT_FN f3 dg_texel(const DisplayView &v, const GradeView &g, const f4 &in, float E)
{
	f3 t;
	if (g.flags & GR_LINEAR)
	{
		const f4 x = (g.flags & GR_EXPOSED) ? dp_exposed(in, E) : in;
		const f3 c = dg_linear(g, mk3(x.x, x.y, x.z));
		t = dp_tone(v, mk4(c.x, c.y, c.z, in.w));
	}
	else if (g.flags & GR_EXPOSED)
		t = dp_tone(v, dp_exposed(in, E));
	else
		t = dp_tone(v, in);
	// (a LUT may hold entries outside [0, 1] — looks with overshoot are ordinary .cube files: what leaves this step keeps dp_tone's
	// contract, v in [0, 1], which FXAA, the encoding and the 8-bit store rely on)
	if (g.flags & GR_LUT)
	{
		t = dg_tetra(g, t);
		t = mk3(dp_clamp01(t.x), dp_clamp01(t.y), dp_clamp01(t.z));
	}
	return t;
}

// the Bayer index B of pixel (x, y), 0 .. 255
RT_FN uint32_t dg_bayer(uint32_t x, uint32_t y)
{
	const uint32_t q = x ^ y;
	uint32_t B = 0u;
	for (uint32_t b = 0u; b < 4u; b++)
		B |= (((q >> b) & 1u) << (2u * (3u - b) + 1u)) | (((y >> b) & 1u) << (2u * (3u - b)));
	return B;
}
// rint(255 v + (B + 0.5) / 256 - 0.5), ties to even, for v in [0, 1], decided exactly: 255 v = hi + lo without error (lo = the product's
// rounding error), hi = m + fr with m whole; the byte is m + 1 when fr + lo + d > 1, d = (B + 0.5) / 256, m when < 1.  fr - (1 - d) is
// exact where the two lie within a factor of two of each other and keeps its sign (and a size far above lo's) elsewhere; adding lo
// rounds, but never across zero.
RT_FN uint32_t dg_byte(float v, uint32_t B)
{
	const float hi = fmaf(v, 255.0f, 0.0f), lo = fmaf(v, 255.0f, -hi); // (hi as an fma: the product rounded once, never fused into hi - m)
	const float m = floorf(hi), fr = hi - m;
	const float rest = (255.5f - (float)B) * (1.0f / 256.0f); // 1 - d: a multiple of 2^-9
	const float z = (fr - rest) + lo;
	int byte = (int)m;
	if (z > 0.0f || (z == 0.0f && (byte & 1)))
		byte++;
	return (uint32_t)(byte < 0 ? 0 : (byte > 255 ? 255 : byte));
}

// display.h's dp_item with the dithered store: dp_encoded on the graded values, and the store in the view's format.
// alpha: the pixel's own in.w, unclamped.
template <bool FXAA, typename Fetch> RT_FN void dg_item(const DisplayView &d, const GradeView &g, const Fetch &fetch, int x, int y, float alpha)
{
	const f3 out = dp_encoded<FXAA>(d, fetch, x, y);
	const float a = dp_clamp01(alpha);
	const size_t i = (size_t)y * d.W + (size_t)x;
	if (d.format == 0u) // RFWHIP_DISPLAY_RGBA8
	{
		uint32_t r, gg, b;
		if (g.flags & GR_DITHER)
		{
			// (FXAA's taps are convex sums of values in [0, 1] and the OETF maps [0, 1] onto itself up to rounding: clamped once more)
			const uint32_t B = dg_bayer((uint32_t)x, (uint32_t)y);
			r = dg_byte(dp_clamp01(out.x), B), gg = dg_byte(dp_clamp01(out.y), B), b = dg_byte(dp_clamp01(out.z), B);
		}
		else
			r = (uint32_t)(int)rintf(out.x * 255.0f), gg = (uint32_t)(int)rintf(out.y * 255.0f), b = (uint32_t)(int)rintf(out.z * 255.0f);
		((uint32_t *)d.out)[i] = r | (gg << 8) | (b << 16) | ((uint32_t)(int)rintf(a * 255.0f) << 24);
	}
	else
		((f4 *)d.out)[i] = mk4(out.x, out.y, out.z, a);
}

// rfwhip_grade_colors: record i = three floats in, three out.  which 0: the LINEAR block (under the flags; all at the identity: the
// colour itself) on a linear colour; 1: tetra on a display colour, clamped to [0, 1] first (a NaN channel is 0) — tetra's own
// result, without the stage's clamp behind it
RT_FN void dg_kat_item(const GradeView &g, int which, const float *in, float *out, uint32_t i)
{
	f3 c = mk3(in[(size_t)i * 3u], in[(size_t)i * 3u + 1u], in[(size_t)i * 3u + 2u]);
	if (which == 0)
	{
		if (g.flags & GR_LINEAR)
			c = dg_linear(g, c);
	}
	else if (g.flags & GR_LUT)
		c = dg_tetra(g, mk3(dp_clamp01(c.x), dp_clamp01(c.y), dp_clamp01(c.z)));
	out[(size_t)i * 3u] = c.x, out[(size_t)i * 3u + 1u] = c.y, out[(size_t)i * 3u + 2u] = c.z;
}
