// display.h — the work item of the display stage (settings "display_*", include/rfwhip.h): what the
// reference does to the linear HDR image on its way to the screen — the ACES tone map of rfw::system::render_frame(.., toneMap)
// (assets/shaders/tone-map.frag, system.cpp:682-711) and the FXAA of the window blit (assets/shaders/draw-tex-fxaa.vert:15-22,
// .frag:17-57) — then an optional sRGB encoding and 8-bit quantisation.  Included by kernels.hip inside namespace rtk, after the
// other work items: the device kernel (k_display) and the host emulation (kernels_emu.inc) run the same item.
//
// Input: the full W x H float4 image, row 0 first.  Output: one pixel per input pixel.
//   TONE (per colour channel)  v = min(max(x - 0.5 contrast + 0.5 + brightness, 0), 65504)          (tone-map.frag:43, system.cpp:702)
//        aces:  v <- M_in v;  v <- (v (v + 0.0245786) - 0.000090537) / (v (0.983729 v + 0.432951) + 0.238081);  v <- M_out v;
//               clamp to [0, 1]                                                                    (tone-map.frag:9-33)
//        none:  clamp v to [0, 1]
//        max is fmaxf: a NaN channel becomes 0.  The UPPER clamp (65504, the largest half float) is this stage's one deviation from
//        the reference: it keeps the rational finite for +inf, and changes nothing for a finite image below it.
//        alpha = clamp(in.w, 0, 1) of the pixel itself; neither FXAA nor the encoding touches it.
//   FXAA (display_fxaa = 1), on the tone-mapped values, in pixel units, c = (x + 0.5, y + 0.5):
//        a tap at q is bilinear over texel centres: u = q - 0.5, i = floor(u), f = u - i, texel indices clamped to the edge;
//        NW = tap(c - 0.75), NE / SW / SE = that position moved by (1, 0) / (0, 1) / (1, 1), M = texel (x, y);
//        luma = (0.299, 0.587, 0.114) . rgb; lumaMin / lumaMax over the five;
//        dir = (-((NW + NE) - (SW + SE)), (NW + SW) - (NE + SE)); dirReduce = max((NW + NE + SW + SE) (0.25 / 8), 1 / 64);
//        dir = clamp(dir / (min(|dir.x|, |dir.y|) + dirReduce), -8, 8);
//        A = (tap(c - dir / 6) + tap(c + dir / 6)) / 2;  B = A / 2 + (tap(c - dir / 2) + tap(c + dir / 2)) / 4;
//        result = A when luma(B) < lumaMin or luma(B) > lumaMax, else B.   (display_fxaa = 0: result = M)
//   ENCODE (display_srgb = 1): the sRGB OETF per colour channel, 12.92 c below 0.0031308, else 1.055 c^(1 / 2.4) - 0.055.
//   FORMAT: RGBA8 = 4 bytes per pixel, R in the lowest byte, each (int)rintf(c 255); RGBA32F = the same values, unquantised.
// Fixed tap order, no atomics: the output depends on the input image and the five parameters only.
#pragma once

// How far a tap reaches: |dir| <= 8, the farthest taps sit at c -+ dir / 2, so their offset o from the texel (x, y) lies in [-4, 4]
// (and likewise in y): x + floor(o) >= x - 4 and x + floor(o) + 1 <= x + 5.  The corner taps reach x - 1 .. x + 1.
constexpr int DP_SPAN = 8;						   // the clamp of dir, in pixels
constexpr int DP_HALO = DP_SPAN / 2 + 1;		   // texels a work item may read beyond its own, per side
constexpr int DP_TILE_X = 64, DP_TILE_Y = 16;	   // pixels of a 256-thread workgroup: a wave64 owns whole 64-pixel row segments
constexpr int DP_LDS_W = DP_TILE_X + 2 * DP_HALO, DP_LDS_H = DP_TILE_Y + 2 * DP_HALO;
constexpr int DP_PITCH = DP_LDS_W | 1;			   // floats per LDS row of one colour plane (odd: rows start on different banks)
static_assert(DP_HALO == 5, "halo = |dir| / 2 (4 px) + 1 texel for the bilinear tap");
static_assert(DP_PITCH >= DP_LDS_W && (DP_PITCH & 1), "LDS row pitch");

constexpr float DP_MAX_IN = 65504.0f;

RT_FN float dp_clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }
RT_FN int dp_edge(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); } // texel index clamped to the edge
RT_FN float dp_luma(f3 c) { return 0.299f * c.x + 0.587f * c.y + 0.114f * c.z; }
RT_FN float dp_rrt_odt(float v)
{
	const float a = v * (v + 0.0245786f) - 0.000090537f, b = v * (0.983729f * v + 0.432951f) + 0.238081f;
	return a / b;
}
// step 1 for one pixel's colour (the alpha is dp_clamp01(in.w))
RT_FN f3 dp_tone(const DisplayView &d, const f4 &in)
{
	const float off = 0.5f + d.brightness - 0.5f * d.contrast;
	const float r = fminf(fmaxf(in.x + off, 0.0f), DP_MAX_IN), g = fminf(fmaxf(in.y + off, 0.0f), DP_MAX_IN),
				b = fminf(fmaxf(in.z + off, 0.0f), DP_MAX_IN);
	if (d.tonemap != 0u) // none
		return mk3(fminf(r, 1.0f), fminf(g, 1.0f), fminf(b, 1.0f));
	// sRGB -> the ACES working space (with the RRT's saturation), the fitted RRT + ODT curve, and back (tone-map.frag:19, 26)
	const float ir = dp_rrt_odt(0.59719f * r + 0.35458f * g + 0.04823f * b), ig = dp_rrt_odt(0.07600f * r + 0.90834f * g + 0.01566f * b),
				ib = dp_rrt_odt(0.02840f * r + 0.13383f * g + 0.83777f * b);
	return mk3(dp_clamp01(1.60475f * ir - 0.53108f * ig - 0.07367f * ib), dp_clamp01(-0.10208f * ir + 1.10813f * ig - 0.00605f * ib),
			   dp_clamp01(-0.00327f * ir - 0.07276f * ig + 1.07602f * ib));
}
// the exposed display (metering.h): every colour channel times E in front of dp_tone, alpha untouched
RT_FN f4 dp_exposed(const f4 &c, float E) { return mk4(c.x * E, c.y * E, c.z * E, c.w); }

// a bilinear tap at c + (ox, oy), c the centre of pixel (x, y); fetch(xi, yi) = the tone-mapped texel, 0 <= xi < W, 0 <= yi < H.
// u = q - 0.5 = x + ox: floor and fraction are taken of the OFFSET, so the weights keep the offset's precision at any x (the sum
// x + 0.5 + ox would round them to the ulp of x: 1.2e-4 px at x = 1900)
template <typename Fetch> RT_FN f3 dp_tap(const Fetch &fetch, int W, int H, int x, int y, float ox, float oy)
{
	const float fx0 = floorf(ox), fy0 = floorf(oy);
	const float fx = ox - fx0, fy = oy - fy0;
	const int ix = x + (int)fx0, iy = y + (int)fy0;
	const int x0 = dp_edge(ix, W), x1 = dp_edge(ix + 1, W), y0 = dp_edge(iy, H), y1 = dp_edge(iy + 1, H);
	const f3 a = fetch(x0, y0), b = fetch(x1, y0), c = fetch(x0, y1), e = fetch(x1, y1);
	const float gx = 1.0f - fx, gy = 1.0f - fy;
	return mk3(gy * (gx * a.x + fx * b.x) + fy * (gx * c.x + fx * e.x), gy * (gx * a.y + fx * b.y) + fy * (gx * c.y + fx * e.y),
			   gy * (gx * a.z + fx * b.z) + fy * (gx * c.z + fx * e.z));
}

RT_FN float dp_srgb(float c) { return c < 0.0031308f ? 12.92f * c : 1.055f * powf(c, 1.0f / 2.4f) - 0.055f; }

// steps 2 - 3 for pixel (x, y): FXAA over `fetch` (or the texel itself) and the encoding — the colour that a store quantises
template <bool FXAA, typename Fetch> RT_FN f3 dp_encoded(const DisplayView &d, const Fetch &fetch, int x, int y)
{
	const int W = (int)d.W, H = (int)d.H;
	f3 out = fetch(x, y);
	if (FXAA)
	{
		const float nw = dp_luma(dp_tap(fetch, W, H, x, y, -0.75f, -0.75f)), ne = dp_luma(dp_tap(fetch, W, H, x, y, 0.25f, -0.75f)),
					sw = dp_luma(dp_tap(fetch, W, H, x, y, -0.75f, 0.25f)), se = dp_luma(dp_tap(fetch, W, H, x, y, 0.25f, 0.25f)),
					m = dp_luma(out);
		const float lmin = fminf(m, fminf(fminf(nw, ne), fminf(sw, se))), lmax = fmaxf(m, fmaxf(fmaxf(nw, ne), fmaxf(sw, se)));
		float dx = -((nw + ne) - (sw + se)), dy = (nw + sw) - (ne + se);
		const float reduce = fmaxf((nw + ne + sw + se) * (0.25f / 8.0f), 1.0f / 64.0f);
		const float rcp = 1.0f / (fminf(fabsf(dx), fabsf(dy)) + reduce);
		dx = fminf(fmaxf(dx * rcp, -(float)DP_SPAN), (float)DP_SPAN), dy = fminf(fmaxf(dy * rcp, -(float)DP_SPAN), (float)DP_SPAN);
		const float ax = dx * (1.0f / 6.0f), ay = dy * (1.0f / 6.0f), bx = dx * 0.5f, by = dy * 0.5f;
		const f3 a0 = dp_tap(fetch, W, H, x, y, -ax, -ay), a1 = dp_tap(fetch, W, H, x, y, ax, ay);
		const f3 b0 = dp_tap(fetch, W, H, x, y, -bx, -by), b1 = dp_tap(fetch, W, H, x, y, bx, by);
		const f3 A = mk3(0.5f * (a0.x + a1.x), 0.5f * (a0.y + a1.y), 0.5f * (a0.z + a1.z));
		const f3 B = mk3(0.5f * A.x + 0.25f * (b0.x + b1.x), 0.5f * A.y + 0.25f * (b0.y + b1.y), 0.5f * A.z + 0.25f * (b0.z + b1.z));
		const float lb = dp_luma(B);
		out = (lb < lmin || lb > lmax) ? A : B;
	}
	if (d.srgb)
		out = mk3(dp_srgb(out.x), dp_srgb(out.y), dp_srgb(out.z));
	return out;
}
// steps 2 - 4 for pixel (x, y): dp_encoded and the store in the view's format.  alpha: the pixel's own in.w, unclamped.
template <bool FXAA, typename Fetch> RT_FN void dp_item(const DisplayView &d, const Fetch &fetch, int x, int y, float alpha)
{
	const f3 out = dp_encoded<FXAA>(d, fetch, x, y);
	const float a = dp_clamp01(alpha);
	const size_t i = (size_t)y * d.W + (size_t)x;
	if (d.format == 0u) // RFWHIP_DISPLAY_RGBA8
		((uint32_t *)d.out)[i] = (uint32_t)(int)rintf(out.x * 255.0f) | ((uint32_t)(int)rintf(out.y * 255.0f) << 8) |
								 ((uint32_t)(int)rintf(out.z * 255.0f) << 16) | ((uint32_t)(int)rintf(a * 255.0f) << 24);
	else
		((f4 *)d.out)[i] = mk4(out.x, out.y, out.z, a);
}
