// bloom.h — the work items of the display stage's bloom (settings "display_bloom*", include/rfwhip.h): an HDR
// glow pyramid of the image the display stage is about to show, added to it in front of the tone map — on the device, stream-ordered,
// nothing read back.  Included by kernels.hip inside namespace rtk, behind metering.h: the device kernels (k_bloom_down0,
// k_bloom_down, k_bloom_up, k_bloom_apply) and the host emulation (kernels_emu.inc) run the same items.
//
// Input: the full W x H linear float4 image, row 0 first, and E, the exposure the display kernel will apply (1 when it applies none).
// Output: a linear float4 image of the same size; alpha is the input's, bit for bit, and nothing else reads it.
//   SANITISE (per colour channel)  c = fminf(fmaxf(x, 0), 65504)      a NaN channel and -inf become 0, +inf becomes 65504 (DP_MAX_IN)
//   PREFILTER (soft knee, in exposed units)  T = threshold, K = knee T
//        br = E max(c.r, c.g, c.b);  soft = clamp((br - T) + K, 0, 2 K);  s2 = soft soft / (4 K + 1e-4)
//        g = fmaxf(s2, br - T) / fmaxf(br, 1e-4);  p = c g                 (0 <= g <= 1, continuous in its inputs)
//   LEVELS  W_0 = W, W_k = (W_{k-1} + 1) >> 1, likewise H;  levels used = max(1, min(levels, first k with W_k = H_k = 1))
//   DOWN 0 -> 1  texel (i, j) of level 1 taps the source texels (2i - 1 .. 2i + 2) x (2j - 1 .. 2j + 2), indices clamped to the edge,
//        with the weights h (x) h, h = (1, 3, 3, 1) / 8, and the Karis weight k_t = 1 / (1 + nz_luma(p_t)) of each tap:
//        D_1 = (sum h_t k_t p_t) / (sum h_t k_t), both sums over the 16 taps in row-major order.  A staged tap is (k p, k).
//   DOWN k -> k + 1 (k >= 1)  the same taps and weights on D_k, no prefilter, no Karis weight.
//   UP, k = levels - 1 .. 1  U_k = D_k + scatter (up(U_{k+1}) - D_k), U_levels = D_levels, written over D_k (a work item reads its
//        own texel of D_k and level k + 1 only).  up at target x: the texels x0 = (x - 1) >> 1 and x0 + 1 of level k + 1, clamped to
//        [0, W_{k+1} - 1], with the weights (1/4, 3/4) for an even x and (3/4, 1/4) for an odd one; two dimensions: the outer
//        product, summed in the order (y0, x0), (y0, x1), (y1, x0), (y1, x1).
//   APPLY  out.rgb = c + intensity up(U_1), out.a = in.a
// Fixed tap order, no atomics, no communication between workgroups: the output depends on the image, E and the five parameters only.
#pragma once

constexpr int BL_TILE_X = 32, BL_TILE_Y = 8;	   // texels of the TARGET level a 256-thread workgroup of a down pass owns
constexpr int BL_LDS_W = 2 * BL_TILE_X + 2, BL_LDS_H = 2 * BL_TILE_Y + 2; // ... and the source texels it stages: the tile and a halo of one
constexpr int BL_PITCH = BL_LDS_W | 1;			   // floats per LDS row of one plane (odd: rows start on different banks)
static_assert(BL_TILE_X * BL_TILE_Y == BLOCK, "one thread per target texel");
static_assert(BL_LDS_W == 66 && BL_LDS_H == 18 && (BL_PITCH & 1) && BL_PITCH >= BL_LDS_W, "the staged tile");

RT_FN uint32_t bl_half(uint32_t n) { return (n + 1u) >> 1; }
// the levels a chain on a W x H image runs: max(1, min(levels, first k with W_k = H_k = 1))
RT_FN uint32_t bl_levels(uint32_t W, uint32_t H, uint32_t levels)
{
	uint32_t k = 0u;
	while (k < levels && (W > 1u || H > 1u))
		W = bl_half(W), H = bl_half(H), k++;
	return k < 1u ? 1u : k;
}
RT_FN float bl_h(int a) { return (a == 0 || a == 3) ? 0.125f : 0.375f; }
RT_FN f3 bl_sanitise(const f4 &x) { return mk3(fminf(fmaxf(x.x, 0.0f), DP_MAX_IN), fminf(fmaxf(x.y, 0.0f), DP_MAX_IN), fminf(fmaxf(x.z, 0.0f), DP_MAX_IN)); }
// the soft-knee gain of a sanitised colour under the exposure E
RT_FN float bl_gain(const f3 &c, float E, const BloomParams &b)
{
	const float br = E * fmaxf(c.x, fmaxf(c.y, c.z)), K = b.knee * b.threshold;
	const float d = br - b.threshold;
	const float soft = fminf(fmaxf(d + K, 0.0f), 2.0f * K);
	const float s2 = soft * soft / (4.0f * K + 1e-4f);
	return fmaxf(s2, d) / fmaxf(br, 1e-4f);
}
// a source texel as the first down pass stages it: (k p, k)
RT_FN f4 bl_stage0(const f4 &x, float E, const BloomParams &b)
{
	const f3 c = bl_sanitise(x);
	const float g = bl_gain(c, E, b);
	const f3 p = mk3(c.x * g, c.y * g, c.z * g);
	const float k = 1.0f / (1.0f + nz_luma(p.x, p.y, p.z));
	return mk4(k * p.x, k * p.y, k * p.z, k);
}
// the 16 taps of target texel (i, j): fetch(x, y) = the staged source texel, x and y NOT yet clamped (the fetch clamps, or was
// staged clamped)
template <typename Fetch> RT_FN f4 bl_taps(const Fetch &fetch, int i, int j)
{
	f4 acc = mk4(0.0f, 0.0f, 0.0f, 0.0f);
	for (int b = 0; b < 4; b++)
		for (int a = 0; a < 4; a++)
		{
			const float w = bl_h(b) * bl_h(a);
			const f4 v = fetch(2 * i - 1 + a, 2 * j - 1 + b);
			acc.x += w * v.x, acc.y += w * v.y, acc.z += w * v.z, acc.w += w * v.w;
		}
	return acc;
}
template <typename Fetch> RT_FN f4 bl_down0_item(const Fetch &fetch, int i, int j)
{
	const f4 s = bl_taps(fetch, i, j); // (s.w >= 2^-17: every k is at least 1 / 65505)
	return mk4(s.x / s.w, s.y / s.w, s.z / s.w, 0.0f);
}
template <typename Fetch> RT_FN f4 bl_down_item(const Fetch &fetch, int i, int j)
{
	const f4 s = bl_taps(fetch, i, j);
	return mk4(s.x, s.y, s.z, 0.0f);
}
// up(next) at the target texel (x, y): next = level k + 1, Wn x Hn texels
RT_FN f3 bl_up(const f4 *next, int Wn, int Hn, int x, int y)
{
	const int xa = (x - 1) >> 1, ya = (y - 1) >> 1;
	const int x0 = dp_edge(xa, Wn), x1 = dp_edge(xa + 1, Wn), y0 = dp_edge(ya, Hn), y1 = dp_edge(ya + 1, Hn);
	const float wx0 = (x & 1) ? 0.75f : 0.25f, wx1 = 1.0f - wx0, wy0 = (y & 1) ? 0.75f : 0.25f, wy1 = 1.0f - wy0;
	const f4 a = next[(size_t)y0 * Wn + x0], b = next[(size_t)y0 * Wn + x1], c = next[(size_t)y1 * Wn + x0], e = next[(size_t)y1 * Wn + x1];
	const float wa = wy0 * wx0, wb = wy0 * wx1, wc = wy1 * wx0, we = wy1 * wx1;
	return mk3(wa * a.x + wb * b.x + wc * c.x + we * e.x, wa * a.y + wb * b.y + wc * c.y + we * e.y, wa * a.z + wb * b.z + wc * c.z + we * e.z);
}
// U_k over D_k, texel i of level k (v.W x v.H; v.next = level k + 1)
RT_FN void bl_up_item(const BloomUpView &v, float scatter, size_t i)
{
	const int x = (int)(i % v.W), y = (int)(i / v.W);
	const f4 d = v.level[i];
	const f3 u = bl_up(v.next, (int)v.Wn, (int)v.Hn, x, y);
	v.level[i] = mk4(d.x + scatter * (u.x - d.x), d.y + scatter * (u.y - d.y), d.z + scatter * (u.z - d.z), 0.0f);
}
// the output pixel i: the sanitised input plus intensity up(U_1)
RT_FN void bl_apply_item(const BloomApplyView &v, float intensity, size_t i)
{
	const int x = (int)(i % v.W), y = (int)(i / v.W);
	const f4 in = v.in[i];
	const f3 c = bl_sanitise(in);
	const f3 u = bl_up(v.next, (int)v.Wn, (int)v.Hn, x, y);
	v.out[i] = mk4(c.x + intensity * u.x, c.y + intensity * u.y, c.z + intensity * u.z, in.w);
}
