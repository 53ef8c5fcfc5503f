// sky_sampling.h — the host side of the sky_sampling setting: the distribution of directions the sky variant of the shade kernel
// draws its next-event samples from (rt_core.h: sky_sample / sky_eval; formulas: include/rfwhip.h).
//
// Texel (i, j) of a W x H sky covers, as pt_sky reads it, phi = atan2(D.x, -D.z) in [-pi + 2 pi i / W, -pi + 2 pi (i + 1) / W) and
// theta = acos(D.y) in [pi j / H, pi (j + 1) / H): a solid angle of (2 pi / W) (cos theta_j - cos theta_{j+1}).  Its weight is its
// luminance times that solid angle; the texel is drawn with probability weight / S (S = the sum of the weights) and a direction
// uniformly in (phi, cos theta) inside it, so the density per steradian is lum / S, constant over the texel.  The table is a
// Walker / Vose alias table over the W * H texels, built in double: one 8-byte entry per texel and one dependent load per sample.
#pragma once
#include "rt_types.h"
#include <cmath>
#include <cstdint>
#include <vector>

namespace skysamp
{
// a texel's weight per steradian: its luminance, 0 for a negative or NaN one (rt_core.h: sky_lum, in float)
inline double luminance(float r, float g, float b)
{
	const double l = 0.2126 * (double)r + 0.7152 * (double)g + 0.0722 * (double)b;
	return l > 0.0 ? l : 0.0; // (NaN > 0 is false)
}

// The alias table of a sky of W x H texels (rgb + pad per texel, row-major).  Returns S, the sum of lum * solid angle; 0 (and an
// empty table) when no texel has a positive weight.
inline double build_alias(const rt::f4 *px, uint32_t W, uint32_t H, std::vector<rt::SkyAlias> &table)
{
	table.clear();
	const size_t n = (size_t)W * H;
	if (!n)
		return 0.0;
	const double pi = 3.14159265358979323846;
	std::vector<double> q(n);
	double S = 0.0;
	size_t heaviest = 0;
	for (uint32_t j = 0; j < H; j++)
	{
		const double omega = (2.0 * pi / W) * (std::cos(pi * j / H) - std::cos(pi * (j + 1) / H));
		for (uint32_t i = 0; i < W; i++)
		{
			const size_t k = (size_t)j * W + i;
			q[k] = luminance(px[k].x, px[k].y, px[k].z) * omega;
			S += q[k];
			if (q[k] > q[heaviest])
				heaviest = k;
		}
	}
	if (!(S > 0.0) || !std::isfinite(S))
		return 0.0;
	// Vose: scale to mean 1; every bucket below 1 is topped up by one above 1, which becomes its alias
	std::vector<uint32_t> small, large;
	small.reserve(n), large.reserve(n);
	for (size_t k = 0; k < n; k++)
	{
		q[k] *= (double)n / S;
		(q[k] < 1.0 ? small : large).push_back((uint32_t)k);
	}
	table.assign(n, rt::SkyAlias{1.0f, 0u});
	for (size_t k = 0; k < n; k++)
		table[k].alias = (uint32_t)k;
	while (!small.empty() && !large.empty())
	{
		const uint32_t s = small.back(), l = large.back();
		small.pop_back();
		table[s].keep = (float)q[s], table[s].alias = l;
		q[l] = (q[l] + q[s]) - 1.0;
		if (q[l] < 1.0)
			large.pop_back(), small.push_back(l);
	}
	// what rounding leaves over keeps its own texel — except a texel of weight 0, which must never be drawn
	for (uint32_t k : small)
		if (q[k] <= 0.0)
			table[k].keep = 0.0f, table[k].alias = (uint32_t)heaviest;
	return S;
}

// The device's view of the table: p = the probability of sampling the sky at a next-event vertex (0: the sky variant is not
// launched), the reciprocals the kernel multiplies by.
inline rt::SkyView view(const rt::SkyAlias *table, double S, float pick, uint32_t W, uint32_t H)
{
	rt::SkyView v;
	v.table = table;
	v.pick = pick;
	v.inv_pick = pick > 0.0f ? (float)(1.0 / pick) : 0.0f;
	v.inv_rest = pick < 1.0f ? (float)(1.0 / (1.0 - (double)pick)) : 0.0f;
	v.inv_total = S > 0.0 ? (float)(1.0 / S) : 0.0f;
	v.inv_w = W ? (float)(1.0 / W) : 0.0f;
	v.inv_2h = H ? (float)(0.5 / H) : 0.0f;
	v.div_w = rt::make_fastdiv(W);
	return v;
}
} // namespace skysamp
