// noise.h — the work items of the noise estimate (settings "noise_*", include/rfwhip.h): the standard error of
// a pixel's mean luminance from the samples actually taken, relative to that mean.  Included by kernels.hip inside namespace rtk,
// in front of resolve_item: the device kernels (k_resolve_noise, k_noise_merge, k_noise_tiles, k_noise_final) and the host
// emulation (kernels_emu.inc) run the same items.
//
// MOMENTS, two floats per local pixel: sumY = sum of Y over the pixel's n samples, M2 = sum of (Y - mean)^2.
//   A sample's value c is what the resolve adds for it: rad.rgb, plus rad_nee.rgb where the resolve adds that (one float32 addition
//   per channel); Y = fmaf(0.0722, c.z, fmaf(0.7152, c.y, 0.2126 c.x)).
//   One call = S samples on top of n_a earlier ones, in sample order, in the resolve's one pass over the slots (NzStep):
//     K = n_a ? sumY / n_a : Y of the first sample          the shift: the mean so far, as the device holds it
//     a = sum (Y_s - K),  b = sum (Y_s - K)^2,  t = sum Y_s
//   and then (nz_merge; Chan, Golub, LeVeque 1979):
//     M2_b = max(0, b - a^2 / S)                            the step's own M2: exact in real arithmetic whatever K is
//     delta = mean_b - mean_a = (K + a / S) - K = a / S     (n_a > 0: mean_a IS K.  Taking a / S, not the float32 difference of the
//                                                            two means, keeps delta at a's precision instead of the ulp of the mean)
//     M2 <- M2 + M2_b + delta^2 n_a S / (n_a + S),   sumY <- sumY + t
//   Why shifted: sum Y^2 - (sum Y)^2 / n in float32 cancels to nothing once n mean^2 exceeds 2^24 M2 — a low-noise pixel after a few
//   hundred samples, exactly the pixel a threshold asks about.  Here every squared quantity is a deviation from the running mean.
//   A NaN or infinite sample makes sumY (and M2) non-finite for good; nz_error answers FLT_MAX for such a pixel.
// METRIC (n >= 2): mean = sumY / n, var = M2 / (n - 1), e = sqrt(var / n) / (mean + noise_floor); e = FLT_MAX where sumY or M2 is
//   not finite or e itself is not a finite number >= 0.  converged: e <= noise_threshold.
// TILES: 32 x 8 pixels, aligned to the ownership strips (STRIP_ROWS rows): a tile never straddles two ranks.  A tile's record counts
//   and sums its real pixels only (x < W, global row < H); sum_e = min(sum, FLT_MAX).  No atomics: a workgroup is a tile, its four
//   waves reduce with a fixed butterfly and thread 0 adds the four partial results in wave order; k_noise_final is one workgroup
//   whose thread t folds the tiles t, t + 256, .. in index order, in double, and whose thread 0 adds the 256 partial results in
//   thread order.  The same state gives the same bytes.
#pragma once
#include <float.h>

static_assert(STRIP_ROWS % NZ_TILE_Y == 0, "a noise tile never straddles two strips");

RT_FN float nz_luma(float r, float g, float b) { return fmaf(0.0722f, b, fmaf(0.7152f, g, 0.2126f * r)); }

// the sums of one call for one pixel
struct NzStep
{
	float K, a, b, t;
	uint32_t S;
	bool shifted;
	RT_FN void begin(uint32_t n_a, float sumY_a)
	{
		shifted = n_a != 0u;
		K = shifted ? sumY_a / (float)n_a : 0.0f;
		a = b = t = 0.0f, S = 0u;
	}
	RT_FN void add(float Y)
	{
		if (!shifted)
			K = Y, shifted = true;
		const float d = Y - K;
		a += d, b = fmaf(d, d, b), t += Y, S++;
	}
};

RT_FN void nz_merge(uint32_t n_a, const NzStep &st, float &sumY, float &M2)
{
	if (!st.S)
		return; // (no sample: a row below the image)
	const float S = (float)st.S, na = (float)n_a;
	const float r = st.b - st.a * st.a / S;
	const float m2b = r < 0.0f ? 0.0f : r; // (a NaN stays one)
	const float delta = st.a / S;
	M2 = (M2 + m2b) + delta * delta * (na * S / (na + S));
	sumY += st.t;
}

// what resolve_item_t hands every sample to, in sample order: rv = the radiance record, qv = the connection record where the resolve
// adds it (nee), else unused
struct NzSink
{
	NzStep st;
	RT_FN void operator()(const f4 &rv, const f4 &qv, bool nee)
	{
		st.add(nee ? nz_luma(rv.x + qv.x, rv.y + qv.y, rv.z + qv.z) : nz_luma(rv.x, rv.y, rv.z));
	}
};
struct ResolveNoSink
{
	RT_FN void operator()(const f4 &, const f4 &, bool) const {}
};

// rfwhip_noise_merge: the step update of pixel i on S given sample values
RT_FN void nz_merge_item(const float *samples_rgb, float *moments, uint32_t n_a, uint32_t S, uint32_t i)
{
	NzStep st;
	st.begin(n_a, moments[2u * i]);
	const float *c = samples_rgb + (size_t)i * S * 3u;
	for (uint32_t s = 0; s < S; s++)
		st.add(nz_luma(c[3u * s], c[3u * s + 1u], c[3u * s + 2u]));
	nz_merge(n_a, st, moments[2u * i], moments[2u * i + 1u]);
}

RT_FN float nz_error(float sumY, float M2, uint32_t n, float floor_)
{
	if (!(fabsf(sumY) <= FLT_MAX) || !(fabsf(M2) <= FLT_MAX))
		return FLT_MAX;
	const float fn = (float)n;
	const float mean = sumY / fn, var = M2 / (fn - 1.0f);
	const float e = sqrtf(var / fn) / (mean + floor_);
	return (e >= 0.0f && e <= FLT_MAX) ? e : FLT_MAX;
}

// is (x, local row yl) a pixel of the image?
RT_FN bool nz_pixel(const NoiseView &v, uint32_t x, uint32_t yl)
{
	return x < v.W && yl < v.local_rows && strip_of_local(yl / STRIP_ROWS, v.rank, v.world) * STRIP_ROWS + yl % STRIP_ROWS < v.H;
}
// one pixel of the metric: its error into the map (0 where there is no pixel); returns whether it is one
RT_FN bool nz_pixel_item(const NoiseView &v, uint32_t x, uint32_t yl, float &e)
{
	const bool real = nz_pixel(v, x, yl);
	e = 0.0f;
	if (x < v.W && yl < v.local_rows)
	{
		const size_t li = (size_t)yl * v.W + x;
		if (real)
			e = nz_error(v.moments[2u * li], v.moments[2u * li + 1u], v.n, v.floor_);
		v.e_map[li] = e;
	}
	return real;
}
// the tiles [first, first + step, ..) folded in that order
RT_FN void nz_fold(const NoiseTile *tiles, uint32_t count, uint32_t first, uint32_t step, NoiseTotal &o)
{
	o.sum_e = 0.0, o.pixels = o.converged = 0ull, o.max_e = 0.0f, o.tiles = count;
	for (uint32_t k = first; k < count; k += step)
		o.sum_e += (double)tiles[k].sum_e, o.pixels += tiles[k].pixels, o.converged += tiles[k].converged, o.max_e = fmaxf(o.max_e, tiles[k].max_e);
}
RT_FN void nz_fold_add(NoiseTotal &o, const NoiseTotal &p)
{
	o.sum_e += p.sum_e, o.pixels += p.pixels, o.converged += p.converged, o.max_e = fmaxf(o.max_e, p.max_e);
}
