// metering.h — the work items of the exposure meter (settings "display_exposure*", include/rfwhip.h): a
// luminance histogram of the image the display stage is about to show, a robust average of it, and a multiplicative exposure with
// temporal adaptation — on the device, stream-ordered, nothing read back.  Included by kernels.hip inside namespace rtk, behind
// display.h: the device kernels (k_meter_hist, k_meter_reduce, k_kat_meter, k_display_exposed) and the host emulation
// (kernels_emu.inc) run the same items.
//
// LUMINANCE AND BIN of a pixel (integer-exact, no transcendental):
//   c = (fmaxf(r, 0), fmaxf(g, 0), fmaxf(b, 0))            a NaN channel becomes 0; alpha is ignored
//   Y = fmaf(0.0722, c.z, fmaf(0.7152, c.y, 0.2126 c.x))   (nz_luma)
//   the pixel is VALID iff 0 < Y < +inf; every other pixel (black, an unrendered remainder, infinite, all-NaN) counts in `excluded`.
//   u = the bit pattern of Y:  bin = clamp((int)(u >> 20) - ((127 - 16) << 3), 0, 255)
//   256 bins, 8 per octave, over [2^-16, 2^16), linear inside an octave; denormals and everything below 2^-16 go to bin 0,
//   everything at or above 2^16 to bin 255.  RFWHIP_KAT_METER_BIN answers the bin of a valid Y and -1 for any other.
//   The representative of bin b in log2 units:  lambda_b = (b >> 3) - 16 + T[b & 7],  T[s] = log2(1 + (s + 0.5) / 8) (MT_T: eight
//   float literals rounded from double).
// HISTOGRAM (k_meter_hist): a workgroup owns MT_RANGE consecutive pixels, counts them into LDS with integer atomics (integer addition
//   commutes: the counts do not depend on scheduling) and stores one partial record of MT_RECORD words, [0..255] the bins, [256]
//   excluded.  No global atomics, no float atomics.
// REDUCE (k_meter_reduce, one workgroup): bin b = the sum of the partial records' word b (integers: any order gives the same
//   word), likewise excluded; then, the counts being exact integers and everything else double, in this fixed shape:
//     N = sum h_b;  C_0 = 0, C_{b+1} = C_b + h_b (a prefix sum of integers);  lo = low N, hi = high N
//     w_b = max(0, min(C_{b+1}, hi) - max(C_b, lo));  p_b = w_b lambda_b (one rounding)
//     num = sum p_b, den = sum w_b over the fixed tree x_b <- x_b + x_{b+s} (b < s) for s = 128, 64, .., 1
//     lambda = (float)(num / den)
//   (the device runs bin b on thread b and the tree through LDS; mt_finish, the emulation's form, walks the same tree)
//   den = 0 (no valid pixel, or an empty window): NO STEP — valid / excluded are written, everything else stays, steps does not
//   advance.  Otherwise, in float32:
//     l_target = clamp((log2_key - lambda) + ev, ev_min, ev_max)       log2_key: log2 of the key, computed by the host in double
//     l = steps == 0 ? l_target : fmaf(speed, l_target - l_prev, l_prev)
//     E = exp2f(l);  steps <- steps + 1
//   The record (MeterRecord, 32 bytes = rfwhip_meter_stats) and the summed histogram stay on the device.
// EXPOSED DISPLAY (k_display_exposed): dp_tone sees x E per colour channel in place of x (one multiplication in front of display.h's
//   expression); alpha is untouched.  E comes from the record through ExposureView, a scalar load.  k_display runs, unchanged,
//   whenever the multiplier is exactly 1 in manual mode.
#pragma once
#include <math.h>

// (MT_BINS, MT_RECORD: kernels.h — the host sizes the records by them)
static_assert(MT_RECORD % 4u == 0u && MT_RECORD > MT_BINS, "a record is whole 16-byte rows and has room for `excluded`");
constexpr uint32_t MT_RANGE = 2048u;						 // pixels a workgroup of k_meter_hist owns
constexpr int MT_BIN0 = (127 - 16) << 3;					 // u >> 20 of 2^-16
static_assert(MT_RANGE % BLOCK == 0, "a workgroup walks its range in whole rounds of one pixel per thread");

RT_FN float mt_luma(const f4 &p) { return nz_luma(fmaxf(p.x, 0.0f), fmaxf(p.y, 0.0f), fmaxf(p.z, 0.0f)); }
RT_FN bool mt_valid(float Y) { return Y > 0.0f && Y <= FLT_MAX; } // (false for a NaN)
RT_FN uint32_t mt_bin(float Y)
{
	const int k = (int)(fbits(Y) >> 20) - MT_BIN0;
	return (uint32_t)(k < 0 ? 0 : (k > (int)MT_BINS - 1 ? (int)MT_BINS - 1 : k));
}
// RFWHIP_KAT_METER_BIN: record i = eight Y values -> eight bins as ints, -1 where Y is not valid
RT_FN void mt_kat_item(const float *in, float *out, uint32_t i)
{
	for (uint32_t k = 0; k < 8u; k++)
	{
		const float Y = in[(size_t)i * 24u + k];
		out[(size_t)i * 8u + k] = ubits(mt_valid(Y) ? mt_bin(Y) : 0xFFFFFFFFu);
	}
}
RT_FN double mt_lambda(uint32_t b)
{
	const float T = (b & 7u) == 0u ? 0.0874628425f : (b & 7u) == 1u ? 0.247927517f : (b & 7u) == 2u ? 0.392317414f : (b & 7u) == 3u ? 0.523561954f
					: (b & 7u) == 4u ? 0.643856168f : (b & 7u) == 5u ? 0.754887521f : (b & 7u) == 6u ? 0.857980967f : 0.954196334f; // MT_T
	return (double)((int)(b >> 3) - 16) + (double)T;
}
// bin b's share of the window [lo, hi] of the cumulative counts: C before the bin, C1 behind it, N in all
RT_FN double mt_weight(uint32_t C, uint32_t C1, uint32_t N, const MeterParams &m)
{
	const double lo = m.low * (double)N, hi = m.high * (double)N;
	const double d = fmin((double)C1, hi) - fmax((double)C, lo);
	return d > 0.0 ? d : 0.0;
}
RT_FN double mt_term(double w, uint32_t b) { return fma(w, mt_lambda(b), 0.0); } // (an fma: the product rounded once, never fused into a sum)
// the step behind the two sums
RT_FN void mt_step(uint32_t N, uint32_t excluded, double num, double den, const MeterParams &m, MeterRecord *rec)
{
	rec->valid = N, rec->excluded = excluded;
	if (!(den > 0.0))
		return; // no step
	const float lambda = (float)(num / den);
	const float t = (m.log2_key - lambda) + m.ev;
	const float target = fminf(fmaxf(t, m.ev_min), m.ev_max);
	const float l = rec->steps == 0u ? target : fmaf(m.speed, target - rec->l, rec->l);
	rec->E = exp2f(l), rec->l = l, rec->l_target = target, rec->lambda = lambda;
	rec->steps = rec->steps + 1u;
}
// the reduce behind the integer sums in one thread (the emulation): `hist` = MT_BINS counts that add up to less than 2^32
RT_FN void mt_finish(const uint32_t *hist, uint32_t excluded, const MeterParams &m, MeterRecord *rec)
{
	double num[MT_BINS], den[MT_BINS];
	uint32_t N = 0u, C = 0u;
	for (uint32_t b = 0; b < MT_BINS; b++)
		N += hist[b];
	for (uint32_t b = 0; b < MT_BINS; b++)
	{
		den[b] = mt_weight(C, C + hist[b], N, m), num[b] = mt_term(den[b], b);
		C += hist[b];
	}
	for (uint32_t s = MT_BINS / 2u; s >= 1u; s >>= 1)
		for (uint32_t b = 0; b < s; b++)
			num[b] += num[b + s], den[b] += den[b + s];
	mt_step(N, excluded, num[0], den[0], m, rec);
}
