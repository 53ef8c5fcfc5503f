// sky_load.h — the sky's two loaders: a Radiance .hdr file decoded on the device into the sky's float4 texels (rfwhip_set_sky_hdr), and
// the alias table of sky_sampling built on the device (sky_table=device) instead of on one host core (include/rfwhip.h; DESIGN.md
// section 23).  Kernel family 17.
//
// The file has two parts.  PART 1 (types, the host's header walk, the work items, and the items run serially over plain host arrays)
// is included by kernels.h at file scope and needs nothing but this file: tests/skyhdr_san_main.cpp includes it alone.  PART 2 (the
// HIP kernels and their launchers, or the emulation's launchers) is included by kernels.hip inside namespace rtk with
// SKY_LOAD_LAUNCHERS defined.  The kernels and the emulation run the same items in the same shapes.
//
// WALK  skyhdr_walk: "#?RADIANCE" or "#?RGBE", header lines up to a blank one (FORMAT=32-bit_rle_rgbe is required, EXPOSURE= is
//   multiplied into the info and not applied, the rest is skipped), the resolution line "-Y H +X W".  Then per scanline: with
//   8 <= W <= 32767 and bytes 2 2 hi lo (hi < 128) it is new-style RLE — hi lo must be W — of four component planes, each a string of
//   count bytes: above 128 a run of count - 128 copies of the next byte, otherwise `count` literal bytes; anything else is W flat
//   RGBE quadruples.  The walk steps over count bytes only and leaves five offsets per scanline: where each plane starts and where
//   the scanline ends (a flat one: its start, SKY_FLAT three times, its end).  A count byte of 0, a run or literal that passes the
//   plane's W bytes, a header with another width and a buffer that ends early are errors that name the scanline; +Y / X-major
//   orientations, 32-bit_rle_xyze and old-style run pixels (1 1 1 n in a flat scanline) are named and not decoded.
// PLANES  skyhdr_plane: item = scanline * 4 + component expands its string into W bytes.  Every read is bounded by the plane's end,
//   every write by W; what the walk would have refused leaves as SKY_ERR_* in the item's flag word, the rest of the plane zero.
// TEXELS  skyhdr_texel: rgb = mantissa * 2^(e - 136), all three 0 when e = 0 (Ward's rgbe2float without the + 0.5, as FreeImage's
//   rgbe_RGBEToFloat).  The float is assembled from integer fields (skyhdr_bits), subnormals included: no rounding, no dependence on
//   a denormal mode.  Row 0 of the sky is the file's first scanline; SKY_FLIP_ROWS turns the rows over.
//
// TABLE  n = W H texels, weight w_k = lum_k * omega_row(k) (lum: 0.2126 r + 0.7152 g + 0.0722 b in double, every product rounded on
//   its own, 0 for a negative or NaN sum; omega: the row's solid angle, made by the host in double), S = sum of w, mu = S / n.  Texel
//   k is heavy when w_k > mu, light otherwise; d_k = max(mu - w_k, 0), e_k = max(w_k - mu, 0), D and E their inclusive prefix sums.
//   The sweep "a light takes its deficit from the current heavy; a heavy pushed below mu is topped up by the next heavy" is decided
//   by cumulative deficit against cumulative excess, so every bucket is found on its own (skytab_assign_item):
//     light k:  a = the first index with E_a > D_k - d_k; found: keep = (float)(w_k / mu), alias = a; none (rounding only): keep = 1,
//               alias = k — or, for w_k = 0, keep = 0, alias = the heaviest texel.
//     heavy k:  nxt = the first index with E_nxt > E_k, i = the first index with D_i >= E_k; both found:
//               keep = (float)clamp(1 - (D_i - E_k) / mu, 0, 1), alias = nxt; otherwise keep = 1, alias = k.
//   REDUCTION (fixed shape, no atomics): a workgroup of 256 threads owns 1024 consecutive texels, a thread 4 consecutive ones, added
//   left to right; the 256 thread sums fold by halving strides (t += t + stride, stride 128 .. 1) into one partial (sum, first index
//   of the maximum) per workgroup; k_skytab_total: thread t adds the partials t, t + 256, ... left to right, the same fold.
//   SCAN (fixed shape): three nested levels of CHAINS.  A thread chains its 4 elements (p_i = fl(p_{i-1} + x_i)); one lane chains the
//   256 thread totals of a block of B = 1024 elements (X_{t+1} = fl(X_t + s_t), X_0 = 0), an element's value local to its block is
//   fl(X_t + p_i); k_skytab_scan_super chains the totals of the B blocks of a super-block the same way (block bases), and
//   k_skytab_scan_top the totals of the at most 2048 super-blocks (n < 2^31).  The prefix is fl(SB_c + fl(BB_b + local_k))
//   (k_skytab_scan_apply).  WHY THIS IS NON-DECREASING: all terms are >= 0 and x -> fl(base + x) is non-decreasing, so (1) a chain is
//   non-decreasing; (2) if the values local to a unit are non-decreasing, the unit's total IS its last local value, and the next
//   unit's base IS fl(base + total), then the last value of a unit, fl(base + total), equals the next unit's base, which is <= the
//   next unit's first value fl(next base + local_0): the values fl(base + local) are non-decreasing across units as well.  (2) holds
//   for threads inside a block, blocks inside a super-block and super-blocks inside the array in turn.  Bases summed from totals in
//   any other association — a tree, or one rounding from the top — can step DOWN at a unit's edge by an ulp; the binary searches
//   above need the order.  An element with x = 0 repeats its predecessor's value exactly (fl(v + 0) = v at every level), so "the
//   first index with E > t" always lands on a texel with e > 0: every alias is heavy, and a texel of weight 0 — keep = 0, never
//   heavy — is never drawn.
//   Arithmetic: double add, multiply, divide and integers only, products rounded on their own (sky_m): the emulation and the device
//   give the same bytes.
#ifndef RFWHIP_SKY_LOAD_H
#define RFWHIP_SKY_LOAD_H

#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#ifndef RT_FN
#define RT_FN inline
#endif

namespace rtk
{

constexpr int SKY_OK = 0, SKY_INVALID = 1, SKY_UNSUPPORTED = 5; // = RFWHIP_OK, RFWHIP_ERR_INVALID_ARGUMENT, RFWHIP_ERR_UNSUPPORTED
constexpr uint32_t SKY_FLIP_ROWS = 1u;							 // = RFWHIP_SKYSRC_FLIP_ROWS
// error flags of a plane item (= RFWHIP_SKYHDR_ERR_*)
constexpr uint32_t SKY_ERR_ZERO = 1u, SKY_ERR_OVERRUN = 2u, SKY_ERR_TRUNCATED = 4u;
constexpr uint32_t SKY_FLAT = 0xFFFFFFFFu; // offsets 1 .. 3 of a flat scanline
// the table's shapes: threads of a workgroup, elements of a thread, elements of a block (= blocks of a super-block)
constexpr uint32_t SKYTAB_THREADS = 256u, SKYTAB_ITEMS = 4u, SKYTAB_B = 1024u, SKYTAB_B_LOG2 = 10u;
static_assert(SKYTAB_THREADS * SKYTAB_ITEMS == SKYTAB_B && (1u << SKYTAB_B_LOG2) == SKYTAB_B, "a block is a workgroup's elements");
// flags of the record (= RFWHIP_SKYTAB_*)
constexpr uint32_t SKYTAB_VALID = 1u, SKYTAB_DEVICE = 2u;

struct alignas(16) SkyF4
{
	float x, y, z, w;
};
// = rt::SkyAlias (rt_types.h), which part 1 does not see
struct SkyAliasEntry
{
	float keep;
	uint32_t alias;
};
// what the table's chain leaves (= rfwhip_sky_table_record)
struct SkyTabRecord
{
	double S;
	uint32_t heaviest, light, heavy, flags, pad[2];
};
static_assert(sizeof(SkyTabRecord) == 32, "the record is 32 bytes");
struct SkyPartial
{
	double sum, maxv;
	uint32_t idx, pad;
};
// One decode.  stream: the file's bytes; ranges: five offsets per scanline; planes: item * W bytes (null when every scanline is flat);
// flags: a word per item; out: W x H texels
struct SkyHdrView
{
	const uint8_t *stream;
	const uint32_t *ranges;
	uint8_t *planes;
	uint32_t *flags;
	SkyF4 *out;
	uint32_t W, H, mods, pad;
};
// One table.  sky / omega / W: where the weights come from (sky = null: w holds them already); D, E: n each; part: a partial per
// block; t1d, t1e, c1: per block, t2d, t2e, c2: per super-block (totals, then exclusive bases; heavy counts)
struct SkyTabView
{
	const SkyF4 *sky;
	const double *omega;
	double *w, *D, *E;
	SkyPartial *part;
	double *t1d, *t1e, *t2d, *t2e;
	uint32_t *c1, *c2;
	SkyTabRecord *rec;
	SkyAliasEntry *table;
	uint32_t W, n, nb1, nb2;
};
RT_FN uint32_t skytab_blocks(uint32_t n) { return (n + SKYTAB_B - 1u) >> SKYTAB_B_LOG2; }

// ---- the host's header walk ---------------------------------------------------------------------------------------------------
struct SkyHdrInfo
{
	uint32_t W = 0, H = 0, rle_lines = 0, flat_lines = 0;
	float exposure = 1.0f;
	std::vector<uint32_t> ranges; // 5 per scanline
	char msg[192] = {};
};
inline int skyhdr_fail(SkyHdrInfo &o, int code, const char *fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(o.msg, sizeof(o.msg), fmt, ap);
	va_end(ap);
	return code;
}
// the header and every scanline's offsets (rfwhip_hdr_info walks the scanlines as well: its `supported` covers them); W and H are
// filled as soon as the resolution line is read, whatever the answer
inline int skyhdr_walk(const uint8_t *d, size_t n, SkyHdrInfo &o)
{
	o.ranges.clear();
	if (!d || n < 7 || memcmp(d, "#?", 2))
		return skyhdr_fail(o, SKY_INVALID, "not a Radiance file (no #? magic)");
	if (n > 0xFFFFFFF0ull)
		return skyhdr_fail(o, SKY_UNSUPPORTED, "a file of %zu bytes (32-bit offsets)", n);
	// a line [p, p + len) and the byte behind its '\n'; false: the buffer ends first
	const auto line = [&](size_t p, size_t &len, size_t &next) {
		const uint8_t *q = p < n ? (const uint8_t *)memchr(d + p, '\n', n - p) : nullptr;
		if (!q)
			return false;
		len = (size_t)(q - d) - p, next = (size_t)(q - d) + 1u;
		if (len && d[p + len - 1u] == '\r')
			len--;
		return true;
	};
	const auto starts = [&](size_t p, size_t len, const char *s) { return len >= strlen(s) && !memcmp(d + p, s, strlen(s)); };
	const auto copy = [&](size_t p, size_t len, char buf[64]) {
		const size_t k = len < 63u ? len : 63u;
		memcpy(buf, d + p, k), buf[k] = 0;
	};
	size_t p = 0, len = 0, next = 0;
	if (!line(0, len, next))
		return skyhdr_fail(o, SKY_INVALID, "the header ends inside its first line (truncated; no blank line)");
	if (!((len == 10u && starts(0, len, "#?RADIANCE")) || (len == 6u && starts(0, len, "#?RGBE"))))
		return skyhdr_fail(o, SKY_INVALID, "not a Radiance file (the magic is neither #?RADIANCE nor #?RGBE)");
	bool format = false, xyze = false;
	char buf[64];
	for (p = next;; p = next)
	{
		if (!line(p, len, next))
			return skyhdr_fail(o, SKY_INVALID, "no blank line ends the header (byte %zu: truncated)", p);
		if (!len)
			break;
		if (len >= 3u && (d[p] == '-' || d[p] == '+') && (d[p + 1u] == 'X' || d[p + 1u] == 'Y') && d[p + 2u] == ' ')
			return skyhdr_fail(o, SKY_INVALID, "no blank line ends the header (a resolution line at byte %zu)", p);
		if (starts(p, len, "FORMAT="))
		{
			copy(p + 7u, len - 7u, buf);
			if (!strcmp(buf, "32-bit_rle_xyze"))
				xyze = true;
			else if (strcmp(buf, "32-bit_rle_rgbe"))
				return skyhdr_fail(o, SKY_INVALID, "FORMAT=%s is no Radiance picture format", buf);
			format = true;
		}
		else if (starts(p, len, "EXPOSURE="))
		{
			copy(p + 9u, len - 9u, buf);
			const double e = strtod(buf, nullptr);
			if (e > 0.0 && e < 1e30)
				o.exposure = (float)((double)o.exposure * e);
		}
	}
	p = next;
	if (!line(p, len, next))
		return skyhdr_fail(o, SKY_INVALID, "the file ends inside the resolution line (truncated)");
	copy(p, len, buf);
	char s1 = 0, a1 = 0, s2 = 0, a2 = 0;
	unsigned n1 = 0, n2 = 0;
	if (sscanf(buf, "%c%c %u %c%c %u", &s1, &a1, &n1, &s2, &a2, &n2) != 6 || (s1 != '-' && s1 != '+') || (s2 != '-' && s2 != '+') ||
		!((a1 == 'Y' && a2 == 'X') || (a1 == 'X' && a2 == 'Y')))
		return skyhdr_fail(o, SKY_INVALID, "the resolution line '%s' is malformed", buf);
	o.H = a1 == 'Y' ? n1 : n2, o.W = a1 == 'Y' ? n2 : n1;
	if (!format)
		return skyhdr_fail(o, SKY_INVALID, "the header has no FORMAT line");
	if (!(a1 == 'Y' && s1 == '-' && s2 == '+'))
		return skyhdr_fail(o, SKY_UNSUPPORTED, "orientation %c%c .. %c%c (only -Y H +X W is decoded)", s1, a1, s2, a2);
	if (xyze)
		return skyhdr_fail(o, SKY_UNSUPPORTED, "FORMAT=32-bit_rle_xyze (XYZE colours are not decoded)");
	if (!o.W || !o.H)
		return skyhdr_fail(o, SKY_INVALID, "a %u x %u picture", o.W, o.H);
	if ((uint64_t)o.W * o.H > 0x3FFFFFFFull)
		return skyhdr_fail(o, SKY_UNSUPPORTED, "a %u x %u picture (more than 2^30 texels)", o.W, o.H);
	const uint32_t W = o.W;
	o.ranges.resize((size_t)o.H * 5u);
	p = next;
	for (uint32_t y = 0; y < o.H; y++)
	{
		uint32_t *r = &o.ranges[(size_t)y * 5u];
		if (n - p < 4u)
			return skyhdr_fail(o, SKY_INVALID, "scanline %u: the file ends in front of it (truncated)", y);
		if (W >= 8u && W <= 32767u && d[p] == 2u && d[p + 1u] == 2u && !(d[p + 2u] & 0x80u))
		{
			const uint32_t width = ((uint32_t)d[p + 2u] << 8) | d[p + 3u];
			if (width != W)
				return skyhdr_fail(o, SKY_INVALID, "scanline %u: its header names width %u, the picture has %u", y, width, W);
			p += 4u;
			for (uint32_t c = 0; c < 4u; c++)
			{
				r[c] = (uint32_t)p;
				for (uint32_t filled = 0; filled < W;)
				{
					if (p >= n)
						return skyhdr_fail(o, SKY_INVALID, "scanline %u: the file ends inside component %u (truncated)", y, c);
					const uint32_t count = d[p++];
					if (!count)
						return skyhdr_fail(o, SKY_INVALID, "scanline %u: a count byte of 0 in component %u", y, c);
					const uint32_t l = count > 128u ? count - 128u : count, bytes = count > 128u ? 1u : count;
					if (n - p < bytes)
						return skyhdr_fail(o, SKY_INVALID, "scanline %u: the file ends inside component %u (truncated)", y, c);
					p += bytes;
					if (filled + l > W)
						return skyhdr_fail(o, SKY_INVALID, "scanline %u: a %s of %u overruns component %u's plane (%u of %u bytes filled)", y,
										   count > 128u ? "run" : "literal", l, c, filled, W);
					filled += l;
				}
			}
			r[4] = (uint32_t)p, o.rle_lines++;
			continue;
		}
		if ((n - p) / 4u < W)
			return skyhdr_fail(o, SKY_INVALID, "scanline %u: the file ends inside it (truncated: %zu of %u flat bytes)", y, n - p, 4u * W);
		for (uint32_t x = 0; x < W; x++)
			if (d[p + 4u * x] == 1u && d[p + 4u * x + 1u] == 1u && d[p + 4u * x + 2u] == 1u)
				return skyhdr_fail(o, SKY_UNSUPPORTED, "scanline %u: an old-style run pixel (1 1 1 n) at column %u", y, x);
		r[0] = (uint32_t)p, r[1] = r[2] = r[3] = SKY_FLAT, r[4] = (uint32_t)(p + 4u * (size_t)W), o.flat_lines++;
		p += 4u * (size_t)W;
	}
	return SKY_OK;
}

// ---- decode: the work items ---------------------------------------------------------------------------------------------------
// item = scanline * 4 + component of an RLE scanline: its W bytes -> the error flags
RT_FN uint32_t skyhdr_plane(const SkyHdrView &v, uint32_t item)
{
	const uint32_t *r = v.ranges + (size_t)(item >> 2) * 5u;
	if (r[1] == SKY_FLAT)
		return 0u;
	const uint32_t c = item & 3u, W = v.W, end = r[c + 1u];
	uint32_t pos = r[c], filled = 0u, err = 0u;
	uint8_t *out = v.planes + (size_t)item * W;
	while (filled < W)
	{
		if (pos >= end)
		{
			err |= SKY_ERR_TRUNCATED;
			break;
		}
		const uint32_t count = v.stream[pos++];
		if (!count)
		{
			err |= SKY_ERR_ZERO;
			break;
		}
		uint32_t l = count > 128u ? count - 128u : count;
		if (l > W - filled)
			err |= SKY_ERR_OVERRUN, l = W - filled;
		if (count > 128u)
		{
			if (pos >= end)
			{
				err |= SKY_ERR_TRUNCATED;
				break;
			}
			const uint8_t b = v.stream[pos++];
			for (uint32_t k = 0; k < l; k++)
				out[filled + k] = b;
		}
		else
		{
			if (l > end - pos)
				err |= SKY_ERR_TRUNCATED, l = end - pos;
			for (uint32_t k = 0; k < l; k++)
				out[filled + k] = v.stream[pos + k];
			pos += l;
		}
		filled += l;
		if (err)
			break;
	}
	for (; filled < W; filled++)
		out[filled] = 0u;
	return err;
}
// the bits of the float m * 2^(e - 136), m = 1 .. 255, e = 1 .. 255: exact, subnormal below 2^-126
RT_FN uint32_t skyhdr_bits(uint32_t m, uint32_t e)
{
	if (!m)
		return 0u;
	const uint32_t hb = 31u - (uint32_t)__builtin_clz(m); // m = 1.xxx * 2^hb
	const int E = (int)(hb + e) - 9;						  // the biased exponent: hb + e - 136 + 127
	if (E >= 1)
		return ((uint32_t)E << 23) | ((m << (23u - hb)) & 0x7FFFFFu);
	return m << (e + 13u); // units of 2^-149; hb + e <= 9: below 2^23
}
RT_FN float skyhdr_float(uint32_t bits)
{
	float f;
	memcpy(&f, &bits, 4);
	return f;
}
// texel i of the sky (row ty = i / W)
RT_FN SkyF4 skyhdr_texel(const SkyHdrView &v, uint32_t i)
{
	const uint32_t ty = i / v.W, x = i - ty * v.W, y = (v.mods & SKY_FLIP_ROWS) ? v.H - 1u - ty : ty;
	const uint32_t *r = v.ranges + (size_t)y * 5u;
	uint32_t q[4];
	if (r[1] == SKY_FLAT)
		for (uint32_t c = 0; c < 4u; c++)
			q[c] = v.stream[(size_t)r[0] + 4u * (size_t)x + c];
	else
		for (uint32_t c = 0; c < 4u; c++)
			q[c] = v.planes[((size_t)y * 4u + c) * v.W + x];
	SkyF4 o = {0.0f, 0.0f, 0.0f, 0.0f};
	if (q[3])
		o.x = skyhdr_float(skyhdr_bits(q[0], q[3])), o.y = skyhdr_float(skyhdr_bits(q[1], q[3])), o.z = skyhdr_float(skyhdr_bits(q[2], q[3]));
	return o;
}

// ---- the table: the work items ------------------------------------------------------------------------------------------------
// a product rounded on its own (rounded() of rt_core.h, for doubles: an empty asm hides it from the contraction pass; it emits nothing)
RT_FN double sky_m(double a, double b)
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
RT_FN double skytab_weight(const SkyTabView &v, uint32_t k)
{
	if (!v.sky)
	{
		const double w = v.w[k];
		return w > 0.0 ? w : 0.0; // (NaN > 0 is false)
	}
	const SkyF4 t = v.sky[k];
	const double l = (sky_m(0.2126, (double)t.x) + sky_m(0.7152, (double)t.y)) + sky_m(0.0722, (double)t.z);
	return l > 0.0 ? sky_m(l, v.omega[k / v.W]) : 0.0;
}
// does (bv, bi) take the place of (av, ai) as the maximum: the larger value, the lower index among equals
RT_FN bool skytab_better(double av, uint32_t ai, double bv, uint32_t bi) { return bv > av || (bv == av && bi < ai); }
// a thread's four texels from `base` on: their weights stored, added left to right; the first index of their maximum (a texel past
// the end weighs 0 and loses every tie to one inside)
RT_FN void skytab_thread_weights(const SkyTabView &v, uint32_t base, double &sum, double &maxv, uint32_t &maxi)
{
	for (uint32_t i = 0; i < SKYTAB_ITEMS; i++)
	{
		const uint32_t k = base + i;
		double w = 0.0;
		if (k < v.n)
			w = skytab_weight(v, k), v.w[k] = w;
		if (!i)
			sum = w, maxv = w, maxi = k;
		else
		{
			sum = sum + w;
			if (w > maxv)
				maxv = w, maxi = k;
		}
	}
}
// a thread's four elements from `base` on: the chains of their deficits and excesses, the number of heavy ones
RT_FN void skytab_thread_scan(const SkyTabView &v, double mu, uint32_t base, double pd[SKYTAB_ITEMS], double pe[SKYTAB_ITEMS], uint32_t &heavy)
{
	heavy = 0u;
	for (uint32_t i = 0; i < SKYTAB_ITEMS; i++)
	{
		const uint32_t k = base + i;
		double d = 0.0, e = 0.0;
		if (k < v.n)
		{
			const double w = v.w[k];
			if (w > mu)
				e = w - mu, heavy++;
			else if (w < mu)
				d = mu - w;
		}
		pd[i] = i ? pd[i - 1u] + d : d, pe[i] = i ? pe[i - 1u] + e : e;
	}
}
// one lane's chain over m values: each value becomes the sum of those in front of it -> the total
RT_FN double skytab_chain(double *x, uint32_t m)
{
	double X = 0.0;
	for (uint32_t j = 0; j < m; j++)
	{
		const double t = x[j];
		x[j] = X, X = X + t;
	}
	return X;
}
RT_FN uint32_t skytab_chain_u(uint32_t *x, uint32_t m)
{
	uint32_t X = 0u;
	for (uint32_t j = 0; j < m; j++)
	{
		const uint32_t t = x[j];
		x[j] = X, X += t;
	}
	return X;
}
RT_FN void skytab_apply_item(const SkyTabView &v, uint32_t k)
{
	const uint32_t b = k >> SKYTAB_B_LOG2, c = b >> SKYTAB_B_LOG2;
	v.D[k] = v.t2d[c] + (v.t1d[b] + v.D[k]);
	v.E[k] = v.t2e[c] + (v.t1e[b] + v.E[k]);
}
// the first index of the non-decreasing a[0 .. n) with a[i] > x (or >= x); n: none
RT_FN uint32_t skytab_first_gt(const double *a, uint32_t n, double x)
{
	uint32_t lo = 0u, hi = n;
	while (lo < hi)
	{
		const uint32_t mid = (lo + hi) >> 1;
		if (a[mid] > x)
			hi = mid;
		else
			lo = mid + 1u;
	}
	return lo;
}
RT_FN uint32_t skytab_first_ge(const double *a, uint32_t n, double x)
{
	uint32_t lo = 0u, hi = n;
	while (lo < hi)
	{
		const uint32_t mid = (lo + hi) >> 1;
		if (a[mid] >= x)
			hi = mid;
		else
			lo = mid + 1u;
	}
	return lo;
}
RT_FN void skytab_assign_item(const SkyTabView &v, uint32_t k)
{
	SkyAliasEntry o;
	o.keep = 1.0f, o.alias = k;
	const double S = v.rec->S;
	if (v.rec->flags & SKYTAB_VALID)
	{
		const double mu = S / (double)v.n, w = v.w[k];
		if (!(w > mu)) // light
		{
			double before = v.D[k] - (mu - w); // the deficit in front of k
			before = before > 0.0 ? before : 0.0;
			const uint32_t a = skytab_first_gt(v.E, v.n, before);
			if (a < v.n)
				o.keep = (float)(w / mu), o.alias = a;
			else if (!(w > 0.0)) // (no heavy left for it, by rounding: it must still never be drawn)
				o.keep = 0.0f, o.alias = v.rec->heaviest;
		}
		else
		{
			const double Ek = v.E[k];
			const uint32_t nxt = skytab_first_gt(v.E, v.n, Ek), i = skytab_first_ge(v.D, v.n, Ek);
			if (nxt < v.n && i < v.n)
			{
				double q = 1.0 - (v.D[i] - Ek) / mu;
				q = q < 0.0 ? 0.0 : q > 1.0 ? 1.0 : q;
				o.keep = (float)q, o.alias = nxt;
			}
		}
	}
	v.table[k] = o;
}
// the fold of a workgroup's 256 (sum, maximum) pairs into entry 0, by halving strides: step `stride` of thread t < stride
RT_FN void skytab_fold(double *s, double *m, uint32_t *mi, uint32_t t, uint32_t stride)
{
	s[t] = s[t] + s[t + stride];
	if (skytab_better(m[t], mi[t], m[t + stride], mi[t + stride]))
		m[t] = m[t + stride], mi[t] = mi[t + stride];
}
RT_FN void skytab_record(const SkyTabView &v, double S, uint32_t heaviest)
{
	SkyTabRecord r;
	r.S = S, r.heaviest = heaviest, r.light = 0u, r.heavy = 0u, r.pad[0] = r.pad[1] = 0u;
	r.flags = SKYTAB_DEVICE | ((S > 0.0 && S < INFINITY) ? SKYTAB_VALID : 0u);
	*v.rec = r;
}

// ---- the items run serially over host arrays (the emulation, the stand-alone program): a workgroup at a time ----
inline void skyhdr_host_planes(const SkyHdrView &v)
{
	for (uint32_t i = 0; i < v.H * 4u; i++)
		v.flags[i] = skyhdr_plane(v, i);
}
inline void skyhdr_host_texels(const SkyHdrView &v)
{
	for (uint32_t i = 0; i < v.W * v.H; i++)
		v.out[i] = skyhdr_texel(v, i);
}
inline void skytab_host_fold(double *s, double *m, uint32_t *mi)
{
	for (uint32_t stride = SKYTAB_THREADS / 2u; stride; stride >>= 1)
		for (uint32_t t = 0; t < stride; t++)
			skytab_fold(s, m, mi, t, stride);
}
inline void skytab_host_weights(const SkyTabView &v)
{
	double s[SKYTAB_THREADS], m[SKYTAB_THREADS];
	uint32_t mi[SKYTAB_THREADS];
	for (uint32_t g = 0; g < v.nb1; g++)
	{
		for (uint32_t t = 0; t < SKYTAB_THREADS; t++)
			skytab_thread_weights(v, g * SKYTAB_B + t * SKYTAB_ITEMS, s[t], m[t], mi[t]);
		skytab_host_fold(s, m, mi);
		v.part[g].sum = s[0], v.part[g].maxv = m[0], v.part[g].idx = mi[0], v.part[g].pad = 0u;
	}
}
inline void skytab_host_total(const SkyTabView &v)
{
	double s[SKYTAB_THREADS], m[SKYTAB_THREADS];
	uint32_t mi[SKYTAB_THREADS];
	for (uint32_t t = 0; t < SKYTAB_THREADS; t++)
	{
		s[t] = 0.0, m[t] = -1.0, mi[t] = 0xFFFFFFFFu;
		for (uint32_t j = t; j < v.nb1; j += SKYTAB_THREADS)
		{
			s[t] = s[t] + v.part[j].sum;
			if (skytab_better(m[t], mi[t], v.part[j].maxv, v.part[j].idx))
				m[t] = v.part[j].maxv, mi[t] = v.part[j].idx;
		}
	}
	skytab_host_fold(s, m, mi);
	skytab_record(v, s[0], mi[0]);
}
inline void skytab_host_scan_block(const SkyTabView &v)
{
	const double mu = v.rec->S / (double)v.n;
	double xd[SKYTAB_THREADS], xe[SKYTAB_THREADS], pd[SKYTAB_THREADS][SKYTAB_ITEMS], pe[SKYTAB_THREADS][SKYTAB_ITEMS];
	uint32_t xc[SKYTAB_THREADS];
	for (uint32_t b = 0; b < v.nb1; b++)
	{
		for (uint32_t t = 0; t < SKYTAB_THREADS; t++)
		{
			skytab_thread_scan(v, mu, b * SKYTAB_B + t * SKYTAB_ITEMS, pd[t], pe[t], xc[t]);
			xd[t] = pd[t][SKYTAB_ITEMS - 1u], xe[t] = pe[t][SKYTAB_ITEMS - 1u];
		}
		v.t1d[b] = skytab_chain(xd, SKYTAB_THREADS), v.t1e[b] = skytab_chain(xe, SKYTAB_THREADS), v.c1[b] = skytab_chain_u(xc, SKYTAB_THREADS);
		for (uint32_t t = 0; t < SKYTAB_THREADS; t++)
			for (uint32_t i = 0; i < SKYTAB_ITEMS; i++)
			{
				const uint32_t k = b * SKYTAB_B + t * SKYTAB_ITEMS + i;
				if (k < v.n)
					v.D[k] = xd[t] + pd[t][i], v.E[k] = xe[t] + pe[t][i];
			}
	}
}
inline void skytab_host_scan_super(const SkyTabView &v)
{
	for (uint32_t c = 0; c < v.nb2; c++)
	{
		const uint32_t first = c * SKYTAB_B, m = v.nb1 - first < SKYTAB_B ? v.nb1 - first : SKYTAB_B;
		v.t2d[c] = skytab_chain(v.t1d + first, m), v.t2e[c] = skytab_chain(v.t1e + first, m), v.c2[c] = skytab_chain_u(v.c1 + first, m);
	}
}
inline void skytab_host_scan_top(const SkyTabView &v)
{
	skytab_chain(v.t2d, v.nb2), skytab_chain(v.t2e, v.nb2);
	v.rec->heavy = skytab_chain_u(v.c2, v.nb2), v.rec->light = v.n - v.rec->heavy;
}
inline void skytab_host_scan_apply(const SkyTabView &v)
{
	for (uint32_t k = 0; k < v.n; k++)
		skytab_apply_item(v, k);
}
inline void skytab_host_assign(const SkyTabView &v)
{
	for (uint32_t k = 0; k < v.n; k++)
		skytab_assign_item(v, k);
}

} // namespace rtk
#endif // RFWHIP_SKY_LOAD_H

// =================================================================================================================================
// PART 2: the kernels and the launchers (kernels.hip, inside namespace rtk)
// =================================================================================================================================
#if defined(SKY_LOAD_LAUNCHERS) && !defined(RFWHIP_SKY_LOAD_LAUNCHERS_DONE)
#define RFWHIP_SKY_LOAD_LAUNCHERS_DONE
#if defined(RT_DEVICE_BUILD)

// (The kernels are templates with one unused parameter for the sake of where their code lands: a template is emitted where it is
// first used — by the launchers at the end of this file, the end of kernels.hip — behind every kernel that existed before, so those
// keep their addresses in the code object.  As plain functions they would be emitted in front of every template kernel and move them.)

// ---- k_skyhdr_planes: a thread per (scanline, component); it walks its plane's count bytes serially (their lengths are data) and
// writes only its own W bytes; its flags leave by a plain store ----
template <int LAST>
__global__ void __launch_bounds__(64) k_skyhdr_planes(const SkyHdrView v)
{
	const uint32_t i = blockIdx.x * 64u + threadIdx.x;
	if (i < v.H * 4u)
		v.flags[i] = skyhdr_plane(v, i);
}
// ---- k_skyhdr_texels: a thread per texel, one 16-byte store ----
template <int LAST>
__global__ void __launch_bounds__(BLOCK) k_skyhdr_texels(const SkyHdrView v)
{
	const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
	if (i < (size_t)v.W * v.H)
		v.out[i] = skyhdr_texel(v, (uint32_t)i);
}

// the fold of part 1 over LDS: every thread reaches every barrier
__device__ __forceinline__ void skytab_fold_lds(double *s, double *m, uint32_t *mi)
{
	__syncthreads();
	for (uint32_t stride = SKYTAB_THREADS / 2u; stride; stride >>= 1)
	{
		if (threadIdx.x < stride)
			skytab_fold(s, m, mi, threadIdx.x, stride);
		__syncthreads();
	}
}
// ---- k_skytab_weights: a workgroup per block of 1024 texels: the weights, and the block's partial ----
template <int LAST>
__global__ void __launch_bounds__(SKYTAB_THREADS) k_skytab_weights(const SkyTabView v)
{
	__shared__ double s_s[SKYTAB_THREADS], s_m[SKYTAB_THREADS];
	__shared__ uint32_t s_i[SKYTAB_THREADS];
	const uint32_t t = threadIdx.x;
	skytab_thread_weights(v, blockIdx.x * SKYTAB_B + t * SKYTAB_ITEMS, s_s[t], s_m[t], s_i[t]);
	skytab_fold_lds(s_s, s_m, s_i);
	if (!t)
	{
		SkyPartial p;
		p.sum = s_s[0], p.maxv = s_m[0], p.idx = s_i[0], p.pad = 0u;
		v.part[blockIdx.x] = p;
	}
}
// ---- k_skytab_total: one workgroup: S, the heaviest texel and the record's flags ----
template <int LAST>
__global__ void __launch_bounds__(SKYTAB_THREADS) k_skytab_total(const SkyTabView v)
{
	__shared__ double s_s[SKYTAB_THREADS], s_m[SKYTAB_THREADS];
	__shared__ uint32_t s_i[SKYTAB_THREADS];
	const uint32_t t = threadIdx.x;
	double s = 0.0, m = -1.0;
	uint32_t mi = 0xFFFFFFFFu;
	for (uint32_t j = t; j < v.nb1; j += SKYTAB_THREADS)
	{
		const SkyPartial p = v.part[j];
		s = s + p.sum;
		if (skytab_better(m, mi, p.maxv, p.idx))
			m = p.maxv, mi = p.idx;
	}
	s_s[t] = s, s_m[t] = m, s_i[t] = mi;
	skytab_fold_lds(s_s, s_m, s_i);
	if (!t)
		skytab_record(v, s_s[0], s_i[0]);
}
// ---- k_skytab_scan_block: a workgroup per block: the threads' chains, then three lanes of three different waves chain the 256
// thread totals of D, of E and of the heavy counts through LDS; the elements' block-local values go to D and E ----
template <int LAST>
__global__ void __launch_bounds__(SKYTAB_THREADS) k_skytab_scan_block(const SkyTabView v)
{
	__shared__ double s_d[SKYTAB_THREADS], s_e[SKYTAB_THREADS];
	__shared__ uint32_t s_c[SKYTAB_THREADS];
	const uint32_t t = threadIdx.x, b = blockIdx.x, base = b * SKYTAB_B + t * SKYTAB_ITEMS;
	const double mu = v.rec->S / (double)v.n;
	double pd[SKYTAB_ITEMS], pe[SKYTAB_ITEMS];
	uint32_t heavy;
	skytab_thread_scan(v, mu, base, pd, pe, heavy);
	s_d[t] = pd[SKYTAB_ITEMS - 1u], s_e[t] = pe[SKYTAB_ITEMS - 1u], s_c[t] = heavy;
	__syncthreads();
	if (t == 0u)
		v.t1d[b] = skytab_chain(s_d, SKYTAB_THREADS);
	else if (t == 64u)
		v.t1e[b] = skytab_chain(s_e, SKYTAB_THREADS);
	else if (t == 128u)
		v.c1[b] = skytab_chain_u(s_c, SKYTAB_THREADS);
	__syncthreads();
	const double xd = s_d[t], xe = s_e[t];
	for (uint32_t i = 0; i < SKYTAB_ITEMS; i++)
		if (base + i < v.n)
			v.D[base + i] = xd + pd[i], v.E[base + i] = xe + pe[i];
}
// ---- k_skytab_scan_super: a workgroup per super-block: its blocks' totals staged in LDS, chained by three lanes, written back as
// the blocks' bases; entries past the last block are 0 and leave the chain as it is ----
template <int LAST>
__global__ void __launch_bounds__(SKYTAB_THREADS) k_skytab_scan_super(const SkyTabView v)
{
	__shared__ double s_d[SKYTAB_B], s_e[SKYTAB_B];
	__shared__ uint32_t s_c[SKYTAB_B];
	const uint32_t t = threadIdx.x, c = blockIdx.x, first = c * SKYTAB_B;
	for (uint32_t j = t; j < SKYTAB_B; j += SKYTAB_THREADS)
	{
		const bool in = first + j < v.nb1;
		s_d[j] = in ? v.t1d[first + j] : 0.0, s_e[j] = in ? v.t1e[first + j] : 0.0, s_c[j] = in ? v.c1[first + j] : 0u;
	}
	__syncthreads();
	if (t == 0u)
		v.t2d[c] = skytab_chain(s_d, SKYTAB_B);
	else if (t == 64u)
		v.t2e[c] = skytab_chain(s_e, SKYTAB_B);
	else if (t == 128u)
		v.c2[c] = skytab_chain_u(s_c, SKYTAB_B);
	__syncthreads();
	for (uint32_t j = t; j < SKYTAB_B; j += SKYTAB_THREADS)
		if (first + j < v.nb1)
			v.t1d[first + j] = s_d[j], v.t1e[first + j] = s_e[j], v.c1[first + j] = s_c[j];
}
// ---- k_skytab_scan_top: one workgroup, three lanes: the chain over the at most 2048 super-blocks, and the record's counts ----
template <int LAST>
__global__ void __launch_bounds__(SKYTAB_THREADS) k_skytab_scan_top(const SkyTabView v)
{
	const uint32_t t = threadIdx.x;
	if (t == 0u)
		skytab_chain(v.t2d, v.nb2);
	else if (t == 64u)
		skytab_chain(v.t2e, v.nb2);
	else if (t == 128u)
	{
		const uint32_t heavy = skytab_chain_u(v.c2, v.nb2);
		v.rec->heavy = heavy, v.rec->light = v.n - heavy;
	}
}
// ---- k_skytab_scan_apply, k_skytab_assign: a thread per texel ----
template <int LAST>
__global__ void __launch_bounds__(BLOCK) k_skytab_scan_apply(const SkyTabView v)
{
	const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
	if (k < v.n)
		skytab_apply_item(v, k);
}
template <int LAST>
__global__ void __launch_bounds__(BLOCK) k_skytab_assign(const SkyTabView v)
{
	const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
	if (k < v.n)
		skytab_assign_item(v, k);
}

static dim3 sky_grid(size_t items, uint32_t per) { return dim3((uint32_t)((items + per - 1u) / per)); }
void launch_skyhdr_planes(const SkyHdrView &v, stream_t s) { hipLaunchKernelGGL(k_skyhdr_planes<0>, sky_grid((size_t)v.H * 4u, 64u), dim3(64), 0, (hipStream_t)s, v); }
void launch_skyhdr_texels(const SkyHdrView &v, stream_t s) { hipLaunchKernelGGL(k_skyhdr_texels<0>, sky_grid((size_t)v.W * v.H, BLOCK), dim3(BLOCK), 0, (hipStream_t)s, v); }
void launch_skytab_weights(const SkyTabView &v, stream_t s) { hipLaunchKernelGGL(k_skytab_weights<0>, dim3(v.nb1), dim3(SKYTAB_THREADS), 0, (hipStream_t)s, v); }
void launch_skytab_total(const SkyTabView &v, stream_t s) { hipLaunchKernelGGL(k_skytab_total<0>, dim3(1), dim3(SKYTAB_THREADS), 0, (hipStream_t)s, v); }
void launch_skytab_scan_block(const SkyTabView &v, stream_t s) { hipLaunchKernelGGL(k_skytab_scan_block<0>, dim3(v.nb1), dim3(SKYTAB_THREADS), 0, (hipStream_t)s, v); }
void launch_skytab_scan_super(const SkyTabView &v, stream_t s) { hipLaunchKernelGGL(k_skytab_scan_super<0>, dim3(v.nb2), dim3(SKYTAB_THREADS), 0, (hipStream_t)s, v); }
void launch_skytab_scan_top(const SkyTabView &v, stream_t s) { hipLaunchKernelGGL(k_skytab_scan_top<0>, dim3(1), dim3(SKYTAB_THREADS), 0, (hipStream_t)s, v); }
void launch_skytab_scan_apply(const SkyTabView &v, stream_t s) { hipLaunchKernelGGL(k_skytab_scan_apply<0>, sky_grid(v.n, BLOCK), dim3(BLOCK), 0, (hipStream_t)s, v); }
void launch_skytab_assign(const SkyTabView &v, stream_t s) { hipLaunchKernelGGL(k_skytab_assign<0>, sky_grid(v.n, BLOCK), dim3(BLOCK), 0, (hipStream_t)s, v); }

#else // the emulation: the same items in the same shapes, serially

#define SKY_EMU_LAUNCHER(name, view, body)   \
	void name(const view &v, stream_t s)     \
	{                                        \
		EMU_DEFER(s, name(v, s));            \
		body(v);                             \
	}
SKY_EMU_LAUNCHER(launch_skyhdr_planes, SkyHdrView, skyhdr_host_planes)
SKY_EMU_LAUNCHER(launch_skyhdr_texels, SkyHdrView, skyhdr_host_texels)
SKY_EMU_LAUNCHER(launch_skytab_weights, SkyTabView, skytab_host_weights)
SKY_EMU_LAUNCHER(launch_skytab_total, SkyTabView, skytab_host_total)
SKY_EMU_LAUNCHER(launch_skytab_scan_block, SkyTabView, skytab_host_scan_block)
SKY_EMU_LAUNCHER(launch_skytab_scan_super, SkyTabView, skytab_host_scan_super)
SKY_EMU_LAUNCHER(launch_skytab_scan_top, SkyTabView, skytab_host_scan_top)
SKY_EMU_LAUNCHER(launch_skytab_scan_apply, SkyTabView, skytab_host_scan_apply)
SKY_EMU_LAUNCHER(launch_skytab_assign, SkyTabView, skytab_host_assign)
#undef SKY_EMU_LAUNCHER
#endif
#endif // SKY_LOAD_LAUNCHERS
