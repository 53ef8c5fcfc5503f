// texture_decode.h — image textures decoded on the device: baseline JPEG -> level 0 of a texture's slot in the flat texel table, and
// the reference's five-level mip chain behind it (rfwhip_set_texture_sources, include/rfwhip.h).
//
// The file has two parts.  PART 1 (types, the host's marker walk, the work items, and the items run serially over plain host arrays)
// is included by kernels.h at file scope and needs nothing but this file: tests/texdec_san_main.cpp includes it alone.  PART 2 (the
// HIP kernels and their launchers, or the emulation's launchers) is included by kernels.hip inside namespace rtk with
// TEXTURE_DECODE_LAUNCHERS defined.  The kernels and the emulation run the same items.
//
// WALK  td_walk: SOF0 / SOF1 with 8-bit samples, 1 component or 3 in one interleaved scan, luma 1x1 / 2x1 / 2x2 over chroma 1x1, 8-bit
//   quantisation tables, up to four DC and four AC Huffman tables, DRI or none.  It yields the geometry, the tables in canonical
//   form (T.81 F.2.2.3: mincode / maxcode / valptr) and the byte range of every restart interval, found by one scan for FF Dn.
// BLOCKS  MCU m (raster order) holds bpm = hs vs + (components - 1) blocks: the luma blocks row by row, then Cb, Cr; block b = m bpm + k
//   has 64 int16 coefficients in zigzag order — the order of the encoder's coefficients (display_jpeg.h).
// ENTROPY  td_entropy_interval: one restart interval, predictors 0 at its start, bytes unstuffed as they are read.  Every read is
//   bounded by the interval's end (zero bits and TD_ERR_TRUNCATED behind it), every coefficient index by 63 (TD_ERR_RUN, the block
//   stops), a code without a match in 16 bits stops the interval (TD_ERR_NOCODE).
// IDCT  the 13-bit-constant "slow integer" inverse DCT in wrapping 32-bit arithmetic: td_idct_col (dequantise, pass 1, descale by 11),
//   td_idct_row (pass 2, descale by 18, + 128, clamp).  One 8-bit plane per component, whole blocks wide and high.
// COLOUR  td_texel: "fancy" triangle upsampling of the chroma at its own size (edges replicated; a chroma plane at most two columns
//   wide is replicated instead), integer YCbCr -> RGB with 16 fractional bits, then the modifiers (td_modify): flip, linearise.
// MIPS  td_mip_texel: the truncated quarter of the aligned 2 x 2 quad per colour, the minimum of the four alphas (the filter of the
//   reference's construct_mipmaps, texture.cpp:163-209); level i is (w >> i) x (h >> i), the levels back to back.
#ifndef RFWHIP_TEXTURE_DECODE_H
#define RFWHIP_TEXTURE_DECODE_H

#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#ifndef RT_FN
#define RT_FN inline
#endif

namespace rtk
{

constexpr int TD_OK = 0, TD_INVALID = 1, TD_UNSUPPORTED = 5; // = RFWHIP_OK, RFWHIP_ERR_INVALID_ARGUMENT, RFWHIP_ERR_UNSUPPORTED
constexpr uint32_t TD_MIP_LEVELS = 5u;						  // MIPLEVELCOUNT
// modifiers (= RFWHIP_TEXSRC_*)
constexpr uint32_t TD_FLIP_ROWS = 1u, TD_LINEARIZE_REFERENCE = 2u, TD_LINEARIZE_SRGB = 4u;
// error flags of a decode (= RFWHIP_TEXDEC_ERR_*)
constexpr uint32_t TD_ERR_TRUNCATED = 1u, TD_ERR_RUN = 2u, TD_ERR_NOCODE = 4u, TD_ERR_MARKER = 8u;
// the path the entropy decoding took (TexRecord::path)
constexpr uint32_t TD_PATH_NONE = 0u, TD_PATH_HOST = 1u, TD_PATH_DEVICE = 2u;

// one Huffman table in canonical form: a code of length l (1 .. 16) is a symbol when code <= maxcode[l] (-1: no code of that length),
// the symbol is vals[valptr[l] + code - mincode[l]]
struct TdHuff
{
	int32_t maxcode[17], mincode[17], valptr[17];
	uint8_t vals[256];
};
// q[table][zigzag position]; izz[natural index] = its zigzag position
struct TdTables
{
	TdHuff dc[4], ac[4];
	uint16_t q[4][64];
	uint8_t izz[64];
};
static_assert(sizeof(TdTables) % 4 == 0, "k_texdec_entropy stages the tables word by word");
// what k_texdec_finish leaves (= rfwhip_texture_decode_record)
struct TexRecord
{
	uint32_t width, height, blocks, intervals, errors, alpha_zero, path, pad;
};
// One decode.  stream: the encoded bytes; ranges: per interval the first byte of its entropy data and the byte behind its last;
// coef: blocks x 64; flags: a word per interval; planes: component c at plane_off[c], pw[c] bytes per row; out: the texture's slot,
// level 0 first; src: W x H RGBA8 in file order (k_texdec_rgba, instead of a stream); lin: the 256-entry table of TD_LINEARIZE_SRGB;
// alpha: a partial count per workgroup of k_tex_mips (tiles of them); ri: MCUs per interval (= mcus without DRI)
struct TexdecView
{
	const uint8_t *stream;
	const uint32_t *ranges;
	const TdTables *tab;
	int16_t *coef;
	uint32_t *flags;
	uint8_t *planes;
	uint32_t *out;
	const uint32_t *src;
	const uint8_t *lin;
	TexRecord *rec;
	uint32_t *alpha;
	uint32_t W, H, ncomp, hs, vs, bpm, ri, mcus_x, mcus, blocks, intervals, mods, path, tiles;
	uint32_t plane_off[3], pw[3];
	uint8_t tq[3], td[3], ta[3], pad_[3];
};

RT_FN uint32_t td_level_texels(uint32_t w, uint32_t h, uint32_t level) { return (w >> level) * (h >> level); }
RT_FN uint32_t td_chain_texels(uint32_t w, uint32_t h)
{
	uint32_t n = 0u;
	for (uint32_t i = 0; i < TD_MIP_LEVELS; i++)
		n += td_level_texels(w, h, i);
	return n;
}
RT_FN uint32_t td_tiles(uint32_t w, uint32_t h) { return ((w + 15u) / 16u) * ((h + 15u) / 16u); }

// ---- the host's marker walk ---------------------------------------------------------------------------------------------------
struct TdInfo
{
	uint32_t W = 0, H = 0, ncomp = 0, hs = 1, vs = 1, ri = 0, mcus_x = 0, mcus_y = 0, mcus = 0, bpm = 0, blocks = 0, intervals = 0;
	uint8_t tq[3] = {}, td[3] = {}, ta[3] = {};
	TdTables tab;
	std::vector<uint32_t> ranges; // 2 per interval
	char msg[192] = {};
};
inline int td_fail(TdInfo &o, int code, const char *fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(o.msg, sizeof(o.msg), fmt, ap);
	va_end(ap);
	return code;
}
inline const uint8_t *td_zigzag()
{
	static const uint8_t zz[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
								   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
	return zz;
}
// a DHT table's 16 counts and its symbols -> the canonical form; false when the counts claim more codes than their lengths hold
inline bool td_canonical(const uint8_t counts[16], const uint8_t *vals, uint32_t total, TdHuff &h)
{
	memset(&h, 0, sizeof(h));
	uint32_t code = 0u, k = 0u;
	for (uint32_t l = 1; l <= 16u; l++)
	{
		h.valptr[l] = (int32_t)k, h.mincode[l] = (int32_t)code;
		code += counts[l - 1u], k += counts[l - 1u];
		h.maxcode[l] = counts[l - 1u] ? (int32_t)code - 1 : -1;
		if (code > (1u << l))
			return false;
		code <<= 1;
	}
	h.maxcode[0] = -1;
	memcpy(h.vals, vals, total);
	return true;
}
inline int td_walk(const uint8_t *d, size_t n, TdInfo &o)
{
	const auto be16 = [&](size_t p) { return ((uint32_t)d[p] << 8) | d[p + 1]; };
	if (!d || n < 4 || d[0] != 0xFF || d[1] != 0xD8)
		return td_fail(o, TD_INVALID, "not a JPEG stream (no SOI)");
	if (n > 0xFFFFFFF0ull)
		return td_fail(o, TD_UNSUPPORTED, "a stream of %zu bytes (32-bit offsets)", n);
	memset(&o.tab, 0, sizeof(o.tab));
	for (uint32_t i = 0; i < 64u; i++)
		o.tab.izz[td_zigzag()[i]] = (uint8_t)i;
	uint32_t have_q = 0u, have_dc = 0u, have_ac = 0u, comp_id[3] = {0, 0, 0};
	bool sof = false;
	int adobe = -1; // APP14's colour transform: 0 = none (RGB, CMYK), 1 = YCbCr, 2 = YCCK
	size_t p = 2;
	for (;;)
	{
		if (p + 2 > n)
			return td_fail(o, TD_INVALID, "truncated in front of the scan (byte %zu)", p);
		if (d[p] != 0xFF)
			return td_fail(o, TD_INVALID, "no marker at byte %zu", p);
		while (p < n && d[p] == 0xFF) // (fill bytes)
			p++;
		if (p >= n)
			return td_fail(o, TD_INVALID, "truncated in front of the scan (byte %zu)", p);
		const uint32_t m = d[p++];
		if (m == 0x01 || (m >= 0xD0 && m <= 0xD8))
			continue;
		if (m == 0xD9)
			return td_fail(o, TD_INVALID, "EOI in front of the scan");
		if (p + 2 > n)
			return td_fail(o, TD_INVALID, "truncated inside the header of segment FF%02X", m);
		const uint32_t L = be16(p);
		if (L < 2u || p + L > n)
			return td_fail(o, TD_INVALID, "truncated inside segment FF%02X (%u bytes declared, %zu left)", m, L, n - p);
		const uint8_t *b = d + p + 2;
		const uint32_t bl = L - 2u;
		p += L;
		if (m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC && bl >= 6u && !sof) // (any frame header: the size, for rfwhip_image_info)
			o.H = ((uint32_t)b[1] << 8) | b[2], o.W = ((uint32_t)b[3] << 8) | b[4], o.ncomp = b[5];
		if (m == 0xC2)
			return td_fail(o, TD_UNSUPPORTED, "progressive JPEG (SOF2)");
		if (m == 0xC3 || (m >= 0xC5 && m <= 0xC7))
			return td_fail(o, TD_UNSUPPORTED, "lossless or hierarchical JPEG (SOF%u)", m - 0xC0u);
		if ((m >= 0xC9 && m <= 0xCB) || (m >= 0xCC && m <= 0xCF))
			return td_fail(o, TD_UNSUPPORTED, "arithmetic coding (marker FF%02X)", m);
		if (m == 0xC0 || m == 0xC1)
		{
			if (sof)
				return td_fail(o, TD_INVALID, "two frame headers");
			if (bl < 6u)
				return td_fail(o, TD_INVALID, "SOF of %u bytes", bl);
			if (b[0] != 8u)
				return td_fail(o, TD_UNSUPPORTED, "%u-bit sample precision", b[0]);
			o.H = ((uint32_t)b[1] << 8) | b[2], o.W = ((uint32_t)b[3] << 8) | b[4], o.ncomp = b[5];
			if (!o.W || !o.H)
				return td_fail(o, TD_INVALID, "a %u x %u image", o.W, o.H);
			if (o.ncomp != 1u && o.ncomp != 3u)
				return td_fail(o, TD_UNSUPPORTED, "%u components", o.ncomp);
			if (bl < 6u + 3u * o.ncomp)
				return td_fail(o, TD_INVALID, "SOF of %u bytes for %u components", bl, o.ncomp);
			for (uint32_t c = 0; c < o.ncomp; c++)
			{
				comp_id[c] = b[6u + 3u * c], o.tq[c] = b[8u + 3u * c];
				const uint32_t hv = b[7u + 3u * c];
				if (o.tq[c] > 3u)
					return td_fail(o, TD_INVALID, "component %u names quantisation table %u", c, o.tq[c]);
				if (o.ncomp == 1u)
					continue; // (a single component's scan is not interleaved: its factors do not matter)
				if (c == 0u ? (hv != 0x11 && hv != 0x21 && hv != 0x22) : hv != 0x11)
					return td_fail(o, TD_UNSUPPORTED, "sampling factors %u x %u of component %u", hv >> 4, hv & 15u, c);
				if (c == 0u)
					o.hs = hv >> 4, o.vs = hv & 15u;
			}
			sof = true;
		}
		else if (m == 0xDB)
			for (uint32_t q = 0; q < bl;)
			{
				const uint32_t pq = b[q] >> 4, t = b[q] & 15u;
				if (pq)
					return td_fail(o, TD_UNSUPPORTED, "a 16-bit quantisation table");
				if (t > 3u || q + 65u > bl)
					return td_fail(o, TD_INVALID, "DQT: table %u, %u bytes left", t, bl - q);
				for (uint32_t k = 0; k < 64u; k++)
					o.tab.q[t][k] = b[q + 1u + k];
				have_q |= 1u << t, q += 65u;
			}
		else if (m == 0xC4)
			for (uint32_t q = 0; q < bl;)
			{
				if (q + 17u > bl)
					return td_fail(o, TD_INVALID, "DHT: %u bytes left for a table header", bl - q);
				const uint32_t tc = b[q] >> 4, th = b[q] & 15u;
				uint32_t total = 0u;
				for (uint32_t l = 0; l < 16u; l++)
					total += b[q + 1u + l];
				if (tc > 1u || th > 3u)
					return td_fail(o, TD_INVALID, "DHT: class %u, table %u", tc, th);
				if (total > 256u || q + 17u + total > bl)
					return td_fail(o, TD_INVALID, "DHT: the counts name %u symbols, the segment has %u bytes left", total, bl - q - 17u);
				if (!td_canonical(b + q + 1u, b + q + 17u, total, tc ? o.tab.ac[th] : o.tab.dc[th]))
					return td_fail(o, TD_INVALID, "DHT: the counts of table %u.%u do not form a prefix code", tc, th);
				if (!tc)
					for (uint32_t k = 0; k < total; k++)
						if (b[q + 17u + k] > 15u)
							return td_fail(o, TD_INVALID, "DHT: DC category %u", b[q + 17u + k]);
				(tc ? have_ac : have_dc) |= 1u << th, q += 17u + total;
			}
		else if (m == 0xDD)
		{
			if (bl != 2u)
				return td_fail(o, TD_INVALID, "DRI of %u bytes", bl);
			o.ri = ((uint32_t)b[0] << 8) | b[1];
		}
		else if (m == 0xEE && bl >= 12u && !memcmp(b, "Adobe", 5))
			adobe = (int)b[11];
		else if (m == 0xDA)
		{
			if (!sof)
				return td_fail(o, TD_INVALID, "SOS in front of the frame header");
			if (bl < 1u || bl != 4u + 2u * b[0])
				return td_fail(o, TD_INVALID, "SOS of %u bytes", bl);
			if (o.ncomp == 3u && adobe >= 0 && adobe != 1)
				return td_fail(o, TD_UNSUPPORTED, "APP14 declares colour transform %d (RGB or CMYK data)", adobe);
			if (b[0] != o.ncomp)
				return td_fail(o, TD_UNSUPPORTED, "a scan of %u of the %u components (non-interleaved)", b[0], o.ncomp);
			for (uint32_t c = 0; c < o.ncomp; c++)
			{
				if (b[1u + 2u * c] != comp_id[c])
					return td_fail(o, TD_UNSUPPORTED, "the scan's components are not in frame order");
				o.td[c] = b[2u + 2u * c] >> 4, o.ta[c] = b[2u + 2u * c] & 15u;
				if (o.td[c] > 3u || o.ta[c] > 3u || !((have_dc >> o.td[c]) & 1u) || !((have_ac >> o.ta[c]) & 1u))
					return td_fail(o, TD_INVALID, "SOS names Huffman tables %u / %u, which no DHT defined", o.td[c], o.ta[c]);
				if (!((have_q >> o.tq[c]) & 1u))
					return td_fail(o, TD_INVALID, "component %u uses quantisation table %u, which no DQT defined", c, o.tq[c]);
			}
			const uint8_t *t = b + 1u + 2u * o.ncomp;
			if (t[0] != 0u || t[1] != 63u || t[2] != 0u)
				return td_fail(o, TD_UNSUPPORTED, "a scan of coefficients %u .. %u, approximation %02X (progressive)", t[0], t[1], t[2]);
			break;
		}
		// (APPn, COM and everything else with a length: skipped)
	}
	o.mcus_x = (o.W + 8u * o.hs - 1u) / (8u * o.hs), o.mcus_y = (o.H + 8u * o.vs - 1u) / (8u * o.vs);
	o.mcus = o.mcus_x * o.mcus_y, o.bpm = o.ncomp == 1u ? 1u : o.hs * o.vs + 2u;
	if ((uint64_t)o.mcus * o.bpm * 64u > 0x7FFFFFFFull)
		return td_fail(o, TD_UNSUPPORTED, "a %u x %u image (more than 2^31 coefficients)", o.W, o.H);
	o.blocks = o.mcus * o.bpm, o.intervals = o.ri ? (o.mcus + o.ri - 1u) / o.ri : 1u;
	// the scan: one pass for FF xx
	size_t begin = p;
	uint32_t expect = 0u;
	o.ranges.clear();
	for (;;)
	{
		const uint8_t *f = p < n ? (const uint8_t *)memchr(d + p, 0xFF, n - p) : nullptr;
		if (!f)
			return td_fail(o, TD_INVALID, "the scan ends without EOI (truncated)");
		const size_t q = (size_t)(f - d);
		size_t r = q + 1;
		if (r < n && d[r] == 0u) // a stuffed byte
		{
			p = r + 1;
			continue;
		}
		while (r < n && d[r] == 0xFF)
			r++;
		if (r >= n)
			return td_fail(o, TD_INVALID, "the scan ends without EOI (truncated)");
		const uint32_t m = d[r];
		if (m >= 0xD0 && m <= 0xD7)
		{
			if (!o.ri)
				return td_fail(o, TD_INVALID, "RST%u without DRI", m - 0xD0u);
			if (m - 0xD0u != expect)
				return td_fail(o, TD_INVALID, "RST%u where RST%u is due (out of sequence)", m - 0xD0u, expect);
			if (o.ranges.size() / 2u + 1u >= o.intervals)
				return td_fail(o, TD_INVALID, "more than the %u restart intervals of %u MCUs", o.intervals, o.mcus);
			o.ranges.push_back((uint32_t)begin), o.ranges.push_back((uint32_t)q);
			begin = p = r + 1, expect = (expect + 1u) & 7u;
			continue;
		}
		if (m == 0xD9)
		{
			o.ranges.push_back((uint32_t)begin), o.ranges.push_back((uint32_t)q);
			break;
		}
		if (m == 0xDA || m == 0xC4 || m == 0xDB || m == 0xDC || m == 0xDD)
			return td_fail(o, TD_UNSUPPORTED, "marker FF%02X behind the first scan (more than one scan)", m);
		return td_fail(o, TD_INVALID, "marker FF%02X inside the scan", m);
	}
	if (o.ranges.size() / 2u != o.intervals)
		return td_fail(o, TD_INVALID, "%zu restart intervals, %u are due", o.ranges.size() / 2u, o.intervals);
	return TD_OK;
}
// the view's geometry from the walk (the pointers stay as they are); planes_bytes: what v.planes needs
inline void td_view_geometry(const TdInfo &o, TexdecView &v, size_t *planes_bytes)
{
	v.W = o.W, v.H = o.H, v.ncomp = o.ncomp, v.hs = o.hs, v.vs = o.vs, v.bpm = o.bpm, v.ri = o.ri ? o.ri : o.mcus;
	v.mcus_x = o.mcus_x, v.mcus = o.mcus, v.blocks = o.blocks, v.intervals = o.intervals;
	size_t off = 0;
	for (uint32_t c = 0; c < 3u; c++)
	{
		v.tq[c] = o.tq[c], v.td[c] = o.td[c], v.ta[c] = o.ta[c];
		v.pw[c] = c < o.ncomp ? o.mcus_x * 8u * (c ? 1u : o.hs) : 0u;
		v.plane_off[c] = (uint32_t)off;
		off += c < o.ncomp ? (size_t)v.pw[c] * o.mcus_y * 8u * (c ? 1u : o.vs) : 0u;
	}
	if (planes_bytes)
		*planes_bytes = off;
}
// the table of TD_LINEARIZE_SRGB: the sRGB EOTF in double, rounded to nearest
inline void td_srgb_table(uint8_t out[256])
{
	for (int i = 0; i < 256; i++)
	{
		const double c = i / 255.0, l = c <= 0.04045 ? c / 12.92 : pow((c + 0.055) / 1.055, 2.4);
		out[i] = (uint8_t)(int)(l * 255.0 + 0.5);
	}
}

// ---- entropy decoding ---------------------------------------------------------------------------------------------------------
struct TdBits
{
	const uint8_t *p;
	uint32_t pos, end; // the next byte, the byte behind the interval
	uint32_t acc;	   // `have` bits at its high end, of which the last `pad` are zeros supplied past the end
	uint32_t have, pad, err;
};
RT_FN void td_fill(TdBits &b) // -> have >= 25
{
	while (b.have <= 24u)
	{
		uint32_t byte = 0u;
		if (b.pos < b.end)
		{
			byte = b.p[b.pos++];
			if (byte == 0xFFu)
			{
				if (b.pos < b.end && b.p[b.pos] == 0u)
					b.pos++;
				else
					b.err |= TD_ERR_MARKER;
			}
		}
		else
			b.pad += 8u;
		b.acc |= byte << (24u - b.have), b.have += 8u;
	}
}
RT_FN void td_skip(TdBits &b, uint32_t n) // n <= 16 <= have
{
	b.acc <<= n, b.have -= n;
	if (b.have < b.pad)
		b.err |= TD_ERR_TRUNCATED, b.pad = b.have;
}
// T.81 F.2.2.3 (DECODE): the symbol, or -1 when no code of 1 .. 16 bits matches
RT_FN int td_symbol(TdBits &b, const TdHuff &h)
{
	td_fill(b);
	const uint32_t look = b.acc >> 16;
	for (uint32_t l = 1; l <= 16u; l++)
	{
		const int32_t code = (int32_t)(look >> (16u - l));
		if (code <= h.maxcode[l])
		{
			td_skip(b, l);
			return (int)h.vals[(uint32_t)(h.valptr[l] + code - h.mincode[l]) & 255u];
		}
	}
	b.err |= TD_ERR_NOCODE;
	return -1;
}
// T.81 F.2.2.1 / F.2.2.4 (RECEIVE, EXTEND): s = 1 .. 15
RT_FN int td_receive(TdBits &b, uint32_t s)
{
	td_fill(b);
	const int v = (int)(b.acc >> (32u - s));
	td_skip(b, s);
	return v < (1 << (s - 1u)) ? v - (1 << s) + 1 : v;
}
// interval i of the view: its blocks' non-zero coefficients into v.coef (zeroed before) -> the error flags
RT_FN uint32_t td_entropy_interval(const TexdecView &v, const TdTables &tab, uint32_t i)
{
	const uint32_t m0 = i * v.ri, n_mcu = v.mcus - m0 < v.ri ? v.mcus - m0 : v.ri, luma = v.bpm - (v.ncomp - 1u);
	TdBits b;
	b.p = v.stream, b.pos = v.ranges[2u * i], b.end = v.ranges[2u * i + 1u], b.acc = 0u, b.have = 0u, b.pad = 0u, b.err = 0u;
	uint32_t pred[3] = {0u, 0u, 0u};
	for (uint32_t m = 0; m < n_mcu; m++)
		for (uint32_t k = 0; k < v.bpm; k++)
		{
			const uint32_t c = k < luma ? 0u : 1u + k - luma;
			int16_t *z = v.coef + ((size_t)(m0 + m) * v.bpm + k) * 64u;
			const int sd = td_symbol(b, tab.dc[v.td[c] & 3u]);
			if (sd < 0)
				return b.err;
			if (sd & 15)
				pred[c] += (uint32_t)td_receive(b, (uint32_t)sd & 15u);
			z[0] = (int16_t)pred[c];
			for (uint32_t kk = 1u; kk < 64u;)
			{
				const int rs = td_symbol(b, tab.ac[v.ta[c] & 3u]);
				if (rs < 0)
					return b.err;
				const uint32_t r = (uint32_t)rs >> 4, s = (uint32_t)rs & 15u;
				if (!s)
				{
					if (r != 15u)
						break; // EOB
					kk += 16u; // ZRL
					continue;
				}
				kk += r;
				if (kk > 63u)
				{
					b.err |= TD_ERR_RUN;
					break;
				}
				z[kk++] = (int16_t)td_receive(b, s);
			}
		}
	return b.err;
}

// ---- inverse DCT --------------------------------------------------------------------------------------------------------------
RT_FN int32_t td_descale(uint32_t x, uint32_t n) { return (int32_t)(x + (1u << (n - 1u))) >> n; }
// the 1-D transform of eight inputs: the eight sums before the descale (wrapping)
RT_FN void td_idct_1d(const uint32_t in[8], uint32_t o[8])
{
	uint32_t z1 = (in[2] + in[6]) * 4433u;
	const uint32_t e2 = z1 - in[6] * 15137u, e3 = z1 + in[2] * 6270u;
	const uint32_t e0 = (in[0] + in[4]) << 13, e1 = (in[0] - in[4]) << 13;
	const uint32_t t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
	uint32_t t0 = in[7], t1 = in[5], t2 = in[3], t3 = in[1];
	z1 = t0 + t3;
	uint32_t z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
	const uint32_t z5 = (z3 + z4) * 9633u;
	t0 *= 2446u, t1 *= 16819u, t2 *= 25172u, t3 *= 12299u;
	z1 *= 0u - 7373u, z2 *= 0u - 20995u, z3 = z3 * (0u - 16069u) + z5, z4 = z4 * (0u - 3196u) + z5;
	t0 += z1 + z3, t1 += z2 + z4, t2 += z2 + z3, t3 += z1 + z4;
	o[0] = t10 + t3, o[7] = t10 - t3, o[1] = t11 + t2, o[6] = t11 - t2;
	o[2] = t12 + t1, o[5] = t12 - t1, o[3] = t13 + t0, o[4] = t13 - t0;
}
// pass 1, column j of a block: its coefficients z[0 .. 63] (zigzag), the table q (zigzag) -> ws[u] for the rows u
RT_FN void td_idct_col(const int16_t *z, const uint16_t *q, const uint8_t *izz, uint32_t j, int32_t ws[8])
{
	uint32_t in[8], o[8], ac = 0u;
	for (uint32_t u = 0; u < 8u; u++)
	{
		const uint32_t k = izz[u * 8u + j] & 63u;
		in[u] = (uint32_t)(int32_t)z[k] * (uint32_t)q[k];
		ac |= u ? in[u] : 0u;
	}
	if (!ac) // (exact: (x << 13 + 1024) >> 11 = x << 2)
	{
		for (uint32_t u = 0; u < 8u; u++)
			ws[u] = (int32_t)(in[0] << 2);
		return;
	}
	td_idct_1d(in, o);
	for (uint32_t u = 0; u < 8u; u++)
		ws[u] = td_descale(o[u], 11u);
}
// pass 2, one row of the workspace -> eight samples
RT_FN void td_idct_row(const int32_t ws[8], uint8_t px[8])
{
	uint32_t in[8], o[8];
	for (uint32_t x = 0; x < 8u; x++)
		in[x] = (uint32_t)ws[x];
	td_idct_1d(in, o);
	for (uint32_t x = 0; x < 8u; x++)
	{
		const int32_t s = td_descale(o[x], 18u) + 128;
		px[x] = (uint8_t)(s < 0 ? 0 : s > 255 ? 255 : s);
	}
}
// where block g lies: its component and the byte of its top-left sample in v.planes
RT_FN uint32_t td_block_place(const TexdecView &v, uint32_t g, size_t *at)
{
	const uint32_t m = g / v.bpm, k = g - m * v.bpm, my = m / v.mcus_x, mx = m - my * v.mcus_x, luma = v.bpm - (v.ncomp - 1u);
	const uint32_t c = k < luma ? 0u : 1u + k - luma;
	const uint32_t bx = c ? mx : mx * v.hs + k % v.hs, by = c ? my : my * v.vs + k / v.hs;
	*at = (size_t)v.plane_off[c] + (size_t)by * 8u * v.pw[c] + (size_t)bx * 8u;
	return c;
}

// ---- upsampling, colour, modifiers --------------------------------------------------------------------------------------------
// chroma sample of component c at pixel (x, y): the component is cw x ch, its plane has pw[c] bytes per row
RT_FN int td_chroma(const TexdecView &v, uint32_t c, uint32_t x, uint32_t y)
{
	const uint8_t *pl = v.planes + v.plane_off[c];
	const uint32_t pw = v.pw[c];
	if (v.hs == 1u)
		return (int)pl[(size_t)y * pw + x];
	const uint32_t cw = (v.W + 1u) >> 1, cx = x >> 1;
	const uint32_t xn = (x & 1u) ? (cx + 1u < cw ? cx + 1u : cx) : (cx ? cx - 1u : 0u); // the neighbour column
	if (v.vs == 1u) // 2 x 1
	{
		const uint8_t *row = pl + (size_t)y * pw;
		if (cw <= 2u)
			return (int)row[cx];
		return (3 * (int)row[cx] + (int)row[xn] + ((x & 1u) ? 2 : 1)) >> 2;
	}
	const uint32_t ch = (v.H + 1u) >> 1, cy = y >> 1;
	if (cw <= 2u)
		return (int)pl[(size_t)cy * pw + cx];
	const uint32_t yn = (y & 1u) ? (cy + 1u < ch ? cy + 1u : cy) : (cy ? cy - 1u : 0u);
	const uint8_t *near = pl + (size_t)cy * pw, *far = pl + (size_t)yn * pw;
	const int a = 3 * (int)near[cx] + (int)far[cx], n = 3 * (int)near[xn] + (int)far[xn];
	return (3 * a + n + ((x & 1u) ? 7 : 8)) >> 4;
}
RT_FN uint32_t td_clamp8(int x) { return (uint32_t)(x < 0 ? 0 : x > 255 ? 255 : x); }
// pixel (x, y) of the image, alpha 255
RT_FN uint32_t td_pixel(const TexdecView &v, uint32_t x, uint32_t y)
{
	const int Y = (int)v.planes[(size_t)v.plane_off[0] + (size_t)y * v.pw[0] + x];
	if (v.ncomp == 1u)
		return (uint32_t)Y * 0x010101u | 0xFF000000u;
	const int cb = td_chroma(v, 1u, x, y) - 128, cr = td_chroma(v, 2u, x, y) - 128;
	const uint32_t R = td_clamp8(Y + ((91881 * cr + 32768) >> 16)), B = td_clamp8(Y + ((116130 * cb + 32768) >> 16));
	const uint32_t G = td_clamp8(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
	return R | (G << 8) | (B << 16) | 0xFF000000u;
}
// linearisation of the three colour bytes (the alpha stays)
RT_FN uint32_t td_modify(uint32_t t, uint32_t mods, const uint8_t *lin)
{
	uint32_t r = t & 255u, g = (t >> 8) & 255u, b = (t >> 16) & 255u;
	if (mods & TD_LINEARIZE_REFERENCE)
		r = (r * r) >> 8, g = (g * g) >> 8, b = (b * b) >> 8;
	else if (mods & TD_LINEARIZE_SRGB)
		r = lin[r], g = lin[g], b = lin[b];
	return r | (g << 8) | (b << 16) | (t & 0xFF000000u);
}
// texel (x, ty) of level 0, from the decoded planes or from the RGBA8 source
RT_FN uint32_t td_texel(const TexdecView &v, uint32_t x, uint32_t ty)
{
	const uint32_t y = (v.mods & TD_FLIP_ROWS) ? v.H - 1u - ty : ty;
	return td_modify(v.src ? v.src[(size_t)y * v.W + x] : td_pixel(v, x, y), v.mods, v.lin);
}

// ---- mips ---------------------------------------------------------------------------------------------------------------------
RT_FN uint32_t td_mip_texel(uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
	uint32_t o = 0u;
	for (uint32_t sh = 0; sh < 24u; sh += 8u)
		o |= ((((a >> sh) & 255u) + ((b >> sh) & 255u) + ((c >> sh) & 255u) + ((d >> sh) & 255u)) >> 2) << sh;
	const uint32_t a0 = a >> 24, a1 = b >> 24, a2 = c >> 24, a3 = d >> 24;
	const uint32_t lo = a0 < a1 ? a0 : a1, hi = a2 < a3 ? a2 : a3;
	return o | ((lo < hi ? lo : hi) << 24);
}
// the record behind a decode: the intervals' flags ORed, the tiles' alpha counts added
RT_FN void td_record(const TexdecView &v, uint32_t errors, uint32_t alpha_zero)
{
	TexRecord r;
	r.width = v.W, r.height = v.H, r.blocks = v.blocks, r.intervals = v.intervals, r.errors = errors, r.alpha_zero = alpha_zero;
	r.path = v.path, r.pad = 0u;
	*v.rec = r;
}

// ---- the items run serially over host arrays (the host path of the entropy decoding, the emulation, the stand-alone program) ----
inline void td_host_zero(const TexdecView &v) { memset(v.coef, 0, (size_t)v.blocks * 128u); }
inline void td_host_entropy(const TexdecView &v)
{
	for (uint32_t i = 0; i < v.intervals; i++)
		v.flags[i] = td_entropy_interval(v, *v.tab, i);
}
inline void td_host_idct(const TexdecView &v)
{
	for (uint32_t g = 0; g < v.blocks; g++)
	{
		size_t at;
		const uint32_t c = td_block_place(v, g, &at);
		int32_t ws[8][8], col[8];
		for (uint32_t j = 0; j < 8u; j++)
		{
			td_idct_col(v.coef + (size_t)g * 64u, v.tab->q[v.tq[c] & 3u], v.tab->izz, j, col);
			for (uint32_t u = 0; u < 8u; u++)
				ws[u][j] = col[u];
		}
		for (uint32_t j = 0; j < 8u; j++)
			td_idct_row(ws[j], v.planes + at + (size_t)j * v.pw[c]);
	}
}
inline void td_host_color(const TexdecView &v)
{
	for (uint32_t ty = 0; ty < v.H; ty++)
		for (uint32_t x = 0; x < v.W; x++)
			v.out[(size_t)ty * v.W + x] = td_texel(v, x, ty);
}
// levels 1 .. 4 behind level 0 at v.out, and the tiles' counts of level-0 texels with alpha 0
inline void td_host_mips(const TexdecView &v)
{
	const uint32_t tx = (v.W + 15u) / 16u;
	for (uint32_t t = 0; t < v.tiles; t++)
	{
		uint32_t n = 0u;
		for (uint32_t y = t / tx * 16u; y < t / tx * 16u + 16u && y < v.H; y++)
			for (uint32_t x = t % tx * 16u; x < t % tx * 16u + 16u && x < v.W; x++)
				n += (v.out[(size_t)y * v.W + x] >> 24) == 0u;
		v.alpha[t] = n;
	}
	const uint32_t *src = v.out;
	uint32_t *dst = v.out + (size_t)v.W * v.H;
	for (uint32_t l = 1; l < TD_MIP_LEVELS; l++)
	{
		const uint32_t pw = v.W >> (l - 1u), w = v.W >> l, h = v.H >> l;
		for (uint32_t y = 0; y < h; y++)
			for (uint32_t x = 0; x < w; x++)
			{
				const uint32_t *s = src + (size_t)(2u * y) * pw + 2u * x;
				dst[(size_t)y * w + x] = td_mip_texel(s[0], s[1], s[pw], s[pw + 1u]);
			}
		src = dst, dst += (size_t)w * h;
	}
}
inline void td_host_finish(const TexdecView &v)
{
	uint32_t e = 0u, a = 0u;
	for (uint32_t i = 0; v.flags && i < v.intervals; i++)
		e |= v.flags[i];
	for (uint32_t t = 0; t < v.tiles; t++)
		a += v.alpha[t];
	td_record(v, e, a);
}
// PNG's filters undone (rfwhip_png_unfilter): `rows` scanlines of a filter byte and `row_bytes` filtered bytes each -> the rows
// alone in `out`; bpp = bytes per whole pixel.  TD_INVALID for a filter type above 4.
inline int td_png_unfilter(const uint8_t *in, size_t rows, size_t row_bytes, size_t bpp, uint8_t *out)
{
	for (size_t y = 0; y < rows; y++)
	{
		const uint8_t *src = in + y * (row_bytes + 1u);
		uint8_t *cur = out + y * row_bytes;
		const uint8_t *prev = y ? cur - row_bytes : nullptr;
		const int type = src[0];
		if (type > 4)
			return TD_INVALID;
		for (size_t i = 0; i < row_bytes; i++)
		{
			const int a = i >= bpp ? cur[i - bpp] : 0, b = prev ? prev[i] : 0, c = (prev && i >= bpp) ? prev[i - bpp] : 0;
			int p = 0;
			if (type == 1)
				p = a;
			else if (type == 2)
				p = b;
			else if (type == 3)
				p = (a + b) >> 1;
			else if (type == 4)
			{
				const int e = a + b - c, pa = e > a ? e - a : a - e, pb = e > b ? e - b : b - e, pc = e > c ? e - c : c - e;
				p = (pa <= pb && pa <= pc) ? a : pb <= pc ? b : c;
			}
			cur[i] = (uint8_t)(src[1u + i] + p);
		}
	}
	return TD_OK;
}

} // namespace rtk
#endif // RFWHIP_TEXTURE_DECODE_H

// =================================================================================================================================
// PART 2: the kernels and the launchers (kernels.hip, inside namespace rtk)
// =================================================================================================================================
#if defined(TEXTURE_DECODE_LAUNCHERS) && !defined(RFWHIP_TEXTURE_DECODE_LAUNCHERS_DONE)
#define RFWHIP_TEXTURE_DECODE_LAUNCHERS_DONE
#if defined(RT_DEVICE_BUILD)

// ---- k_texdec_zero: the coefficient buffer, 16 bytes a thread (a block is 128 bytes) ----
__global__ void __launch_bounds__(BLOCK) k_texdec_zero(const TexdecView v)
{
	const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
	if (i < (size_t)v.blocks * 8u)
		((uint4 *)v.coef)[i] = make_uint4(0u, 0u, 0u, 0u);
}

// ---- k_texdec_entropy: one wave per workgroup, one lane per restart interval; the tables are staged in LDS word by word.  A lane
// walks its interval's bytes serially (the code lengths are data: there is nothing to share between lanes) and writes only the
// blocks of its own interval; its flags leave by a plain store.  Lanes past the last interval idle behind the barrier. ----
__global__ void __launch_bounds__(64) k_texdec_entropy(const TexdecView v)
{
	__shared__ TdTables s_tab;
	const uint32_t *src = (const uint32_t *)v.tab;
	uint32_t *dst = (uint32_t *)&s_tab;
	for (uint32_t w = threadIdx.x; w < (uint32_t)(sizeof(TdTables) / 4u); w += 64u)
		dst[w] = src[w];
	__syncthreads();
	const uint32_t i = blockIdx.x * 64u + threadIdx.x;
	if (i < v.intervals)
		v.flags[i] = td_entropy_interval(v, s_tab, i);
}

// ---- k_texdec_idct: eight lanes share a block, 32 blocks a workgroup.  Lane j dequantises and transforms column j, the eight exchange
// the workspace through LDS, lane j transforms row j and stores its eight samples as one 8-byte row of the component's plane
// (the planes are whole blocks wide: every row of a block is 8-byte aligned).  Groups past the last block idle. ----
constexpr uint32_t TD_IDCT_GROUP = BLOCK / 8u;
__global__ void __launch_bounds__(BLOCK) k_texdec_idct(const TexdecView v)
{
	__shared__ int32_t s_ws[TD_IDCT_GROUP][64];
	const uint32_t l = threadIdx.x >> 3, j = threadIdx.x & 7u, g = blockIdx.x * TD_IDCT_GROUP + l;
	const bool live = g < v.blocks;
	size_t at = 0;
	uint32_t c = 0u;
	if (live)
	{
		c = td_block_place(v, g, &at);
		int32_t col[8];
		td_idct_col(v.coef + (size_t)g * 64u, v.tab->q[v.tq[c] & 3u], v.tab->izz, j, col);
		for (uint32_t u = 0; u < 8u; u++)
			s_ws[l][u * 8u + j] = col[u];
	}
	__syncthreads();
	if (live)
	{
		uint8_t px[8];
		td_idct_row(&s_ws[l][j * 8u], px);
		uint2 w;
		w.x = (uint32_t)px[0] | ((uint32_t)px[1] << 8) | ((uint32_t)px[2] << 16) | ((uint32_t)px[3] << 24);
		w.y = (uint32_t)px[4] | ((uint32_t)px[5] << 8) | ((uint32_t)px[6] << 16) | ((uint32_t)px[7] << 24);
		*(uint2 *)(v.planes + at + (size_t)j * v.pw[c]) = w;
	}
}

// ---- k_texdec_color: a thread per texel of level 0 (decoded planes, or the RGBA8 source: k_texdec_rgba is this kernel with v.src) ----
__global__ void __launch_bounds__(BLOCK) k_texdec_color(const TexdecView v)
{
	const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
	if (i >= (size_t)v.W * v.H)
		return;
	const uint32_t ty = (uint32_t)(i / v.W), x = (uint32_t)(i - (size_t)ty * v.W);
	v.out[i] = td_texel(v, x, ty);
}

// ---- k_tex_mips: a workgroup owns a 16 x 16 tile of level 0.  The quads are aligned, so the tile's 8 x 8, 4 x 4, 2 x 2 and 1 x 1
// descendants need nothing from outside it: one launch builds levels 1 .. 4.  A texel of level l exists when it lies inside
// (W >> l) x (H >> l); its four sources then exist as well.  The level-0 texels with alpha 0 are counted by a ballot per wave; the
// workgroup's count leaves by a plain store.  Every thread reaches every barrier. ----
__global__ void __launch_bounds__(256) k_tex_mips(const TexdecView v)
{
	__shared__ uint32_t s_a[256], s_b[64], s_n[4];
	const uint32_t tx = (v.W + 15u) / 16u, t = blockIdx.x, x0 = t % tx * 16u, y0 = t / tx * 16u;
	const uint32_t lx = threadIdx.x & 15u, ly = threadIdx.x >> 4;
	const bool in0 = x0 + lx < v.W && y0 + ly < v.H;
	const uint32_t texel = in0 ? v.out[(size_t)(y0 + ly) * v.W + x0 + lx] : 0xFFFFFFFFu;
	s_a[threadIdx.x] = texel;
	const unsigned long long zero = __ballot(in0 && (texel >> 24) == 0u);
	if ((threadIdx.x & 63u) == 0u)
		s_n[threadIdx.x >> 6] = (uint32_t)__popcll(zero);
	__syncthreads();
	if (threadIdx.x == 0u)
		v.alpha[t] = s_n[0] + s_n[1] + s_n[2] + s_n[3];
	uint32_t *src = s_a, *dst = s_b;
	size_t base = (size_t)v.W * v.H;
	for (uint32_t l = 1u; l < TD_MIP_LEVELS; l++)
	{
		const uint32_t side = 16u >> l, w = v.W >> l, h = v.H >> l, x = threadIdx.x % side, y = threadIdx.x / side;
		uint32_t o = 0u;
		const bool mine = threadIdx.x < side * side;
		if (mine)
		{
			const uint32_t *s = src + (2u * y) * (2u * side) + 2u * x;
			o = td_mip_texel(s[0], s[1], s[2u * side], s[2u * side + 1u]);
			const uint32_t gx = (x0 >> l) + x, gy = (y0 >> l) + y;
			if (gx < w && gy < h)
				v.out[base + (size_t)gy * w + gx] = o;
		}
		if (mine) // (dst was the source two levels up: everybody read it before the last barrier)
			dst[threadIdx.x] = o;
		__syncthreads();
		uint32_t *const sw = src;
		src = dst, dst = sw;
		base += (size_t)w * h;
	}
}

// ---- k_texdec_finish: one workgroup folds the intervals' flags and the tiles' counts into the record ----
__global__ void __launch_bounds__(BLOCK) k_texdec_finish(const TexdecView v)
{
	__shared__ uint32_t s_e[BLOCK], s_c[BLOCK];
	uint32_t e = 0u, a = 0u;
	if (v.flags)
		for (uint32_t i = threadIdx.x; i < v.intervals; i += BLOCK)
			e |= v.flags[i];
	for (uint32_t i = threadIdx.x; i < v.tiles; i += BLOCK)
		a += v.alpha[i];
	s_e[threadIdx.x] = e, s_c[threadIdx.x] = a;
	__syncthreads();
	if (threadIdx.x == 0u)
	{
		for (uint32_t k = 1; k < (uint32_t)BLOCK; k++)
			e |= s_e[k], a += s_c[k];
		td_record(v, e, a);
	}
}

static dim3 td_grid(size_t items, uint32_t per) { return dim3((uint32_t)((items + per - 1u) / per)); }
void launch_texdec_zero(const TexdecView &v, stream_t s) { hipLaunchKernelGGL(k_texdec_zero, td_grid((size_t)v.blocks * 8u, BLOCK), dim3(BLOCK), 0, (hipStream_t)s, v); }
void launch_texdec_entropy(const TexdecView &v, stream_t s) { hipLaunchKernelGGL(k_texdec_entropy, td_grid(v.intervals, 64u), dim3(64), 0, (hipStream_t)s, v); }
void launch_texdec_idct(const TexdecView &v, stream_t s) { hipLaunchKernelGGL(k_texdec_idct, td_grid(v.blocks, TD_IDCT_GROUP), dim3(BLOCK), 0, (hipStream_t)s, v); }
void launch_texdec_color(const TexdecView &v, stream_t s) { hipLaunchKernelGGL(k_texdec_color, td_grid((size_t)v.W * v.H, BLOCK), dim3(BLOCK), 0, (hipStream_t)s, v); }
void launch_tex_mips(const TexdecView &v, stream_t s) { hipLaunchKernelGGL(k_tex_mips, dim3(v.tiles), dim3(256), 0, (hipStream_t)s, v); }
void launch_texdec_finish(const TexdecView &v, stream_t s) { hipLaunchKernelGGL(k_texdec_finish, dim3(1), dim3(BLOCK), 0, (hipStream_t)s, v); }

#else // the emulation: the same items, serially

void launch_texdec_zero(const TexdecView &v, stream_t s)
{
	EMU_DEFER(s, launch_texdec_zero(v, s));
	td_host_zero(v);
}
void launch_texdec_entropy(const TexdecView &v, stream_t s)
{
	EMU_DEFER(s, launch_texdec_entropy(v, s));
	td_host_entropy(v);
}
void launch_texdec_idct(const TexdecView &v, stream_t s)
{
	EMU_DEFER(s, launch_texdec_idct(v, s));
	td_host_idct(v);
}
void launch_texdec_color(const TexdecView &v, stream_t s)
{
	EMU_DEFER(s, launch_texdec_color(v, s));
	td_host_color(v);
}
void launch_tex_mips(const TexdecView &v, stream_t s)
{
	EMU_DEFER(s, launch_tex_mips(v, s));
	td_host_mips(v);
}
void launch_texdec_finish(const TexdecView &v, stream_t s)
{
	EMU_DEFER(s, launch_texdec_finish(v, s));
	td_host_finish(v);
}
#endif
#endif // TEXTURE_DECODE_LAUNCHERS
